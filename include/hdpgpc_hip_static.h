/* hdpgpc_hip_static.h - the filter chain of a STATIC cluster model (Gamma = 0: the template does not evolve) on the device: a
 * further header of libhdpgpc_hip.so's C-ABI, in the conventions of hdpgpc_hip.h (device pointers owned by the caller, `stream` a
 * hipStream_t as void*, nothing allocated, freed or synchronised inside a call; 0 = work enqueued, -1 = bad argument, -2 = size not
 * supported, >= 1000 = 1000 + hipError_t; fp64, row-major).  The entries below belong to the same library and version as
 * hdpgpc_hip.h: its HGP_ABI_VERSION covers them.
 */
#ifndef HDPGPC_HIP_STATIC_H
#define HDPGPC_HIP_STATIC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* One chain: a static model absorbs n observations, one after the other (GPI_model.include_sample with h = 1 on the shared grid;
 * GPI.posterior, GPI.py:134-151, with Gamma = 0).  Member i (0 <= i < n) reads the state in row pos0 + i of the stacks and the
 * observation y = Y[y_idx[i], :], and appends row pos0 + i + 1:
 *     x_m = A m                     P_k = A P A^T        (first member with `first` set: P_k = P as it stands)
 *     f*  = C x_m,  cov_f = Sigma                        (first member with `first` set: f* = 0, cov_f = white I)
 *     S   = C P_k C^T + cov_f       K = P_k C^T S^-1
 *     m'  = x_m + K (y - f*)
 *     P'  = (I - K C) P_k (I - K C)^T + (K cov_f) K^T    (Joseph form)
 * S^-1 = Z^T Z with Z = chol(0.5 (S + S^T))^-1: the matrix is symmetrised as it is loaded and nothing is added to its diagonal -
 * the regulariser of hgp_chol_inverse_batched_f64 with jitter_rel = 0 and add_diag = 0, applied in that one pass.
 *
 * *pos is the chain's progress: on entry rows 0 .. *pos are valid, pos0 <= *pos <= pos0 + n; a call takes the members
 * i = *pos - pos0 .. and advances *pos by one per member, so the same descriptor continues the chain in a later call and
 * n1 + n2 members in two calls leave the bits of n1 + n2 members in one.  Fs and Ps need pos0 + n + 1 rows.
 *
 * A pivot of S that is not positive sets *info to its 1-based index (LAPACK), writes NaN to every row the chain would still
 * append (pos0 + i + 1 .. pos0 + n), sets *pos = pos0 + n and ends the chain; a chain whose *info is not 0 on entry is left
 * alone.  The caller zeroes *info before the chain's first call.  No chain reads or writes anything of another chain.
 *
 * A product with A or C is skipped when that matrix is the identity bit for bit AND every entry of the other factor is finite:
 * then the product's bits are those of `x + 0.0` (a 1 + sum b 0 is exact), which is what is used.  With a NaN or Inf in the other
 * factor the full product runs, so both propagate as through the products.  flags bit 0 switches the short-cut off (every
 * product runs): the result has the same bits either way.
 *
 * Nothing of y_idx beyond its first n entries is read; nothing but the appended rows of Fs and Ps, *pos, *info and the
 * chain's slice of the workspace is written. */
typedef struct hgp_static_chain_desc {
  const double* A;         /* [T,T] */
  const double* C;         /* [T,T] */
  const double* Sigma;     /* [T,T] */
  double* Fs;              /* [rows,T]   filtered means */
  double* Ps;              /* [rows,T,T] filtered covariances */
  int64_t* pos;            /* [1] last valid row */
  const double* Y;         /* [*,T] observations */
  const int64_t* y_idx;    /* [n] rows of Y, in the order the chain absorbs them */
  int32_t* info;           /* [1] */
  double white;            /* cov_f = white I of the first-step branch */
  int64_t pos0;            /* row the chain's first member starts from */
  int32_t n;               /* members of the chain */
  int32_t first;           /* != 0: member 0 takes the first-step branch (the prior covariance is the kernel Gram itself, GPI.py:136-139) */
  int32_t flags;           /* bit 0: no identity short-cut */
  int32_t reserved;
} hgp_static_chain_desc;

/* Workspace of a call over B chains of order T (bytes; 0 for B <= 0 or T outside [1, 128]). */
size_t hgp_static_chain_ws_bytes(int B, int T);
/* Up to max_steps members of each of the B chains descs[0 .. B) (an array in DEVICE memory), all in ONE launch: one workgroup per
 * chain walks its members; chains of different lengths end at different times.  T <= 128 (HGP_MAX_T_WAVE): above that -2, and the
 * caller keeps the eager path.  B == 0 or max_steps == 0 is a no-op; B < 0, T < 1, max_steps < 0, descs == NULL, ws == NULL or
 * ws_bytes < hgp_static_chain_ws_bytes(B, T) is -1.  All of these are decided before any HIP call. */
int hgp_static_chain_steps_f64(const hgp_static_chain_desc* descs, int B, int T, int max_steps, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HDPGPC_HIP_STATIC_H */
