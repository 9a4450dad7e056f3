/* hdpgpc_hip_segops.h - the per-(segment, cluster) path of libhdpgpc_hip.so with the per-segment operators kept from call to call:
 * a further header of the same C-ABI, in the conventions of hdpgpc_hip.h (device pointers owned by the caller, `stream` a
 * hipStream_t as void*, nothing allocated, freed or synchronised inside a call; 0 = work enqueued, -1 = bad argument, -2 = size
 * not supported, >= 1000 = 1000 + hipError_t; fp64, row-major).  The entries below belong to the same library and version as
 * hdpgpc_hip.h: its HGP_ABI_VERSION covers them.  Usable alone or next to hdpgpc_hip.h, whose plan they take (the typedef below
 * repeats that header's: C11 / C++).
 */
#ifndef HDPGPC_HIP_SEGOPS_H
#define HDPGPC_HIP_SEGOPS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hgp_pairs_plan hgp_pairs_plan;

/* A sampler scores the SAME segments against cluster states that change from call to call.  What the band pair kernel (padded
 * size 96 or 128) builds per segment before it meets a cluster - the blocks of E = exp(-0.5 ((xb_k - x_j) / ell)^2), the tiles of
 * K**, the decision between the static and the mask-driven sweeps - depends on the segment's grid and length, the basis grid and
 * the length-scale only.  The segment-operator store keeps it: a device buffer of the caller,
 * hgp_pairs_segops_bytes(plan, N, ld) bytes for batches of N rows of ld points, 256-byte aligned, one record per (length-scale
 * group of the plan, segment).  A record carries its key - the x row, its length, the basis grid, the length-scale, T, ld - and
 * every call compares the key with its arguments ON THE BITS (a NaN equals itself) before it uses the record; a record that
 * differs or is not valid is rebuilt first.  The caller never invalidates anything: a zero-filled buffer holds nothing valid,
 * and a buffer filled by another plan, another batch or an interrupted call is merely rebuilt where it differs.
 *
 * Returns 0 where no band kernel serves the shape (plan NULL, N < 1, ld < 1 or above the plan's padded size, padded size below
 * 96 or above 128, HGP_PAIRS_GENERIC set in the environment): hgp_loglik_pairs_segops_f64 then needs no store. */
size_t hgp_pairs_segops_bytes(const hgp_pairs_plan* plan, int N, int ld);

/* hgp_loglik_pairs_f64 (seg_len == NULL: every row has ld points) or hgp_loglik_pairs_ragged_f64 (seg_len [N] int32 on the
 * device) with the store `segops` of `segops_bytes` bytes.  Same arguments, routing, outputs and one-stream rule as those entries,
 * and the same bits in every output.  The store belongs to the calls of one stream at a time, like the plan.
 * Where hgp_pairs_segops_bytes(plan, N, ld) is 0 the call forwards to those entries and segops is not looked at.  Otherwise a
 * NULL segops, one that is not 16-byte aligned or segops_bytes below hgp_pairs_segops_bytes(plan, N, ld) is -1, like a NULL plan,
 * x, y or out_quad, N < 0 or ld < 1; all before any HIP call.  N == 0 is a no-op. */
int hgp_loglik_pairs_segops_f64(const hgp_pairs_plan* plan, void* segops, size_t segops_bytes, const double* x, const double* y,
                                int N, int ld, const int32_t* seg_len, const double* first_noise, const int32_t* sel,
                                double* out_quad, double* out_logdet, int32_t* out_info, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HDPGPC_HIP_SEGOPS_H */
