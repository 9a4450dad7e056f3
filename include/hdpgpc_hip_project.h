/* hdpgpc_hip_project.h - projection of segments of different lengths onto the basis grid: a further header of libhdpgpc_hip.so's
 * C-ABI, in the conventions of hdpgpc_hip.h (device pointers owned by the caller, `stream` a hipStream_t as void*, nothing
 * allocated, freed or synchronised inside a call; 0 = work enqueued, -1 = bad argument, -2 = size not supported, >= 1000 =
 * 1000 + hipError_t; fp64, row-major).  The entries below belong to the same library and version as hdpgpc_hip.h: its HGP_ABI_VERSION covers them.
 */
#ifndef HDPGPC_HIP_PROJECT_H
#define HDPGPC_HIP_PROJECT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* IterativeGaussianProcess.project_y (GPI.py:194-238) with C = I for a RAGGED batch, one call:
 *     yp[n] = K(xb, x_n) (K(x_n, x_n) + jitter I)^-1 y_n,      K(a, b)_ij = c exp(-0.5 ((a_i - b_j) / ell)^2)   (no white noise)
 * for segment n with L = lengths[n] points: grid x_n = x[n, :L], values y_n = y[n, :L, :] (D leads = D right-hand sides).
 * x [N,ld], y [N,ld,D], lengths [N] int32 on the DEVICE (read by the kernels only; NULL: every row has ld points), xb [T],
 * yp [N,T,D], info [N].  Nothing of a row beyond its length is read: the padding may hold anything, NaN included.
 *
 * A row with L == T whose grid equals xb bit for bit is copied, yp[n] = y[n] bit for bit and info[n] = 0 (the reference's
 * torch.equal short-circuit).  Every other row is factored: jitter is added to the diagonal as it stands (absolute, no relative
 * part; the reference passes 1e-4), and a pivot that is not positive gives info[n] = its 1-based index and yp[n] = NaN.
 * A lengths[n] outside [1, ld] gives info[n] = -1 and yp[n] = NaN without reading the row.  No row affects another, and a
 * row's result bits depend on ld, T and the row alone - not on N, its position, its neighbours or D (column d of a call with
 * D leads has the bits of the one-lead call on that column).
 *
 * ld <= HGP_MAX_T_WAVE (128): one wavefront per (segment, 16 leads), nothing but x, y, yp in HBM; ws may be NULL.
 * ld <= HGP_MAX_T_COOP (256): factored by the cooperative kernels through ws (hgp_project_ragged_ws_bytes; 2 N ld^2 doubles).
 * N == 0 is a no-op.  N < 0, ld < 1, D < 1, T < 1, a NULL x, y, xb, yp or info, c <= 0, ell <= 0 or jitter < 0 (or NaN) is -1;
 * ld or T above HGP_MAX_T_COOP, or a workspace that is missing or too small, is -2; both before any HIP call. */
size_t hgp_project_ragged_ws_bytes(int N, int ld, int T, int D);
int hgp_project_ragged_f64(const double* x, const double* y, const int32_t* lengths, int N, int ld, int D, const double* xb, int T,
                           double c, double ell, double jitter, double* yp, int32_t* info, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HDPGPC_HIP_PROJECT_H */
