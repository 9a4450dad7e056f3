/* hdpgpc_hip_ragged.h - the per-(segment, cluster) path of libhdpgpc_hip.so for segments of different lengths: a further header
 * of the same C-ABI, in the conventions of hdpgpc_hip.h (device pointers owned by the caller, `stream` a hipStream_t as void*,
 * nothing allocated, freed or synchronised inside a call; 0 = work enqueued, -1 = bad argument, -2 = size not supported,
 * >= 1000 = 1000 + hipError_t; fp64, row-major).  The entry below belongs to the same library and version as hdpgpc_hip.h: its
 * HGP_ABI_VERSION covers it.  Usable alone or next to hdpgpc_hip.h, whose plan it takes (the typedef below repeats that header's: C11 / C++).
 */
#ifndef HDPGPC_HIP_RAGGED_H
#define HDPGPC_HIP_RAGGED_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hgp_pairs_plan hgp_pairs_plan;

/* a2 + a5 for a RAGGED batch - GPI_model.log_sq_error (GPI_model.py:250-286) takes one segment of any length, and the general
 * loop of compute_sq_err_all (GPI_model.py:535-545) calls it segment by segment; this is that loop as one call.
 *
 * hgp_loglik_pairs_f64 of hdpgpc_hip.h with a length per segment: x[N,ld], y[N,ld] hold segment n in the first seg_len[n]
 * entries of row n, 1 <= seg_len[n] <= ld; seg_len [N] int32 lives on the DEVICE and is read by the kernels only (no copy to the
 * host, no synchronisation).  Nothing beyond seg_len[n] in a row is read: the padding may hold anything, NaN included.
 * Row n's outputs are, bit for bit, those of hgp_loglik_pairs_f64 on the same plan for the one segment x[n, :seg_len[n]],
 * y[n, :seg_len[n]] with Ts = seg_len[n]: the length only says where a row ends.  That covers the score output
 * (hgp_pairs_plan_set_score_output): the offset -0.5 seg_len[n] log(2 pi) is formed per segment by the kernels.
 *
 * The same plan, routing (hgp_pairs_plan_set_accuracy: explicit operator / solve-based kernel per cluster, the static sweeps
 * of a block-tridiagonal E or the mask-driven ones per segment), first_noise, sel and output shapes as hgp_loglik_pairs_f64,
 * and the same one-stream rule: calls on one plan, ragged or not, must be ordered on one stream.
 *
 * A seg_len[n] outside [1, ld] is handled on the device: nothing of row n is read and its pairs get out_quad = NaN,
 * out_logdet = NaN, out_info = -1; every other row is scored as if the bad row were not there.
 * N == 0 is a no-op.  A NULL plan, x, y, seg_len or out_quad, N < 0 or ld < 1 is -1; ld above the plan's padded size (Ts_max of
 * hgp_pairs_plan_create rounded up to the kernels' tile) or above HGP_MAX_T_COOP is -2; both before any HIP call.
 * A segment costs what a segment of the plan's padded size costs, whatever its length. */
int hgp_loglik_pairs_ragged_f64(const hgp_pairs_plan* plan, const double* x, const double* y, int N, int ld,
                                const int32_t* seg_len, const double* first_noise, const int32_t* sel, double* out_quad,
                                double* out_logdet, int32_t* out_info, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HDPGPC_HIP_RAGGED_H */
