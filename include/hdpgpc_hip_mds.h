/* hdpgpc_hip_mds.h - the MDS embedding of a distance matrix (metric SMACOF) of libhdpgpc_hip.so: a further header of the same
 * C-ABI, in the conventions of hdpgpc_hip.h (device pointers owned by the caller, `stream` a hipStream_t as void*, nothing
 * allocated, freed or synchronised inside a call; 0 = work enqueued, -1 = bad argument, >= 1000 = 1000 + hipError_t; fp64,
 * row-major).  The entries below belong to the same library and version as hdpgpc_hip.h: HGP_ABI_VERSION there covers them.
 */
#ifndef HDPGPC_HIP_MDS_H
#define HDPGPC_HIP_MDS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* a15 - what plot_MDS / plot_MDS_plotly run on the distance matrix (util_plots.py:619-620): sklearn.manifold.MDS(dissimilarity=
 * 'precomputed'), that is metric SMACOF (sklearn/manifold/_mds.py::_smacof_single), for B start configurations X[B,n,p] of the
 * same matrix delta[n,n] (row stride ld; symmetric, zero diagonal, zeros elsewhere allowed) at once and resumable: a call
 * advances every start that is still running by up to n_steps passes; everything a start carries between passes lives in its
 * row of `state`.
 *
 * Pass k = 0, 1, ... of start b, with X_k = X[b] as the pass finds it:
 *   d_ij = sqrt(sum_c (x_ic - x_jc)^2)   by direct differences, c ascending;   dd_ij = d_ij == 0 ? 1e-5 : d_ij
 *   X_{k+1}[i] = (1/n) sum_j (delta_ij / dd_ij) (X_k[i] - X_k[j])             (the Guttman transform B X / n in difference form)
 *   S_k = sum_ij (d_ij - delta_ij)^2 / 2,   N_k = sum_ij d_ij^2 / 2           (the raw stress and the norm of X_k, full matrix)
 *   then, per start:  a non-finite S_k or N_k ends it with status -2;
 *                     k >= 2 and (S_{k-1} - S_k) / N_k < eps ends it with status 1   (a NaN compares false: the start goes on);
 *                     k >= max_iter ends it with status 2;
 *                     otherwise X[b] <- X_{k+1} and the start goes on.
 * scikit-learn's iteration `it` computes X_{it+1} and the stress of X_{it+1}; that stress is S_{it+1} here, the by-product of the
 * NEXT pass, so the stop decision of iteration `it` is taken in pass it + 1 and the X_{it+2} that pass computed is dropped.
 * A start that ends in pass k therefore holds X[b] = X_k, stress[b] = S_k and n_iter[b] = k: the triple _smacof_single returns
 * (normalized_stress=False).  The end at max_iter needs S of the last iterate: a start runs max_iter + 1 passes at the most.
 *
 * state [B, HGP_MDS_STATE_DOUBLES] per start: [0] the passes completed = k of the current iterate X_k = scikit-learn's iterations
 *   done, [1] S_{k-1}, [2] S_{k-2}, [3] N_{k-1}; four reserved doubles (left as they are).
 * status [B]: 0 running, 1 ended by the stop rule, 2 ended at max_iter, -2 a non-finite stress (non-finite delta or X): X[b] is
 *   left as it was before the failing pass.  While status[b] is 0, X[b] is the current iterate and stress[b], n_iter[b] are not
 *   written.  A start whose status is not 0 is frozen: no call touches its X, state, status, stress or n_iter again.
 * An all-zero state and status is the beginning: there is no init entry.
 * n < 1, p outside 1..3, B < 1, n_steps < 0, ld < n or a NULL delta, X, state, status, stress, n_iter or ws is -1, before any
 * HIP call.  ws: caller-provided workspace of at least hgp_smacof_ws_bytes(B, n, p) bytes (X_{k+1} of every start, then the two
 * partial sums of every row of every start; 0 for B, n or p < 1); ws_bytes: what the caller provides - less than that is -1,
 * before any HIP call.
 *
 * Every pass is two launches whatever B is (the sweep over delta for all starts; the reduction, stop rule and hand-over of
 * every start); nothing returns to the host between them, no launch waits on another workgroup, and a call enqueues n_steps
 * such pairs whatever the starts do.  A start's trajectory depends on delta, eps, max_iter and its own X_0 only and every sum
 * runs in an order fixed by n and p: the same bits for any B, any position in the batch and any split of the passes over
 * calls. */
#define HGP_MDS_STATE_DOUBLES 8
size_t hgp_smacof_ws_bytes(int B, int n, int p);
int hgp_smacof_steps_f64(const double* delta, int ld, int n, int p, int B, double* X /* [B,n,p] in/out */, double eps, int n_steps,
                         int max_iter, double* state /* [B, HGP_MDS_STATE_DOUBLES] */, int32_t* status /* [B] */,
                         double* stress /* [B] */, int32_t* n_iter /* [B] */, void* ws, size_t ws_bytes /* hgp_smacof_ws_bytes(B, n, p) */,
                         void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HDPGPC_HIP_MDS_H */
