/* hdpgpc_hip_fit.h - the kernel hyper-parameter fit of libhdpgpc_hip.so: a second header of the same C-ABI, in the conventions
 * of hdpgpc_hip.h (device pointers owned by the caller, `stream` a hipStream_t as void*, nothing allocated, freed or synchronised
 * inside a call; 0 = work enqueued, -1 = bad argument, -2 = size not supported, >= 1000 = 1000 + hipError_t; fp64, row-major).
 * The entries below belong to the same library and version as hdpgpc_hip.h: HGP_ABI_VERSION there covers them.
 */
#ifndef HDPGPC_HIP_FIT_H
#define HDPGPC_HIP_FIT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 8f-2, batched - IterativeGaussianProcess.fit_torch (GPI.py:610-770): Adam on the exact marginal log-likelihood of ONE segment
 * (constant mean, ScaleKernel(RBFKernel), Gaussian likelihood with the noise in a sigmoid interval, gpytorch's defaults), for B
 * independent segments Y[B,T] at once and resumable: a call advances every fit that is still running by up to n_steps Adam
 * iterations; everything a fit carries between iterations lives in its row of `state`.
 *
 * Iteration `it` (1-based) of fit b, raw parameters p = (raw noise, mean, raw output-scale, raw length-scale):
 *   s = sigmoid(p0); noise = lo_b + (hi_b - lo_b) s; c = softplus(p2); ell = softplus(p3);  r = y_b - p1
 *   K_ij = c exp(-0.5 (x_i/ell - x_j/ell)^2), K_ii = c + noise   (the one-argument Gram of hgp_gram_rbf_f64; nothing else added)
 *   K = L L^T; alpha = K^-1 r; quad = r^T alpha; logdet = log det K
 *   loss = (0.5 quad + 0.5 logdet + 0.5 T log 2pi) / T                                      -> loss_out[b, it - 1]
 *   glog = 0.5 tr((alpha alpha^T - K^-1) dK/d(log c, log ell, log noise))                   (as hgp_lml_grad_f64)
 *   g = -(1/T) (glog2 / noise (hi_b - lo_b) s (1 - s),  sum(alpha),  glog0 / c sigmoid(p2),  glog1 / ell sigmoid(p3))
 *   Adam (beta1 0.9, beta2 0.999, eps 1e-8, bias correction, torch.optim.Adam's operation order) with step lr
 *   stop: after the update, if it > min_iter (and it >= 11) and |sum of the last ten loss increments, oldest first| <= 1e-4 the
 *   fit ends with status 1 (GPI.py:689-693); it == max_iter ends it with status 2.
 *
 * state [B, HGP_FIT_STATE_DOUBLES] per fit: p[4], Adam's first moments [4], second moments [4], the number of completed
 *   iterations (n_iter once the fit has ended), the last eleven losses (oldest first), eight reserved doubles (left as they are).
 * status [B]: 0 running, 1 ended by the stop rule, 2 ended by the budget, < 0 failed: -1 = a pivot of K was not positive,
 *   -2 = a non-finite loss or gradient (non-finite x, y or parameters).  A failed fit keeps the state it had before the failing
 *   iteration.  A fit whose status is not 0 is frozen: no call touches its state, status or losses again.
 * An all-zero state and status is the start of a fit (gpytorch starts every raw parameter at 0): there is no init entry.
 *
 * x: the grid, [T] shared by every fit (x_stride 0) or one grid per fit (fit b reads x + b x_stride); bounds [B,2] = (lo, hi) of
 * the noise; loss_out (may be NULL) [B, loss_ld]: iteration `it` writes column it - 1 if it <= loss_ld.
 * T <= HGP_MAX_T_COOP of hdpgpc_hip.h (-2 above); T < 1, B < 1, n_steps < 0, x_stride < 0 or a NULL x, Y, bounds, state, status
 * or ws is -1, before any HIP call.
 * ws: caller-provided workspace of at least hgp_kernel_fit_ws_bytes(B, T) bytes (K then K^-1, the inverse factor, the factor's
 * status; 0 for B < 1 or T < 1); ws_bytes: what the caller provides - less than that is -1, before any HIP call.
 *
 * Every Adam step is a fixed sequence of launches for all B fits (Gram, the batched Cholesky family of hdpgpc_hip.h, one
 * product, one update: four launches for T <= HGP_MAX_T_WAVE, five above); nothing returns to the host between them, no launch
 * waits on another workgroup, and a call enqueues n_steps such sequences whatever the fits do.  A fit's trajectory depends on its
 * own x, y and bounds only and every sum runs in an order fixed by T: the same bits for any B, any position in the batch and
 * any split of the iterations over calls. */
#define HGP_FIT_STATE_DOUBLES 32
size_t hgp_kernel_fit_ws_bytes(int B, int T);
int hgp_kernel_fit_steps_f64(const double* x, long x_stride, const double* Y, int T, int B, const double* bounds, double lr,
                             int n_steps, int min_iter, int max_iter, double* state, int32_t* status, double* loss_out,
                             int loss_ld, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HDPGPC_HIP_FIT_H */
