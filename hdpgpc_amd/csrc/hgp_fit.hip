// The kernel hyper-parameter fit of a new cluster for B segments at once (include/hdpgpc_hip_fit.h; SURVEY.md 8f-2, batched):
// Adam on the exact marginal log-likelihood, what kernel_fit.fit_kernel_adam runs from the host one segment and one iteration at a
// time.  One Adam step of ALL fits is a fixed sequence of launches and nothing returns to the host between them:
//   1. k_fit_gram     K_b = c RBF(ell) + noise I from the raw parameters in the fit's state row (a frozen fit: the identity,
//                     so that the shared factor launch has nothing to fail on)
//   2. the batched inverse factor of the L^-1 family (hgp_inverse.hip): Z_b = L_b^-1, info_b
//                     (T <= 128: one launch, one wave per block column;  above: in-place cooperative factor + k_trtri, two launches)
//   3. K^-1 = Z^T Z   one batched product on the matrix core (hgp_gemm.hip), into the buffer K came from
//   4. k_fit_update   one workgroup per fit: alpha = K^-1 r, the loss, the three traces of hgp_lml_grad_f64, the chain rule to the
//                     raw parameters, the Adam update, the loss window, the stop rule; writes the state row, status and loss
// A fit is touched by its own workgroups only and every reduction runs in an order fixed by T (strided partial sums over 256
// threads, then a fixed tree over 256 slots): the same bits for any B, any position in the batch, any split into calls.
#include <math.h>

#include "../../include/hdpgpc_hip_fit.h"
#include "hgp_internal.hpp"

namespace {

constexpr int FIT_IT = 12;     // state row: p[0..4), m1[4..8), m2[8..12), completed iterations, eleven losses [13..24), reserved
constexpr int FIT_LOSS = 13;
constexpr int FIT_WIN = 11;

struct FitArgs {
  const double* x;
  long x_stride;
  const double* Y;
  int T, B;
  const double* bounds;
  double lr;
  int min_iter, max_iter;
  double* state;
  int32_t* status;
  double* loss_out;
  int loss_ld;
  double* K;             // [B,T,T] Gram matrix, then K^-1
  const double* Z;       // [B,T,T] L^-1
  const int32_t* info;   // [B] status of the factorisation
};

// the stable forms of kernel_fit.py:26-31
__device__ __forceinline__ double softplus_d(double v) { return log1p(exp(-fabs(v))) + fmax(v, 0.0); }
__device__ __forceinline__ double sigmoid_d(double v) { return v >= 0.0 ? 1.0 / (1.0 + exp(-v)) : exp(v) / (1.0 + exp(v)); }

// the sum of red[0..256) of each of NV vectors by a fixed tree, valid in red[v][0]; every thread of the workgroup calls it
template <int NV>
__device__ __forceinline__ void tree_sum(double (*red)[256], int tid) {
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o)
#pragma unroll
      for (int v = 0; v < NV; ++v) red[v][tid] += red[v][tid + o];
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void k_fit_gram(FitArgs a, int tiles) {
  const int b = blockIdx.x / tiles, T = a.T;
  const int idx = (blockIdx.x % tiles) * 256 + threadIdx.x;
  if (idx >= T * T) return;
  const int i = idx / T, j = idx % T;
  double* __restrict__ K = a.K + (size_t)b * T * T;
  if (a.status[b] != 0) {   // frozen: the identity
    K[idx] = (i == j) ? 1.0 : 0.0;
    return;
  }
  const double* __restrict__ p = a.state + (size_t)b * HGP_FIT_STATE_DOUBLES;
  const double* __restrict__ x = a.x + (size_t)b * a.x_stride;
  const double lo = a.bounds[2 * b], hi = a.bounds[2 * b + 1];
  const double noise = lo + (hi - lo) * sigmoid_d(p[0]);
  const double c = softplus_d(p[2]), ell = softplus_d(p[3]);
  const double u = x[i] / ell - x[j] / ell;   // sklearn divides by the length-scale first (k_gram_rbf)
  double v = c * exp(-0.5 * (u * u));
  if (i == j) v = c + noise;
  K[idx] = v;
}

__global__ __launch_bounds__(256) void k_fit_update(FitArgs a) {
  __shared__ double r_s[256], al_s[256];
  __shared__ double red[3][256];
  const int b = blockIdx.x, tid = threadIdx.x, T = a.T;
  if (a.status[b] != 0) return;   // frozen (uniform over the workgroup; read before the first barrier, written after the last)
  double* __restrict__ st = a.state + (size_t)b * HGP_FIT_STATE_DOUBLES;
  const int it = (int)st[FIT_IT] + 1;
  if (it > a.max_iter) {          // the budget was already used up when the call began
    if (tid == 0) a.status[b] = 2;
    return;
  }
  const double* __restrict__ x = a.x + (size_t)b * a.x_stride;
  const double* __restrict__ y = a.Y + (size_t)b * T;
  const double* __restrict__ Kinv = a.K + (size_t)b * T * T;
  const double* __restrict__ Z = a.Z + (size_t)b * T * T;
  const double p0 = st[0], p1 = st[1], p2 = st[2], p3 = st[3];
  const double lo = a.bounds[2 * b], hi = a.bounds[2 * b + 1];
  const double s_n = sigmoid_d(p0);
  const double noise = lo + (hi - lo) * s_n;
  const double c = softplus_d(p2), ell = softplus_d(p3);

  r_s[tid] = tid < T ? y[tid] - p1 : 0.0;
  __syncthreads();
  // alpha_i = sum_j K^-1[j][i] r_j, j ascending (a column of the symmetric K^-1: consecutive threads, consecutive addresses)
  double al = 0.0;
  if (tid < T)
    for (int j = 0; j < T; ++j) al = fma(Kinv[(size_t)j * T + tid], r_s[j], al);
  al_s[tid] = al;
  red[0][tid] = tid < T ? r_s[tid] * al : 0.0;                               // quad = r^T alpha
  red[1][tid] = al;                                                          // sum(alpha) = d/d mean
  red[2][tid] = tid < T ? log(Z[(size_t)tid * T + tid]) : 0.0;               // log det K = -2 sum log (L^-1)_ii
  tree_sum<3>(red, tid);
  const double quad = red[0][0], sum_alpha = red[1][0], logdet = -2.0 * red[2][0];
  __syncthreads();
  // the three traces, element order and arithmetic of k_lml_grad
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  const int tt = T * T;
  for (int idx = tid; idx < tt; idx += 256) {
    const int i = idx / T, j = idx % T;
    const double t = al_s[i] * al_s[j] - Kinv[idx];
    const double u = x[i] / ell - x[j] / ell, d2 = u * u;
    const double cr = c * exp(-0.5 * d2);
    s0 = fma(t, cr, s0);
    s1 = fma(t, cr * d2, s1);
    if (i == j) s2 += t;
  }
  red[0][tid] = s0;
  red[1][tid] = s1;
  red[2][tid] = s2;
  tree_sum<3>(red, tid);
  if (tid != 0) return;

  {
#pragma clang fp contract(off)   // the host loop's operation order, no fused multiply-add
    const double glog0 = 0.5 * red[0][0], glog1 = 0.5 * red[1][0], glog2 = 0.5 * noise * red[2][0];
    const double val = -0.5 * quad - 0.5 * logdet - 0.5 * T * LOG_2PI;
    const double loss = -val / T;
    if (a.info[b] != 0) {
      a.status[b] = -1;
      return;
    }
    const double sc = -1.0 / T;
    double g[4];
    g[0] = glog2 / noise * (hi - lo) * s_n * (1.0 - s_n) * sc;
    g[1] = sum_alpha * sc;
    g[2] = glog0 / c * sigmoid_d(p2) * sc;
    g[3] = glog1 / ell * sigmoid_d(p3) * sc;
    const double big = 1.79769313486231570815e308;
    if (!(fabs(loss) <= big) || !(fabs(g[0]) <= big) || !(fabs(g[1]) <= big) || !(fabs(g[2]) <= big) || !(fabs(g[3]) <= big)) {
      a.status[b] = -2;
      return;
    }
    const double b1 = 0.9, b2 = 0.999, eps = 1e-8;   // torch.optim.Adam defaults
    const double c1 = 1.0 - pow(b1, (double)it), c2 = 1.0 - pow(b2, (double)it);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double m1 = b1 * st[4 + k] + (1.0 - b1) * g[k];
      const double m2 = b2 * st[8 + k] + (1.0 - b2) * g[k] * g[k];
      st[4 + k] = m1;
      st[8 + k] = m2;
      st[k] = st[k] - a.lr * (m1 / c1) / (sqrt(m2 / c2) + eps);
    }
    double h[FIT_WIN];
#pragma unroll
    for (int k = 0; k + 1 < FIT_WIN; ++k) h[k] = st[FIT_LOSS + k + 1];
    h[FIT_WIN - 1] = loss;
    double inc = 0.0;
#pragma unroll
    for (int k = 0; k < FIT_WIN; ++k) {
      st[FIT_LOSS + k] = h[k];
      if (k > 0) inc += h[k] - h[k - 1];
    }
    st[FIT_IT] = (double)it;
    if (a.loss_out && it <= a.loss_ld) a.loss_out[(size_t)b * a.loss_ld + it - 1] = loss;
    if (it > a.min_iter && it >= FIT_WIN && fabs(inc) <= 1e-4) a.status[b] = 1;   // GPI.py:689-693
    else if (it >= a.max_iter) a.status[b] = 2;
  }
}

// The caller's workspace of hgp_kernel_fit_steps_f64 (doubles), stated once for hgp_kernel_fit_ws_bytes and the entry point
struct FitWs {
  double *K, *Z;   // K then K^-1 [B,T,T]; the inverse factor [B,T,T]
  int32_t* info;   // [B] the factor's status, in the room of B doubles
  static constexpr size_t tt(int B, int T) { return (size_t)B * T * T; }
  static constexpr size_t K_off(int, int) { return 0; }
  static constexpr size_t Z_off(int B, int T) { return K_off(B, T) + tt(B, T); }
  static constexpr size_t info_off(int B, int T) { return Z_off(B, T) + tt(B, T); }
  static constexpr size_t bytes(int B, int T) { return sizeof(double) * (info_off(B, T) + B); }
  static FitWs carve(void* ws, int B, int T) {
    double* w = static_cast<double*>(ws);
    return {w + K_off(B, T), w + Z_off(B, T), reinterpret_cast<int32_t*>(w + info_off(B, T))};
  }
};
static_assert(FitWs::bytes(7, 129) == 8 * (2 * 7 * 129 * 129 + 7), "hgp_kernel_fit_steps_f64: the workspace callers have sized so far");

}  // namespace

extern "C" size_t hgp_kernel_fit_ws_bytes(int B, int T) { return B < 1 || T < 1 ? 0 : FitWs::bytes(B, T); }

extern "C" int hgp_kernel_fit_steps_f64(const double* x, long x_stride, const double* Y, int T, int B, const double* bounds, double lr,
                                        int n_steps, int min_iter, int max_iter, double* state, int32_t* status, double* loss_out,
                                        int loss_ld, void* ws, size_t ws_bytes, void* stream) {
  if (T < 1 || B < 1 || n_steps < 0 || x_stride < 0 || !x || !Y || !bounds || !state || !status || !ws) return -1;
  if (loss_out && loss_ld < 1) return -1;
  if (T > HGP_MAX_T_COOP) return -2;
  const long tt = (long)T * T;
  const int tiles = (int)((tt + 255) / 256);
  if ((long)tiles * B > 2147483647L) return -2;
  if (ws_bytes < FitWs::bytes(B, T)) return -1;
  hipStream_t st = (hipStream_t)stream;
  const FitWs w = FitWs::carve(ws, B, T);
  double *K = w.K, *Z = w.Z;
  int32_t* info = w.info;
  FitArgs a{x, x_stride, Y, T, B, bounds, lr, min_iter, max_iter, state, status, loss_out, loss_ld, K, Z, info};
  for (int s = 0; s < n_steps; ++s) {
    hipLaunchKernelGGL(k_fit_gram, dim3((unsigned)(tiles * B)), dim3(256), 0, st, a, tiles);
    if (int rc = launch_status()) return rc;
    // one route per T whatever B is (the bits of a fit must not depend on the batch): the wave kernels' inverse factor for
    // T <= HGP_MAX_T_WAVE; above, the cooperative factor in place (K <- L) followed by k_trtri
    int rc = T <= HGP_MAX_T_WAVE ? hgp_chol_inverse_batched_f64(K, T, B, 0.0, 0.0, Z, info, stream)
                                 : hgp_potrf_batched_f64(K, T, B, 0.0, 0.0, Z, nullptr, info, stream);
    if (rc) return rc;
    if ((rc = hgp_gemm_batched_f64(1, 0, T, T, T, 1.0, Z, T, tt, Z, T, tt, 0.0, K, T, tt, B, stream))) return rc;
    hipLaunchKernelGGL(k_fit_update, dim3(B), dim3(256), 0, st, a);
    if ((rc = launch_status())) return rc;
  }
  return 0;
}
