// libhdpgpc_hip.so - the Gaussian-process kernels outside the pair path (Gram matrices a1 / a11, the a10 solve and gradient),
// the two lane-map / exp probes and hgp_abi_version.  The other subsystems of the C-ABI (include/hdpgpc_hip.h) have one unit each.
#include "hgp_internal.hpp"
#include "tile_f64.hpp"

using namespace hgp;

namespace {

// ------------------------------------------------------------------------------------------ a1
__global__ void k_gram_rbf(const double* __restrict__ x, int nx, const double* __restrict__ y, int ny, double c,
                           double ell, double noise, int one_arg, double* __restrict__ K) {
  size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)nx * ny) return;
  int i = (int)(idx / ny), j = (int)(idx % ny);
  double u = x[i] / ell - (one_arg ? x[j] : y[j]) / ell;   // sklearn divides by the length-scale first
  double v = c * exp(-0.5 * (u * u));
  if (one_arg && i == j) v = c + noise;
  K[idx] = v;
}

// diagnostics: one 16x16x16 product through the operand / accumulator lane maps tile_f64.hpp assumes
__global__ void k_mfma_probe(const double* __restrict__ A, const double* __restrict__ B, double* __restrict__ C) {
  const int lane = threadIdx.x & 63, g = lane >> 4, c = lane & 15;
  d4 acc = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int s = 0; s < 4; ++s) acc = mfma(A[c * 16 + 4 * s + g], B[(4 * s + g) * 16 + c], acc);
#pragma unroll
  for (int r = 0; r < 4; ++r) C[(g + 4 * r) * 16 + c] = acc[r];
}

// diagnostics: the kernels' own exp(-h), four values per lane
__global__ void k_exp_probe(const double* __restrict__ h, int n, double* __restrict__ out) {
  const int i = 4 * (blockIdx.x * blockDim.x + threadIdx.x);
  if (i + 3 >= n + 0 && i >= n) return;
  double hv[4], ev[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) hv[j] = (i + j < n) ? h[i + j] : 0.0;
  exp_neg4(hv, ev);
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (i + j < n) out[i + j] = ev[j];
}

// a11: omega^2 exp(-0.5 dx^2 / rho^2) + diag_add I on the (optionally [0,1]-normalised) grid
__global__ void k_warp_cov(const double* __restrict__ x, int T, double rho, double omega, double diag_add, int normalize,
                           double* __restrict__ K) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)T * T) return;
  const int i = (int)(idx / T), j = (int)(idx % T);
  double xi = x[i], xj = x[j];
  if (normalize) {
    const double x0 = x[0];
    const double rng = fabs((x[T - 1] - x0) - (x0 - x0)) + 1e-12;   // amtgp_warping_system.py:163-166
    xi = (xi - x0) / rng;
    xj = (xj - x0) / rng;
  }
  const double dx = xi - xj;
  double v = (omega * omega) * exp(-0.5 * (dx * dx) / (rho * rho));
  if (i == j) v += diag_add;
  K[idx] = v;
}

// a10 (reference as written, GPI.py:1043): || G^{-1} y ||^2 with G = tril(K) used as if it were a Cholesky factor.
// One workgroup, column-oriented forward substitution in LDS; T <= 2048.
__global__ __launch_bounds__(256) void k_trsv_lower_quad(const double* __restrict__ G, int ld, const double* __restrict__ y,
                                                          int T, double* __restrict__ out, double* __restrict__ alpha) {
  extern __shared__ double w[];
  for (int i = threadIdx.x; i < T; i += 256) w[i] = y[i];
  __syncthreads();
  for (int k = 0; k < T; ++k) {
    if (threadIdx.x == 0) w[k] = w[k] / G[(size_t)k * ld + k];
    __syncthreads();
    const double wk = w[k];
    for (int i = k + 1 + threadIdx.x; i < T; i += 256) w[i] = fma(-G[(size_t)i * ld + k], wk, w[i]);
    __syncthreads();
  }
  __shared__ double red[256];
  double s = 0.0;
  for (int i = threadIdx.x; i < T; i += 256) s = fma(w[i], w[i], s);
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0 && out) out[0] = red[0];
  if (alpha) {   // alpha = G^{-T} w  (cho_solve((G, True), y), the second half of the reference's call)
    for (int k = T - 1; k >= 0; --k) {
      __syncthreads();
      if (threadIdx.x == 0) w[k] = w[k] / G[(size_t)k * ld + k];
      __syncthreads();
      const double wk = w[k];
      for (int i = threadIdx.x; i < k; i += 256) w[i] = fma(-G[(size_t)k * ld + i], wk, w[i]);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < T; i += 256) alpha[i] = w[i];
  }
}

// a10 gradient (GPI.py:1046-1051): out[k] = 0.5 tr((alpha alpha^T - Kinv) dK/dtheta_k) for theta = (log c, log ell, log noise)
// with scikit-learn's kernel gradients: c R, c R d^2 / ell^2, noise I  (R_ij = exp(-0.5 d^2 / ell^2)).
__global__ __launch_bounds__(256) void k_lml_grad(const double* __restrict__ x, const double* __restrict__ alpha,
                                                  const double* __restrict__ Kinv, int T, double c, double ell,
                                                  double noise, double* __restrict__ out) {
  __shared__ double red[3][256];
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  const long tt = (long)T * T;
  for (long idx = threadIdx.x; idx < tt; idx += 256) {
    const int i = (int)(idx / T), j = (int)(idx % T);
    const double t = alpha[i] * alpha[j] - Kinv[idx];
    const double u = x[i] / ell - x[j] / ell, d2 = u * u;
    const double cr = c * exp(-0.5 * d2);
    s0 = fma(t, cr, s0);
    s1 = fma(t, cr * d2, s1);
    if (i == j) s2 += t;
  }
  red[0][threadIdx.x] = s0;
  red[1][threadIdx.x] = s1;
  red[2][threadIdx.x] = s2;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o)
      for (int k = 0; k < 3; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[0] = 0.5 * red[0][0];
    out[1] = 0.5 * red[1][0];
    out[2] = 0.5 * noise * red[2][0];
  }
}

}  // namespace

extern "C" {

int hgp_abi_version(void) { return HGP_ABI_VERSION; }

int hgp_debug_mfma_f64(const double* A, const double* B, double* C, void* stream) {
  if (!A || !B || !C) return -1;
  hipLaunchKernelGGL(k_mfma_probe, dim3(1), dim3(64), 0, (hipStream_t)stream, A, B, C);
  return launch_status();
}

int hgp_debug_exp_neg_f64(const double* h, int n, double* out, void* stream) {
  if (!h || !out || n < 0) return -1;
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_exp_probe, dim3((unsigned)((n + 1023) / 1024)), dim3(256), 0, (hipStream_t)stream, h, n, out);
  return launch_status();
}

int hgp_gram_rbf_f64(const double* x, int nx, const double* y, int ny, double c, double ell, double noise,
                     double* K_out, void* stream) {
  if (!x || !K_out || nx <= 0 || ell <= 0.0) return -1;
  const int one = (y == nullptr);
  if (one) ny = nx;
  if (ny <= 0) return -1;
  size_t tot = (size_t)nx * ny;
  hipLaunchKernelGGL(k_gram_rbf, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, nx, y, ny, c,
                     ell, noise, one, K_out);
  return launch_status();
}

int hgp_warp_cov_f64(const double* x, int T, double rho, double omega, double diag_add, int normalize, double* K_out,
                     void* stream) {
  if (!x || !K_out || T <= 0 || !(rho > 0.0)) return -1;
  const size_t tot = (size_t)T * T;
  hipLaunchKernelGGL(k_warp_cov, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, T, rho, omega,
                     diag_add, normalize, K_out);
  return launch_status();
}

int hgp_trsv_lower_quad_f64(const double* G, int ld, const double* y, int T, double* out, void* stream) {
  if (!G || !y || !out || T <= 0 || ld < T) return -1;
  if (T > 2048) return -2;
  hipLaunchKernelGGL(k_trsv_lower_quad, dim3(1), dim3(256), sizeof(double) * T, (hipStream_t)stream, G, ld, y, T, out,
                     (double*)nullptr);
  return launch_status();
}

int hgp_trsv_lower_solve_f64(const double* G, int ld, const double* y, int T, double* alpha, double* quad, void* stream) {
  if (!G || !y || !alpha || T <= 0 || ld < T) return -1;
  if (T > 2048) return -2;
  hipLaunchKernelGGL(k_trsv_lower_quad, dim3(1), dim3(256), sizeof(double) * T, (hipStream_t)stream, G, ld, y, T, quad, alpha);
  return launch_status();
}

int hgp_lml_grad_f64(const double* x, const double* alpha, const double* Kinv, int T, double c, double ell, double noise,
                     double* out3, void* stream) {
  if (!x || !alpha || !Kinv || !out3 || T <= 0 || !(ell > 0.0)) return -1;
  hipLaunchKernelGGL(k_lml_grad, dim3(1), dim3(256), 0, (hipStream_t)stream, x, alpha, Kinv, T, c, ell, noise, out3);
  return launch_status();
}

}  // extern "C"
