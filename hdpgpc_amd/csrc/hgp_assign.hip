// Assignment tail of the switching variable on the device: GPI_HDP.LogLik (GPI_HDP.py:632-661) and the
// one-hot arg-max GPI_HDP._safe_exp (GPI_HDP.py:338-350) applied to log(alpha * beta), so that the [N,K] score matrix goes
// from the pair kernels through the message kernel to the label vector without leaving the GPU.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "hgp_internal.hpp"
#include "tile_f64.hpp"

using namespace hgp;

namespace {

// LogLik(axis = 1): out[n,:] = q[n,:] - max_k q[n,k], rowmax[n] = that maximum - unless ANY row maximum is infinite, in
// which case the reference returns its input unchanged (GPI_HDP.py:646-648).  One workgroup: the any-infinite test spans all rows.
__global__ __launch_bounds__(1024) void k_loglik_rows(const double* __restrict__ q, int N, int K, double* __restrict__ out,
                                                      double* __restrict__ rowmax) {
  __shared__ int any_inf;
  q += (size_t)blockIdx.x * N * K;            // blockIdx.x = variant of a batch (the rule below is per score matrix)
  out += (size_t)blockIdx.x * N * K;
  if (rowmax) rowmax += (size_t)blockIdx.x * N;
  if (threadIdx.x == 0) any_inf = 0;
  __syncthreads();
  int bad = 0;
  for (int n = threadIdx.x; n < N; n += blockDim.x) {
    double m = q[(size_t)n * K];
    for (int k = 1; k < K; ++k) {
      const double v = q[(size_t)n * K + k];
      m = (v > m || v != v) ? ((m != m) ? m : v) : m;      // torch.max: a NaN anywhere in the row is the row's maximum
    }
    if (rowmax) rowmax[n] = m;
    bad |= isinf(m) ? 1 : 0;
  }
  if (bad) atomicOr(&any_inf, 1);
  __syncthreads();
  const bool keep = any_inf != 0;
  for (int n = threadIdx.x; n < N; n += blockDim.x) {
    double m = 0.0;
    if (!keep) {
      m = q[(size_t)n * K];
      for (int k = 1; k < K; ++k) {
        const double v = q[(size_t)n * K + k];
        m = (v > m || v != v) ? ((m != m) ? m : v) : m;
      }
    }
    for (int k = 0; k < K; ++k) out[(size_t)n * K + k] = q[(size_t)n * K + k] - m;
  }
}

// labels[n] = first arg-max over k of log(fmsg[n,k] * bmsg[n,k]); resp (optional) = its one-hot row.  torch.argmax treats NaN
// as the maximum (first NaN wins): a failed factorisation upstream lands on the NaN column here as it does in the reference.
__global__ __launch_bounds__(256) void k_assign(const double* __restrict__ fmsg, const double* __restrict__ bmsg, int N, int K,
                                                int64_t* __restrict__ labels, double* __restrict__ resp) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  int best = 0;
  double bv = log(fmsg[(size_t)n * K] * bmsg[(size_t)n * K]);
  for (int k = 1; k < K; ++k) {
    const double v = log(fmsg[(size_t)n * K + k] * bmsg[(size_t)n * K + k]);
    if ((v > bv || v != v) && bv == bv) {      // a NaN already held is never replaced; the first NaN replaces any number
      bv = v;
      best = k;
    }
  }
  if (labels) labels[n] = best;
  if (resp)
    for (int k = 0; k < K; ++k) resp[(size_t)n * K + k] = (k == best) ? 1.0 : 0.0;
}

// last_log[v, k] = log(fmsg[v, N-1, k] * bmsg[v, N-1, k]) (what variational_local_terms hands back for the newest segment)
__global__ __launch_bounds__(64) void k_last_log(const double* __restrict__ fmsg, const double* __restrict__ bmsg, int N, int K,
                                                 double* __restrict__ out) {
  const size_t o = ((size_t)blockIdx.x * N + (N - 1)) * K;
  for (int k = threadIdx.x; k < K; k += 64) out[(size_t)blockIdx.x * K + k] = log(fmsg[o + k] * bmsg[o + k]);
}

// ------------------------------------------------------------------ messages of the switching variable
// GPI_HDP.forward / backward / coupled_state_coef (GPI_HDP.py:3546-3700) on the device, so that the [N, K] score matrix
// never leaves HBM between evaluation and assignment.  Sequential in N, K <= 64 states: one wave per direction, lane i
// = state i, its row of the (clamped, max-shifted) transition matrix in LDS, the message vector broadcast through LDS.
__device__ __forceinline__ double hmm_exp(double x, double m) {   // the reference's safe_exp element: NaN -> 1e-8
  const double e = exp(x - m);
  return (e != e) ? 1e-8 : e;
}
// one step of the row maximum safe_exp subtracts.  torch.max: a NaN anywhere in the row IS the row's maximum (the expression of
// k_loglik_rows), so that every entry of such a row becomes 1e-8 as in the reference - fmax would drop the NaN.
__device__ __forceinline__ double hmm_max(double m, double v) { return (v > m || v != v) ? ((m != m) ? m : v) : m; }
// the same maximum over the lanes of the wave: the fmax reduction ignores NaN, a wave-wide "any NaN" puts it back
__device__ __forceinline__ double hmm_wave_max(double v) {
  const double m = wave_allreduce<true>(v);
  return __any(v != v) ? __builtin_nan("") : m;
}
struct HmmArgs {
  const double* q;          // [N,K] log-observations
  const double* log_pi;     // [K]
  const double* log_trans;  // [K,K]
  int N, K;
  double* fmsg;             // [N,K]
  double* marg;             // [N]
  double* bmsg;             // [N,K]
};

__global__ __launch_bounds__(64) void k_hmm_messages(HmmArgs a) {
  extern __shared__ double sm[];
  const int K = a.K, N = a.N, i = threadIdx.x, LD = K + 1;
  double* P = sm;            // [K][K+1]
  double* f = P + K * LD;    // [K]
  const bool fwd = blockIdx.x == 0;
  {                          // blockIdx.y = variant of a batch of score matrices sharing log_pi / log_trans
    const size_t vo = (size_t)blockIdx.y * N * K;
    a.q += vo;
    a.fmsg += vo;
    a.bmsg += vo;
    a.marg += (size_t)blockIdx.y * N;
  }
  const bool live = i < K;
  const double ninf = -__builtin_inf();
  // my row of the transition operator: forward uses safe_exp(log_trans^T) clamped at 1e-6, backward safe_exp(log_trans)
  // clamped at 1e-5 (GPI_HDP.py:3586-3589, 3637-3642)
  if (live) {
    double m = ninf;
    for (int j = 0; j < K; ++j) m = hmm_max(m, fwd ? a.log_trans[(size_t)j * K + i] : a.log_trans[(size_t)i * K + j]);
    for (int j = 0; j < K; ++j) {
      double e = hmm_exp(fwd ? a.log_trans[(size_t)j * K + i] : a.log_trans[(size_t)i * K + j], m);
      if (e < (fwd ? 1e-6 : 1e-5)) e += 1e-4;
      P[i * LD + j] = e;
    }
  }
  __builtin_amdgcn_wave_barrier();
  if (fwd) {
    double pi_ = live ? exp(a.log_pi[i]) : 0.0;
    if (live && pi_ < 1e-10) pi_ += 1e-4;
    for (int t0 = 0; t0 < N; t0 += 8) {   // the observations of 8 steps are requested together: one load latency per 8 steps
      double qv8[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) qv8[u] = (live && t0 + u < N) ? a.q[(size_t)(t0 + u) * K + i] : ninf;
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int t = t0 + u;
        if (t >= N) break;
        const double qv = qv8[u];
        const double qm = hmm_wave_max(qv);                             // (all 64 lanes take part in the shuffles)
        const double qe = live ? hmm_exp(qv, qm) : 0.0;
        double g = pi_;
        if (t > 0) {
          g = 0.0;
          if (live)
            for (int j = 0; j < K; ++j) g = fma(P[i * LD + j], f[j], g);
        }
        const double v = live ? g * qe : 0.0;
        const double mg = wave_allreduce<false>(v);
        const double fi = v / mg;
        __builtin_amdgcn_wave_barrier();
        if (live) {
          f[i] = fi;
          a.fmsg[(size_t)t * K + i] = fi;
        }
        if (i == 0) a.marg[t] = mg;
        __builtin_amdgcn_wave_barrier();
      }
    }
  } else {
    double b = 1.0;
    if (live) a.bmsg[(size_t)(N - 1) * K + i] = 1.0;
    for (int t0 = N - 2; t0 >= 0; t0 -= 8) {
      double qv8[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) qv8[u] = (live && t0 - u >= 0) ? a.q[(size_t)(t0 - u + 1) * K + i] : ninf;
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int t = t0 - u;
        if (t < 0) break;
        const double qv = qv8[u];
        const double qm = hmm_wave_max(qv);
        const double qe = live ? hmm_exp(qv, qm) : 0.0;
        if (live) f[i] = b * qe;
        __builtin_amdgcn_wave_barrier();
        double v = 0.0;
        if (live)
          for (int j = 0; j < K; ++j) v = fma(P[i * LD + j], f[j], v);
        const double nrm = wave_allreduce<false>((live && i < K - 1) ? v : 0.0);   // the reference leaves the last state out (:3645)
        b = v / nrm;
        if (live) a.bmsg[(size_t)t * K + i] = b;
        __builtin_amdgcn_wave_barrier();
      }
    }
  }
}

// log of the normalised pair responsibilities (coupled_state_coef): one workgroup per step t
__global__ __launch_bounds__(256) void k_hmm_pair(const double* __restrict__ q, const double* __restrict__ log_trans,
                                                  const double* __restrict__ alpha, const double* __restrict__ beta, int N,
                                                  int K, double* __restrict__ out) {
  extern __shared__ double sm[];
  double* soft = sm;          // [K]  safe_exp(q[t]) * beta[t]
  double* rmax = soft + K;    // [K]  row maxima of log_trans
  __shared__ double red[256];
  const int t = blockIdx.x, tid = threadIdx.x;
  double* o = out + (size_t)t * K * K;
  if (t == 0) {               // respPair[0] = 0 -> log 0
    for (int e = tid; e < K * K; e += 256) o[e] = -__builtin_inf();
    return;
  }
  double qm = -__builtin_inf();
  for (int j = 0; j < K; ++j) qm = hmm_max(qm, q[(size_t)t * K + j]);
  for (int j = tid; j < K; j += 256) {
    soft[j] = hmm_exp(q[(size_t)t * K + j], qm) * beta[(size_t)t * K + j];
    double m = -__builtin_inf();
    for (int l = 0; l < K; ++l) m = hmm_max(m, log_trans[(size_t)j * K + l]);
    rmax[j] = m;
  }
  __syncthreads();
  double s = 0.0;
  for (int e = tid; e < K * K; e += 256) {
    const int i = e / K, j = e % K;
    s += alpha[(size_t)(t - 1) * K + i] * soft[j] * hmm_exp(log_trans[e], rmax[i]);
  }
  red[tid] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) red[tid] += red[tid + w];
    __syncthreads();
  }
  double den = red[0];
  if (den == 0.0) den = 1e-10;
  for (int e = tid; e < K * K; e += 256) {
    const int i = e / K, j = e % K;
    o[e] = log(alpha[(size_t)(t - 1) * K + i] * soft[j] * hmm_exp(log_trans[e], rmax[i]) / den);
  }
}

// The same table reduced on the spot to what the hard assignment keeps of it: the FIRST arg-max of row t over the flattened
// K x K entries (GPI_HDP._safe_exp on the pair table; row 0 is all -inf -> 0; a row holding a NaN -> 0, as the host layer's
// first-arg-max did).  Same arithmetic, element by element, as k_hmm_pair; grid (N, variants).
__global__ __launch_bounds__(256) void k_hmm_pair_first(const double* __restrict__ q_all, const double* __restrict__ log_trans,
                                                        const double* __restrict__ alpha_all, const double* __restrict__ beta_all,
                                                        int N, int K, int64_t* __restrict__ first_all) {
  extern __shared__ double sm[];
  double* soft = sm;
  double* rmax = soft + K;
  __shared__ double red[256];
  __shared__ int redi[256];
  __shared__ int any_nan;
  const int t = blockIdx.x, tid = threadIdx.x;
  const size_t vo = (size_t)blockIdx.y * N * K;
  const double* q = q_all + vo;
  const double* alpha = alpha_all + vo;
  const double* beta = beta_all + vo;
  int64_t* first = first_all + (size_t)blockIdx.y * N;
  if (t == 0) {
    if (tid == 0) first[0] = 0;
    return;
  }
  if (tid == 0) any_nan = 0;
  double qm = -__builtin_inf();
  for (int j = 0; j < K; ++j) qm = hmm_max(qm, q[(size_t)t * K + j]);
  for (int j = tid; j < K; j += 256) {
    soft[j] = hmm_exp(q[(size_t)t * K + j], qm) * beta[(size_t)t * K + j];
    double m = -__builtin_inf();
    for (int l = 0; l < K; ++l) m = hmm_max(m, log_trans[(size_t)j * K + l]);
    rmax[j] = m;
  }
  __syncthreads();
  double s = 0.0;
  for (int e = tid; e < K * K; e += 256) {
    const int i = e / K, j = e % K;
    s += alpha[(size_t)(t - 1) * K + i] * soft[j] * hmm_exp(log_trans[e], rmax[i]);
  }
  red[tid] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) red[tid] += red[tid + w];
    __syncthreads();
  }
  double den = red[0];
  if (den == 0.0) den = 1e-10;
  __syncthreads();
  double bv = -__builtin_inf();
  int bi = K * K;                       // K * K = "nothing yet": an all -inf row keeps index 0 below
  bool nan = false;
  for (int e = tid; e < K * K; e += 256) {
    const int i = e / K, j = e % K;
    const double v = log(alpha[(size_t)(t - 1) * K + i] * soft[j] * hmm_exp(log_trans[e], rmax[i]) / den);
    nan |= (v != v);
    if (v > bv || (bi == K * K && v == bv)) {
      bv = v;
      bi = e;
    }
  }
  if (nan) atomicOr(&any_nan, 1);
  red[tid] = bv;
  redi[tid] = bi;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) {
      const double ov = red[tid + w];
      const int oi = redi[tid + w];
      if (ov > red[tid] || (ov == red[tid] && oi < redi[tid])) {
        red[tid] = ov;
        redi[tid] = oi;
      }
    }
    __syncthreads();
  }
  if (tid == 0) first[t] = (any_nan || redi[0] >= K * K) ? 0 : redi[0];
}

// batched LogLik normalisation / arg-max of the state posterior (B score matrices [N, K] back to back)
int loglik_rows_b(const double* q, int N, int K, int B, double* out, hipStream_t st) {
  hipLaunchKernelGGL(k_loglik_rows, dim3(B), dim3(1024), 0, st, q, N, K, out, (double*)nullptr);
  return launch_status();
}

int assign_b(const double* fmsg, const double* bmsg, int N, int K, int B, int64_t* labels, double* last_log, hipStream_t st) {
  const long rows = (long)N * B;
  hipLaunchKernelGGL(k_assign, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, fmsg, bmsg, (int)rows, K, labels, (double*)nullptr);
  if (last_log) hipLaunchKernelGGL(k_last_log, dim3(B), dim3(64), 0, st, fmsg, bmsg, N, K, last_log);
  return launch_status();
}

}  // namespace

extern "C" {

int hgp_loglik_rows_f64(const double* q, int N, int K, double* out, double* rowmax, void* stream) {
  if (N == 0) return 0;
  if (!q || !out || N < 0 || K <= 0) return -1;
  hipLaunchKernelGGL(k_loglik_rows, dim3(1), dim3(1024), 0, (hipStream_t)stream, q, N, K, out, rowmax);
  return launch_status();
}

int hgp_assign_f64(const double* fmsg, const double* bmsg, int N, int K, int64_t* labels, double* resp, void* stream) {
  if (N == 0) return 0;
  if (!fmsg || !bmsg || (!labels && !resp) || N < 0 || K <= 0) return -1;
  hipLaunchKernelGGL(k_assign, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream, fmsg, bmsg, N, K, labels, resp);
  return launch_status();
}

int hgp_hmm_messages_f64(const double* q, const double* log_pi, const double* log_trans, int N, int K, double* fmsg,
                         double* marg, double* bmsg, double* log_resp_pair, void* stream) {
  if (N == 0) return 0;
  if (!q || !log_pi || !log_trans || !fmsg || !marg || !bmsg || N < 0 || K <= 0) return -1;
  if (K > 64) return -2;
  HmmArgs a{q, log_pi, log_trans, N, K, fmsg, marg, bmsg};
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_hmm_messages, dim3(2), dim3(64), sizeof(double) * ((size_t)K * (K + 1) + K), st, a);
  if (log_resp_pair)
    hipLaunchKernelGGL(k_hmm_pair, dim3(N), dim3(256), sizeof(double) * 2 * K, st, q, log_trans, (const double*)fmsg,
                       (const double*)bmsg, N, K, log_resp_pair);
  return launch_status();
}

int hgp_hmm_local_terms_f64(const double* q, const double* log_pi, const double* log_trans, int N, int K, int B, double* qnorm,
                            double* fmsg, double* marg, double* bmsg, int64_t* labels, int64_t* pair_first, double* last_log,
                            void* stream) {
  if (N == 0 || B == 0) return 0;
  if (!q || !log_pi || !log_trans || !qnorm || !fmsg || !marg || !bmsg || !labels || N < 0 || K <= 0 || B < 0) return -1;
  if (K > 64) return -2;
  hipStream_t st = (hipStream_t)stream;
  if (int rc = loglik_rows_b(q, N, K, B, qnorm, st)) return rc;
  HmmArgs a{qnorm, log_pi, log_trans, N, K, fmsg, marg, bmsg};
  hipLaunchKernelGGL(k_hmm_messages, dim3(2, B), dim3(64), sizeof(double) * ((size_t)K * (K + 1) + K), st, a);
  if (int rc = assign_b(fmsg, bmsg, N, K, B, labels, last_log, st)) return rc;
  if (pair_first)
    hipLaunchKernelGGL(k_hmm_pair_first, dim3(N, B), dim3(256), sizeof(double) * 2 * K, st, (const double*)qnorm, log_trans,
                       (const double*)fmsg, (const double*)bmsg, N, K, pair_first);
  return launch_status();
}

}  // extern "C"
