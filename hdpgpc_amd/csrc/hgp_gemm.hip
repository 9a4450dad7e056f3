// Batched tile GEMM: C[b] = alpha op(A[b]) op(B[b]) + beta C[b], any M x N x Kd, one wave per 16x16 tile of C, operands straight
// from global memory (L2).  Used for per-cluster operators and for the matrix-valued likelihood terms (a8, a9),
// never per (segment, cluster) pair (GemmArgs: hgp_internal.hpp).  With it, the three small batched reductions of the a9 composition.
#include <algorithm>

#include "hgp_internal.hpp"
#include "tile_f64.hpp"

using namespace hgp;

namespace {

// TRIP = k-steps whose operand loads are issued before the first MFMA of a trip.  TRIP = 24 covers Kd <= 96 in ONE
// trip (the LDS recursion's 90 x 90 products: one load latency instead of three per tile).
template <int TRIP>
__global__ __launch_bounds__(64 * WAVES) void k_gemm(GemmArgs a) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int g = lane >> 4, c = lane & 15;
  const int ntn = (a.N + 15) / 16, ntm = (a.M + 15) / 16;
  const int tile = blockIdx.x * WAVES + wave;
  if (tile >= ntm * ntn) return;
  const int ti = tile / ntn, tj = tile % ntn;
  const int by = (int)blockIdx.y + a.boff;
  const int b1 = by / a.nb2, b2 = by % a.nb2;
  const double* A = a.A + (size_t)b1 * a.sA + (size_t)b2 * a.sA2;
  const double* B = a.B + (size_t)b1 * a.sB + (size_t)b2 * a.sB2;
  double* C = a.C + (size_t)b1 * a.sC + (size_t)b2 * a.sC2;
  d4 acc = (d4){0.0, 0.0, 0.0, 0.0};
  const int row = 16 * ti + c, col = 16 * tj + c;
  int nk = (a.Kd + 3) / 4;
  if (a.triA && !a.tA) nk = min(nk, 4 * (ti + 1));
  for (int k0 = 0; k0 < nk; k0 += TRIP) {   // TRIP k-steps per trip: their 2 TRIP operand loads are issued before the first MFMA
    double av[TRIP], bv[TRIP];
#pragma unroll
    for (int u = 0; u < TRIP; ++u) {
      const int k = 4 * (k0 + u) + g;
      av[u] = 0.0;
      bv[u] = 0.0;
      if (k < a.Kd) {
        if (row < a.M) av[u] = a.tA ? A[(size_t)k * a.lda + row] : A[(size_t)row * a.lda + k];
        if (col < a.N) bv[u] = a.tB ? B[(size_t)col * a.ldb + k] : B[(size_t)k * a.ldb + col];
      }
    }
#pragma unroll
    for (int u = 0; u < TRIP; ++u) acc = mfma(av[u], bv[u], acc);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = 16 * ti + g + 4 * r;
    if (i < a.M && col < a.N) {
      double v = a.alpha * acc[r];
      if (a.beta != 0.0)
        v += a.beta * (a.D ? a.D[(size_t)b1 * a.sD + (size_t)i * a.ldd + col] : C[(size_t)i * a.ldc + col]);
      C[(size_t)i * a.ldc + col] = v;
    }
  }
}

// Large products (M, N, Kd multiples of 32, Kd > 128, no transposes: the a9 composition at 128 < T <= 256): one wave per
// 32 x 32 block of C - four accumulator tiles fed by two A and two B fragments per k-step, i.e. half the L2 operand traffic per
// MFMA of k_gemm (which is bound by exactly that traffic at these sizes: 14 TFLOP/s on the 2 T^3 product at T = 256).
__global__ __launch_bounds__(64 * WAVES) void k_gemm22(GemmArgs a) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int g = lane >> 4, c = lane & 15;
  const int ntn = a.N / 32, ntm = a.M / 32;
  const int tile = blockIdx.x * WAVES + wave;
  if (tile >= ntm * ntn) return;
  const int ti = tile / ntn, tj = tile % ntn;
  const int by = (int)blockIdx.y + a.boff;
  const int b1 = by / a.nb2, b2 = by % a.nb2;
  const double* A = a.A + (size_t)b1 * a.sA + (size_t)b2 * a.sA2 + (size_t)(32 * ti + c) * a.lda + g;
  const double* B = a.B + (size_t)b1 * a.sB + (size_t)b2 * a.sB2 + (size_t)g * a.ldb + 32 * tj + c;
  double* C = a.C + (size_t)b1 * a.sC + (size_t)b2 * a.sC2;
  d4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = (d4){0.0, 0.0, 0.0, 0.0};
  int nk = a.Kd / 4;
  if (a.triA) nk = min(nk, 8 * (ti + 1));   // lower-triangular A: rows 32 ti .. 32 ti + 31 only reach k < 32 (ti + 1)
  constexpr int TR = 8;                      // k-steps per trip (Kd is a multiple of 32 here)
  for (int k0 = 0; k0 < nk; k0 += TR) {
    double av[TR][2], bv[TR][2];
#pragma unroll
    for (int u = 0; u < TR; ++u) {
      const size_t k = 4 * (size_t)(k0 + u);
      av[u][0] = A[k];
      av[u][1] = A[k + 16 * (size_t)a.lda];
      bv[u][0] = B[k * a.ldb];
      bv[u][1] = B[k * a.ldb + 16];
    }
#pragma unroll
    for (int u = 0; u < TR; ++u) {
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = mfma(av[u][i], bv[u][j], acc[i][j]);
    }
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 32 * ti + 16 * i + g + 4 * r, col = 32 * tj + 16 * j + c;
        double v = a.alpha * acc[i][j][r];
        if (a.beta != 0.0) v += a.beta * (a.D ? a.D[(size_t)b1 * a.sD + (size_t)row * a.ldd + col] : C[(size_t)row * a.ldc + col]);
        C[(size_t)row * a.ldc + col] = v;
      }
}

// out[b] = scale * sum_i X[b][i] * Y[b][i]  (+ out[b] if accumulate)
__global__ __launch_bounds__(256) void k_dot_batched(const double* __restrict__ X, const double* __restrict__ Y, long sX,
                                                      long sY, long n, double scale, int accumulate, double* out) {
  __shared__ double red[256];
  const double* x = X + (size_t)blockIdx.x * sX;
  const double* y = Y + (size_t)blockIdx.x * sY;
  double s = 0.0;
  for (long i = threadIdx.x; i < n; i += 256) s = fma(x[i], y[i], s);
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[blockIdx.x] = (accumulate ? out[blockIdx.x] : 0.0) + scale * red[0];
}

// out[b] (+)= scale * sum_ij Z[b][i][j]^2 S[j][j]: trace(Sigma^-1 S) for a DIAGONAL prior scale S from Z = L^-1 alone
__global__ __launch_bounds__(256) void k_colnorm_diag(const double* __restrict__ Z, const double* __restrict__ S, long sS, int T,
                                                       double scale, int accumulate, double* out) {
  __shared__ double red[256];
  const double* z = Z + (size_t)blockIdx.x * T * T;
  const double* sd = S + (size_t)blockIdx.x * sS;
  double s = 0.0;
  for (long i = threadIdx.x; i < (long)T * T; i += 256) {
    const int r = (int)(i / T), cidx = (int)(i % T);
    if (cidx <= r) {
      const double v = z[i];
      s = fma(v * v, sd[(size_t)cidx * T + cidx], s);
    }
  }
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[blockIdx.x] = (accumulate ? out[blockIdx.x] : 0.0) + scale * red[0];
}

// C[b] = A[b] - B[b]  (elementwise, n per item)
__global__ void k_sub_batched(const double* __restrict__ A, const double* __restrict__ B, long sA, long sB, long n,
                              double* __restrict__ C, int b) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)n) return;
  for (int m = blockIdx.y; m < b; m += gridDim.y) C[(size_t)m * n + i] = A[(size_t)m * sA + i] - B[(size_t)m * sB + i];
}

}  // namespace

int hgp_internal_gemm(const GemmArgs& a0, int batch, hipStream_t st) {
  const int nt = ((a0.M + 15) / 16) * ((a0.N + 15) / 16);
  for (int b0 = 0; b0 < batch; b0 += 65535) {   // gridDim.y <= 65535
    GemmArgs a = a0;
    a.boff = b0;
    const int nb = std::min(65535, batch - b0);
    // (only for launches that fill the chip: a single 256^3 product is 64 waves here against 256 in k_gemm - latency-bound,
    // 25.8 vs ~12 us in the member step of the online path at T = 256)
    if (!a.tA && !a.tB && a.M % 32 == 0 && a.N % 32 == 0 && a.Kd % 32 == 0 && a.Kd > 128 &&
        (long)(a.M / 32) * (a.N / 32) * nb >= 2048) {
      const int nt2 = (a.M / 32) * (a.N / 32);
      hipLaunchKernelGGL(k_gemm22, dim3((nt2 + WAVES - 1) / WAVES, nb), dim3(64 * WAVES), 0, st, a);
      continue;
    }
    if (a.Kd <= 96 && a.Kd > 32)
      hipLaunchKernelGGL(k_gemm<24>, dim3((nt + WAVES - 1) / WAVES, nb), dim3(64 * WAVES), 0, st, a);
    else if (a.Kd <= 128 && a.Kd > 96)
      hipLaunchKernelGGL(k_gemm<32>, dim3((nt + WAVES - 1) / WAVES, nb), dim3(64 * WAVES), 0, st, a);
    else
      hipLaunchKernelGGL(k_gemm<8>, dim3((nt + WAVES - 1) / WAVES, nb), dim3(64 * WAVES), 0, st, a);
  }
  return launch_status();
}

void hgp_internal_dot_batched(const double* X, const double* Y, long sX, long sY, long n, double scale, int accumulate, double* out, int b, hipStream_t st) {
  hipLaunchKernelGGL(k_dot_batched, dim3(b), dim3(256), 0, st, X, Y, sX, sY, n, scale, accumulate, out);
}

void hgp_internal_colnorm_diag(const double* Z, const double* S, long sS, int T, double scale, int accumulate, double* out, int b, hipStream_t st) {
  hipLaunchKernelGGL(k_colnorm_diag, dim3(b), dim3(256), 0, st, Z, S, sS, T, scale, accumulate, out);
}

void hgp_internal_sub_batched(const double* A, const double* B, long sA, long sB, long n, double* C, int b, hipStream_t st) {
  hipLaunchKernelGGL(k_sub_batched, dim3((unsigned)((n + 255) / 256), std::min(b, 65535)), dim3(256), 0, st, A, B, sA, sB, n, C, b);
}

extern "C" {

int hgp_gemm_batched_f64(int transA, int transB, int M, int N, int Kd, double alpha, const double* A, int lda, long strideA,
                         const double* B, int ldb, long strideB, double beta, double* C, int ldc, long strideC, int batch,
                         void* stream) {
  if (!A || !B || !C || M <= 0 || N <= 0 || Kd <= 0 || batch < 0) return -1;
  if (batch == 0) return 0;
  GemmArgs g{A, B, C, M, N, Kd, lda, ldb, ldc, strideA, strideB, strideC, alpha, beta, transA, transB};
  return hgp_internal_gemm(g, batch, (hipStream_t)stream);
}

int hgp_gemm_add_batched_f64(int transA, int transB, int M, int N, int Kd, double alpha, const double* A, int lda, long strideA,
                             const double* B, int ldb, long strideB, double beta, const double* D, int ldd, long strideD,
                             double* C, int ldc, long strideC, int batch, void* stream) {
  if (!A || !B || !C || !D || M <= 0 || N <= 0 || Kd <= 0 || batch < 0) return -1;
  if (batch == 0) return 0;
  GemmArgs g{A, B, C, M, N, Kd, lda, ldb, ldc, strideA, strideB, strideC, alpha, beta, transA, transB};
  g.D = D;
  g.ldd = ldd;
  g.sD = strideD;
  return hgp_internal_gemm(g, batch, (hipStream_t)stream);
}

}  // extern "C"
