// Projection of segments of different lengths onto the basis grid (include/hdpgpc_hip_project.h):
//     yp[n] = K(xb, x_n) (K(x_n, x_n) + jitter I)^-1 y_n        IterativeGaussianProcess.project_y, GPI.py:194-238, C = I
// for N segments, each on its own grid of L_n <= ld points, D leads as D right-hand sides, in one call.
//
// ld <= 128: ONE wavefront per (segment, 16 leads).  The wave builds K~ = K(x, x) + jitter I in registers (accumulator layout,
// rows and columns beyond L_n padded with the identity), factors it with the leads riding as one block column of right-hand
// sides (wave_factor<NB, 1>: Z = L^-1 y), keeps the factor (U tiles in registers, W_K in LDS) and walks over the basis grid in
// tiles of 16 points: the cross-Gram tile column K(x, xb_J) is built on the fly, taken through the same forward substitution
// (wave_fwd_solve: V_J = L^-1 K(x, xb_J)) and multiplied, yp_J = V_J^T Z - a product X^T Y of two accumulator tiles, which is
// what the layout gives for free.  That is K* ^T L^-T L^-1 y: two triangular solves against the factor itself (no explicit inverse,
// whose product form loses two digits at the drivers' length-scale 3), arranged so that neither needs a transposed tile.  The
// [T, L] cross-Gram never exists in memory: HBM sees x, y and yp.
//
// 128 < ld <= 256: composed from the cooperative factor (hgp_factor.hip) and k_trtri (hgp_inverse.hip) - k_project_build writes K~ (identity for rows that
// need no factor), hgp_internal_chol_inverse leaves L and Z = L^-1 in the workspace, k_project_apply (one workgroup per (segment,
// 16 leads)) forms alpha = Z^T Z y with one step of refinement against K~ rebuilt on the fly, alpha += Z^T Z (y - K~ alpha)
// (IterativeGaussianProcess._spd_solve), and yp = K(xb, x) alpha.  Two launches plus the factor's two, one C call.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "hgp_internal.hpp"
#include "tile_f64.hpp"
#include "../../include/hdpgpc_hip_project.h"

using namespace hgp;

namespace {

struct ProjectArgs {
  const double* x;          // [N,ld]
  const double* y;          // [N,ld,D]
  const int32_t* lengths;   // [N] or NULL
  int N, ld, D;
  const double* xb;         // [T]
  int T;
  double c, ell, jitter;
  double* yp;               // [N,T,D]
  int32_t* info;            // [N]
  double* Kt;               // ld > 128: [N,ld,ld] K~, then L
  double* Z;                // ld > 128: [N,ld,ld] L^-1
};

__device__ __forceinline__ bool same_bits(double a, double b) { return __double_as_longlong(a) == __double_as_longlong(b); }

// c exp(-0.5 u^2) for four arguments with the kernels' own exponential; a NaN argument stays NaN (exp_neg4 clamps its input
// with fmin, which drops it)
__device__ __forceinline__ void rbf4(const double (&u)[4], double cs, double (&o)[4]) {
  double h[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) h[r] = 0.5 * (u[r] * u[r]);
  exp_neg4(h, o);
#pragma unroll
  for (int r = 0; r < 4; ++r) o[r] = (h[r] == h[r]) ? cs * o[r] : h[r];
}

// the wave's 16 leads of row n: yp[n, :, d0 .. d0 + 15] = y[n, :, same] (src != NULL, an on-basis row: T points) or NaN
__device__ __forceinline__ void fill_cols(const ProjectArgs& a, int n, int d0, const double* src, int lane) {
  const int cc = lane & 15, d = d0 + cc;
  if (d >= a.D) return;
  for (int t = lane >> 4; t < a.T; t += 4)
    a.yp[((size_t)n * a.T + t) * a.D + d] = src ? src[(size_t)t * a.D + d] : __builtin_nan("");
}

// -------------------------------------------------------------------------------------------- ld <= 128: one wave per (n, 16 leads)
// Dynamic LDS of k_project_wave<NB>, per wave: the 16x18 staging tile of diag16_acc, the inverses W_K of the diagonal factors
// ([NB][4][64], written by wave_factor, read by wave_fwd_solve) and the segment's grid divided by the length-scale.
template <int NB>
struct ProjectLds {
  static constexpr int SCR = 0, W = SCR + DIAG_SCR, XS = W + NB * 4 * 64, PER_WAVE = XS + 16 * NB;   // doubles
  static constexpr size_t BYTES = sizeof(double) * PER_WAVE * WAVES;
  static_assert(W % 2 == 0 && XS % 2 == 0 && PER_WAVE % 2 == 0 && BYTES <= LDS_MAX_BYTES, "k_project_wave: LDS");
  __device__ static __forceinline__ double* wave_base(double* base, int wave) { return base + wave * PER_WAVE; }
  HGP_LDS_DOUBLES(scr, SCR)   // [DIAG_SCR]
  HGP_LDS_DOUBLES(w, W)       // [NB][4][64]
  HGP_LDS_DOUBLES(xs, XS)     // [16 NB]
};

template <int NB>
__global__ __launch_bounds__(64 * WAVES) void k_project_wave(ProjectArgs a) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  using Lds = ProjectLds<NB>;
  const int wave = threadIdx.x >> 6, lane_in = threadIdx.x & 63;
  const int nch = (a.D + 15) >> 4;
  const long long w = (long long)blockIdx.x * WAVES + wave;
  if (w >= (long long)a.N * nch) return;
  const int n = (int)(w / nch), d0 = 16 * (int)(w % nch);
  double* mine = Lds::wave_base(smem, wave);
  double *scr = Lds::scr(mine), *Wl = Lds::w(mine), *xs = Lds::xs(mine);
  const int L = a.lengths ? a.lengths[n] : a.ld;
  if (L < 1 || L > a.ld) {   // nothing of the row is read
    fill_cols(a, n, d0, nullptr, lane_in);
    if (d0 == 0 && lane_in == 0) a.info[n] = -1;
    return;
  }
  const double* xr = a.x + (size_t)n * a.ld;
  const double* yr = a.y + (size_t)n * a.ld * a.D;
  if (L == a.T) {   // the reference's torch.equal short-circuit: the row is on the basis
    bool eq = true;
    for (int i = lane_in; i < L; i += 64) eq = eq && same_bits(xr[i], a.xb[i]);
    if (__all(eq)) {
      fill_cols(a, n, d0, yr, lane_in);
      if (d0 == 0 && lane_in == 0) a.info[n] = 0;
      return;
    }
  }
  const double rl = a.ell;
  for (int i = lane_in; i < 16 * NB; i += 64) xs[i] = (i < L) ? xr[i] / rl : 0.0;
  __builtin_amdgcn_wave_barrier();
  d4 U[NB * (NB + 1) / 2];
  d4 R[NB];
#pragma unroll
  for (int I = 0; I < NB; ++I) {
#pragma unroll
    for (int J = I; J < NB; ++J) {
      const int lane = launder(lane_in);
      const int g = lane >> 4, c = lane & 15;
      const double xj = xs[16 * J + c];
      double u[4], o[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) u[r] = xs[16 * I + g + 4 * r] - xj;
      rbf4(u, a.c, o);
      d4 v;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = 16 * I + g + 4 * r, j = 16 * J + c;
        v[r] = (i < L && j < L) ? ((i == j) ? o[r] + a.jitter : o[r]) : ((i == j) ? 1.0 : 0.0);
      }
      // a finished tile goes to the accumulation registers at once, and the next tile's exponentials start behind it: left to
      // the allocator the tiles pile up in VGPRs and 83 of them spill at NB = 8 (336 bytes of scratch per lane; 36 with this)
      asm volatile("" : "+a"(v));
      U[tix(I, J, NB)] = v;
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  {
    const int lane = launder(lane_in);
    const int g = lane >> 4, d = d0 + (lane & 15);
#pragma unroll
    for (int K = 0; K < NB; ++K)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = 16 * K + g + 4 * r;
        R[K][r] = (i < L && d < a.D) ? yr[(size_t)i * a.D + d] : 0.0;
      }
  }
  PivotAcc pa;
  pa.init();
  wave_factor<NB, 1>(U, R, scr, Wl, nullptr, lane_in, pa, nullptr, 0, L);   // R = Z = L^-1 y
  __builtin_amdgcn_wave_barrier();
  const bool bad = pa.info != 0;
  const int ntj = (a.T + 15) >> 4;
#pragma unroll 1
  for (int Jt = 0; Jt < ntj; ++Jt) {
    const int lane = launder(lane_in);
    const int g = lane >> 4, c = lane & 15;
    const int j = 16 * Jt + c;
    const double xj = (j < a.T) ? a.xb[j] / rl : 0.0;
    d4 V[NB];
#pragma unroll
    for (int K = 0; K < NB; ++K) {
      double u[4], o[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) u[r] = xs[16 * K + g + 4 * r] - xj;
      rbf4(u, a.c, o);
#pragma unroll
      for (int r = 0; r < 4; ++r) V[K][r] = (16 * K + g + 4 * r < L && j < a.T) ? o[r] : 0.0;
    }
    wave_fwd_solve<NB>(U, Wl, V, lane);   // V = L^-1 K(x, xb_J)
    d4 acc = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int K = 0; K < NB; ++K)
#pragma unroll
      for (int s = 0; s < 4; ++s) acc = mfma(V[K][s], R[K][s], acc);   // V^T Z: [16 basis points, 16 leads]
    const int d = d0 + c;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int t = 16 * Jt + g + 4 * r;
      if (t < a.T && d < a.D) a.yp[((size_t)n * a.T + t) * a.D + d] = bad ? __builtin_nan("") : acc[r];
    }
  }
  if (d0 == 0 && lane_in == 0) a.info[n] = pa.info;
}

template <int NB>
int launch_project_wave(const ProjectArgs& a, hipStream_t st) {
  using Lds = ProjectLds<NB>;
  const long long waves = (long long)a.N * ((a.D + 15) >> 4);
  const long long blocks = (waves + WAVES - 1) / WAVES;
  if (blocks > INT_MAX) return -2;
  if (int rc_ = hgp_internal_ensure_dynamic_lds(reinterpret_cast<const void*>(&k_project_wave<NB>), Lds::BYTES)) return rc_;
  hipLaunchKernelGGL(k_project_wave<NB>, dim3((unsigned)blocks), dim3(64 * WAVES), Lds::BYTES, st, a);
  return launch_status();
}

// -------------------------------------------------------------------------------------------- 128 < ld <= 256: composed
constexpr int PROJ_THREADS = 64 * WAVES;

// 0 = factor it, 1 = on the basis (copy), -1 = length out of range; decided by the whole workgroup (uniform)
__device__ __forceinline__ int row_kind(const ProjectArgs& a, int n, int L) {
  if (L < 1 || L > a.ld) return -1;
  if (L != a.T) return 0;
  const double* xr = a.x + (size_t)n * a.ld;
  bool eq = true;
  for (int i = threadIdx.x; i < L; i += PROJ_THREADS) eq = eq && same_bits(xr[i], a.xb[i]);
  return __syncthreads_and(eq) ? 1 : 0;
}

// K~[n] [ld,ld] = K(x_n, x_n) + jitter I, identity beyond L_n - and the identity for a row that is copied or refused
__global__ __launch_bounds__(PROJ_THREADS) void k_project_build(ProjectArgs a) {
  __shared__ double xs[HGP_MAX_T_COOP];
  const int n = blockIdx.x, ld = a.ld;
  const int L = a.lengths ? a.lengths[n] : ld;
  const bool live = row_kind(a, n, L) == 0;
  if (live)
    for (int i = threadIdx.x; i < L; i += PROJ_THREADS) xs[i] = a.x[(size_t)n * ld + i] / a.ell;
  __syncthreads();
  double* A = a.Kt + (size_t)n * ld * ld;
  for (int idx = threadIdx.x; idx < ld * ld; idx += PROJ_THREADS) {
    const int i = idx / ld, j = idx - i * ld;
    double v = (i == j) ? 1.0 : 0.0;
    if (live && i < L && j < L) {
      const double u = xs[i] - xs[j];
      v = a.c * exp(-0.5 * (u * u)) + ((i == j) ? a.jitter : 0.0);
    }
    A[idx] = v;
  }
}

// Dynamic LDS of k_project_apply: the grid over the length-scale and three panels of 16 right-hand sides ([HGP_MAX_T_COOP][16]).
struct ProjectApplyLds {
  static constexpr int PANEL = HGP_MAX_T_COOP * 16;
  static constexpr int XS = 0, YB = XS + HGP_MAX_T_COOP, AB = YB + PANEL, TB = AB + PANEL, END = TB + PANEL;   // doubles
  static constexpr size_t BYTES = sizeof(double) * END;
  static_assert(BYTES <= LDS_MAX_BYTES, "k_project_apply: LDS");
  HGP_LDS_DOUBLES(xs, XS)
  HGP_LDS_DOUBLES(yb, YB)
  HGP_LDS_DOUBLES(ab, AB)
  HGP_LDS_DOUBLES(tb, TB)
};

// out(i, cc, value) for the [rows, 16] product M in, M(row, k) given entry by entry (read from memory or built), in [kdim][16]
// in LDS; row tiles dealt over the waves, one MFMA chain per tile in ascending k.  The caller places the barrier.
template <class MF, class OutF>
__device__ __forceinline__ void skinny_prod(int rows, int kdim, MF&& M, const double* in, OutF&& out) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, c = lane & 15;
  const int nt = (rows + 15) >> 4;
  for (int ti = wave; ti < nt; ti += WAVES) {
    const int row = 16 * ti + c;
    d4 acc = (d4){0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < kdim; k0 += 4) {
      const int k = k0 + g;
      const bool on = k < kdim;
      const double av = (on && row < rows) ? M(row, k) : 0.0;
      const double bv = on ? in[k * 16 + c] : 0.0;
      acc = mfma(av, bv, acc);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = 16 * ti + g + 4 * r;
      if (i < rows) out(i, c, acc[r]);
    }
  }
}

__global__ __launch_bounds__(PROJ_THREADS) void k_project_apply(ProjectArgs a) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  using Lds = ProjectApplyLds;
  double *xs = Lds::xs(smem), *yb = Lds::yb(smem), *ab = Lds::ab(smem), *tb = Lds::tb(smem);
  const int n = blockIdx.x, d0 = 16 * blockIdx.y, ld = a.ld, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int L = a.lengths ? a.lengths[n] : ld;
  const int kind = row_kind(a, n, L);
  const double* yr = a.y + (size_t)n * ld * a.D;
  if (kind != 0 || a.info[n] != 0) {   // uniform over the workgroup: copied, refused, or not positive definite (info stands)
    for (int t0 = 4 * wave; t0 < a.T; t0 += 4 * WAVES) {
      const int cc = lane & 15, d = d0 + cc, t = t0 + (lane >> 4);
      if (t < a.T && d < a.D) a.yp[((size_t)n * a.T + t) * a.D + d] = (kind == 1) ? yr[(size_t)t * a.D + d] : __builtin_nan("");
    }
    if (kind == -1 && d0 == 0 && threadIdx.x == 0) a.info[n] = -1;
    return;
  }
  for (int i = threadIdx.x; i < L; i += PROJ_THREADS) xs[i] = a.x[(size_t)n * ld + i] / a.ell;
  for (int idx = threadIdx.x; idx < L * 16; idx += PROJ_THREADS) {
    const int i = idx >> 4, d = d0 + (idx & 15);
    yb[idx] = (d < a.D) ? yr[(size_t)i * a.D + d] : 0.0;
  }
  __syncthreads();
  const double* Z = a.Z + (size_t)n * ld * ld;   // lower triangular; only its leading L x L block is touched
  auto Zn = [&](int row, int k) { return (k <= row) ? Z[(size_t)row * ld + k] : 0.0; };
  auto Zt = [&](int row, int k) { return (k >= row) ? Z[(size_t)k * ld + row] : 0.0; };
  const double cs = a.c, jit = a.jitter;
  auto Kt = [&](int row, int k) {
    const double u = xs[row] - xs[k];
    return cs * exp(-0.5 * (u * u)) + ((row == k) ? jit : 0.0);
  };
  skinny_prod(L, L, Zn, yb, [&](int i, int cc, double v) { tb[i * 16 + cc] = v; });             // t = Z y
  __syncthreads();
  skinny_prod(L, L, Zt, tb, [&](int i, int cc, double v) { ab[i * 16 + cc] = v; });             // alpha = Z^T t
  __syncthreads();
  skinny_prod(L, L, Kt, ab, [&](int i, int cc, double v) { tb[i * 16 + cc] = yb[i * 16 + cc] - v; });   // r = y - K~ alpha
  __syncthreads();
  skinny_prod(L, L, Zn, tb, [&](int i, int cc, double v) { yb[i * 16 + cc] = v; });             // t = Z r
  __syncthreads();
  skinny_prod(L, L, Zt, yb, [&](int i, int cc, double v) { ab[i * 16 + cc] += v; });            // alpha += Z^T t
  __syncthreads();
  const double* xb = a.xb;
  const double rl = a.ell;
  auto Ks = [&](int row, int k) {
    const double u = xb[row] / rl - xs[k];
    return cs * exp(-0.5 * (u * u));
  };
  double* out = a.yp + (size_t)n * a.T * a.D;
  const int D = a.D;
  skinny_prod(a.T, L, Ks, ab, [&](int t, int cc, double v) {                                    // yp = K(xb, x) alpha
    if (d0 + cc < D) out[(size_t)t * D + d0 + cc] = v;
  });
}

}  // namespace

extern "C" {

size_t hgp_project_ragged_ws_bytes(int N, int ld, int T, int D) {
  (void)T;
  (void)D;
  if (N <= 0 || ld <= HGP_MAX_T_WAVE) return 0;
  return sizeof(double) * 2 * (size_t)N * (size_t)ld * (size_t)ld;
}

int hgp_project_ragged_f64(const double* x, const double* y, const int32_t* lengths, int N, int ld, int D, const double* xb, int T,
                           double c, double ell, double jitter, double* yp, int32_t* info, void* ws, size_t ws_bytes, void* stream) {
  if (N < 0) return -1;
  if (N == 0) return 0;
  if (!x || !y || !xb || !yp || !info || ld < 1 || D < 1 || T < 1 || !(c > 0.0) || !(ell > 0.0) || !(jitter >= 0.0)) return -1;
  if (ld > HGP_MAX_T_COOP || T > HGP_MAX_T_COOP) return -2;
  const size_t need = hgp_project_ragged_ws_bytes(N, ld, T, D);
  if (need && (!ws || ws_bytes < need)) return -2;
  const int nch = (D + 15) >> 4;
  if (nch > 65535) return -2;
  hipStream_t st = (hipStream_t)stream;
  ProjectArgs a{x, y, lengths, N, ld, D, xb, T, c, ell, jitter, yp, info, nullptr, nullptr};
  if (ld <= HGP_MAX_T_WAVE) return dispatch_nb_wave(ld, [&](auto nb) { return launch_project_wave<decltype(nb)::value>(a, st); });
  a.Kt = static_cast<double*>(ws);
  a.Z = a.Kt + (size_t)N * ld * ld;
  hipLaunchKernelGGL(k_project_build, dim3(N), dim3(PROJ_THREADS), 0, st, a);
  if (int rc_ = launch_status()) return rc_;
  InvArgs pf{a.Kt, ld, N, 0.0, 0.0, a.Z, info};
  if (int rc_ = hgp_internal_chol_inverse(pf, (ld + 15) >> 4, a.Kt, st)) return rc_;   // K~ <- L
  if (int rc_ = hgp_internal_ensure_dynamic_lds(reinterpret_cast<const void*>(&k_project_apply), ProjectApplyLds::BYTES)) return rc_;
  hipLaunchKernelGGL(k_project_apply, dim3(N, nch), dim3(PROJ_THREADS), ProjectApplyLds::BYTES, st, a);
  return launch_status();
}

}  // extern "C"
