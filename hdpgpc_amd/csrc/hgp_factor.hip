// The Cholesky family (a3 / a4 / a6): factor and scoring of batched SPD matrices (the inverse factor: hgp_inverse.hip).
// One wavefront owns one SPD matrix (<= 128 x 128) in MFMA accumulator registers, one workgroup a larger one (<= 256); see tile_f64.hpp.
#include <mutex>

#include "hgp_internal.hpp"
#include "tile_f64.hpp"

using namespace hgp;

namespace {

template <int NB>
__global__ __launch_bounds__(64 * WAVES) void k_wave_potrf(PotrfArgs a) {
  __shared__ __attribute__((aligned(16))) double scr_all[WAVES * DIAG_SCR];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int g = lane >> 4, c = lane & 15;
  const int m = blockIdx.x * WAVES + wave;
  if (m >= a.b) return;
  double* scr = scr_all + wave * DIAG_SCR;
  const int T = a.T;
  double* A = (a.Aout ? a.Aout : a.A) + (size_t)m * T * T;     // where L goes
  d4 U[NB * (NB + 1) / 2];
  d4 R[NB];
  load_sym_upper<NB>(U, a.A + (size_t)(a.src_idx ? a.src_idx[m] : m) * T * T, T, T, lane, scr);
  // TWO passes: add first, the mean of the diagonal so shifted, then the jitter - an entry rounds as (d + add) + jit
  if (a.add != 0.0) add_diag<NB>(U, a.add, T, lane);
  if (a.jitter_rel != 0.0) {
    double dm = diag_abs_mean<NB>(U, T, lane);
    add_diag<NB>(U, a.jitter_rel * fmax(dm, F64_EPS), T, lane);
  }
  PivotAcc pa;
  pa.init();
  wave_factor<NB, 0>(U, R, scr, nullptr, nullptr, lane, pa, A, T, T);
  // zero the strictly upper blocks of the in-place result (torch.linalg.cholesky returns zeros there)
#pragma unroll
  for (int I = 0; I < NB; ++I)
#pragma unroll
    for (int J = I + 1; J < NB; ++J) {
      const int ln = launder(lane);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int i = 16 * I + (ln >> 4) + 4 * r, j = 16 * J + (ln & 15);
        if (i < T && j < T) A[(size_t)i * T + j] = 0.0;
      }
    }
  if (lane == 0) {
    if (a.info) a.info[m] = pa.info;
    if (a.logdet) a.logdet[m] = pa.logdet();
  }
}

// -------------------------------------------------------------------------------------- a4 + a6
struct ScoreArgs {
  const double* Y;
  int ldy;
  const double* mean;
  long mean_stride;
  const double* Sigma;
  long sigma_stride;
  int T;
  int ld_sigma;               // leading dimension of every Sigma matrix (= T for the public entry point)
  const int32_t* item_mat;
  const int32_t* item_mean;   // optional: row of `mean` per item (default: item_mat)
  const double* item_add;
  const int32_t* item_off;
  const int32_t* item_cnt;
  int n_items;
  const int32_t* seg_ids;
  double jitter_rel;
  double* out_quad;
  double* out_logdet;
  int32_t* out_info;
};

template <int NB>
__global__ __launch_bounds__(64 * WAVES) void k_wave_score(ScoreArgs a) {
  __shared__ __attribute__((aligned(16))) double scr_all[WAVES * DIAG_SCR];
  __shared__ __attribute__((aligned(16))) double w_all[WAVES * NB * 256];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int g = lane >> 4, c = lane & 15;
  const int it = blockIdx.x * WAVES + wave;
  if (it >= a.n_items) return;
  double* scr = scr_all + wave * DIAG_SCR;
  const int T = a.T;
  const int mat = a.item_mat[it];
  const double* S = a.Sigma + (size_t)mat * a.sigma_stride;
  const double* mu = a.mean ? a.mean + (size_t)(a.item_mean ? a.item_mean[it] : mat) * a.mean_stride : nullptr;
  d4 U[NB * (NB + 1) / 2];
  d4 R[NB];
  double* Wl = w_all + wave * NB * 256;
  load_sym_upper<NB>(U, S, a.ld_sigma, T, lane, scr);
  const double add = a.item_add ? a.item_add[it] : 0.0;
  // TWO passes, as in k_wave_potrf: an entry rounds as (d + add) + jit
  if (add != 0.0) add_diag<NB>(U, add, T, lane);
  if (a.jitter_rel != 0.0) {
    double dm = diag_abs_mean<NB>(U, T, lane);
    add_diag<NB>(U, a.jitter_rel * fmax(dm, F64_EPS), T, lane);
  }
  const int off = a.item_off[it], cnt = a.item_cnt[it];
  PivotAcc pa;
  pa.init();
  double ld = 0.0;
  // the first 16 segments ride along with the factorisation; further chunks reuse the stored factor
  for (int base = 0; base < cnt; base += 16) {
    const int j = base + c;
    const bool live = j < cnt;
    const int seg = live ? (a.seg_ids ? a.seg_ids[off + j] : off + j) : 0;
    const double* yr = a.Y + (size_t)seg * a.ldy;
#pragma unroll
    for (int K = 0; K < NB; ++K)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int i = 16 * K + g + 4 * r;
        double v = 0.0;
        if (live && i < T) v = yr[i] - (mu ? mu[i] : 0.0);
        R[K][r] = v;
      }
    if (base == 0) {
      wave_factor<NB, 1>(U, R, scr, cnt > 16 ? Wl : nullptr, nullptr, lane, pa, nullptr, 0, T);
      ld = pa.logdet();
    } else {
      wave_fwd_solve<NB>(U, Wl, R, lane);
    }
    double q = wave_colnorm2<NB>(R);
    if (live && g == 0) {
      a.out_quad[seg] = q;
      if (a.out_logdet) a.out_logdet[seg] = ld;
      if (a.out_info) a.out_info[seg] = pa.info;
    }
  }
}

// ------------------------------------------------------------------------- a6, one state per segment
// The reference's real dataflow on a shared grid: every member segment i of a cluster is scored against ITS OWN
// Sigma_i (GPI_model.py:508-531), i.e. one factorisation per segment with a single right-hand side.  Lean variant
// of k_wave_score: the right-hand side is an LDS vector eliminated on the VALU (no RHS tiles), which brings the
// NB <= 6 instantiations under 256 registers -> two waves per SIMD, so one matrix's pivot chain overlaps another's
// loads and MFMAs.  HBM-bound in principle: 8 T^2 + 16 T + 8 bytes per evaluation.
struct EachArgs {
  const double* Y;
  int ldy;
  const double* mean;
  long mean_stride;
  const double* Sigma;
  long sigma_stride;
  int T, n;
  const int32_t* seg_mat;    // [n] Sigma index of segment i
  const int32_t* seg_mean;   // [n] mean row of segment i (NULL: seg_mat)
  const double* seg_add;     // [n] additive diagonal (NULL: 0)
  double jitter_rel;
  double* out_quad;
  double* out_logdet;
  int32_t* out_info;
  int symmetric;             // caller guarantees Sigma == Sigma^T bit for bit: read the upper triangle only
};

// (SYM: one instantiation per loader - with both in one function the NB = 8 kernel spilled 290 VGPRs)
template <int NB, bool SYM>
__global__ __launch_bounds__(64 * WAVES, (NB <= 6) ? 2 : 1) void k_wave_score1(EachArgs a) {
  __shared__ __attribute__((aligned(16))) double scr_all[WAVES * DIAG_SCR];
  __shared__ __attribute__((aligned(16))) double dv_all[WAVES * 16 * NB];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int seg = blockIdx.x * WAVES + wave;
  if (seg >= a.n) return;
  double* scr = scr_all + wave * DIAG_SCR;
  double* dv = dv_all + wave * 16 * NB;
  const int T = a.T;
  const int mat = a.seg_mat[seg];
  const double* S = a.Sigma + (size_t)mat * a.sigma_stride;
  const double* mu = a.mean ? a.mean + (size_t)(a.seg_mean ? a.seg_mean[seg] : mat) * a.mean_stride : nullptr;
  const double* yr = a.Y + (size_t)seg * a.ldy;
  for (int i = lane; i < 16 * NB; i += 64) dv[i] = (i < T) ? yr[i] - (mu ? mu[i] : 0.0) : 0.0;
  d4 U[NB * (NB + 1) / 2];
  d4 Rnone[NB];
  if constexpr (SYM) load_upper_only<NB>(U, S, T, T, lane);
  else load_sym_upper<NB>(U, S, T, T, lane, scr);
  {
    double sh = a.seg_add ? a.seg_add[seg] : 0.0;
    if (a.jitter_rel != 0.0) sh += a.jitter_rel * fmax(diag_abs_mean<NB>(U, T, lane, sh), F64_EPS);
    if (sh != 0.0) add_diag<NB>(U, sh, T, lane);
  }
  __builtin_amdgcn_wave_barrier();
  PivotAcc pa;
  pa.init();
  const double q = wave_factor<NB, 2, (NB < 8)>(U, Rnone, scr, nullptr, dv, lane, pa, nullptr, 0, T);
  if (lane == 0) {
    a.out_quad[seg] = q;
    if (a.out_logdet) a.out_logdet[seg] = pa.logdet();
    if (a.out_info) a.out_info[seg] = pa.info;
  }
}

// ------------------------------------------------------------------ 128 < T <= 256: cooperative kernels
// One workgroup (4 waves) per matrix / work item; see Coop<> in tile_f64.hpp.
template <int NB>
__global__ __launch_bounds__(64 * WAVES) void k_coop_score(ScoreArgs a) {
  using C = Coop<NB>;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const auto [rowbuf, Rbuf, Wbuf, scr, red, redi] = C::lds(smem);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int g = lane >> 4, c = lane & 15;
  const int it = blockIdx.x;
  const int T = a.T;
  const int mat = a.item_mat[it];
  const double* S = a.Sigma + (size_t)mat * a.sigma_stride;
  const double* mu = a.mean ? a.mean + (size_t)(a.item_mean ? a.item_mean[it] : mat) * a.mean_stride : nullptr;
  const double add = a.item_add ? a.item_add[it] : 0.0;
  const int off = a.item_off[it], cnt = a.item_cnt[it];
  d4 U[C::NT];
  for (int base = 0; base < cnt; base += 16) {     // every chunk of 16 segments refactors (rare for T > 128)
    coop_load_sym_upper<NB>(U, S, a.ld_sigma, T, wave, lane, rowbuf + wave * DIAG_SCR);
    __syncthreads();   // rowbuf served as per-wave staging for the loader
    coop_regularise<NB>(U, add, a.jitter_rel, T, wave, lane, red);
    const int j = base + c;
    const bool live = j < cnt;
    const int seg = live ? (a.seg_ids ? a.seg_ids[off + j] : off + j) : 0;
    const double* yr = a.Y + (size_t)seg * a.ldy;
    for (int K = wave; K < NB; K += WAVES) {
      d4 v;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = 16 * K + g + 4 * r;
        v[r] = (live && i < T) ? yr[i] - (mu ? mu[i] : 0.0) : 0.0;
      }
      lds_tile_store(Rbuf, K, lane, v);
    }
    __syncthreads();
    PivotAcc pa;
    pa.init();
    coop_factor<NB, true>(U, rowbuf, Rbuf, Wbuf, scr, wave, lane, pa, nullptr, 0, T);
    int info;
    const double ld = coop_logdet_info(pa, wave, lane, red, redi, info);
    // quad_j = sum over all tiles of Z^2 in column j
    double q = 0.0;
    for (int K = wave; K < NB; K += WAVES) {
      const d4 z = lds_tile_load(Rbuf, K, lane);
#pragma unroll
      for (int r = 0; r < 4; ++r) q = fma(z[r], z[r], q);
    }
    q = xrow_sum(q);
    if (g == 0) Wbuf[wave * 16 + c] = q;
    __syncthreads();
    if (wave == 0 && g == 0 && live) {
      a.out_quad[seg] = Wbuf[c] + Wbuf[16 + c] + Wbuf[32 + c] + Wbuf[48 + c];
      if (a.out_logdet) a.out_logdet[seg] = ld;
      if (a.out_info) a.out_info[seg] = info;
    }
    __syncthreads();
  }
}

// in-place factor: A <- L (zeros above), info, logdet
template <int NB>
__global__ __launch_bounds__(64 * WAVES) void k_coop_potrf(PotrfArgs a) {
  using C = Coop<NB>;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const auto [rowbuf, Rbuf, Wbuf, scr, red, redi] = C::lds(smem);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int m = blockIdx.x;
  const int T = a.T;
  double* A = (a.Aout ? a.Aout : a.A) + (size_t)m * T * T;     // where L goes
  d4 U[C::NT];
  coop_load_sym_upper<NB>(U, a.A + (size_t)(a.src_idx ? a.src_idx[m] : m) * T * T, T, T, wave, lane, rowbuf + wave * DIAG_SCR);
  __syncthreads();   // rowbuf served as per-wave staging for the loader
  coop_regularise<NB>(U, a.add, a.jitter_rel, T, wave, lane, red);
  __syncthreads();   // every wave has loaded its tiles before anyone overwrites A
  PivotAcc pa;
  pa.init();
  coop_factor<NB, false>(U, rowbuf, Rbuf, Wbuf, scr, wave, lane, pa, A, T, T, nullptr,
                         a.Linv ? a.Linv + (size_t)m * T * T : nullptr, T);   // + the diagonal blocks of L^-1 (k_trtri does the rest)
  int info;
  const double ld = coop_logdet_info(pa, wave, lane, red, redi, info);
  if (threadIdx.x == 0) {
    if (a.info) a.info[m] = info;
    if (a.logdet) a.logdet[m] = ld;
  }
  for (int idx = threadIdx.x; idx < T * T; idx += 64 * WAVES) {   // zeros above the diagonal blocks
    const int i = idx / T, j = idx % T;
    if ((j >> 4) > (i >> 4)) A[idx] = 0.0;
  }
}

template <int NB>
int launch_coop_score(const ScoreArgs& a, hipStream_t st) {
  const size_t lds = sizeof(double) * Coop<NB>::LDS_DOUBLES;
  if (int rc_ = hgp_internal_ensure_dynamic_lds(reinterpret_cast<const void*>(&k_coop_score<NB>), lds)) return rc_;
  hipLaunchKernelGGL(k_coop_score<NB>, dim3(a.n_items), dim3(64 * WAVES), lds, st, a);
  return launch_status();
}

template <int NB>
int launch_coop_potrf(const PotrfArgs& a, hipStream_t st) {
  const size_t lds = sizeof(double) * Coop<NB>::LDS_DOUBLES;
  if (int rc_ = hgp_internal_ensure_dynamic_lds(reinterpret_cast<const void*>(&k_coop_potrf<NB>), lds)) return rc_;
  hipLaunchKernelGGL(k_coop_potrf<NB>, dim3(a.b), dim3(64 * WAVES), lds, st, a);
  // L^-1 from L: the factor kernel left the diagonal blocks' inverses in Linv, k_trtri (hgp_inverse.hip) fills in the block columns
  if (a.Linv) hgp_internal_trtri(a.Aout ? a.Aout : a.A, a.Linv, a.T, a.b, a.info, st);
  return launch_status();
}

}  // namespace

// hipFuncAttributeMaxDynamicSharedMemorySize is a per-device property of a kernel: set it once for every (kernel, device)
// this process launches on, under a lock (the launchers are called from any host thread).
int hgp_internal_ensure_dynamic_lds(const void* fn, size_t bytes) {
  static std::mutex mu;
  static std::vector<std::pair<const void*, int>> done;
  int dv = 0;
  if (hipGetDevice(&dv) != hipSuccess) return launch_status();
  std::lock_guard<std::mutex> lk(mu);
  for (const auto& d : done)
    if (d.first == fn && d.second == dv) return 0;
  const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e != hipSuccess) return 1000 + (int)e;
  done.emplace_back(fn, dv);
  return 0;
}

int hgp_internal_potrf_coop(const PotrfArgs& a, hipStream_t st) {
  return dispatch_nb_coop(a.T, [&](auto nb) { return launch_coop_potrf<decltype(nb)::value>(a, st); });
}

int hgp_internal_potrf_ws(const double* A, const int32_t* idx, int T, int b, double jitter_rel, double* L, int32_t* info, hipStream_t st) {
  PotrfArgs a{const_cast<double*>(A), T, b, jitter_rel, 0.0, nullptr, nullptr, info};
  a.Aout = L;
  a.src_idx = idx;
  if (T > HGP_MAX_T_WAVE) return hgp_internal_potrf_coop(a, st);
  dispatch_nb_wave(T, [&](auto nb) {
    hipLaunchKernelGGL(k_wave_potrf<decltype(nb)::value>, dim3((b + WAVES - 1) / WAVES), dim3(64 * WAVES), 0, st, a);
  });
  return launch_status();
}

extern "C" {

int hgp_potrf_batched_f64(double* A, int T, int b, double jitter_rel, double add_diag, double* Linv, double* logdet,
                          int32_t* info, void* stream) {
  if (b == 0) return 0;
  if (!A || T <= 0 || b < 0) return -1;
  if (T > HGP_MAX_T_COOP) return -2;
  PotrfArgs a{A, T, b, jitter_rel, add_diag, Linv, logdet, info};
  hipStream_t st = (hipStream_t)stream;
  if (T > HGP_MAX_T_WAVE) return hgp_internal_potrf_coop(a, st);
  // L^-1 first, from the input still in A (one wave per block column); info comes from the factor kernel behind it
  if (Linv) hgp_internal_wave_inverse(InvArgs{A, T, b, jitter_rel, add_diag, Linv, /*info=*/nullptr}, st);
  dispatch_nb_wave(T, [&](auto nb) {
    hipLaunchKernelGGL(k_wave_potrf<decltype(nb)::value>, dim3((b + WAVES - 1) / WAVES), dim3(64 * WAVES), 0, st, a);
  });
  return launch_status();
}

int hgp_score_groups_f64(const double* Y, int ldy, const double* mean, long mean_stride, const double* Sigma,
                         long sigma_stride, int T, const int32_t* item_mat, const int32_t* item_mean,
                         const double* item_add, const int32_t* item_off, const int32_t* item_cnt, int n_items,
                         const int32_t* seg_ids, double jitter_rel, double* out_quad, double* out_logdet,
                         int32_t* out_info, void* stream) {
  if (n_items == 0) return 0;
  if (!Y || !Sigma || !item_mat || !item_off || !item_cnt || !out_quad || T <= 0 || ldy < T || n_items < 0) return -1;
  if (T > HGP_MAX_T_COOP) return -2;
  ScoreArgs a{Y, ldy, mean, mean_stride, Sigma, sigma_stride, T, T, item_mat, item_mean, item_add, item_off, item_cnt, n_items,
              seg_ids, jitter_rel, out_quad, out_logdet, out_info};
  hipStream_t st = (hipStream_t)stream;
  if (T > HGP_MAX_T_WAVE) return dispatch_nb_coop(T, [&](auto nb) { return launch_coop_score<decltype(nb)::value>(a, st); });
  dispatch_nb_wave(T, [&](auto nb) {
    hipLaunchKernelGGL(k_wave_score<decltype(nb)::value>, dim3((n_items + WAVES - 1) / WAVES), dim3(64 * WAVES), 0, st, a);
  });
  return launch_status();
}

int hgp_score_each_f64(const double* Y, int ldy, const double* mean, long mean_stride, const double* Sigma,
                       long sigma_stride, int T, const int32_t* seg_mat, const int32_t* seg_mean, const double* seg_add,
                       int n, double jitter_rel, int symmetric, double* out_quad, double* out_logdet, int32_t* out_info,
                       void* stream) {
  if (n == 0) return 0;
  if (!Y || !Sigma || !seg_mat || !out_quad || T <= 0 || ldy < T || n < 0) return -1;
  if (T > HGP_MAX_T_WAVE) return -2;   // larger T: hgp_score_groups_f64 with one segment per item
  EachArgs a{Y, ldy, mean, mean_stride, Sigma, sigma_stride, T, n, seg_mat, seg_mean, seg_add, jitter_rel, out_quad, out_logdet,
             out_info, symmetric};
  hipStream_t st = (hipStream_t)stream;
  dispatch_nb_wave(T, [&](auto nb) {
    dispatch_bool(symmetric != 0, [&](auto sym) {
      hipLaunchKernelGGL((k_wave_score1<decltype(nb)::value, decltype(sym)::value>), dim3((n + WAVES - 1) / WAVES), dim3(64 * WAVES), 0, st, a);
    });
  });
  return launch_status();
}

}  // extern "C"
