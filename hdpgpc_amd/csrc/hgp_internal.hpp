// Host-side declarations shared by the translation units of libhdpgpc_hip.so (not part of the C-ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include <type_traits>
#include <vector>

#include "../../include/hdpgpc_hip.h"

constexpr int WAVES = 4;  // waves per workgroup of the one-wave-per-item kernels: one per SIMD of a CU
constexpr double LOG_2PI = 1.8378770664093453;   // log(2 pi): a Gaussian log-density of Ts points carries -0.5 Ts LOG_2PI

static inline int launch_status() {
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : 1000 + (int)e;
}

static inline int nb_for(int n) {  // tile count, rounded to the instantiated sizes {2,4,6,8}
  int nb = (n + 15) / 16;
  nb = (nb + 1) & ~1;
  return nb < 2 ? 2 : nb;
}

// The runtime tile count as a compile-time NB, decided once: f(std::integral_constant<int, NB>) with the instantiated size for a
// matrix of order T - the one-wave kernels {2,4,6,8} (T <= HGP_MAX_T_WAVE) and the cooperative kernels {12,16} (T <= HGP_MAX_T_COOP).
template <class F> static inline auto dispatch_nb_wave(int T, F&& f) {
  switch (nb_for(T)) {
    case 2: return f(std::integral_constant<int, 2>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 6: return f(std::integral_constant<int, 6>{});
    default: return f(std::integral_constant<int, 8>{});
  }
}
template <class F> static inline auto dispatch_nb_coop(int T, F&& f) {
  return T <= 192 ? f(std::integral_constant<int, 12>{}) : f(std::integral_constant<int, 16>{});
}
template <class F> static inline auto dispatch_nb(int NB, F&& f) {   // a plan's tile count NB = TP / 16: either family
  return NB <= 8 ? dispatch_nb_wave(16 * NB, f) : dispatch_nb_coop(16 * NB, f);
}
template <class F> static inline auto dispatch_bool(bool on, F&& f) {   // the same for a template flag: f(std::true_type) or f(std::false_type)
  return on ? f(std::true_type{}) : f(std::false_type{});
}

static inline bool env_on(const char* name) {
  const char* v = getenv(name);
  return v && v[0] && v[0] != '0';
}

// Entries of E = exp(-h) and of K** / c with h > PAIRS_CUT (value < 2^-80 = 8.3e-25) are exact zeros, and a 16x16 block (k_pairs'
// static sweeps: a 4-row k-step of a block) whose entries are ALL below that is neither built nor multiplied.  What is dropped
// changes a covariance entry by less than 2 T max|M'| 2^-80 in absolute terms: at most 2e-15 for a cluster the explicit-operator
// kernels score (the plan routes eps c^2 |K~^-1|^2 > 1e-9 to the solve-based kernel), about one ulp of the covariance's diagonal
// and six orders below the rounding error eps c^2 |K~^-1|^2 of the explicit operator itself.  Against 40-digit truth the cut is
// not visible on either side of that threshold (tests/test_gpu_pairs_truth.py).  With the reference's length-scale 1.2 on a
// unit-spaced grid the band is |k - j| <= 12 points: only the blocks |Kt - J| <= 1 survive (~60 % of the MFMA work at T = 128 gone)
// and, of their 12 k-steps per column panel, 10.  (Rounds 1-3 cut at 1e-36: |k - j| <= 15, no dead k-step.)  The decision is taken
// from the data (any grid), never from an assumed band structure.
constexpr double PAIRS_CUT = 55.45177444479562;   // 80 ln 2
// segments per launch pair of k_pairs<NB, true> / k_pairs<NB, false> (capacity of the fall-back list of the plan)
constexpr int PAIRS_FB_CAP = 65536;

// number of workgroups (and S scratch areas) of the solve-based pairs kernel (hgp_pairs_acc.hip)
static inline int acc_grid_for(int nb) { return nb > 8 ? 256 : 512; }

struct hgp_pairs_plan {
  int T, K, TP, NB;
  std::vector<double> theta;           // host copy [K,3]
  std::vector<int32_t> perm;           // clusters sorted by length-scale
  std::vector<int> grp_beg, grp_end;   // ranges of `perm` sharing one length-scale
  std::vector<double> grp_ell;
  // device carve-up
  double *d_theta, *d_scal, *d_A, *d_S, *d_Z, *d_Kinv, *d_P, *d_Q, *d_Mp, *d_ap, *d_xb;
  int32_t* d_perm;
  bool coop = false;   // one workgroup per pair (k_pairs_coop): always for T > 128
  // cooperative kernel: overflow areas for the E blocks of dense grids
  double* d_escr = nullptr;
  int32_t* d_eflags = nullptr;
  int nscr = 0;
  long escr_stride = 0;
  // solve-based evaluation (hgp_pairs_acc.hip) for the clusters whose explicit operator M' would lose digits:
  double acc_tol = 1e-9;        // cluster k takes the solve-based kernel when eps (c ||K~^-1||_inf)^2 > acc_tol
  double* d_Lop = nullptr;      // [K][NB(NB-1)/2 strictly lower tiles][64][4]: A operand of L[K,K']
  double* d_LTop = nullptr;     // same tiles: A operand of L[K,K']^T
  double* d_Dop = nullptr;      // [K][4 kinds][NB][64][4]: diagonal-block operands (W4, masked L_KK; plain and transposed)
  double* d_Sop = nullptr;      // [K][NB][NB][64][4]: A operand of tile (K,K') of 0.5 (Sigma + Sigma^T)
  double* d_mu = nullptr;       // [K][TP] prior means on the basis grid (zero padded)
  int32_t* d_acc_list = nullptr;   // [1 + K]: number of flagged clusters, then their ids
  double* d_sscr = nullptr;     // [acc_grid][NB*NB][64][4]: per-workgroup storage of S = K~^{-1} K*
  int32_t* d_fb = nullptr;      // [PAIRS_FB_CAP + 2]: fall-back list of k_pairs (see PairsArgs::fb); zero between launches
  int score_out = 0;            // hgp_pairs_plan_set_score_output: out_quad receives -0.5 quad - 0.5 Ts log(2 pi)
};

// TP <= 128: what the plan update keeps per cluster from call to call.  K~ = ker(xb, xb; theta) + jitter I, its
// inverse factor Z and K~^-1 depend on the basis grid and, through the jitter 1e-4 mean|diag Sigma_k|, on ONE number of cluster k's
// Sigma: a cluster whose grid and jitter have the bits of the call that computed them keeps d_A, d_Z, d_Kinv and info.  The
// words live at the start of the Q area, which these sizes do not use otherwise; hgp_pairs_plan_create zeroes them.
struct PlanReuse {
  long long* key_jit;   // [K] bits of the jitter that d_A, d_Z, d_Kinv of cluster k were computed with
  int32_t* valid;       // [K] d_Z, d_Kinv, key_jit, info of cluster k are complete and belong to d_xb: set LAST by k_plan_ops
  int32_t* same;        // [K] this call's decision of k_prep_build, read by the launches behind it
  int32_t* factored;    // [K] d_A of cluster k holds the factor L instead of K~ (k_acc_factor ran on it)
  int32_t* info;        // [K] status of the factorisation that produced d_Z
  static constexpr size_t BYTES_PER_CLUSTER = sizeof(long long) + 4 * sizeof(int32_t);
};
static inline PlanReuse plan_reuse(const hgp_pairs_plan* p) {
  long long* key = reinterpret_cast<long long*>(p->d_Q);
  int32_t* w = reinterpret_cast<int32_t*>(key + p->K);
  return PlanReuse{key, w, w + p->K, w + 2 * p->K, w + 3 * p->K};
}

// hgp_factor.hip: arguments of the factor kernels
struct PotrfArgs {
  double* A;
  int T, b;
  double jitter_rel, add;
  double* Linv;     // L^-1 is wanted too: read by the cooperative factor (T > 128: its diagonal blocks, the rest by k_trtri); the one-wave factor ignores it
  double* logdet;
  int32_t* info;
  double* Aout = nullptr;   // L goes here instead of over A (hgp_internal_potrf_ws, hgp_internal_chol_inverse)
  const int32_t* src_idx = nullptr;   // item m reads matrix src_idx[m] of A (NULL: m); needs Aout
};
// L[b,T,T] = the a3 factor of A[idx[m]] (idx NULL: A[m]) for m < b, zeros above the diagonal; A is only read.  One launch.
int hgp_internal_potrf_ws(const double* A, const int32_t* idx, int T, int b, double jitter_rel, double* L, int32_t* info, hipStream_t st);
// 128 < T <= HGP_MAX_T_COOP: the cooperative factor as the arguments say, and L^-1 -> a.Linv behind it when that is set (hgp_internal_trtri)
int hgp_internal_potrf_coop(const PotrfArgs& a, hipStream_t st);

// hgp_inverse.hip: arguments of every kernel that produces L^-1 (one 16-column panel per wave / workgroup rides a factorisation)
struct InvArgs {
  // the first 64 bytes, one cache line of kernel arguments: everything the plain forms read (the one-wave kernel is latency-bound from
  // its first instruction to its last store, and a second line costs it 0.2 us - profiles/inverse_ab_bench.txt)
  const double* A;       // [b,T,T], only read
  int T, b;
  double jitter_rel, add;
  double* Linv;          // [b,T,T]  Z = L^-1 (may be NULL when rhs is given: only the solves are wanted)
  int32_t* info;         // [b] or NULL: not reported (a factor kernel behind this launch writes it)
  const double* rhs = nullptr;   // [b,T,T] or NULL
  int rhs_trans = 0;     // solve against rhs^T
  int symmetric = 0;     // the caller guarantees A == A^T bit for bit: only the upper tiles are read (k_wave_inv<NB, false>; the others ignore it)
  // read by the forms with right-hand sides only
  const int32_t* rhs_on = nullptr;   // [b] or NULL: item m carries a right-hand side iff rhs_on[m] != 0 (NULL: all do when rhs != NULL)
  double* rhs_out = nullptr;         // [b,T,T]  Y = L^-1 op(rhs)
  // the plan update only (NULL for every other caller, who runs the kernels compiled without this test): item m is left alone -
  // Linv and info of m keep what an earlier launch wrote - iff keep[m] != 0
  const int32_t* keep = nullptr;     // [b]
};
static_assert(offsetof(InvArgs, rhs_on) == 64, "InvArgs: the plain forms' arguments fill the first 64 bytes");
// Z = chol(A)^-1 -> a.Linv for a plan of NB tiles (a.T = 16 NB; no right-hand sides).  Below NB = 12 only a.A is read and
// factor_out is not touched; from NB = 12 on the matrix is factored first and factor_out [b,T,T] RECEIVES L (zeros above the
// diagonal blocks) - it may be a.A itself, which is then overwritten: both callers pass their own matrix.
int hgp_internal_chol_inverse(const InvArgs& a, int NB, double* factor_out, hipStream_t st);
// T <= HGP_MAX_T_WAVE, no right-hand sides: Z -> a.Linv by one wave per (matrix, block column), one launch; a.A is only read
void hgp_internal_wave_inverse(const InvArgs& a, hipStream_t st);
// Z = L^-1 from L [b,T,T] and the inverses of its diagonal blocks already in Z's diagonal blocks (T > 128); NaN where info[m] != 0
void hgp_internal_trtri(const double* L, double* Z, int T, int b, const int32_t* info, hipStream_t st);
// hipFuncAttributeMaxDynamicSharedMemorySize once per (kernel, device), under a lock
int hgp_internal_ensure_dynamic_lds(const void* fn, size_t bytes);

// hgp_gemm.hip: C[b] = alpha op(A[b]) op(B[b]) + beta C[b] (or + beta D[b]), and the batched reductions of the a9 composition
struct GemmArgs {
  const double* A;
  const double* B;
  double* C;
  int M, N, Kd, lda, ldb, ldc;
  long sA, sB, sC;
  double alpha, beta;
  int tA, tB;
  int nb2 = 1;                 // optional second batch level: item b = b1 * nb2 + b2 uses offsets b1 * s?  + b2 * s?2
  long sA2 = 0, sB2 = 0, sC2 = 0;
  const double* D = nullptr;   // optional addend (instead of C): C = alpha op(A) op(B) + beta D
  int ldd = 0;
  long sD = 0;
  int boff = 0;                // first batch item of this launch (gridDim.y is capped at 65535: larger batches go in chunks)
  int triA = 0;                // A (not transposed) is lower triangular: row tile ti only needs k < 16 (ti + 1)
};
int hgp_internal_gemm(const GemmArgs& a, int batch, hipStream_t st);
void hgp_internal_dot_batched(const double* X, const double* Y, long sX, long sY, long n, double scale, int accumulate, double* out, int b, hipStream_t st);
void hgp_internal_colnorm_diag(const double* Z, const double* S, long sS, int T, double scale, int accumulate, double* out, int b, hipStream_t st);
void hgp_internal_sub_batched(const double* A, const double* B, long sA, long sB, long n, double* C, int b, hipStream_t st);

// hgp_pairs_acc.hip
// flags_done: the plan update has written the routing flags already (k_plan_ops, TP <= 128)
int hgp_internal_acc_prep(hgp_pairs_plan* p, const double* mean, bool flags_done, hipStream_t st);
size_t hgp_internal_acc_bytes(int TP, int K, size_t* sizes /*[6]*/);

// hgp_matlik_coop.hip: the same two terms for 128 < T <= HGP_MAX_T_COOP, one workgroup per item (factor once, packed factor in ws)
int hgp_internal_lat_coop(const double* f_cur, const double* f_prev, const double* A, const double* Gamma, const double* P, int T, int b,
                          double* out, int32_t* info, double* ws, hipStream_t st);
int hgp_internal_mniw_coop(const double* M, const double* Sigma, const double* m_mean, const double* scale, long prior_stride, int T, int b,
                           double* out, int32_t* info, double* ws, hipStream_t st);

// arguments of the explicit-operator pair kernels (hgp_pairs.hip)
struct PairsArgs {
  const double* x;
  const double* y;
  int N, Ts;
  const double* xb;
  int T;
  const double* Mp;
  const double* ap;
  const double* scal;
  const int32_t* perm;   // sorted position -> original cluster id
  int kbeg, kend;        // range of sorted positions sharing one length-scale
  double ell;
  const double* first_noise;
  const int32_t* sel;    // optional [N]: segment n is scored against cluster sel[n] only; outputs are then [N]
#ifdef HGP_STAMPS
  unsigned long long* stamps;
#endif
  int K;
  double* out_quad;
  double* out_logdet;
  int32_t* out_info;
  // cooperative kernel only: global scratch for the E blocks that do not fit its LDS slots (dense grids)
  double* escr;          // [nscr][escr_stride]
  int32_t* eflags;       // [nscr] 0 = free
  int nscr;
  long escr_stride;
  int flags;             // bit 0: generic (mask-driven) sweeps even for a block-tridiagonal E (HGP_PAIRS_GENERIC=1: A/B runs and tests)
  double score_add;      // score output (hgp_pairs_plan_set_score_output): out_quad = score_on ? -0.5 quad + score_add : quad
  int score_on;
  int32_t* fb;           // k_pairs: fall-back list [0] = count, [1 .. PAIRS_FB_CAP] = segments, [1 + PAIRS_FB_CAP] = finished workgroups
};

// The same for a ragged batch (hgp_loglik_pairs_ragged_f64, hgp_pairs_ragged.hip): segment n has seg_len[n] real points, the first
// of its row; Ts above is then the row stride ld of x and y and nothing else, and score_add is not read (the kernels form the
// offset from the segment's own length).  A struct of its own: the rectangular kernels keep their kernarg layout.
struct PairsRagArgs : PairsArgs {
  const int32_t* seg_len;   // [N], 1 <= seg_len[n] <= Ts; anything else: NaN / info = -1 for the row's pairs
};
template <class Args> constexpr bool pairs_ragged = std::is_base_of<PairsRagArgs, Args>::value;

// The same for the streamed band kernel (hgp_loglik_pairs_segops_f64, hgp_segops.hip): segment n's length, band decision, E blocks
// and K** tiles come from record n of the segment-operator store (hgp_segops.hpp), which k_segops has brought up to date on the
// same stream; x and xb are not read, Ts is the row stride of y.  score_add is not read.
struct PairsSegArgs : PairsArgs {
  const double* store;   // record of segment 0 of this launch, this length-scale group
};

#ifdef HGP_STAMPS
extern unsigned long long* hgp_internal_stamp_dev;
#endif

// What a caller of hgp_loglik_pairs_f64, hgp_loglik_pairs_ragged_f64 or hgp_loglik_pairs_segops_f64 passes
struct PairsCall {
  const double* x;
  const double* y;
  int N, ld;                  // rows of x and y lie ld apart
  const int32_t* seg_len;     // [N] or NULL: every row has ld points
  const double* first_noise;
  const int32_t* sel;
  double* out_quad;
  double* out_logdet;
  int32_t* out_info;
};
// HGP_PAIRS_GENERIC=1: the mask-driven sweeps for every segment (A/B runs and tests)
static inline bool pairs_generic_forced() { return env_on("HGP_PAIRS_GENERIC"); }

// The arguments of segments [off, off + n) of a batch, given those of the whole batch: everything per segment moves
template <class Args> static inline Args pairs_slice(Args a, int off, int n) {
  const size_t oo = a.sel ? (size_t)off : (size_t)off * a.K;
  a.N = n;
  a.x += (size_t)off * a.Ts;
  a.y += (size_t)off * a.Ts;
  if (a.first_noise) a.first_noise += oo;
  if (a.sel) a.sel += off;
  a.out_quad += oo;
  if (a.out_logdet) a.out_logdet += oo;
  if (a.out_info) a.out_info += oo;
  if constexpr (pairs_ragged<Args>) a.seg_len += off;
  return a;
}

// The one driver behind the three entries (hgp_plan.hip): every launch of a call, in order.  store: the caller's segment-operator
// store, checked by the entry, or NULL: the band kernel builds its own prologue.  Sizes that no kernel serves: -2.
int hgp_internal_pairs_score(const hgp_pairs_plan* p, const PairsCall& c, void* store, hipStream_t st);

// What the driver launches, one function per launch step and one overload per argument type: hgp_pairs.hip defines those of
// PairsArgs, hgp_pairs_ragged.hip those of PairsRagArgs.  a.N segments, one workgroup each (cooperative: one per pair).
// - every segment by one kernel, no list: the cooperative kernel, or the mask-driven one (NB < 6, generic forced)
int hgp_internal_pairs_all(const PairsArgs& a, int NB, bool coop, hipStream_t st);
int hgp_internal_pairs_all(const PairsRagArgs& a, int NB, bool coop, hipStream_t st);
// - the band kernel (NB = 6, 8): segments that are not of the static pattern go on the list a.fb
int hgp_internal_pairs_band(const PairsArgs& a, int NB, hipStream_t st);
int hgp_internal_pairs_band(const PairsRagArgs& a, int NB, hipStream_t st);
// - the mask-driven kernel on the segments that the band step before it has put on the list a.fb; it hands the list back empty
int hgp_internal_pairs_listed(const PairsArgs& a, int NB, hipStream_t st);
int hgp_internal_pairs_listed(const PairsRagArgs& a, int NB, hipStream_t st);
// - the band step from the store (hgp_segops.hip): k_segops brings the records of a's segments up to date, k_pairs_seg streams
//   them.  Record `first` of the store ([length-scale group][segment]) is that of a's first segment; seg_len belongs to a's
//   segments too, or is NULL.
int hgp_internal_pairs_streamed(const PairsArgs& a, const int32_t* seg_len, void* store, size_t first, int NB, hipStream_t st);
// - the solve-based kernel over the whole batch (hgp_pairs_acc.hip; std::true_type: its ragged form, hgp_pairs_acc_ragged.hip)
int hgp_internal_pairs_acc(const hgp_pairs_plan* p, const PairsCall& c, std::false_type, hipStream_t st);
int hgp_internal_pairs_acc(const hgp_pairs_plan* p, const PairsCall& c, std::true_type, hipStream_t st);
