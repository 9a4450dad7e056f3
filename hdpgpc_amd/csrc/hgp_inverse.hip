// The L^-1 family: Z = chol(0.5 (A + A^T) + shift I)^-1 by block columns, with optional right-hand sides Y = Z op(B).
// Every 16-column PANEL (a block column of the identity, or of op(B)) rides one factorisation as its 16 right-hand sides; the
// kernels differ in who factors: one wave (k_wave_inv), four waves behind workgroup barriers (k_coop_inv) or NB / 2 waves in
// dataflow order (k_cooph_inv).  Per tile all three do the operations of wave_factor in its order: the same bits whichever runs.
// Above 128 and for large batches L^-1 follows from a factor L instead (k_trtri).  The routing table stands above the entries.
#include "hgp_internal.hpp"
#include "tile_f64.hpp"

using namespace hgp;

namespace {

// One panel of one item: what it starts from, where it goes, whether anybody wants it and whether it reports the status.
// Panels Jq < nblk are the block columns of L^-1, panels nblk <= Jq < 2 nblk those of L^-1 op(rhs) (RHS kernels only).
template <bool RHS>
struct InvPanel {
  int Jq, Jc, nblk;
  bool is_rhs;
  __device__ __forceinline__ InvPanel(int Jq_, int nblk_) : Jq(Jq_), nblk(nblk_) {
    is_rhs = RHS && Jq >= nblk;
    Jc = is_rhs ? Jq - nblk : Jq;
  }
  // Nobody wants this panel (no Linv asked for / right-hand side absent or switched off).  An item nobody factors at all still
  // reports a defined status: panel 0 writes info = 0 (writer: one thread of the panel's team).
  __device__ __forceinline__ bool skip(const InvArgs& a, int m, bool writer) const {
    if constexpr (!RHS) return false;
    auto rhs_off = [&] { return !a.rhs || (a.rhs_on && a.rhs_on[m] == 0); };
    if (is_rhs ? !rhs_off() : a.Linv != nullptr) return false;
    if (Jq == 0 && writer && a.info && rhs_off()) a.info[m] = 0;
    return true;
  }
  // tile K of the panel as the factorisation takes it in (accumulator layout): the identity block, or the tile of op(rhs), zero outside T
  __device__ __forceinline__ d4 seed(const InvArgs& a, int m, int K, int lane) const {
    const int g = lane >> 4, c = lane & 15, T = a.T;
    d4 v;
    if (!is_rhs) {
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = (K == Jc && g + 4 * r == c) ? 1.0 : 0.0;
    } else {
      const double* B = a.rhs + (size_t)m * T * T;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = 16 * K + g + 4 * r, j = 16 * Jc + c;
        v[r] = (i < T && j < T) ? (a.rhs_trans ? B[(size_t)j * T + i] : B[(size_t)i * T + j]) : 0.0;
      }
    }
    return v;
  }
  // tile K of the solved panel to its place; L^-1 is lower triangular: zeros above block Jc
  __device__ __forceinline__ void store(const InvArgs& a, int m, int K, const d4& v, int lane) const {
    const int g = lane >> 4, c = lane & 15, T = a.T;
    double* Z = (is_rhs ? a.rhs_out : a.Linv) + (size_t)m * T * T;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = 16 * K + g + 4 * r, j = 16 * Jc + c;
      if (i < T && j < T) Z[(size_t)i * T + j] = (is_rhs || K >= Jc) ? v[r] : 0.0;
    }
  }
  // the item's status comes from ONE panel that saw every pivot: the first one that is factored
  __device__ __forceinline__ bool reports(const InvArgs& a) const { return a.info && Jq == ((!RHS || a.Linv) ? 0 : nblk); }
};

// One wave per (matrix, panel), T <= 128.  Reads A (never writes it), so it may run BEFORE an in-place factor of the same A.
// KEEP (the plan update, a.keep != NULL): an item whose keep word is set is left alone; the instances without it are the kernels
// of every other caller, and do not read the word.
template <int NB, bool RHS, bool KEEP = false>
__global__ __launch_bounds__(64 * WAVES) void k_wave_inv(InvArgs a) {
  __shared__ __attribute__((aligned(16))) double scr_all[WAVES * DIAG_SCR];
  constexpr int NP = (RHS ? 2 : 1) * NB;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int w = blockIdx.x * WAVES + wave;
  const int m = w / NP;
  const int T = a.T;
  if (m >= a.b) return;
  if constexpr (KEEP) {
    if (a.keep[m] != 0) return;
  }
  const InvPanel<RHS> pn(w % NP, NB);
  if (16 * pn.Jc >= T || pn.skip(a, m, lane == 0)) return;
  double* scr = scr_all + wave * DIAG_SCR;
  const double* A = a.A + (size_t)m * T * T;
  d4 U[NB * (NB + 1) / 2];
  d4 R[NB];
  if (!RHS && a.symmetric) load_upper_only<NB>(U, A, T, T, lane);   // plain form only: no caller with right-hand sides sets it
  else if constexpr (NB <= 6) load_sym_upper_burst<NB>(U, A, T, T, lane, scr);   // latency-bound: all loads in flight at once
  else load_sym_upper<NB>(U, A, T, T, lane, scr);
  {   // the regulariser in ONE pass, written out
    double sh = a.add;
    if (a.jitter_rel != 0.0) sh += a.jitter_rel * fmax(diag_abs_mean<NB>(U, T, lane, a.add), F64_EPS);
    if (sh != 0.0) add_diag<NB>(U, sh, T, lane);
  }
#pragma unroll
  for (int K = 0; K < NB; ++K) R[K] = pn.seed(a, m, K, lane);
  PivotAcc pa;
  pa.init();
  wave_factor<NB, 1>(U, R, scr, nullptr, nullptr, lane, pa, nullptr, 0, T);
#pragma unroll
  for (int K = 0; K < NB; ++K) pn.store(a, m, K, R[K], lane);
  if (pn.reports(a) && lane == 0) a.info[m] = pa.info;
}

template <int NB, bool RHS>
void launch_wave_inv(const InvArgs& a, hipStream_t st) {
  const int waves = a.b * (RHS ? 2 : 1) * NB;
  if constexpr (!RHS && NB < 8) {   // the plan's sizes of the one-wave form (hgp_internal_chol_inverse)
    if (a.keep) {
      hipLaunchKernelGGL((k_wave_inv<NB, false, true>), dim3((waves + WAVES - 1) / WAVES), dim3(64 * WAVES), 0, st, a);
      return;
    }
  }
  hipLaunchKernelGGL((k_wave_inv<NB, RHS>), dim3((waves + WAVES - 1) / WAVES), dim3(64 * WAVES), 0, st, a);
}

// A WORKGROUP of four waves per (matrix, panel): the tiles are dealt over the waves (Coop<NB>), only the pivot chain stays serial.
// For small batches, where the launch is one exposed latency and a wave that factors the whole matrix by itself is the whole of
// it (31 us at T = 90: six serial diag16 plus ~280 dependent MFMAs on one SIMD), and for 128 < T <= 256, which no wave holds.
// NB is padded to a multiple of four (identity blocks).  The form with right-hand sides does not take the padded steps (kstop =
// nblk; only NB = 4 is instantiated) and has one workgroup per real panel.  The plain form takes all NB steps and is launched
// with NB panels, of which those beyond T leave at once, exactly as before the two forms shared this body: the steps over the
// padding change no bit, and a run-time stop costs the instances for T > 128 the unrolled step loop (NB = 12: 800 bytes of
// scratch, 154 us instead of 55 at T = 144; DESIGN.md 4, "The L^-1 family").
template <int NB, bool RHS, bool KEEP = false>
__global__ __launch_bounds__(64 * WAVES) void k_coop_inv(InvArgs a) {
  using C = Coop<NB>;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const auto [rowbuf, Rbuf, Wbuf, scr, red, redi] = C::lds(smem);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int T = a.T, nblk = (T + 15) >> 4;
  const int m = blockIdx.x;
  if constexpr (KEEP) {
    if (a.keep[m] != 0) return;   // the plan update: this item's Z and info stand (see k_wave_inv)
  }
  if constexpr (!RHS) {
    if (16 * (int)blockIdx.y >= T) return;   // plain form: gridDim.y = NB
  }
  const InvPanel<RHS> pn(blockIdx.y, nblk);
  if (pn.skip(a, m, threadIdx.x == 0)) return;
  const int kend = RHS ? nblk : NB;   // block steps taken
  const double* A = a.A + (size_t)m * T * T;
  d4 U[C::NT];
  coop_load_sym_upper<NB>(U, A, T, T, wave, lane, rowbuf + wave * DIAG_SCR);
  __syncthreads();   // rowbuf served as per-wave staging for the loader
  coop_regularise<NB>(U, a.add, a.jitter_rel, T, wave, lane, red);
  for (int K = wave; K < NB; K += WAVES) lds_tile_store(Rbuf, K, lane, pn.seed(a, m, K, lane));
  __syncthreads();
  PivotAcc pa;
  pa.init();
  coop_factor<NB, true>(U, rowbuf, Rbuf, Wbuf, scr, wave, lane, pa, nullptr, 0, T, nullptr, nullptr, 0, nullptr, nullptr, kend);
  for (int K = wave; K < nblk; K += WAVES) pn.store(a, m, K, lds_tile_load(Rbuf, K, lane), lane);
  if (pn.reports(a)) {
    int info;
    (void)coop_logdet_info(pa, wave, lane, red, redi, info);
    if (threadIdx.x == 0) a.info[m] = info;
  }
}

template <int NB, bool RHS>
int launch_coop_inv(const InvArgs& a, hipStream_t st) {
  const size_t lds = sizeof(double) * Coop<NB>::LDS_DOUBLES;
  if constexpr (!RHS && NB == 8) {   // the plan's size of this form (hgp_internal_chol_inverse)
    if (a.keep) {
      if (int rc_ = hgp_internal_ensure_dynamic_lds(reinterpret_cast<const void*>(&k_coop_inv<NB, false, true>), lds)) return rc_;
      hipLaunchKernelGGL((k_coop_inv<NB, false, true>), dim3(a.b, NB), dim3(64 * WAVES), lds, st, a);
      return launch_status();
    }
  }
  if (int rc_ = hgp_internal_ensure_dynamic_lds(reinterpret_cast<const void*>(&k_coop_inv<NB, RHS>), lds)) return rc_;
  hipLaunchKernelGGL((k_coop_inv<NB, RHS>), dim3(a.b, RHS ? 2 * ((a.T + 15) >> 4) : NB), dim3(64 * WAVES), lds, st, a);
  return launch_status();
}

// ... and with the DATAFLOW factorisation (cooph_factor_df<NB, 1>, NB / 2 waves per workgroup, NB = the even number of 16-blocks:
// no padding at T = 90): no workgroup barrier inside the factorisation - the wave that owns block K + 1 solves only that panel tile,
// updates its diagonal tile from the accumulator, factors it and publishes W_{K+1} and Z_{K+1} while the others are still in the
// trailing update of step K.  The barrier version above spends 4.5 us per block step for 1.2 us of diag16_acc.
// Its dynamic LDS: the factorisation's buffers (three row buffers, W and Z of every block, per-wave scratch), red[8], then the
// factorisation's flag block with the waves' status words behind it.
template <int NB>
struct CoophInvLds {
  using C = CoopH<NB>;
  using Df = typename C::template DfLds<1>;
  static constexpr int DF = 0, RED = DF + Df::DOUBLES, FLAGS = RED + 8;   // doubles
  static constexpr size_t BYTES = sizeof(double) * FLAGS + sizeof(int) * C::DF_INTS;
  static_assert(RED % 2 == 0 && BYTES <= LDS_MAX_BYTES, "k_cooph_inv: LDS");
  HGP_LDS_DOUBLES(df, DF)     // base of the Df members
  HGP_LDS_DOUBLES(red, RED)   // [8]
  HGP_LDS_INTS(flags, FLAGS, 0)
  HGP_LDS_INTS(redi, FLAGS, C::DF_REDI)
};

// This kernel keeps the panel's rules WRITTEN OUT - the text of InvPanel<true>, which the two kernels above use: with the helper
// its two instances run 0.4 us longer (T = 90: 22.0 against 21.6 us, T = 128: 28.3 against 27.8; seed and store each carry part of
// it, profiles/inverse_ab_bench.txt), as the one-wave kernels do with the regulariser in a function.  A change to
// InvPanel is repeated here.  What holds the two texts to the same bits: test_chol_inverse_rhs_small_and_large_batches_agree_bit_for_bit
// (small batches run this kernel, large ones k_wave_inv<NB, true>: Z, Y and info with rhs_on and both values of rhs_trans) and, without
// right-hand sides, test_chol_inverse_plain_entry_equals_rhs_entry_bit_for_bit (tests/test_gpu_chain_kernels.py).
template <int NB>
__global__ __launch_bounds__(64 * CoopH<NB>::NW) void k_cooph_inv(InvArgs a) {
  using C = CoopH<NB>;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  using L = CoophInvLds<NB>;
  using Df = typename L::Df;
  double *df = L::df(smem), *red = L::red(smem);
  int *flags = L::flags(smem), *redi = L::redi(smem);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int T = a.T, nblk = (T + 15) >> 4;
  const int m = blockIdx.x;
  const int g = lane >> 4, c = lane & 15;
  const int Jq = blockIdx.y;                            // gridDim.y = 2 nblk: panels of L^-1, then panels of L^-1 op(B)
  const bool is_rhs = Jq >= nblk;
  const int Jc = is_rhs ? Jq - nblk : Jq;
  const bool skip = (is_rhs && (!a.rhs || (a.rhs_on && a.rhs_on[m] == 0))) || (!is_rhs && !a.Linv);
  if (skip) {
    if (Jq == 0 && !a.Linv && threadIdx.x == 0 && a.info && (!a.rhs || (a.rhs_on && a.rhs_on[m] == 0))) a.info[m] = 0;
    return;
  }
  double* scr = Df::scr(df) + wave * DIAG_SCR;
  const double* A = a.A + (size_t)m * T * T;
  d4 U[C::NT];
#pragma unroll
  for (int i_ = 0; i_ < C::NT; ++i_) U[i_] = (d4){0.0, 0.0, 0.0, 0.0};
  cooph_load_sym_upper<NB>(U, A, T, T, wave, lane, scr);
  cooph_regularise<NB>(U, a.add, a.jitter_rel, T, wave, lane, red);
  // my two tiles of the panel: block rows JA = wave and JB = NB - 1 - wave
  const double* B = is_rhs ? a.rhs + (size_t)m * T * T : nullptr;
  d4 RA, RB;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int K = h == 0 ? wave : NB - 1 - wave;
    d4 v;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = 16 * K + g + 4 * r, j = 16 * Jc + c;
      if (!is_rhs) v[r] = (K == Jc && g + 4 * r == c) ? 1.0 : 0.0;
      else v[r] = (i < T && j < T) ? (a.rhs_trans ? B[(size_t)j * T + i] : B[(size_t)i * T + j]) : 0.0;
    }
    if (h == 0) RA = v;
    else RB = v;
  }
  PivotAcc pa;
  pa.init();
  cooph_factor_df<NB, 1>(U, Df::row0(df), Df::row1(df), Df::row2(df), Df::Wall(df), scr, flags, wave, lane, pa, T, nullptr, &RA, &RB,
                         Df::zbuf(df));
  double* Z = (is_rhs ? a.rhs_out : a.Linv) + (size_t)m * T * T;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int K = h == 0 ? wave : NB - 1 - wave;
    const d4 z = h == 0 ? RA : RB;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = 16 * K + g + 4 * r, j = 16 * Jc + c;
      if (i < T && j < T) Z[(size_t)i * T + j] = (is_rhs || K >= Jc) ? z[r] : 0.0;
    }
  }
  if (Jq == (a.Linv ? 0 : nblk) && a.info) {   // the first panel sees every pivot: the earliest bad one over the waves
    if (lane == 0) redi[wave] = pa.info;
    __syncthreads();
    if (threadIdx.x == 0) {
      int inf = 0;
      for (int w = 0; w < C::NW; ++w)
        if (redi[w] != 0 && (inf == 0 || redi[w] < inf)) inf = redi[w];
      a.info[m] = inf;
    }
  }
}

template <int NB>
int launch_cooph_inv(const InvArgs& a, hipStream_t st) {
  const size_t lds = CoophInvLds<NB>::BYTES;
  if (int rc_ = hgp_internal_ensure_dynamic_lds(reinterpret_cast<const void*>(&k_cooph_inv<NB>), lds)) return rc_;
  hipLaunchKernelGGL(k_cooph_inv<NB>, dim3(a.b, 2 * ((a.T + 15) >> 4)), dim3(64 * CoopH<NB>::NW), lds, st, a);
  return launch_status();
}

// Z = L^-1 from L and the inverses of its diagonal blocks (already sitting in Z's diagonal blocks): block column Kc of Z by ONE
// wave - forward substitution by blocks,  Z_IK = -W_I sum_{K <= j < I} L_Ij Z_jK  (I = K + 1 .. NB - 1), the column's tiles in
// registers (accumulator layout = the B operand of the next product), L and W read from memory in A-operand order.  The block
// columns are independent: 16 waves per 256 x 256 matrix, each one pass over its part of L - instead of one more cooperative
// factorisation per block column (k_coop_inv: NB redundant factorisations per matrix, 3.4 ms for 256 matrices of 256).
template <int NB>
__global__ __launch_bounds__(64 * WAVES) void k_trtri(const double* __restrict__ Lall, double* __restrict__ Zall, int T, int b,
                                                      const int32_t* __restrict__ info) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int g = lane >> 4, c = lane & 15;
  const int w = blockIdx.x * WAVES + wave;
  const int m = w / NB, Kc = w % NB;
  if (m >= b || 16 * Kc >= T) return;
  const double* L = Lall + (size_t)m * T * T;
  double* Z = Zall + (size_t)m * T * T;
  const int nb = (T + 15) >> 4;
  d4 Zc[NB];                                       // Z_IK, I = Kc .. nb - 1 (statically indexed: slot I)
#pragma unroll
  for (int I = 0; I < NB; ++I) {
    if (I == Kc) {                                 // diagonal block: W_K, read back in accumulator layout v[r] = X[g + 4 r][c]
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 16 * I + g + 4 * r, col = 16 * I + c;
        Zc[I][r] = (row < T && col < T) ? Z[(size_t)row * T + col] : ((row == col) ? 1.0 : 0.0);
      }
    } else {
      Zc[I] = (d4){0.0, 0.0, 0.0, 0.0};
    }
  }
#pragma unroll
  for (int I = 1; I < NB; ++I) {
    if (I > Kc && I < nb) {
      d4 acc0 = (d4){0.0, 0.0, 0.0, 0.0}, acc1 = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int j = 0; j < I; ++j) {
        if (j >= Kc) {
          double av[4];
#pragma unroll
          for (int s = 0; s < 4; ++s) {            // A operand of L_Ij: lane (g, c) holds L[16 I + c][16 j + 4 s + g]
            const int row = 16 * I + c, col = 16 * j + 4 * s + g;
            av[s] = (row < T) ? L[(size_t)row * T + col] : 0.0;
          }
          if (j & 1) {
#pragma unroll
            for (int s = 0; s < 4; ++s) acc1 = mfma(av[s], Zc[j][s], acc1);
          } else {
#pragma unroll
            for (int s = 0; s < 4; ++s) acc0 = mfma(av[s], Zc[j][s], acc0);
          }
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) acc0[r] += acc1[r];
      double wv[4];
#pragma unroll
      for (int s = 0; s < 4; ++s) {                // A operand of W_I (diagonal block I of Z)
        const int row = 16 * I + c, col = 16 * I + 4 * s + g;
        wv[s] = (row < T && col < T) ? Z[(size_t)row * T + col] : ((row == col) ? 1.0 : 0.0);
      }
      d4 z = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int s = 0; s < 4; ++s) z = mfma_sub(wv[s], acc0[s], z);      // -W_I acc
      Zc[I] = z;
    }
  }
  const bool bad = info && info[m] != 0;
#pragma unroll
  for (int I = 0; I < NB; ++I) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * I + g + 4 * r, col = 16 * Kc + c;
      if (row < T && col < T && I != Kc) Z[(size_t)row * T + col] = bad ? __builtin_nan("") : ((I > Kc) ? Zc[I][r] : 0.0);
    }
  }
}

}  // namespace

void hgp_internal_trtri(const double* L, double* Z, int T, int b, const int32_t* info, hipStream_t st) {
  dispatch_nb_coop(T, [&](auto nb) {
    constexpr int NB = decltype(nb)::value;
    const int waves = b * NB;
    hipLaunchKernelGGL(k_trtri<NB>, dim3((waves + WAVES - 1) / WAVES), dim3(64 * WAVES), 0, st, L, Z, T, b, info);
  });
}

void hgp_internal_wave_inverse(const InvArgs& a, hipStream_t st) {
  dispatch_nb_wave(a.T, [&](auto nb) { launch_wave_inv<decltype(nb)::value, false>(a, st); });
}

// Who computes L^-1 (b matrices of order T, nblk = ceil(T / 16) blocks; Wave / Coop / CoopH = k_wave_inv / k_coop_inv / k_cooph_inv):
//
//   entry                              range                                   kernels
//   hgp_chol_inverse_batched_f64       T <= 128                                Wave<2|4|6|8, plain>, b nblk waves
//                                      128 < T <= 256                          Coop<12|16, plain>, b NB workgroups (those beyond T leave at once)
//   hgp_chol_inverse_ws_f64            T <= 128, no workspace, b nb <= 512     as hgp_chol_inverse_batched_f64  (nb = 12 | 16)
//                                      otherwise                               factor into the workspace + k_trtri
//   hgp_chol_inverse_rhs_batched_f64   T > 64,  2 b nblk <= 256 (512 at NB=6)  CoopH<6|8>
//     (T <= 128)                       32 < T <= 64,  2 b nblk <= 256          Coop<4, rhs>
//                                      otherwise                               Wave<2|4|6|8, rhs>, 2 b nblk waves
//   hgp_internal_chol_inverse          NB < 8                                  Wave<2|4|6, plain> (the only reader of `symmetric`)
//     (a plan of NB tiles)             NB == 8                                 Coop<8, plain>
//                                      NB <= 8 with a.keep (the plan update)   the KEEP instances of the two rows above
//                                      NB > 8                                  factor into factor_out + k_trtri
//   hgp_potrf_batched_f64 with Linv    T <= 128: Wave<2|4|6|8, plain> with info = NULL (hgp_internal_wave_inverse) before the in-place factor;
//                                      above: factor + k_trtri
int hgp_internal_chol_inverse(const InvArgs& a, int NB, double* factor_out, hipStream_t st) {
  if (NB > 8) {
    if (!factor_out) return -1;
    PotrfArgs f{const_cast<double*>(a.A), a.T, a.b, a.jitter_rel, a.add, a.Linv, nullptr, a.info};
    f.Aout = factor_out;
    return hgp_internal_potrf_coop(f, st);
  }
  // one workgroup per block column (the trailing updates split over its four waves) halves the latency at T = 128
  if (NB == 8) return launch_coop_inv<8, false>(a, st);
  hgp_internal_wave_inverse(a, st);
  return launch_status();
}

extern "C" {

int hgp_chol_inverse_batched_f64(const double* A, int T, int b, double jitter_rel, double add_diag, double* Linv,
                                 int32_t* info, void* stream) {
  if (b == 0) return 0;
  if (!A || !Linv || T <= 0 || b < 0) return -1;
  if (T > HGP_MAX_T_COOP) return -2;
  const InvArgs a{A, T, b, jitter_rel, add_diag, Linv, info};
  hipStream_t st = (hipStream_t)stream;
  if (T > HGP_MAX_T_WAVE) return dispatch_nb_coop(T, [&](auto nb) { return launch_coop_inv<decltype(nb)::value, false>(a, st); });
  hgp_internal_wave_inverse(a, st);
  return launch_status();
}

// The same inverse with a caller-provided workspace work[b,T,T] (T > 128 only; may be NULL): for batches that would fill the
// chip several times over with the per-block-column kernel (b * NB workgroups, every one a full factorisation) the matrix is
// factored ONCE into the workspace and L^-1 follows from L by block columns (k_trtri).  Small batches keep the per-block-column
// kernel: one launch, 97 us at T = 256 against 146 + 73 us for factor + k_trtri.
int hgp_chol_inverse_ws_f64(const double* A, int T, int b, double jitter_rel, double add_diag, double* Linv, double* work,
                            int32_t* info, void* stream) {
  if (b == 0) return 0;
  if (!A || !Linv || T <= 0 || b < 0) return -1;
  if (T > HGP_MAX_T_COOP) return -2;
  const int nb = T <= 192 ? 12 : 16;
  if (T <= HGP_MAX_T_WAVE || !work || (long)b * nb <= 512) return hgp_chol_inverse_batched_f64(A, T, b, jitter_rel, add_diag, Linv, info, stream);
  return hgp_internal_chol_inverse(InvArgs{A, T, b, jitter_rel, add_diag, Linv, info}, nb, work, (hipStream_t)stream);
}

int hgp_chol_inverse_rhs_batched_f64(const double* A, int T, int b, double jitter_rel, double add_diag, double* Linv, const double* rhs,
                                     const int32_t* rhs_on, int rhs_trans, double* rhs_out, int32_t* info, void* stream) {
  if (b == 0) return 0;
  if (!A || T <= 0 || b < 0 || (!Linv && !rhs) || (rhs && !rhs_out)) return -1;
  if (T > HGP_MAX_T_WAVE) return -2;
  const InvArgs a{A, T, b, jitter_rel, add_diag, Linv, info, rhs, rhs_trans, /*symmetric=*/0, rhs_on, rhs_out};
  hipStream_t st = (hipStream_t)stream;
  // few matrices (the member step of a few chains): one workgroup per (matrix, panel) - latency; many: one wave each - throughput
  // (tools/time_inv_rhs.py; while the workgroups fit the chip in one round - beyond that the one-wave kernel wins)
  constexpr int coop_max_wg = 256;
  // T > 64: the dataflow form (T = 90: 21.7 us, barrier form 27.1, one wave per panel 30.3; T = 128: 28.0 / 30.6 / 51.5; two
  // workgroups per CU at NB = 6); 32 < T <= 64: the barrier form (T = 50: 13.1 us against 14.7 / 16.5); T <= 32 is one wave anyway
  const long wgs = (long)b * 2 * ((T + 15) >> 4);
  if (T > 64 && wgs <= (nb_for(T) == 6 ? 2 : 1) * (long)coop_max_wg) {
    return nb_for(T) == 6 ? launch_cooph_inv<6>(a, st) : launch_cooph_inv<8>(a, st);   // own choice: T > 64 only has {6, 8}
  } else if (T > 32 && T <= 64 && wgs <= coop_max_wg) {
    return launch_coop_inv<4, true>(a, st);
  }
  dispatch_nb_wave(T, [&](auto nb) { launch_wave_inv<decltype(nb)::value, true>(a, st); });
  return launch_status();
}

}  // extern "C"
