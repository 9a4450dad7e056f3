// hgp_loglik_pairs_segops_f64 (include/hdpgpc_hip_segops.h): the band pair kernel with its prologue taken out of the call.
//  * k_segops<NB>: one workgroup per segment brings the segment's record of the segment-operator store (hgp_segops.hpp) up to
//    date - it compares the record's key with the call's arguments on the bits and leaves, or rebuilds the record with the
//    expressions of k_pairs' prologue (hgp_pairs.hip), so that every stored value has the bits the in-kernel build produces.
//  * k_pairs_seg<NB, true>: the text of hgp_pairs.hip compiled a third time (HGP_PAIRS_SEGOPS_TU), its prologue a copy of the
//    record's tiles into LDS.  k_pairs, k_pairs_rag and their cooperative forms stay the code they were, in their own units.
//  * segments that are not of the band pattern go to the plan's fall-back list and the mask-driven kernel of hgp_pairs.hip /
//    hgp_pairs_ragged.hip, which builds its own E as ever; flagged clusters go to the solve-based kernel as ever.
// The unit's part of a call is one launch step, hgp_internal_pairs_streamed (k_segops, then k_pairs_seg, on one slice of the
// batch); the driver hgp_internal_pairs_score (hgp_plan.hip) takes it in place of the band kernel when the entry hands it a store.
#include "hgp_segops.hpp"
#include "../../include/hdpgpc_hip_segops.h"

#define HGP_PAIRS_SEGOPS_TU 1
#define k_pairs k_pairs_seg
#define k_pairs_cooph k_pairs_cooph_seg
#include "hgp_pairs.hip"
#undef k_pairs
#undef k_pairs_cooph

namespace {

struct SegOpsArgs {
  const double* x;            // [N, ld]
  const int32_t* seg_len;     // [N] or NULL: every row has ld points
  int N, ld;
  const double* xb;           // [T] the plan's basis grid
  int T;
  double ell;
  double* store;              // record of segment 0, this length-scale group
};

__device__ __forceinline__ long long f64_bits(double v) { return __double_as_longlong(v); }

// Every store the workgroup has issued so far has been acknowledged by the L2 it writes through before any of its threads goes
// on: each thread waits for its own stores, then the barrier.  That is the order the valid mark needs - the record is read by
// later launches only, and the end of this one makes it visible to them.  (Not __threadfence(): at device scope it writes back
// and invalidates the whole L2 of the XCD, per workgroup - a call that rebuilt all 2 048 records took 1.31 ms with it, 0.91 without the store.)
__device__ __forceinline__ void stores_landed() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
}

// One workgroup of four waves per segment; no tile is resident, so several workgroups share a SIMD and hide each other's latencies.
template <int NB>
__global__ __launch_bounds__(64 * WAVES) void k_segops(SegOpsArgs a) {
  using SO = SegOps<NB>;
  using PB = PairsBand<NB>;
  constexpr int TP = 16 * NB, NH = NB / 2, PW = WAVES;
  __shared__ double xs[TP], xbs[TP];
  __shared__ int amask[8], kmask[8], amask4[8], differs;
  const int tid = threadIdx.x, wave = tid >> 6, n = blockIdx.x;
  const int T = a.T, ld = a.ld;
  double* rec = a.store + (size_t)n * SO::REC;
  int* words = reinterpret_cast<int*>(rec + SO::WORDS);
  const int Ts = a.seg_len ? a.seg_len[n] : ld;
  const bool badlen = Ts < 1 || Ts > ld;   // nothing of such a row is read
  const double* xrow = a.x + (size_t)n * ld;

  // the key, on the bits
  if (tid == 0) differs = 0;
  __syncthreads();
  {
    int d = 0;
    if (tid == 0)
      d = !(words[SO::W_FLAG] & SEG_VALID) || words[SO::W_LEN] != Ts || words[SO::W_T] != T || words[SO::W_LD] != ld ||
          words[SO::W_NB] != NB || f64_bits(rec[SO::ELL]) != f64_bits(a.ell);
    if (!badlen)
      for (int i = tid; i < Ts; i += 64 * PW) d |= f64_bits(rec[SO::KEYX + i]) != f64_bits(xrow[i]);
    for (int i = tid; i < T; i += 64 * PW) d |= f64_bits(rec[SO::KEYXB + i]) != f64_bits(a.xb[i]);
    if (d) differs = 1;
  }
  __syncthreads();
  if (!differs) return;

  // rebuild: the record says "differs" until its last word is written
  if (tid == 0) words[SO::W_FLAG] = 0;
  stores_landed();
  int flag = SEG_VALID;
  if (badlen) {
    flag |= SEG_BADLEN;
  } else {
    // k_pairs' prologue from here on, expression by expression; the blocks go to their tiles of the record instead of LDS
    for (int i = tid; i < TP; i += 64 * PW) {
      xs[i] = (i < Ts) ? xrow[i] / a.ell : 1e150 * (double)(1 + i);
      xbs[i] = (i < T) ? a.xb[i] / a.ell : -1e150 * (double)(1 + i);
    }
    if (tid < 8) amask[tid] = kmask[tid] = amask4[tid] = 0;
    __syncthreads();
    const int lane = tid & 63, g = lane >> 4, c = lane & 15;
    for (int Jb = wave; Jb < NB; Jb += PW) {
      const int j = 16 * Jb + c;
      const double xj = xs[j];
      unsigned am = 0, a4 = 0, km = 0;
#pragma unroll
      for (int Kt = 0; Kt < NB; ++Kt) {
        double h[4];
        bool near = false;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const double u = xbs[16 * Kt + g + 4 * r] - xj;
          h[r] = 0.5 * (u * u);
          near = near || (h[r] < PAIRS_CUT);
        }
        if (__any(near)) {
          double ev[4];
          exp_neg4(h, ev);
          const bool inband = Kt + 1 >= Jb && Kt <= Jb + 1;   // a block outside the pattern means "not band": nobody reads it
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            if (inband) rec[SO::TILE * SO::e_slot(Kt, Jb) + 16 * (g + 4 * r) + c] = (h[r] < PAIRS_CUT) ? ev[r] : 0.0;
            if (__any(h[r] < PAIRS_CUT)) a4 |= 1u << ((4 * Kt + r) & 31);
          }
          am |= 1u << Kt;
        }
        if (Kt <= Jb) {
          bool nk = false;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const double u = xs[16 * Kt + g + 4 * r] - xj;
            nk = nk || (0.5 * (u * u) < PAIRS_CUT);
          }
          if (__any(nk)) km |= 1u << Kt;
        }
      }
      if (lane == 0) {
        amask[Jb] = (int)am;
        kmask[Jb] = (int)km;
        amask4[Jb] = (int)a4;
      }
    }
    __syncthreads();
    int kbad = 0, bbad = 0;
#pragma unroll
    for (int J = 0; J < NB; ++J) {
      const int km = kmask[J], am = amask[J], a4 = amask4[J];
      const int rot = ((km << NH) | (km >> (NB - NH))) & ((1 << NB) - 1);
      kbad |= rot & am;
      bbad |= (am ^ PB::emask(J)) | (km ^ PB::kmask(J)) | (int)((unsigned)a4 & ~PB::emask4(J));
    }
    if (kbad == 0 && bbad == 0) {
      flag |= SEG_BAND;
      for (int k = wave; k < SO::NK; k += PW) {   // K** tiles (without the factor c)
        const auto t = SO::k_tile(k);
        const int I = t.Kt, J = t.J;
        double hk[4], ev[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const double u = xs[16 * I + g + 4 * r] - xs[16 * J + c];
          hk[r] = 0.5 * (u * u);
        }
        exp_neg4(hk, ev);
#pragma unroll
        for (int r = 0; r < 4; ++r) rec[SO::TILE * (SO::NE + k) + 16 * (g + 4 * r) + c] = (hk[r] < PAIRS_CUT) ? ev[r] : 0.0;
      }
    }
    for (int i = tid; i < Ts; i += 64 * PW) rec[SO::KEYX + i] = xrow[i];
  }
  for (int i = tid; i < T; i += 64 * PW) rec[SO::KEYXB + i] = a.xb[i];
  if (tid == 0) {
    words[SO::W_LEN] = Ts;
    words[SO::W_T] = T;
    words[SO::W_LD] = ld;
    words[SO::W_NB] = NB;
    rec[SO::ELL] = a.ell;
  }
  stores_landed();
  if (tid == 0) words[SO::W_FLAG] = flag;   // the valid mark, last
}

template <int NB>
int launch_segops(const SegOpsArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(k_segops<NB>, dim3(a.N), dim3(64 * WAVES), 0, st, a);
  return launch_status();
}

template <class F> inline auto dispatch_nb_band(int NB, F&& f) {   // the sizes with a band kernel
  return NB == 6 ? f(std::integral_constant<int, 6>{}) : f(std::integral_constant<int, 8>{});
}

inline bool segops_serves(const hgp_pairs_plan* p) { return !p->coop && (p->NB == 6 || p->NB == 8) && !pairs_generic_forced(); }
inline size_t segops_rec_bytes(int NB) { return NB == 6 ? SegOps<6>::BYTES : SegOps<8>::BYTES; }

}  // namespace

int hgp_internal_pairs_streamed(const PairsArgs& a, const int32_t* seg_len, void* store, size_t first, int NB, hipStream_t st) {
  if (!a.fb) return -1;
  double* rec0 = static_cast<double*>(store) + first * (segops_rec_bytes(NB) / sizeof(double));
  const SegOpsArgs sa{a.x, seg_len, a.N, a.Ts, a.xb, a.T, a.ell, rec0};
  if (int rc = dispatch_nb_band(NB, [&](auto nb) { return launch_segops<decltype(nb)::value>(sa, st); })) return rc;
  return dispatch_nb_band(NB, [&](auto nb) { return launch_pairs<decltype(nb)::value, true>(PairsSegArgs{a, rec0}, st); });
}

extern "C" {

size_t hgp_pairs_segops_bytes(const hgp_pairs_plan* p, int N, int ld) {
  if (!p || N < 1 || ld < 1 || ld > p->TP || !segops_serves(p)) return 0;
  return p->grp_beg.size() * (size_t)N * segops_rec_bytes(p->NB);
}

// Where no band kernel serves the plan the size function says 0: the call is that of the entries without a store
int hgp_loglik_pairs_segops_f64(const hgp_pairs_plan* p, void* segops, size_t segops_bytes, const double* x, const double* y, int N,
                                int ld, const int32_t* seg_len, const double* first_noise, const int32_t* sel, double* out_quad,
                                double* out_logdet, int32_t* out_info, void* stream) {
  if (N == 0) return 0;
  if (!p || !x || !y || !out_quad || N < 0 || ld <= 0) return -1;
  const size_t need = hgp_pairs_segops_bytes(p, N, ld);
  if (need && (!segops || ((uintptr_t)segops & 15) || segops_bytes < need)) return -1;
  return hgp_internal_pairs_score(p, PairsCall{x, y, N, ld, seg_len, first_noise, sel, out_quad, out_logdet, out_info},
                                  need ? segops : nullptr, (hipStream_t)stream);
}

}  // extern "C"
