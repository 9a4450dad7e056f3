// The filter chain of a static cluster model (include/hdpgpc_hip_static.h): Gamma = 0, h = 1, every member on the
// basis grid - GPI.posterior (GPI.py:134-151) member after member,
//     x_m = A m,  P_k = A P A^T,  S = C P_k C^T + cov_f,  K = P_k C^T S^-1,  m' = x_m + K (y - f*),
//     P' = (I - K C) P_k (I - K C)^T + (K cov_f) K^T.
//
// ONE workgroup of four waves per chain, persistent over the chain's members; one launch for all chains and all their members.
// What crosses a member stays where the caller wants it anyway: the new P' is the appended row of the caller's stack, read back
// by the next member (the same compute unit wrote it: L1 / L2), m' also sits in LDS.  Every intermediate [T,T] matrix lives in
// the chain's slice of the workspace (ST_SLOTS matrices, L2-resident) and is handed from the waves that wrote it to the waves that
// read it by a workgroup barrier: __syncthreads() is a workgroup-scope release / acquire, and the waves of a workgroup share
// their compute unit's L1, which their own stores write through.
//   products   st_gemm: wave w owns the block rows w, w + 4 of the result, all NB column tiles of a block row in accumulators; the
//              operands stream from the workspace with run-time strides (one body for N / T operands), v_mfma_f64_16x16x4_f64;
//   S^-1       every wave with a block column of its own (16 w < T) factors S in registers - the text of k_wave_inv (hgp_inverse.hip):
//              symmetrised load, wave_factor<NB, 1> with the identity panel w riding - and, for T > 64, takes the panel w + 4 through
//              the factor it kept (wave_fwd_solve, as k_project_wave does): Z = L^-1 in one factorisation time, S^-1 = Z^T Z;
//   vectors    m, x_m, y - f* in LDS; matrix-vector products two lanes per row.
// A product with A or C is skipped when the matrix is the identity bit for bit and the other factor is finite throughout (the
// flag each product's epilogue hands to its barrier): the product's bits are then x + 0.0, which is what is written where the
// value is used element-wise; where it is only an MFMA operand the unchanged matrix serves (the sign of a zero factor cannot
// change a sum that starts from +0).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "hgp_internal.hpp"
#include "tile_f64.hpp"
#include "../../include/hdpgpc_hip_static.h"

using namespace hgp;

namespace {

constexpr int ST_THREADS = 64 * WAVES;
constexpr int ST_SLOTS = 8;   // [T,T] matrices of a chain's workspace slice
constexpr int ST_VEC = HGP_MAX_T_WAVE;

// Dynamic LDS of k_static_chain<NB>: per wave the 16 x 18 staging tile of the loader and of diag16_acc and the inverses W_K of the
// diagonal factors ([NB][4][64], written by wave_factor, read by wave_fwd_solve); then the chain's vectors and one status word.
template <int NB>
struct StaticLds {
  static constexpr int PER_WAVE = DIAG_SCR + NB * 4 * 64;
  static constexpr int WAVE0 = 0, MV = WAVE0 + WAVES * PER_WAVE, XM = MV + ST_VEC, RV = XM + ST_VEC, WORDS = RV + ST_VEC, END = WORDS + 2;   // doubles
  static constexpr size_t BYTES = sizeof(double) * END;
  static_assert(PER_WAVE % 2 == 0 && MV % 2 == 0 && BYTES <= LDS_MAX_BYTES && ST_VEC == 128 && ST_THREADS == 2 * ST_VEC, "k_static_chain: LDS, st_each");
  __device__ static __forceinline__ double* scr(double* base, int wave) { return base + WAVE0 + wave * PER_WAVE; }
  __device__ static __forceinline__ double* w(double* base, int wave) { return base + WAVE0 + wave * PER_WAVE + DIAG_SCR; }
  HGP_LDS_DOUBLES(mv, MV)   // [ST_VEC] m, then m'
  HGP_LDS_DOUBLES(xm, XM)   // [ST_VEC] x_m
  HGP_LDS_DOUBLES(rv, RV)   // [ST_VEC] y - f*
  HGP_LDS_INTS(words, WORDS, 0)   // [0] status of the factorisation
};

__device__ __forceinline__ bool fin(double v) { return (v - v) == 0.0; }

enum { E_NONE = 0, E_ADD = 1, E_EYE_SUB = 2 };

// out = op(A) op(B) (E_NONE), E + op(A) op(B) (E_ADD) or I - op(A) op(B) (E_EYE_SUB); [T,T] row-major, op(A)[i][k] = A[i sAi + k sAk],
// op(B)[k][j] = B[k sBk + j sBj].  The sum over k runs k tile ascending in every output tile.  Returns: every value this lane wrote is finite.
template <int NB>
__device__ __attribute__((noinline)) bool st_gemm(const double* A, int sAi, int sAk, const double* B, int sBk, int sBj, const double* E,
                                                  int emode, double* out, int T, int wave, int lane) {
  const int nb = (T + 15) >> 4;
  const int g = lane >> 4, c = lane & 15;
  bool ok = true;
  // 32-bit element offsets throughout (T <= 128: below 2^14): one add per load next to the uniform base
  int offB[NB];
  bool cok[NB];
#pragma unroll
  for (int J = 0; J < NB; ++J) {
    const int col = 16 * J + c;
    cok[J] = col < T;
    offB[J] = (cok[J] ? col : T - 1) * sBj;
  }
  for (int I = wave; I < nb; I += WAVES) {
    d4 acc[NB];
#pragma unroll
    for (int J = 0; J < NB; ++J) acc[J] = (d4){0.0, 0.0, 0.0, 0.0};
    const int row = 16 * I + c;
    const bool rok = row < T;
    const int offA = (rok ? row : T - 1) * sAi;
    auto load_a = [&](int kt, double (&a)[4]) {
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int k = 16 * kt + 4 * g + s;
        const double v = A[offA + (k < T ? k : T - 1) * sAk];
        a[s] = (rok && k < T) ? v : 0.0;
      }
    };
    double an[4];
    load_a(0, an);
    for (int kt = 0; kt < nb; ++kt) {
      double a[4];
      int offk[4];
      bool kok[4];
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int k = 16 * kt + 4 * g + s;
        a[s] = an[s];
        kok[s] = k < T;
        offk[s] = (kok[s] ? k : T - 1) * sBk;
      }
      if (kt + 1 < nb) load_a(kt + 1, an);   // the next k tile of op(A) travels while this one is multiplied
#pragma unroll
      for (int J = 0; J < NB; ++J) {
        if (J < nb) {
          double b[4];
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            const double v = B[offk[s] + offB[J]];
            b[s] = (cok[J] && kok[s]) ? v : 0.0;
          }
#pragma unroll
          for (int s = 0; s < 4; ++s) acc[J] = mfma(a[s], b[s], acc[J]);
        }
      }
    }
#pragma unroll
    for (int J = 0; J < NB; ++J) {
      if (J < nb) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = 16 * I + g + 4 * r, j = 16 * J + c;
          if (i < T && j < T) {
            double v = acc[J][r];
            if (emode == E_ADD) v = E[i * T + j] + v;
            else if (emode == E_EYE_SUB) v = ((i == j) ? 1.0 : 0.0) - v;
            out[i * T + j] = v;
            ok = ok && fin(v);
          }
        }
      }
    }
  }
  return ok;
}

// f(e, i, j) for every element e = i T + j of a [T,T] matrix, the workgroup's threads two rows at a time (T <= 128 columns: no division)
template <class F>
__device__ __forceinline__ void st_each(int T, int tid, F&& f) {
  const int j = tid & (ST_VEC - 1);
  if (j < T)
    for (int i = tid >> 7; i < T; i += ST_THREADS / ST_VEC) f(i * T + j, i, j);
}

// Z = chol(0.5 (S + S^T))^-1 -> Z [T,T] (zeros above the diagonal blocks), the status of the factorisation -> *word.  Wave w: panels w
// and w + 4.  The regulariser is hgp_chol_inverse_batched_f64's with jitter_rel = 0 and add_diag = 0: the symmetrised load alone.
template <int NB>
__device__ __forceinline__ void st_inverse(const double* S, double* Z, int T, int wave, int lane, double* scr, double* Wl, int* word) {
  if (16 * wave >= T) return;
  const int g = lane >> 4, c = lane & 15;
  d4 U[NB * (NB + 1) / 2];
  d4 R[NB];
  load_sym_upper<NB>(U, S, T, T, lane, scr);
  auto seed = [&](int Jc) {
#pragma unroll
    for (int K = 0; K < NB; ++K)
#pragma unroll
      for (int r = 0; r < 4; ++r) R[K][r] = (K == Jc && g + 4 * r == c) ? 1.0 : 0.0;
  };
  auto store = [&](int Jc) {
#pragma unroll
    for (int K = 0; K < NB; ++K)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = 16 * K + g + 4 * r, j = 16 * Jc + c;
        if (i < T && j < T) Z[(long)i * T + j] = (K >= Jc) ? R[K][r] : 0.0;
      }
  };
  seed(wave);
  PivotAcc pa;
  pa.init();
  wave_factor<NB, 1>(U, R, scr, Wl, nullptr, lane, pa, nullptr, 0, T);
  __builtin_amdgcn_wave_barrier();
  store(wave);
  if constexpr (NB > WAVES) {
    const int J2 = wave + WAVES;
    if (16 * J2 < T) {
      seed(J2);
      wave_fwd_solve<NB>(U, Wl, R, lane, J2);
      store(J2);
    }
  }
  if (wave == 0 && lane == 0) *word = pa.info;
}

// out[i] = sum_k M[i][k] v[k] for row i = tid / 2 (two lanes per row, k interleaved; the value is valid in both); v in LDS
__device__ __forceinline__ double st_matvec(const double* M, const double* v, int T, int tid) {
  const int row = tid >> 1, half = tid & 1;
  double s = 0.0;
  if (row < T) {
    const double* Mr = M + row * T;
#pragma unroll 8
    for (int k = half; k < T; k += 2) s = fma(Mr[k], v[k], s);   // (the loads do not wait for the sum: eight in flight)
  }
  s += __shfl_xor(s, 1, 64);
  return s;
}

template <int NB>
__global__ __launch_bounds__(ST_THREADS) void k_static_chain(const hgp_static_chain_desc* descs, int T, int max_steps, double* ws_all) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  using L = StaticLds<NB>;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const hgp_static_chain_desc d = descs[blockIdx.x];
  if (d.n <= 0 || *d.info != 0) return;
  const long i0 = (long)(*d.pos - d.pos0);
  if (i0 < 0 || i0 >= d.n) return;
  const long iend = (i0 + max_steps < d.n) ? i0 + max_steps : d.n;
  const long tt = (long)T * T;
  double* ws = ws_all + (size_t)blockIdx.x * ST_SLOTS * tt;
  double *W0 = ws, *W1 = ws + tt, *W2 = ws + 2 * tt, *W3 = ws + 3 * tt, *W4 = ws + 4 * tt, *W5 = ws + 5 * tt, *W6 = ws + 6 * tt,
         *W7 = ws + 7 * tt;
  double *mv = L::mv(smem), *xm = L::xm(smem), *rv = L::rv(smem);
  int* words = L::words(smem);
  const double *A = d.A, *C = d.C;
  const bool shortcut = (d.flags & 1) == 0;
  // A, C the identity bit for bit?  The state the chain starts from finite?
  bool idA, idC, finP, finm;
  {
    bool ea = true, ec = true, fp = true;
    const double* P0 = d.Ps + (size_t)(d.pos0 + i0) * tt;
    st_each(T, tid, [&](int e, int i, int j) {
      const long long want = __double_as_longlong((i == j) ? 1.0 : 0.0);
      ea = ea && __double_as_longlong(A[e]) == want;
      ec = ec && __double_as_longlong(C[e]) == want;
      fp = fp && fin(P0[e]);
    });
    bool fm = true;
    if (tid < T) {
      const double v = d.Fs[(size_t)(d.pos0 + i0) * T + tid];
      mv[tid] = v;
      fm = fin(v);
    }
    idA = __syncthreads_and(ea) != 0 && shortcut;
    idC = __syncthreads_and(ec) != 0 && shortcut;
    finP = __syncthreads_and(fp) != 0;
    finm = __syncthreads_and(fm) != 0;
  }
  for (long i = i0; i < iend; ++i) {
    const double* P = d.Ps + (size_t)(d.pos0 + i) * tt;
    double* Pn = d.Ps + (size_t)(d.pos0 + i + 1) * tt;
    double* Fn = d.Fs + (size_t)(d.pos0 + i + 1) * T;
    const double* y = d.Y + (size_t)d.y_idx[i] * T;
    const bool firstb = d.first != 0 && i == 0;
    const bool skipA = idA && finP && finm;
    // ---- x_m = A m
    bool fx = true;
    {
      const double v = skipA ? ((tid < T) ? mv[tid] + 0.0 : 0.0) : st_matvec(A, mv, T, tid);
      const int row = skipA ? tid : (tid >> 1);
      if (row < T && (skipA || (tid & 1) == 0)) {
        xm[row] = v;
        fx = fin(v);
      }
    }
    const bool finxm = __syncthreads_and(fx) != 0;
    // ---- P_k = A P A^T (the first-step branch takes the prior covariance as it stands)
    const double* Pk = P;
    bool finPk = finP;
    if (!firstb && !skipA) {
      st_gemm<NB>(A, T, 1, P, T, 1, nullptr, E_NONE, W0, T, wave, lane);
      __syncthreads();
      const bool ok = st_gemm<NB>(W0, T, 1, A, 1, T, nullptr, E_NONE, W1, T, wave, lane);
      finPk = __syncthreads_and(ok) != 0;
      Pk = W1;
    }
    // ---- cov_f: Sigma, or white I
    const double* covf = d.Sigma;
    if (firstb) {
      st_each(T, tid, [&](int e, int i, int j) { W7[e] = (i == j) ? d.white : 0.0; });
      covf = W7;   // (the barrier behind S hands it over)
    }
    // ---- S = C P_k C^T + cov_f
    const bool skipC = idC && finPk && finxm;
    if (skipC) {
      if (firstb) __syncthreads();
      st_each(T, tid, [&](int e, int, int) { W2[e] = (Pk[e] + 0.0) + covf[e]; });
    } else {
      st_gemm<NB>(C, T, 1, Pk, T, 1, nullptr, E_NONE, W0, T, wave, lane);
      __syncthreads();
      st_gemm<NB>(W0, T, 1, C, 1, T, covf, E_ADD, W2, T, wave, lane);
    }
    __syncthreads();
    // ---- Z = chol(S)^-1, its status
    st_inverse<NB>(W2, W3, T, wave, lane, L::scr(smem, wave), L::w(smem, wave), words);
    __syncthreads();
    const int info = words[0];
    if (info != 0) {   // uniform: NaN to every row the chain would still append, and the chain ends
      const double qnan = __builtin_nan("");
      for (long r = d.pos0 + i + 1; r <= d.pos0 + d.n; ++r) {
        for (long e = tid; e < tt; e += ST_THREADS) d.Ps[(size_t)r * tt + e] = qnan;
        if (tid < T) d.Fs[(size_t)r * T + tid] = qnan;
      }
      if (tid == 0) {
        *d.info = info;
        *d.pos = d.pos0 + d.n;
      }
      return;
    }
    // ---- S^-1 = Z^T Z,  P_k C^T
    st_gemm<NB>(W3, 1, T, W3, T, 1, nullptr, E_NONE, W4, T, wave, lane);
    const double* PkCt = Pk;
    if (!skipC) {
      st_gemm<NB>(Pk, T, 1, C, 1, T, nullptr, E_NONE, W5, T, wave, lane);
      PkCt = W5;
    }
    __syncthreads();
    // ---- K = P_k C^T S^-1
    const bool okK = st_gemm<NB>(PkCt, T, 1, W4, T, 1, nullptr, E_NONE, W6, T, wave, lane);
    // ---- y - f*,  f* = C x_m (0 on the first-step branch)
    {
      double f = 0.0;
      if (!firstb) f = skipC ? ((tid < T) ? xm[tid] + 0.0 : 0.0) : st_matvec(C, xm, T, tid);
      const int row = (firstb || skipC) ? tid : (tid >> 1);
      if (row < T && (firstb || skipC || (tid & 1) == 0)) rv[row] = y[row] - f;
    }
    const bool finK = __syncthreads_and(okK) != 0;
    // ---- m' = x_m + K (y - f*)
    bool fm = true;
    {
      const double s = st_matvec(W6, rv, T, tid);
      const int row = tid >> 1;
      if (row < T && (tid & 1) == 0) {
        const double v = xm[row] + s;
        mv[row] = v;
        Fn[row] = v;
        fm = fin(v);
      }
    }
    // ---- I - K C
    if (idC && finK) {
      st_each(T, tid, [&](int e, int i, int j) { W5[e] = ((i == j) ? 1.0 : 0.0) - (W6[e] + 0.0); });
    } else {
      st_gemm<NB>(W6, T, 1, C, T, 1, nullptr, E_EYE_SUB, W5, T, wave, lane);
    }
    finm = __syncthreads_and(fm) != 0;
    // ---- (I - K C) P_k,  K cov_f
    st_gemm<NB>(W5, T, 1, Pk, T, 1, nullptr, E_NONE, W0, T, wave, lane);
    st_gemm<NB>(W6, T, 1, covf, T, 1, nullptr, E_NONE, W2, T, wave, lane);
    __syncthreads();
    // ---- (K cov_f) K^T, then the Joseph form into the appended row
    st_gemm<NB>(W2, T, 1, W6, 1, T, nullptr, E_NONE, W4, T, wave, lane);
    __syncthreads();
    const bool okP = st_gemm<NB>(W0, T, 1, W5, 1, T, W4, E_ADD, Pn, T, wave, lane);
    finP = __syncthreads_and(okP) != 0;
    if (tid == 0) *d.pos = d.pos0 + i + 1;
  }
}

template <int NB>
int launch_static_chain(const hgp_static_chain_desc* descs, int B, int T, int max_steps, double* ws, hipStream_t st) {
  using L = StaticLds<NB>;
  if (int rc_ = hgp_internal_ensure_dynamic_lds(reinterpret_cast<const void*>(&k_static_chain<NB>), L::BYTES)) return rc_;
  hipLaunchKernelGGL(k_static_chain<NB>, dim3((unsigned)B), dim3(ST_THREADS), L::BYTES, st, descs, T, max_steps, ws);
  return launch_status();
}

}  // namespace

extern "C" {

size_t hgp_static_chain_ws_bytes(int B, int T) {
  if (B <= 0 || T < 1 || T > HGP_MAX_T_WAVE) return 0;
  return sizeof(double) * ST_SLOTS * (size_t)B * (size_t)T * (size_t)T;
}

int hgp_static_chain_steps_f64(const hgp_static_chain_desc* descs, int B, int T, int max_steps, void* ws, size_t ws_bytes, void* stream) {
  if (B < 0 || T < 1 || max_steps < 0) return -1;
  if (B == 0 || max_steps == 0) return 0;
  if (!descs) return -1;
  if (T > HGP_MAX_T_WAVE) return -2;
  if (!ws || ws_bytes < hgp_static_chain_ws_bytes(B, T)) return -1;
  hipStream_t st = (hipStream_t)stream;
  return dispatch_nb_wave(T, [&](auto nb) { return launch_static_chain<decltype(nb)::value>(descs, B, T, max_steps, static_cast<double*>(ws), st); });
}

}  // extern "C"
