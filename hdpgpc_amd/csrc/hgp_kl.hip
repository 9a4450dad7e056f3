// a13 - the symmetric Kullback-Leibler distance matrix between Gaussian cluster states (GPI.py:1058-1094 through
// GPI_model.py:899-931, looped over every pair by util_plots.py:598-688), with prec = cov^-1 supplied by the caller:
//
//   out[i,j] = 1/4 (<precB_j, covA_i> + <precA_i, covB_j> - 2T) + 1/4 d^T (precA_i + precB_j) d,   d = meanA_i - meanB_j.
//
// Three launches, whatever nA and nB are:
//   1. k_kl_quad  (fixed = A, others = B):  out[i,j]  = d^T precA_i d
//   2. k_kl_quad  (fixed = B, others = A):  out[i,j] += d^T precB_j d
//   3. k_kl_frob:                           out[i,j]  = 1/4 ((F1 + F2) - 2T) + 1/4 out[i,j]
// F1 = <covA_i, precB_j> and F2 = <precA_i, covB_j> are one "NT" product each over the flat T^2 axis on
// v_mfma_f64_16x16x4_f64: a 128 x 128 output block per workgroup, both operands staged through LDS in K-chunks, so every
// operand row is read once per 128 partners.  The quadratic terms form the differences explicitly (no cancellation
// between large second moments): for one fixed state p and 256 partners o, W = prec_p D with D[:,o] = m_p - m_o is a
// T x 256 x T product on the same instruction, and q_o = sum_t D[t,o] W[t,o].
//
// Position independence: every output element is reduced in one fixed order (k ascending, one accumulator per term, the
// two terms of a sum joined by one commutative addition), nothing depends on the call's shape and nothing is split or
// accumulated atomically.  Swapping the roles of a pair swaps F1 with F2 and the two quadratic terms and negates d, all of
// which leave every rounded intermediate unchanged, so out[i,j] of a self call equals out[j,i] bit for bit; the self call
// computes the blocks on and above the diagonal only and mirrors them.
#include "hgp_internal.hpp"
#include "tile_f64.hpp"

using namespace hgp;

namespace {

constexpr int KL_BT = 128;       // output block edge of k_kl_frob
constexpr int KL_KC = 16;        // K-chunk staged per barrier pair
constexpr int KL_LD = KL_KC + 2; // LDS row stride (doubles): rows c = 0..15, columns g = 0..1 of a half wave hit 32 distinct 8-byte banks
constexpr int KL_QO = 256;       // partners per workgroup of k_kl_quad (4 waves x 4 column tiles)
constexpr int KL_QR = 64;        // precision rows staged per pass of k_kl_quad (4 row tiles)

// rows [r0, r0 + ROWS) x columns [k0, k0 + KL_KC) of a row-major [nrows, K] matrix into registers (rows clamped to the last
// valid one, columns beyond K read as zero) and from there into LDS
template <int ROWS, int NT>
struct Stage {
  static constexpr int PER = ROWS * KL_KC / NT;
  double v[PER];
  __device__ __forceinline__ void load(const double* __restrict__ X, long K, long r0, long nrows, long k0, int tid) {
#pragma unroll
    for (int e = 0; e < PER; ++e) {
      const int idx = e * NT + tid, row = idx / KL_KC, col = idx % KL_KC;
      long r = r0 + row;
      r = r < nrows ? r : nrows - 1;
      const long k = k0 + col;
      v[e] = k < K ? X[r * K + k] : 0.0;
    }
  }
  __device__ __forceinline__ void store(double* __restrict__ S, int tid) const {
#pragma unroll
    for (int e = 0; e < PER; ++e) {
      const int idx = e * NT + tid, row = idx / KL_KC, col = idx % KL_KC;
      S[row * KL_LD + col] = v[e];
    }
  }
};

// acc[4][2] += X[i0 + 64 wm ..][0..K) Y[j0 + 32 wn ..][0..K)^T for the calling wave of a 512-thread workgroup
__device__ __forceinline__ void frob_term(const double* __restrict__ X, const double* __restrict__ Y, long K, long i0, long nX,
                                          long j0, long nY, double* Xs, double* Ys, d4 (&acc)[4][2]) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 15, g = lane >> 4;
  const int wm = w & 1, wn = w >> 1;
  Stage<KL_BT, 512> sx, sy;
  sx.load(X, K, i0, nX, 0, tid);
  sy.load(Y, K, j0, nY, 0, tid);
  for (long k0 = 0; k0 < K; k0 += KL_KC) {
    __syncthreads();   // every wave has finished reading the previous chunk
    sx.store(Xs, tid);
    sy.store(Ys, tid);
    __syncthreads();
    if (k0 + KL_KC < K) {   // the next chunk travels while this one is multiplied
      sx.load(X, K, i0, nX, k0 + KL_KC, tid);
      sy.load(Y, K, j0, nY, k0 + KL_KC, tid);
    }
#pragma unroll
    for (int ks = 0; ks < KL_KC / 4; ++ks) {
      double a[4], b[2];
#pragma unroll
      for (int I = 0; I < 4; ++I) a[I] = Xs[(wm * 64 + I * 16 + c) * KL_LD + ks * 4 + g];
#pragma unroll
      for (int J = 0; J < 2; ++J) b[J] = Ys[(wn * 32 + J * 16 + c) * KL_LD + ks * 4 + g];
#pragma unroll
      for (int I = 0; I < 4; ++I)
#pragma unroll
        for (int J = 0; J < 2; ++J) acc[I][J] = mfma(a[I], b[J], acc[I][J]);
    }
  }
  __syncthreads();
}

__global__ __launch_bounds__(512) void k_kl_frob(const double* __restrict__ covA, const double* __restrict__ precA,
                                                 const double* __restrict__ covB, const double* __restrict__ precB, int nA, int nB,
                                                 int T, int self, double* __restrict__ out) {
  __shared__ double Xs[KL_BT * KL_LD];
  __shared__ double Ys[KL_BT * KL_LD];
  const int bi = blockIdx.y, bj = blockIdx.x;
  if (self && bj < bi) return;   // mirrored from block (bj, bi)
  const long K = (long)T * T, i0 = (long)bi * KL_BT, j0 = (long)bj * KL_BT;
  d4 f1[4][2], f2[4][2];
#pragma unroll
  for (int I = 0; I < 4; ++I)
#pragma unroll
    for (int J = 0; J < 2; ++J) {
      f1[I][J] = d4{0.0, 0.0, 0.0, 0.0};
      f2[I][J] = d4{0.0, 0.0, 0.0, 0.0};
    }
  frob_term(covA, precB, K, i0, nA, j0, nB, Xs, Ys, f1);
  frob_term(precA, covB, K, i0, nA, j0, nB, Xs, Ys, f2);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const int wm = w & 1, wn = w >> 1;
  const double twoT = 2.0 * (double)T;
  const bool mirror = self && bj > bi;
#pragma unroll
  for (int I = 0; I < 4; ++I)
#pragma unroll
    for (int J = 0; J < 2; ++J)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const long i = i0 + wm * 64 + I * 16 + g + 4 * r, j = j0 + wn * 32 + J * 16 + c;
        if (i < nA && j < nB) {
          const double q = out[i * nB + j];
          const double v = 0.25 * ((f1[I][J][r] + f2[I][J][r]) - twoT) + 0.25 * q;
          out[i * nB + j] = v;
          if (mirror) out[j * nB + i] = v;
        }
      }
}

// mode 0: out[p, o] = q(p; o);  mode 1: out[o, p] += q(p; o);  q(p; o) = (mP_p - mO_o)^T P_p (mP_p - mO_o).
// self != 0: only the entries of the 128-blocks on and above the diagonal of `out` are produced.
__global__ __launch_bounds__(256) void k_kl_quad(const double* __restrict__ P, const double* __restrict__ mP, int nP,
                                                 const double* __restrict__ mO, int nO, int T, int mode, int self, int ldo,
                                                 double* __restrict__ out) {
  __shared__ double Ps[KL_QR * KL_LD];
  const int p = blockIdx.x;   // the state index rides the x dimension: no 65535 limit
  const long o_blk = (long)blockIdx.y * KL_QO;
  if (self) {
    const long pb = (p / KL_BT) * (long)KL_BT;
    if (mode == 0 ? (o_blk + KL_QO <= pb) : (o_blk >= pb + KL_BT)) return;
  }
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 15, g = lane >> 4;
  const double* __restrict__ Pp = P + (long)p * T * T;
  const double* __restrict__ mp = mP + (long)p * T;
  const double* mo[4];
  long o_of[4];
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) {
    o_of[ct] = o_blk + (w * 4 + ct) * 16 + c;
    const long oc = o_of[ct] < nO ? o_of[ct] : nO - 1;
    mo[ct] = mO + oc * T;
  }
  double part[4] = {0.0, 0.0, 0.0, 0.0};
  for (int R = 0; R < T; R += KL_QR) {
    d4 acc[4][4];
#pragma unroll
    for (int rb = 0; rb < 4; ++rb)
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) acc[rb][ct] = d4{0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < T; k0 += KL_KC) {
      __syncthreads();
#pragma unroll
      for (int e = 0; e < KL_QR * KL_KC / 256; ++e) {
        const int idx = e * 256 + tid, row = idx / KL_KC, col = idx % KL_KC;
        Ps[row * KL_LD + col] = (R + row < T && k0 + col < T) ? Pp[(long)(R + row) * T + k0 + col] : 0.0;
      }
      __syncthreads();
#pragma unroll
      for (int ks = 0; ks < KL_KC / 4; ++ks) {
        const int k = k0 + ks * 4 + g;
        double a[4], b[4];
        const bool in = k < T;
        const double mpk = in ? mp[k] : 0.0;
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) b[ct] = in ? mpk - mo[ct][k] : 0.0;
#pragma unroll
        for (int rb = 0; rb < 4; ++rb) a[rb] = Ps[(rb * 16 + c) * KL_LD + ks * 4 + g];
#pragma unroll
        for (int rb = 0; rb < 4; ++rb)
#pragma unroll
          for (int ct = 0; ct < 4; ++ct) acc[rb][ct] = mfma(a[rb], b[ct], acc[rb][ct]);
      }
    }
    // acc[rb][ct][r] = W[R + 16 rb + g + 4 r][o]:  q += D[t,o] W[t,o]
#pragma unroll
    for (int rb = 0; rb < 4; ++rb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int t = R + rb * 16 + g + 4 * r;
        if (t < T) {
          const double mpt = mp[t];
#pragma unroll
          for (int ct = 0; ct < 4; ++ct) part[ct] += (mpt - mo[ct][t]) * acc[rb][ct][r];
        }
      }
  }
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) {
    double q = part[ct];
    q += __shfl_xor(q, 16);
    q += __shfl_xor(q, 32);
    // a self call produces the entries of the 128-blocks on and above the diagonal only (k_kl_frob mirrors them): an entry
    // of a lower block is neither written by mode 0 nor touched by mode 1, so mode 1 never adds to an unwritten value
    const bool owned = !self || (mode == 0 ? o_of[ct] / KL_BT >= p / KL_BT : o_of[ct] / KL_BT <= p / KL_BT);
    if (g == 0 && o_of[ct] < nO && owned) {
      if (mode == 0) {
        out[(long)p * ldo + o_of[ct]] = q;
      } else {
        out[o_of[ct] * ldo + p] += q;
      }
    }
  }
}

}  // namespace

extern "C" int hgp_kl_sym_f64(const double* meanA, const double* covA, const double* precA, int nA, const double* meanB,
                              const double* covB, const double* precB, int nB, int T, double* out, void* stream) {
  const bool self = meanB == nullptr && covB == nullptr && precB == nullptr;
  if (!self && (!meanB || !covB || !precB)) return -1;
  if (self) nB = nA;
  if (nA < 0 || nB < 0 || T < 1) return -1;
  if (nA == 0 || nB == 0) return 0;
  if (!meanA || !covA || !precA || !out) return -1;
  if (self) {
    meanB = meanA;
    covB = covA;
    precB = precA;
  }
  hipStream_t st = (hipStream_t)stream;
  const int s = self ? 1 : 0;
  hipLaunchKernelGGL(k_kl_quad, dim3(nA, (nB + KL_QO - 1) / KL_QO), dim3(256), 0, st, precA, meanA, nA, meanB, nB, T, 0, s, nB, out);
  int rc = launch_status();
  if (rc) return rc;
  hipLaunchKernelGGL(k_kl_quad, dim3(nB, (nA + KL_QO - 1) / KL_QO), dim3(256), 0, st, precB, meanB, nB, meanA, nA, T, 1, s, nB, out);
  rc = launch_status();
  if (rc) return rc;
  hipLaunchKernelGGL(k_kl_frob, dim3((nB + KL_BT - 1) / KL_BT, (nA + KL_BT - 1) / KL_BT), dim3(512), 0, st, covA, precA, covB, precB,
                     nA, nB, T, s, out);
  return launch_status();
}
