// a2 for a batch of states on a query grid, mean and POINTWISE variance only: what IterativeGaussianProcess.pred_dist
// (GPI.py:457-503) returns as f_star and diag(cov_f), for every state s of a call and every query point q,
//
//   jitter_s = 1e-4 max(mean|diag Sigma_s|, eps),   K~_s = ker(x_b, x_b) + jitter_s I,   W = K~_s^-1 K*,   K* = ker(x_b, xq)
//   mean_q = W^T mean_s,     var_q = (c + noise) - sum_t K*[t,q] W[t,q] + sum_t W[t,q] (Sigma_s W)[t,q] + 1e-6
//   (diag Sigma_s isclose to its mean m:  var_q = m),
//
// without the [Q,Q] covariance or any [T,Q] intermediate ever reaching HBM.  Three launches whatever S and Q are:
//   1. k_bands_prep   one workgroup per state: jitter_s, the iso decision, K~_s into the workspace
//   2. the batched inverse factor Z_s = chol(K~_s)^-1 of the L^-1 family (hgp_inverse.hip), workspace to workspace
//   3. k_bands        one workgroup per (state, share of the query panels): per panel of 64 queries
//        E = K* (exp_neg4, registers -> LDS)        V  = Z E          W0 = Z^T V
//        R = E - K~ W0                              V2 = Z R          W  = W0 + Z^T V2      (one refinement step: the solve
//        SW = Sigma W                                                                         of _spd_solve, GPI.py of the mirror)
//      every product on v_mfma_f64_16x16x4_f64: wave w owns the row tiles w, w + 4, ... of the [T, 64] result in accumulator
//      registers, the B operand (the previous [T, 64] panel) sits in LDS in accumulator-tile order, the A operand (Z, K~, Sigma)
//      streams from L2 and every element of it feeds the four column tiles of the panel.  The three sums over t are taken from
//      the accumulator layout: per lane over its rows, xor-16 / xor-32 across the four row groups, then the four waves through LDS.
//
// Position independence: a query point's two outputs are reduced in one fixed order that depends on T alone - its column of
// every MFMA sees k ascending, the row sums run tile, register, row group, wave ascending - and on nothing else: not on Q, not
// on the point's position in xq or in its panel (all column slots run the same instruction sequence), not on S or the state's
// position in the call.  Nothing is split over workgroups or accumulated atomically.
#include <math.h>

#include "hgp_internal.hpp"
#include "panel_prod.hpp"
#include "tile_f64.hpp"

using namespace hgp;

namespace {

constexpr int BN_SC = 4;           // per-state scalars: jitter, mean(diag Sigma), iso, bad

struct BandArgs {
  const double* xb;
  int T, nb;
  const double* theta3;
  const double* mean;
  const double* Sigma;
  const int32_t* sigma_idx;
  int S;
  const double* xq;
  int Q;
  double* mean_q;
  double* var_q;
  int32_t* info;
  const double* Kt;     // [S,T,T]
  const double* Z;      // [S,T,T]
  const double* scal;   // [S,BN_SC]
  const int32_t* finfo; // [S] info of the factorisation
};

__global__ __launch_bounds__(256) void k_bands_prep(const double* __restrict__ xb, int T, const double* __restrict__ theta3,
                                                    const double* __restrict__ Sigma, const int32_t* __restrict__ sigma_idx,
                                                    double* __restrict__ Kt_all, double* __restrict__ scal) {
  __shared__ double red[2][256];
  const int s = blockIdx.x, tid = threadIdx.x;
  const long m = sigma_idx ? (long)sigma_idx[s] : (long)s;
  const double* __restrict__ Sg = Sigma + m * T * T;
  const double d = tid < T ? Sg[(long)tid * T + tid] : 0.0;   // T <= 256: one diagonal entry per thread
  red[0][tid] = d;
  red[1][tid] = fabs(d);
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) {
      red[0][tid] += red[0][tid + o];
      red[1][tid] += red[1][tid + o];
    }
    __syncthreads();
  }
  const double mS = red[0][0] / (double)T, am = red[1][0] / (double)T;
  const bool bad = !(am <= 1.79769313486231570815e308);   // NaN or infinite diagonal
  // torch.isclose defaults (GPI.py:497): |d - m| <= 1e-8 + 1e-5 |m| for every diagonal entry
  const int iso = __syncthreads_and(tid >= T || fabs(d - mS) <= 1e-8 + 1e-5 * fabs(mS));
  const double jitter = 1e-4 * fmax(am, F64_EPS);
  if (tid == 0) {
    scal[s * BN_SC + 0] = jitter;
    scal[s * BN_SC + 1] = mS;
    scal[s * BN_SC + 2] = iso ? 1.0 : 0.0;
    scal[s * BN_SC + 3] = bad ? 1.0 : 0.0;
  }
  const double c = theta3[3 * s], ell = theta3[3 * s + 1];
  double* __restrict__ Kt = Kt_all + (long)s * T * T;
  for (int idx = tid; idx < T * T; idx += 256) {
    const int i = idx / T, j = idx % T;
    const double u = xb[i] / ell - xb[j] / ell;   // scikit-learn divides by the length-scale first
    double v = c * exp(-0.5 * (u * u));
    if (i == j) v = c + jitter;                   // two-argument Gram (no white noise) + the state's jitter
    if (bad) v = (i == j) ? 1.0 : 0.0;            // nothing of a bad state is used; the factorisation still gets a matrix
    Kt[idx] = v;
  }
}

// The dynamic LDS of k_bands<RT>, sized by the run-time tile count nb <= 4 RT
template <int RT>
struct BandsLds {
  static constexpr int BN_CT = bands_ct(RT), BN_P = 16 * BN_CT;
  __host__ __device__ static constexpr int red_off(int nb) { return nb * BN_CT * 256; }   // doubles
  __host__ __device__ static constexpr size_t bytes(int nb) { return sizeof(double) * ((size_t)red_off(nb) + 3 * WAVES * BN_P); }
  static_assert(bytes(4 * RT) <= LDS_MAX_BYTES, "k_bands: LDS");
  __device__ static __forceinline__ double* Xs(double* smem) { return smem; }                          // [nb * BN_CT tiles][4][64]
  __device__ static __forceinline__ double* red(double* smem, int nb) { return smem + red_off(nb); }   // [3][WAVES][BN_P]
};

template <int RT>
__global__ __launch_bounds__(256) void k_bands(BandArgs a) {
  constexpr int BN_CT = bands_ct(RT), BN_P = 16 * BN_CT;   // queries per panel
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int T = a.T, nb = a.nb, Q = a.Q;
  double *Xs = BandsLds<RT>::Xs(smem), *red = BandsLds<RT>::red(smem, nb);
  const int s = blockIdx.x, tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int g = lane >> 4, c = lane & 15;
  const double mS = a.scal[s * BN_SC + 1];
  const bool iso = a.scal[s * BN_SC + 2] != 0.0, bad = a.scal[s * BN_SC + 3] != 0.0;
  const int fi = a.finfo[s];
  if (blockIdx.y == 0 && tid == 0) a.info[s] = bad ? -1 : fi;
  double* __restrict__ mq = a.mean_q + (long)s * Q;
  double* __restrict__ vq = a.var_q + (long)s * Q;
  if (bad || fi != 0) {   // failed factorisation: both rows of the state are NaN, nothing else is touched
    const double nan = __builtin_nan("");
    for (long q = (long)blockIdx.y * 256 + tid; q < Q; q += (long)gridDim.y * 256) {
      mq[q] = nan;
      vq[q] = nan;
    }
    return;
  }
  const double cs = a.theta3[3 * s], ell = a.theta3[3 * s + 1], noise = a.theta3[3 * s + 2];
  const long m = a.sigma_idx ? (long)a.sigma_idx[s] : (long)s;
  const double* __restrict__ Sg = a.Sigma + m * T * T;
  const double* __restrict__ Kt = a.Kt + (long)s * T * T;
  const double* __restrict__ Z = a.Z + (long)s * T * T;
  const double* __restrict__ mu = a.mean + (long)s * T;

  const int npanels = (Q + BN_P - 1) / BN_P;
  for (int p = blockIdx.y; p < npanels; p += gridDim.y) {
    const int q0 = p * BN_P;
    double xql[BN_CT];
#pragma unroll
    for (int ct = 0; ct < BN_CT; ++ct) {
      const int q = q0 + 16 * ct + c;
      xql[ct] = a.xq[q < Q ? q : Q - 1] / ell;
    }
    // K* tiles of the wave's rows: c exp(-0.5 u^2), rows beyond T are zero
    auto build_e = [&](d4 (&e)[RT][BN_CT]) {
#pragma unroll
      for (int i = 0; i < RT; ++i)
#pragma unroll
        for (int ct = 0; ct < BN_CT; ++ct) {
          double h[4], o[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int t = 16 * (wave + WAVES * i) + launder(g) + 4 * r;   // read next to its use: sixteen resident values per lane spill
            const double u = a.xb[t < T ? t : T - 1] / ell - xql[ct];
            h[r] = 0.5 * (u * u);
          }
          exp_neg4(h, o);
#pragma unroll
          for (int r = 0; r < 4; ++r) e[i][ct][r] = (16 * (wave + WAVES * i) + g + 4 * r < T) ? cs * o[r] : 0.0;
        }
    };
    d4 acc[RT][BN_CT], w[RT][BN_CT];
    build_e(acc);
    bands_publish<RT, BN_CT>(acc, Xs, nb, wave, lane);          // Xs = E
    bands_zero<RT, BN_CT>(acc);
    bands_prod<RT, BN_CT, 0, false>(Z, T, nb, Xs, wave, lane, acc);
    bands_publish<RT, BN_CT>(acc, Xs, nb, wave, lane);          // Xs = V = Z E
    bands_zero<RT, BN_CT>(w);
    bands_prod<RT, BN_CT, 1, false>(Z, T, nb, Xs, wave, lane, w);
    bands_publish<RT, BN_CT>(w, Xs, nb, wave, lane);            // Xs = W0 = Z^T V
    build_e(acc);
    bands_prod<RT, BN_CT, 2, true>(Kt, T, nb, Xs, wave, lane, acc);
    bands_publish<RT, BN_CT>(acc, Xs, nb, wave, lane);          // Xs = R = E - K~ W0
    bands_zero<RT, BN_CT>(acc);
    bands_prod<RT, BN_CT, 0, false>(Z, T, nb, Xs, wave, lane, acc);
    bands_publish<RT, BN_CT>(acc, Xs, nb, wave, lane);          // Xs = V2 = Z R
    bands_prod<RT, BN_CT, 1, false>(Z, T, nb, Xs, wave, lane, w);
    bands_publish<RT, BN_CT>(w, Xs, nb, wave, lane);            // Xs = W = W0 + Z^T V2
    // sum_t K* W and sum_t W mean, from the accumulator layout
    double pe[BN_CT], pm[BN_CT], ps[BN_CT];
    build_e(acc);
#pragma unroll
    for (int ct = 0; ct < BN_CT; ++ct) {
      pe[ct] = 0.0;
      pm[ct] = 0.0;
      ps[ct] = 0.0;
#pragma unroll
      for (int i = 0; i < RT; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int t = 16 * (wave + WAVES * i) + launder(g) + 4 * r;
          pe[ct] = fma(acc[i][ct][r], w[i][ct][r], pe[ct]);
          pm[ct] = fma(w[i][ct][r], t < T ? mu[t] : 0.0, pm[ct]);
        }
    }
    if (!iso) {   // uniform in the workgroup
      bands_zero<RT, BN_CT>(acc);
      bands_prod<RT, BN_CT, 2, false>(Sg, T, nb, Xs, wave, lane, acc);   // SW = Sigma W (the quadratic form sees Sigma's symmetric part)
#pragma unroll
      for (int ct = 0; ct < BN_CT; ++ct)
#pragma unroll
        for (int i = 0; i < RT; ++i)
#pragma unroll
          for (int r = 0; r < 4; ++r) ps[ct] = fma(w[i][ct][r], acc[i][ct][r], ps[ct]);
    }
#pragma unroll
    for (int ct = 0; ct < BN_CT; ++ct) {
      double v3[3] = {pe[ct], pm[ct], ps[ct]};
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        double v = v3[k];
        v += __shfl_xor(v, 16);
        v += __shfl_xor(v, 32);
        if (g == 0) red[(k * WAVES + wave) * BN_P + 16 * ct + c] = v;
      }
    }
    __syncthreads();   // also ends every wave's reads of Xs before the next panel's E is stored
    if (tid < BN_P && q0 + tid < Q) {
      double r3[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        double v = red[(k * WAVES + 0) * BN_P + tid];
#pragma unroll
        for (int ww = 1; ww < WAVES; ++ww) v += red[(k * WAVES + ww) * BN_P + tid];
        r3[k] = v;
      }
      mq[q0 + tid] = r3[1];
      vq[q0 + tid] = iso ? mS : (((cs + noise) - r3[0]) + r3[2]) + 1e-6;
    }
    // the next write to `red` lies behind the barriers of the next panel's products
  }
}

template <int RT>
int launch_bands(const BandArgs& a, hipStream_t st) {
  constexpr int BN_CT = bands_ct(RT), BN_P = 16 * BN_CT;
  const size_t lds = BandsLds<RT>::bytes(a.nb);
  if (int rc = hgp_internal_ensure_dynamic_lds(reinterpret_cast<const void*>(&k_bands<RT>), lds)) return rc;
  const int npanels = (a.Q + BN_P - 1) / BN_P;
  int ny = (768 + a.S - 1) / a.S;   // enough workgroups to fill the chip when the call holds few states
  ny = ny < 1 ? 1 : (ny > npanels ? npanels : ny);
  hipLaunchKernelGGL(k_bands<RT>, dim3(a.S, ny), dim3(256), lds, st, a);
  return launch_status();
}

// The caller's workspace of hgp_pred_bands_f64 (doubles), stated once for hgp_pred_bands_ws_bytes and the entry point
struct BandsWs {
  double *Kt, *Z, *work, *scal;   // K~ and its inverse factor [S,T,T]; the factor's scratch [S,T,T] (cooperative sizes only); [S,BN_SC]
  int32_t* finfo;                 // [S] info of the factorisation, in the room of S doubles
  static constexpr size_t tt(int S, int T) { return (size_t)S * T * T; }
  static constexpr size_t Kt_off(int, int) { return 0; }
  static constexpr size_t Z_off(int S, int T) { return Kt_off(S, T) + tt(S, T); }
  static constexpr size_t work_off(int S, int T) { return Z_off(S, T) + tt(S, T); }
  static constexpr size_t scal_off(int S, int T) { return work_off(S, T) + (T > HGP_MAX_T_WAVE ? tt(S, T) : 0); }
  static constexpr size_t finfo_off(int S, int T) { return scal_off(S, T) + (size_t)BN_SC * S; }
  static constexpr size_t bytes(int S, int T) { return sizeof(double) * (finfo_off(S, T) + S); }
  static BandsWs carve(void* ws, int S, int T) {
    double* w = static_cast<double*>(ws);
    return {w + Kt_off(S, T), w + Z_off(S, T), T > HGP_MAX_T_WAVE ? w + work_off(S, T) : nullptr, w + scal_off(S, T),
            reinterpret_cast<int32_t*>(w + finfo_off(S, T))};
  }
};
static_assert(BandsWs::bytes(7, 128) == 8 * (2 * 7 * 128 * 128 + 5 * 7) && BandsWs::bytes(7, 129) == 8 * (3 * 7 * 129 * 129 + 5 * 7),
              "hgp_pred_bands_f64: the workspace callers have sized so far");

}  // namespace

extern "C" size_t hgp_pred_bands_ws_bytes(int S, int T) { return S < 1 || T < 1 ? 0 : BandsWs::bytes(S, T); }

extern "C" int hgp_pred_bands_f64(const double* x_basis, int T, const double* theta3, const double* mean, const double* Sigma,
                                  const int32_t* sigma_idx, int S, const double* xq, int Q, double* mean_q, double* var_q,
                                  int32_t* info, void* ws, size_t ws_bytes, void* stream) {
  if (S < 0 || T < 1 || Q < 0) return -1;
  if (S == 0 || Q == 0) return 0;
  if (!x_basis || !theta3 || !mean || !Sigma || !xq || !mean_q || !var_q || !info || !ws) return -1;
  if (T > HGP_MAX_T_COOP) return -2;
  if (ws_bytes < BandsWs::bytes(S, T)) return -1;
  hipStream_t st = (hipStream_t)stream;
  const BandsWs w = BandsWs::carve(ws, S, T);
  hipLaunchKernelGGL(k_bands_prep, dim3(S), dim3(256), 0, st, x_basis, T, theta3, Sigma, sigma_idx, w.Kt, w.scal);
  int rc = launch_status();
  if (rc) return rc;
  rc = hgp_chol_inverse_ws_f64(w.Kt, T, S, 0.0, 0.0, w.Z, w.work, w.finfo, stream);
  if (rc) return rc;
  const int nb = (T + 15) / 16;
  BandArgs a{x_basis, T, nb, theta3, mean, Sigma, sigma_idx, S, xq, Q, mean_q, var_q, info, w.Kt, w.Z, w.scal, w.finfo};
  if (nb <= 4) return launch_bands<1>(a, st);
  if (nb <= 8) return launch_bands<2>(a, st);
  if (nb <= 12) return launch_bands<3>(a, st);
  return launch_bands<4>(a, st);
}
