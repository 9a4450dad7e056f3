// Draws from the Gaussians of a batch of states: what GPI_model.sample_last (GPI_model.py:953-961) and
// IterativeGaussianProcess.sample_y (GPI.py:564-608) take from numpy's multivariate_normal, as the map from standard normals
//
//   A_s = 0.5 (cov_m + cov_m^T) + jitter_rel mean|diag cov_m| I,   m = cov_idx[s],      A_s = L_s L_s^T,
//   out[s, j, :] = mean[s, :] + L_s z_j
//
// for every state s of a call and every draw j.  Two launches whatever S and n are:
//   1. the batched factor of the Cholesky family (hgp_factor.hip), input stack to workspace: L_s, info
//   2. k_sample   one workgroup per (state, share of the draw panels): per panel of 64 (32 above T = 128) draws
//        Zp = the panel's normals, draws as columns (registers -> LDS, accumulator-tile order)
//        acc = mean (every column) + L Zp     on v_mfma_f64_16x16x4_f64 (panel_prod.hpp): wave w owns the row tiles w, w + 4, ...,
//                                             L streams from L2, k tiles <= the row tile only, the diagonal tile masked to its
//                                             lower triangle in the loader
//        out  <- acc, transposed per 16 x 16 tile through a per-wave LDS tile: 16 lanes write the 128 contiguous bytes of
//                one draw's 16 values
//
// Position independence: a draw's T outputs see k ascending in every MFMA column slot, the same instruction sequence in every
// slot, seeded with the mean; nothing depends on n, on the draw's position in z or in its panel, on S, on the state's position
// or on z_shared.  Nothing is split over workgroups or accumulated atomically.
#include <math.h>

#include "hgp_internal.hpp"
#include "panel_prod.hpp"
#include "tile_f64.hpp"

using namespace hgp;

namespace {

constexpr int STG_LD = 17;             // row stride (doubles) of the per-wave 16 x 16 staging tile: its ds_write_b64 goes out in groups
constexpr int STG = 16 * STG_LD;       // of 16 lanes (one row group g, sixteen draws c): 34 c mod 32 dwords = conflict-free

struct SampleArgs {
  const double* mean;       // [S,T]
  const double* cov;        // [*,T,T]: only its diagonal is read here (non-finite input)
  const int32_t* cov_idx;   // [S] or NULL
  int T, nb, S;
  const double* z;          // [n,T] (zstride 0) or [S,n,T]
  int n;
  long zstride;
  double* out;              // [S,n,T]
  int32_t* info;            // [S]
  const double* L;          // [S,T,T] the factors
  const int32_t* finfo;     // [S] info of the factorisation
};

// The dynamic LDS of k_sample<RT>, sized by the run-time tile count nb <= 4 RT
template <int RT>
struct SampleLds {
  static constexpr int BN_CT = bands_ct(RT);
  __host__ __device__ static constexpr int stg_off(int nb) { return nb * BN_CT * 256; }   // doubles
  __host__ __device__ static constexpr size_t bytes(int nb) { return sizeof(double) * ((size_t)stg_off(nb) + WAVES * STG); }
  static_assert(bytes(4 * RT) <= LDS_MAX_BYTES, "k_sample: LDS");
  __device__ static __forceinline__ double* Xs(double* smem) { return smem; }                          // [nb * BN_CT tiles][4][64]
  __device__ static __forceinline__ double* stg(double* smem, int nb) { return smem + stg_off(nb); }   // [WAVES][STG]: one staging tile per wave
};

template <int RT>
__global__ __launch_bounds__(256) void k_sample(SampleArgs a) {
  constexpr int BN_CT = bands_ct(RT), BN_P = 16 * BN_CT;   // draws per panel
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int T = a.T, nb = a.nb, n = a.n;
  const int s = blockIdx.x, tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int g = lane >> 4, c = lane & 15;
  double* Xs = SampleLds<RT>::Xs(smem);
  double* stg = SampleLds<RT>::stg(smem, nb) + wave * STG;   // this wave's staging tile
  const long m = a.cov_idx ? (long)a.cov_idx[s] : (long)s;
  const double d = tid < T ? a.cov[(m * T + tid) * T + tid] : 0.0;   // T <= 256: one diagonal entry per thread
  const int bad = __syncthreads_or(!(fabs(d) <= 1.79769313486231570815e308));   // NaN or infinite diagonal
  const int fi = a.finfo[s];
  if (blockIdx.y == 0 && tid == 0) a.info[s] = bad ? -1 : fi;
  double* __restrict__ out = a.out + (long)s * n * T;
  if (bad || fi != 0) {   // failed factorisation: every draw of the state is NaN, nothing else is touched
    const double nan = __builtin_nan("");
    for (long i = (long)blockIdx.y * 256 + tid; i < (long)n * T; i += (long)gridDim.y * 256) out[i] = nan;
    return;
  }
  const double* __restrict__ L = a.L + (long)s * T * T;
  const double* __restrict__ mu = a.mean + (long)s * T;
  const double* __restrict__ z = a.z + (long)s * a.zstride;

  const int npanels = (n + BN_P - 1) / BN_P;
  for (int p = blockIdx.y; p < npanels; p += gridDim.y) {
    const int j0 = p * BN_P;
    d4 acc[RT][BN_CT];
    // the panel's normals as accumulator tiles, X[t][j] = z[j][t]: lane (g, c) reads the 32 contiguous bytes t = 4 r + g of draw c,
    // r = 0 .. 3 cover the draw's 128-byte line.  Rows beyond T and draws beyond n are zero.
#pragma unroll
    for (int i = 0; i < RT; ++i)
#pragma unroll
      for (int ct = 0; ct < BN_CT; ++ct) {
        const int j = j0 + 16 * ct + launder(c);
        const double* __restrict__ zj = z + (long)(j < n ? j : n - 1) * T;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int t = 16 * (wave + WAVES * i) + g + 4 * r;
          const double v = zj[t < T ? t : T - 1];
          acc[i][ct][r] = (t < T && j < n) ? v : 0.0;
        }
      }
    bands_publish<RT, BN_CT>(acc, Xs, nb, wave, lane);          // Xs = Zp
#pragma unroll
    for (int i = 0; i < RT; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int t = 16 * (wave + WAVES * i) + launder(g) + 4 * r;
        const double v = t < T ? mu[t] : 0.0;
#pragma unroll
        for (int ct = 0; ct < BN_CT; ++ct) acc[i][ct][r] = v;
      }
    bands_prod<RT, BN_CT, 0, false, true>(L, T, nb, Xs, wave, lane, acc);   // acc = mean + L Zp
    // out[j][16 I ..] <- acc[i][ct]: tile (row t = g + 4 r, draw c) through the staging tile, read back with the 16 lanes of a
    // row group along t
#pragma unroll
    for (int i = 0; i < RT; ++i) {
      const int I = wave + WAVES * i;
      if (I >= nb) continue;
#pragma unroll
      for (int ct = 0; ct < BN_CT; ++ct) {
        const int ln = launder(lane);
        const int gg = ln >> 4, cc = ln & 15;
#pragma unroll
        for (int r = 0; r < 4; ++r) stg[cc * STG_LD + gg + 4 * r] = acc[i][ct][r];
        __builtin_amdgcn_wave_barrier();
        const int t = 16 * I + cc;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int dl = 4 * q + gg, j = j0 + 16 * ct + dl;
          const double v = stg[dl * STG_LD + cc];
          if (j < n && t < T) out[(long)j * T + t] = v;
        }
        __builtin_amdgcn_wave_barrier();
      }
    }
    // the next panel's stores to Xs lie behind the barrier of its bands_publish
  }
}

template <int RT>
int launch_sample(const SampleArgs& a, hipStream_t st) {
  constexpr int BN_CT = bands_ct(RT), BN_P = 16 * BN_CT;
  const size_t lds = SampleLds<RT>::bytes(a.nb);
  if (int rc = hgp_internal_ensure_dynamic_lds(reinterpret_cast<const void*>(&k_sample<RT>), lds)) return rc;
  const int npanels = (a.n + BN_P - 1) / BN_P;
  int ny = (768 + a.S - 1) / a.S;   // enough workgroups to fill the chip when the call holds few states
  ny = ny < 1 ? 1 : (ny > npanels ? npanels : ny);
  hipLaunchKernelGGL(k_sample<RT>, dim3(a.S, ny), dim3(256), lds, st, a);
  return launch_status();
}

// The caller's workspace of hgp_sample_states_f64 (doubles), stated once for hgp_sample_states_ws_bytes and the entry point
struct SampleWs {
  double* L;        // the factors [S,T,T]
  int32_t* finfo;   // [S] their status, in the room of S doubles
  static constexpr size_t L_off(int, int) { return 0; }
  static constexpr size_t finfo_off(int S, int T) { return L_off(S, T) + (size_t)S * T * T; }
  static constexpr size_t bytes(int S, int T) { return sizeof(double) * (finfo_off(S, T) + S); }
  static SampleWs carve(void* ws, int S, int T) {
    double* w = static_cast<double*>(ws);
    return {w + L_off(S, T), reinterpret_cast<int32_t*>(w + finfo_off(S, T))};
  }
};
static_assert(SampleWs::bytes(7, 129) == 8 * (7 * 129 * 129 + 7), "hgp_sample_states_f64: the workspace callers have sized so far");

}  // namespace

extern "C" size_t hgp_sample_states_ws_bytes(int S, int T) { return S < 1 || T < 1 ? 0 : SampleWs::bytes(S, T); }

extern "C" int hgp_sample_states_f64(const double* mean, const double* cov, const int32_t* cov_idx, int T, int S, const double* z,
                                     int n, int z_shared, double jitter_rel, double* out, int32_t* info, void* ws, size_t ws_bytes,
                                     void* stream) {
  if (S < 0 || T < 1 || n < 0) return -1;
  if (S == 0 || n == 0) return 0;
  if (!mean || !cov || !z || !out || !info || !ws) return -1;
  if (T > HGP_MAX_T_COOP) return -2;
  if (ws_bytes < SampleWs::bytes(S, T)) return -1;
  hipStream_t st = (hipStream_t)stream;
  const SampleWs w = SampleWs::carve(ws, S, T);
  if (int rc = hgp_internal_potrf_ws(cov, cov_idx, T, S, jitter_rel, w.L, w.finfo, st)) return rc;
  const int nb = (T + 15) / 16;
  SampleArgs a{mean, cov, cov_idx, T, nb, S, z, n, z_shared ? 0L : (long)n * T, out, info, w.L, w.finfo};
  if (nb <= 4) return launch_sample<1>(a, st);
  if (nb <= 8) return launch_sample<2>(a, st);
  if (nb <= 12) return launch_sample<3>(a, st);
  return launch_sample<4>(a, st);
}
