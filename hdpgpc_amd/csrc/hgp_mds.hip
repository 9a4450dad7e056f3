// The MDS embedding of a distance matrix for B start configurations at once (include/hdpgpc_hip_mds.h): metric
// SMACOF, what sklearn.manifold.MDS(dissimilarity='precomputed') runs on the host one start after the other.  One pass of ALL
// starts is two launches and nothing returns to the host between them:
//   1. k_mds_sweep    one workgroup per tile of MDS_ROWS rows of delta, one wave per row.  The running starts are taken
//                     MDS_SLOTS at a time; per group the workgroup walks the columns in chunks of MDS_COLS with X_k of the chunk
//                     staged in LDS, and every element delta_ij read from memory serves the whole group.  Per (row, start) a
//                     lane sums its columns j = lane, lane + 64, ... in ascending order, a fixed shuffle tree sums the 64
//                     lanes, and lane 0 writes row i of X_{k+1} and the row's partial sums of (d - delta)^2 and d^2.
//   2. k_mds_finish   one workgroup per start: the row partials in an order fixed by n (strided sums over 256 threads, then
//                     a fixed tree), the stop rule, and - where the start goes on - X <- X_{k+1}.
// A start is written by its own lanes only, the arithmetic of a slot does not depend on what the other slots hold, and no sum's
// order depends on B: the same bits for any B, any position in the batch, any split into calls.
#include <math.h>

#include "../../include/hdpgpc_hip_mds.h"
#include "hgp_internal.hpp"

namespace {

constexpr int MDS_ROWS = 4;      // rows per workgroup: one per wave
constexpr int MDS_COLS = 256;    // columns per LDS chunk
constexpr int MDS_SLOTS = 4;     // starts that share one read of delta
constexpr int MDS_K = 0, MDS_S1 = 1, MDS_S2 = 2, MDS_N1 = 3;   // state row: passes done, S_{k-1}, S_{k-2}, N_{k-1}, reserved

struct MdsArgs {
  const double* delta;
  int ld, n, B;
  double* X;             // [B,n,P] the current iterate
  double eps;
  int max_iter;
  double* state;
  int32_t* status;
  double* stress;
  int32_t* n_iter;
  double* Xn;            // [B,n,P] X_{k+1}
  double* part;          // [B,n,2] per row: sum_j (d - delta)^2, sum_j d^2
};

__device__ __forceinline__ double wave_sum(double v) {   // fixed tree over the 64 lanes, valid in lane 0
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

template <int P>
__global__ __launch_bounds__(64 * MDS_ROWS) void k_mds_sweep(MdsArgs a) {
#pragma clang fp contract(off)   // every product and sum below is written out: one rounding sequence for every slot
  __shared__ double xs[MDS_SLOTS][P][MDS_COLS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = a.n;
  const long i = (long)blockIdx.x * MDS_ROWS + wave;   // this wave's row (i >= n: the wave only helps staging)
  const bool row = i < n;
  const size_t np = (size_t)n * P;
  const double* __restrict__ drow = a.delta + (size_t)(row ? i : 0) * a.ld;
  const double inv_n = 1.0 / (double)n;

  int b = 0;
  while (true) {
    // the next MDS_SLOTS running starts, in batch order (uniform over the grid: status is not written by this launch)
    int bs[MDS_SLOTS], cnt = 0;
    for (; b < a.B && cnt < MDS_SLOTS; ++b)
      if (a.status[b] == 0) bs[cnt++] = b;
    if (cnt == 0) return;
    for (int s = cnt; s < MDS_SLOTS; ++s) bs[s] = bs[0];   // an empty slot repeats slot 0 and writes nothing

    double xi[MDS_SLOTS][P], acc[MDS_SLOTS][P], ss[MDS_SLOTS], sd[MDS_SLOTS];
#pragma unroll
    for (int s = 0; s < MDS_SLOTS; ++s) {
      ss[s] = 0.0;
      sd[s] = 0.0;
#pragma unroll
      for (int c = 0; c < P; ++c) {
        acc[s][c] = 0.0;
        xi[s][c] = a.X[(size_t)bs[s] * np + (size_t)(row ? i : 0) * P + c];
      }
    }
    for (long c0 = 0; c0 < n; c0 += MDS_COLS) {
      __syncthreads();   // the previous chunk (or group) has been read
      if (c0 + tid < n) {
#pragma unroll
        for (int s = 0; s < MDS_SLOTS; ++s)
#pragma unroll
          for (int c = 0; c < P; ++c) xs[s][c][tid] = a.X[(size_t)bs[s] * np + (size_t)(c0 + tid) * P + c];
      }
      __syncthreads();
      if (!row) continue;
#pragma unroll
      for (int m = 0; m < MDS_COLS / 64; ++m) {
        const int jl = lane + 64 * m;
        const long j = c0 + jl;
        if (j >= n) break;
        const double dl = drow[j];
#pragma unroll
        for (int s = 0; s < MDS_SLOTS; ++s) {
          double df[P], q = 0.0;
#pragma unroll
          for (int c = 0; c < P; ++c) {
            df[c] = xi[s][c] - xs[s][c][jl];
            q = c == 0 ? df[c] * df[c] : fma(df[c], df[c], q);
          }
          const double d = sqrt(q);
          const double r = dl / (d == 0.0 ? 1e-5 : d);
#pragma unroll
          for (int c = 0; c < P; ++c) acc[s][c] = fma(r, df[c], acc[s][c]);
          const double e = d - dl;
          ss[s] = fma(e, e, ss[s]);
          sd[s] = fma(d, d, sd[s]);
        }
      }
    }
    if (row) {
#pragma unroll
      for (int s = 0; s < MDS_SLOTS; ++s) {
        double v[P];
#pragma unroll
        for (int c = 0; c < P; ++c) v[c] = wave_sum(acc[s][c]);
        const double t0 = wave_sum(ss[s]), t1 = wave_sum(sd[s]);
        if (lane == 0 && s < cnt) {
#pragma unroll
          for (int c = 0; c < P; ++c) a.Xn[(size_t)bs[s] * np + (size_t)i * P + c] = v[c] * inv_n;
          a.part[((size_t)bs[s] * n + (size_t)i) * 2] = t0;
          a.part[((size_t)bs[s] * n + (size_t)i) * 2 + 1] = t1;
        }
      }
    }
  }
}

__global__ __launch_bounds__(256) void k_mds_finish(MdsArgs a, int P) {
#pragma clang fp contract(off)
  __shared__ double red[2][256];
  const int b = blockIdx.x, tid = threadIdx.x;
  if (a.status[b] != 0) return;   // frozen (uniform over the workgroup; read before the first barrier, written after the last)
  const size_t n = (size_t)a.n;
  const double* __restrict__ part = a.part + (size_t)b * n * 2;
  double s0 = 0.0, s1 = 0.0;
  for (size_t i = tid; i < n; i += 256) {
    s0 += part[2 * i];
    s1 += part[2 * i + 1];
  }
  red[0][tid] = s0;
  red[1][tid] = s1;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) {
      red[0][tid] += red[0][tid + o];
      red[1][tid] += red[1][tid + o];
    }
    __syncthreads();
  }
  const double S = red[0][0] / 2.0, N = red[1][0] / 2.0;
  double* __restrict__ st = a.state + (size_t)b * HGP_MDS_STATE_DOUBLES;
  const int k = (int)st[MDS_K];
  const double S1 = st[MDS_S1];
  const double big = 1.79769313486231570815e308;
  int end = 0;
  if (!(fabs(S) <= big) || !(fabs(N) <= big)) end = -2;
  else if (k >= 2 && (S1 - S) / N < a.eps) end = 1;   // _mds.py: (old_stress - stress) / (sum_squared_distances / 2) < eps
  else if (k >= a.max_iter) end = 2;
  if (end == 0) {
    const size_t np = n * P;
    const double* __restrict__ src = a.Xn + (size_t)b * np;
    double* __restrict__ dst = a.X + (size_t)b * np;
    for (size_t e = tid; e < np; e += 256) dst[e] = src[e];
  }
  __syncthreads();   // every thread has read the state row
  if (tid != 0) return;
  if (end == 0) {
    st[MDS_S2] = S1;
    st[MDS_S1] = S;
    st[MDS_N1] = N;
    st[MDS_K] = (double)(k + 1);
    return;
  }
  if (end > 0) {
    a.stress[b] = S;
    a.n_iter[b] = k;
  }
  a.status[b] = end;
}

// The caller's workspace of hgp_smacof_steps_f64 (doubles), stated once for hgp_smacof_ws_bytes and the entry point
struct MdsWs {
  double *Xn, *part;   // X_{k+1} of every start [B,n,p]; the two partial sums of every row of every start [B,n,2]
  static constexpr size_t Xn_off(int, int, int) { return 0; }
  static constexpr size_t part_off(int B, int n, int p) { return Xn_off(B, n, p) + (size_t)B * n * p; }
  static constexpr size_t bytes(int B, int n, int p) { return sizeof(double) * (part_off(B, n, p) + (size_t)B * n * 2); }
  static MdsWs carve(void* ws, int B, int n, int p) {
    double* w = static_cast<double*>(ws);
    return {w + Xn_off(B, n, p), w + part_off(B, n, p)};
  }
};
static_assert(MdsWs::bytes(4, 97, 3) == 8 * 4 * 97 * 5, "hgp_smacof_steps_f64: the workspace callers have sized so far");

}  // namespace

extern "C" size_t hgp_smacof_ws_bytes(int B, int n, int p) { return B < 1 || n < 1 || p < 1 ? 0 : MdsWs::bytes(B, n, p); }

extern "C" int hgp_smacof_steps_f64(const double* delta, int ld, int n, int p, int B, double* X, double eps, int n_steps, int max_iter,
                                    double* state, int32_t* status, double* stress, int32_t* n_iter, void* ws, size_t ws_bytes, void* stream) {
  if (n < 1 || p < 1 || p > 3 || B < 1 || n_steps < 0 || ld < n) return -1;
  if (!delta || !X || !state || !status || !stress || !n_iter || !ws) return -1;
  if (ws_bytes < MdsWs::bytes(B, n, p)) return -1;
  hipStream_t st = (hipStream_t)stream;
  const MdsWs w = MdsWs::carve(ws, B, n, p);
  MdsArgs a{delta, ld, n, B, X, eps, max_iter, state, status, stress, n_iter, w.Xn, w.part};
  const unsigned tiles = (unsigned)(((long)n + MDS_ROWS - 1) / MDS_ROWS);
  for (int s = 0; s < n_steps; ++s) {
    if (p == 1) hipLaunchKernelGGL(k_mds_sweep<1>, dim3(tiles), dim3(64 * MDS_ROWS), 0, st, a);
    else if (p == 2) hipLaunchKernelGGL(k_mds_sweep<2>, dim3(tiles), dim3(64 * MDS_ROWS), 0, st, a);
    else hipLaunchKernelGGL(k_mds_sweep<3>, dim3(tiles), dim3(64 * MDS_ROWS), 0, st, a);
    if (int rc = launch_status()) return rc;
    hipLaunchKernelGGL(k_mds_finish, dim3((unsigned)B), dim3(256), 0, st, a, p);
    if (int rc = launch_status()) return rc;
  }
  return 0;
}
