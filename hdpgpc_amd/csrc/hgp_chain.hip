// SURVEY.md 8f-1, the per-member step of the LDS recursion with ONE launch per dependency level.
//
// The step (Kalman update, pair smoother, two MNIW updates; GPI.py:72-151,272-300, GPI_model.py:1300-1344) is ~30 small dense
// products at T = 90.  Measured (rocprofv3, record 100): every dependent launch costs ~4.5 us whatever it does - a 90^3
// product adds ~2 us of work on top - so the step's ~40 launches (one per product, plus element-wise glue) WERE its 0.28 ms.
// Here every dependency level is one launch of k_gemm_list: a device-resident list of heterogeneous items
//     C = alpha op(A) op(B) + beta D        (any M x N x K <= 256; vectors are N = 1; D may alias nothing or be a vector)
// with all pointers fixed for the life of the chain (the state rows of the step are gathered into one workspace first), and
// the two Cholesky inversions of the step carry their right-hand sides along (hgp_inverse.hip: Z = L^-1 and Y = L^-1 op(B) from
// one factorisation), which removes a product level behind each of them.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "hgp_internal.hpp"
#include "tile_f64.hpp"

using namespace hgp;

namespace {

// -------------------------------------------------------------------------------------------- list GEMM
// tile_map (may be NULL): tile_map[t] = (item << 16) | tile-within-item for the t-th output tile of the list.  Without it a
// wave finds its item by walking the list - one dependent global load per item, fine for the 1-5 items of one chain's level,
// 25 us for the 50 items of ten chains side by side.
__global__ __launch_bounds__(64 * WAVES) void k_gemm_list(const hgp_gemm_item* __restrict__ items, int n_items,
                                                          const uint32_t* __restrict__ tile_map, int total_tiles) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int g = lane >> 4, c = lane & 15;
  int tile = blockIdx.x * WAVES + wave;
  int it = 0;
  if (tile_map) {
    if (tile >= total_tiles) return;
    const uint32_t e = tile_map[tile];
    it = (int)(e >> 16);
    tile = (int)(e & 0xffffu);
  } else {
    for (; it < n_items; ++it) {           // which item does this wave's tile belong to?
      const int nt = ((items[it].M + 15) >> 4) * ((items[it].N + 15) >> 4);
      if (tile < nt) break;
      tile -= nt;
    }
    if (it >= n_items) return;
  }
  const hgp_gemm_item q = items[it];
  const int ntn = (q.N + 15) >> 4;
  const int ti = tile / ntn, tj = tile % ntn;
  const int row = 16 * ti + c, col = 16 * tj + c;
  d4 acc = (d4){0.0, 0.0, 0.0, 0.0};
  double dv[4] = {0.0, 0.0, 0.0, 0.0};   // the addend travels with the operands (behind the products it was one more round trip)
  if (q.D) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = 16 * ti + g + 4 * r;
      if (i < q.M && col < q.N) dv[r] = q.D[(size_t)i * q.ldd + col];
    }
  }
  const int nk = (q.K + 3) >> 2;
  constexpr int TRIP = 24;               // K <= 96 in one trip: all operand loads are in flight before the first MFMA
  for (int k0 = 0; k0 < nk; k0 += TRIP) {
    double av[TRIP], bv[TRIP];
#pragma unroll
    for (int u = 0; u < TRIP; ++u) {
      const int k = 4 * (k0 + u) + g;
      av[u] = 0.0;
      bv[u] = 0.0;
      if (k < q.K) {
        if (row < q.M) av[u] = q.tA ? q.A[(size_t)k * q.lda + row] : q.A[(size_t)row * q.lda + k];
        if (col < q.N) bv[u] = q.tB ? q.B[(size_t)col * q.ldb + k] : q.B[(size_t)k * q.ldb + col];
      }
    }
#pragma unroll
    for (int u = 0; u < TRIP; ++u) acc = mfma(av[u], bv[u], acc);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = 16 * ti + g + 4 * r;
    if (i < q.M && col < q.N) {
      double v = q.alpha * acc[r];
      if (q.D) v += q.beta * dv[r];
      if (q.add_eye && i == col) v += q.add_eye;
      q.C[(size_t)i * q.ldc + col] = v;
      if (q.C2) q.C2[(size_t)i * q.ldc + col] = v;
    }
  }
}

// -------------------------------------------------------------------------------------------- fused glue of the step
// gather (rows `pos` of the stacks -> workspace, the member's observation) + the jittered right covariances of the two MNIW
// updates  R' = R + 1e-2 max(mean |diag scale|, eps) I  (GPI_model.py:1312-1316), one launch.
using Gather2Args = hgp_chain_gather_desc;   // include/hdpgpc_hip.h

__device__ __forceinline__ void chain_gather2_body(const Gather2Args& a, double (&red)[2][4]) {
  const long tt = (long)a.T * a.T, p = a.pos[0];
  const long total = 6 * tt + 2 * a.T;
  // mean |diag scale| of both MNIW distributions, by every block (2 T strided loads, one LDS reduction)
  {
    double s0 = 0.0, s1 = 0.0;
    for (int d = threadIdx.x; d < a.T; d += 256) {
      s0 += fabs(a.W[4 * tt + (size_t)d * a.T + d]);
      s1 += fabs(a.W[5 * tt + (size_t)d * a.T + d]);
    }
    s0 = wave_sum(s0);
    s1 = wave_sum(s1);
    if ((threadIdx.x & 63) == 0) {
      red[0][threadIdx.x >> 6] = s0;
      red[1][threadIdx.x >> 6] = s1;
    }
    __syncthreads();
  }
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total + 2 * tt; i += (long)gridDim.x * 256) {
    if (i < total) {
      if (i < 6 * tt) {
        const int k = (int)(i / tt);
        a.out[i] = a.st[k][p * tt + (i - k * tt)];
      } else {
        const long j = i - 6 * tt;
        const int k = 6 + (int)(j / a.T);
        a.out[i] = a.st[k][p * a.T + (j % a.T)];
      }
      if (a.Y && i < a.T) a.y_out[i] = a.Y[(a.y_row0 < 0 ? 0 : p - a.y_row0) * a.T + i];   // y_row0 < 0: Y is the observation itself
    } else {
      const long e = i - total;                 // element of R' [2,T,T]
      const int mtx = (int)(e / tt);
      const long ij = e % tt;
      double v = a.W[2 * tt + e];               // R
      if (ij / a.T == ij % a.T) {
        const double s = ((red[mtx][0] + red[mtx][1]) + red[mtx][2]) + red[mtx][3];
        v += 1e-2 * fmax(s / a.T, F64_EPS);
      }
      a.Rp[e] = v;
    }
  }
}

// a BATCH of independent chains (one chain: n_chains = 1): blockIdx.y = chain, one descriptor per chain in device memory
__global__ __launch_bounds__(256) void k_chain_gather2_b(const Gather2Args* __restrict__ descs) {
  __shared__ double red[2][4];
  const Gather2Args a = descs[blockIdx.y];
  chain_gather2_body(a, red);
}

// scatter + finish: append the new filtered state, overwrite the re-smoothed previous one (GPI_model.py:317,705-716), the
// element-wise tail of both MNIW updates with (y1 - y2)(y1 - y2)^T formed here, the annealed scales, the append of
// A, Gamma, C, Sigma and the counters (GPI_model.py:1068-1106,1326-1336).
using Finish2Args = hgp_chain_finish_desc;   // include/hdpgpc_hip.h

#pragma clang fp contract(off)   // the reference's op order, no fused multiply-adds
__device__ __forceinline__ void chain_finish2_body(const Finish2Args& a, int& last) {
  const int T = a.T;
  const long tt = (long)T * T;
  // bit 3 = parameters frozen (the cluster reached its estimation limit, GPI_model.py:974,1092): the state rows as always, no
  // MNIW update - part, Snew, info1[2..3] and info2 may be stale: part and Snew are not read, and the four status words, which
  // come in with the other scalars of this preamble in ONE round of loads (a second, dependent round costs every step of every
  // chain about a microsecond), are ignored - and the four parameter rows copied forward, so that row pos + 1 of every stack
  // holds the last estimated parameters for whoever indexes the stacks by row
  const bool frozen = (a.annealing & 8) != 0;
  const bool bad = ((a.info1[2] | a.info1[3] | a.info2[0] | a.info2[1]) != 0) & !frozen;
  const double n0 = a.n0[0], Nf = a.Nf[0] + 1.0;
  const long p = a.pos[0], nxt = p + 1;
  const double n0n = bad ? n0 : n0 + 1.0;
  const double scl = n0n / (n0n - 2.0);
  const double ann = (a.annealing & 1) ? 1.0 / (Nf * Nf) : 0.0;
  // online path (hdpgpc_amd/online_chain.py): bit 1 = dry run - a CANDIDATE step: the new rows are written behind the chain's
  // end (row pos + 1) but the distributions W, the counters and the position stay as they are; bit 2 = the previous smoothed
  // state is not rewritten (a step without backwards_pair: the committed online step, GPI_HDP.py:2186-2196)
  const bool dry = (a.annealing & 2) != 0, keep_prev = (a.annealing & 4) != 0;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < 2 * tt; i += (long)gridDim.x * 256) {
    const bool obs = i >= tt;           // item 0 = internal (A, Gamma): (f_post, f_sm_prev); item 1 = observation (C, Sigma): (y, f_post)
    const long e = obs ? i - tt : i;
    const int r_ = (int)(e / T), c_ = (int)(e % T);
    double* sm = obs ? a.stC : a.stA;
    double* sg = obs ? a.stS : a.stG;
    if (frozen) {
      sm[nxt * tt + e] = sm[p * tt + e];
      sg[nxt * tt + e] = sg[p * tt + e];
    } else {
      double m = a.W[i], r = a.W[2 * tt + i], sc = a.W[4 * tt + i];
      if (!bad) {
        const double er = obs ? a.y[r_] - a.f_post[r_] : a.f_post[r_] - a.f_sm_prev[r_];
        const double ec = obs ? a.y[c_] - a.f_post[c_] : a.f_post[c_] - a.f_sm_prev[c_];
        m = ((n0 - 2.0) * m + a.part[i]) / (n0 - 1.0);
        r = a.Snew[i];
        sc = ((n0 - 2.0) * sc + er * ec) / (n0 - 1.0);
        if (!dry) {
          a.W[i] = m;
          a.W[2 * tt + i] = r;
          a.W[4 * tt + i] = sc;
        }
      }
      sm[nxt * tt + e] = m;
      sg[nxt * tt + e] = sc * scl + sg[e] * ann;
    }
    if (!obs) {                          // the state lists (scatter)
      const double cp = a.c_post[e];
      a.stP[nxt * tt + e] = cp;
      a.stPsm[nxt * tt + e] = cp;
      if (!keep_prev) a.stPsm[p * tt + e] = a.P_sm_prev[e];
      if (e < T) {
        const double f = a.f_post[e];
        a.stF[nxt * T + e] = f;
        a.stFsm[nxt * T + e] = f;
        if (!keep_prev) a.stFsm[p * T + e] = a.f_sm_prev[e];
      }
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    __threadfence();
    last = (atomicAdd(a.sync, 1) == (int)gridDim.x - 1);
  }
  __syncthreads();
  if (last && threadIdx.x == 0) {
    if (!dry) {
      if (!frozen) a.n0[0] = n0n;
      a.Nf[0] = Nf;
      a.pos[0] = nxt;
    }
    if (!frozen) a.bad_count[0] += bad ? 1 : 0;
    if (a.bad_count[1] == 0 && (a.info1[0] | a.info1[1]) != 0) a.bad_count[1] = (int32_t)nxt;
    a.sync[0] = 0;
  }
}

__global__ __launch_bounds__(256) void k_chain_finish2_b(const Finish2Args* __restrict__ descs) {
  __shared__ int last;
  const Finish2Args a = descs[blockIdx.y];
  chain_finish2_body(a, last);
}
#pragma clang fp contract(on)

// -------------------------------------------------------------------------------------------- list of copies
// The online step assembles the inputs of ONE batched a8 / a9 launch from rows of many clusters' stacks (three members per
// candidate, two parameter pairs): dozens of T- and T^2-sized copies as one launch instead of one hipMemcpyAsync each.
__global__ __launch_bounds__(256) void k_copy_list(const hgp_copy_item* __restrict__ items) {
  const hgp_copy_item q = items[blockIdx.y];
  const long n2 = q.n >> 1;                                   // pairs of doubles (src / dst 16-byte aligned when n is even)
  const bool vec = ((reinterpret_cast<uintptr_t>(q.src) | reinterpret_cast<uintptr_t>(q.dst)) & 15) == 0;
  if (vec) {
    const double2* s2 = reinterpret_cast<const double2*>(q.src);
    double2* d2 = reinterpret_cast<double2*>(q.dst);
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n2; i += (long)gridDim.x * 256) d2[i] = s2[i];
    if ((q.n & 1) && blockIdx.x == 0 && threadIdx.x == 0) q.dst[q.n - 1] = q.src[q.n - 1];
  } else {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < q.n; i += (long)gridDim.x * 256) q.dst[i] = q.src[i];
  }
}

// k_rts_chain: the sequential part of the RTS smoother (GPI.backward, GPI.py:240-270) for ALL steps in one launch.
// The gains J_t, the predictive covariances P_t and A_t m_t only depend on the filtered states and are batched by the
// caller; what remains is, for t = n-2 .. 0:
//     m_t <- m_t + J_t (m_{t+1} - A_t m_t),      C_t <- C_t + J_t (C_{t+1} - P_t) J_t^T.
// One workgroup of 12 waves walks the chain; wave w owns the output tiles w, w + 12, w + 24 of the 6 x 6 tile grid.
// What crosses a step stays on chip: the new C_t tiles are still in the registers of the wave that formed them when the
// next step needs them as C_{t+1} (D = C_{t+1} - P_t is formed tile-wise in registers and written to LDS), m_t sits in
// LDS; and everything the NEXT step reads from memory (J, P, C, A m, m of step t - 1: filtered quantities, independent of
// the recursion) is requested before the two product phases of the current step.  Per step: stage J and D in LDS (row
// pitch 100 doubles), X = J D on the matrix core (kept in registers until D is dead, then written over it), C_t + X J^T.
// The floor is the matrix core of ONE compute unit: 2 x 36 tiles x 24 MFMAs x 64 cycles / 4 SIMDs = 27.6 k cycles per step.
struct RtsArgs {
  const double* J;    // [n-1,T,T]
  const double* P;    // [n-1,T,T]
  const double* AM;   // [n-1,T]
  double* M;          // [n,T]   in/out
  double* Cv;         // [n,T,T] in/out
  int n, T;
};

constexpr int RTS_WAVES = 12;   // three waves per SIMD: the LDS operand latency of one hides under the MFMAs of the others

struct RtsLds {
  static constexpr int PITCH = 100;     // row pitch (doubles) of the two staged matrices
  static constexpr int JL = 0, DL = JL + 96 * PITCH, VL = DL + 96 * PITCH, ML = VL + 96, DOUBLES = ML + 96;
  static constexpr size_t BYTES = sizeof(double) * DOUBLES;
  static_assert(DL % 2 == 0 && BYTES <= LDS_MAX_BYTES, "k_rts_chain: LDS");
  HGP_LDS_DOUBLES(Jl, JL)   // [96][PITCH]
  HGP_LDS_DOUBLES(Dl, DL)   // [96][PITCH]  D, then X
  HGP_LDS_DOUBLES(vl, VL)   // [96]  m_{t+1} - A_t m_t
  HGP_LDS_DOUBLES(ml, ML)   // [96]  m_{t+1} (smoothed), then m_t
};

__global__ __launch_bounds__(64 * RTS_WAVES) void k_rts_chain(RtsArgs a) {
  constexpr int NBR = 6, PITCH = RtsLds::PITCH;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double *Jl = RtsLds::Jl(smem), *Dl = RtsLds::Dl(smem), *vl = RtsLds::vl(smem), *ml = RtsLds::ml(smem);
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, c = lane & 15;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int T = a.T;
  const long tt = (long)T * T;
  const int kpad = (T + 3) & ~3;          // k-steps beyond T multiply the zero padding
  for (int i = tid; i < 96 * PITCH; i += 64 * RTS_WAVES) {   // zero padding once (rows/cols >= T are never written below)
    Jl[i] = 0.0;
    Dl[i] = 0.0;
  }
  if (tid < 96) {
    vl[tid] = 0.0;
    ml[tid] = (tid < T) ? a.M[(size_t)(a.n - 1) * T + tid] : 0.0;
  }
  // my tiles (I, Jc) = (wave / 2, 3 (wave % 2) + i), i = 0 .. 2, of a row-major [T,T] matrix, accumulator layout, zero outside
  auto load_tiles = [&](const double* __restrict__ X, d4 (&v)[3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int I = wave >> 1, Jc = 3 * (wave & 1) + i;   // my three tiles share block row I (one A operand per k-step for three MFMAs)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 16 * I + g + 4 * r, col = 16 * Jc + c;
        v[i][r] = (row < T && col < T) ? X[(size_t)row * T + col] : 0.0;
      }
    }
  };
  // rows wave, wave + 12, ... of J (8 rows per wave), columns lane and lane + 64
  auto load_rows = [&](const double* __restrict__ X, double (&v)[8][2]) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int r = wave + RTS_WAVES * u;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int q = lane + 64 * h;
        v[u][h] = (r < T && q < T) ? X[(size_t)r * T + q] : 0.0;
      }
    }
  };
  d4 cn[3], pt[3], ct[3];
  double jv[8][2];
  double am = 0.0, mt = 0.0;
  load_tiles(a.Cv + (size_t)(a.n - 1) * tt, cn);          // C_{n-1}: the last filtered state is its own smoothed state
  {
    const int t = a.n - 2;
    load_rows(a.J + (size_t)t * tt, jv);
    load_tiles(a.P + (size_t)t * tt, pt);
    load_tiles(a.Cv + (size_t)t * tt, ct);
    if (tid < T) {
      am = a.AM[(size_t)t * T + tid];
      mt = a.M[(size_t)t * T + tid];
    }
  }
  __syncthreads();
  for (int t = a.n - 2; t >= 0; --t) {
    // ---- stage J_t (rows) and D = C_{t+1} - P_t (my tiles), v = m_{t+1} - A_t m_t
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int r = wave + RTS_WAVES * u;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int q = lane + 64 * h;
        if (r < T && q < T) Jl[r * PITCH + q] = jv[u][h];
      }
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int I = wave >> 1, Jc = 3 * (wave & 1) + i;   // my three tiles share block row I (one A operand per k-step for three MFMAs)
#pragma unroll
      for (int r = 0; r < 4; ++r) Dl[(16 * I + g + 4 * r) * PITCH + 16 * Jc + c] = cn[i][r] - pt[i][r];
    }
    const double mt_cur = mt;
    if (tid < T) vl[tid] = ml[tid] - am;
    __syncthreads();
    // ---- requests of step t - 1 (filtered quantities only): in flight under both product phases
    if (t > 0) {
      load_rows(a.J + (size_t)(t - 1) * tt, jv);
      load_tiles(a.P + (size_t)(t - 1) * tt, pt);
      if (tid < T) {
        am = a.AM[(size_t)(t - 1) * T + tid];
        mt = a.M[(size_t)(t - 1) * T + tid];
      }
    }
    // ---- X = J D
    d4 X[3];
    {
      const int I = wave >> 1, J0 = 3 * (wave & 1);
#pragma unroll
      for (int i = 0; i < 3; ++i) X[i] = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll 8
      for (int k = 0; k < kpad; k += 4) {
        const double av = Jl[(16 * I + c) * PITCH + k + g];
#pragma unroll
        for (int i = 0; i < 3; ++i) X[i] = mfma(av, Dl[(k + g) * PITCH + 16 * (J0 + i) + c], X[i]);
      }
    }
    // ---- m_t += J v : eight lanes per row, 12 columns each, summed inside the 8-lane group
    double mnew = 0.0;
    {
      const int row = tid >> 3, part = tid & 7;
      double sv = 0.0;
      if (row < T)
        for (int j = part; j < T; j += 8) sv = fma(Jl[row * PITCH + j], vl[j], sv);
      sv += __shfl_xor(sv, 1, 64);
      sv += __shfl_xor(sv, 2, 64);
      sv += __shfl_xor(sv, 4, 64);
      mnew = sv;                             // valid in the lanes with part == 0
    }
    __syncthreads();                         // every wave has finished reading D, v and m_{t+1}
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int I = wave >> 1, Jc = 3 * (wave & 1) + i;   // my three tiles share block row I (one A operand per k-step for three MFMAs)
#pragma unroll
      for (int r = 0; r < 4; ++r) Dl[(16 * I + g + 4 * r) * PITCH + 16 * Jc + c] = X[i][r];
    }
    if ((tid & 7) == 0 && (tid >> 3) < T) vl[tid >> 3] = mnew;        // J v, row-indexed (v is dead)
    __syncthreads();
    if (tid < T) {                           // m_t = (filtered m_t) + J v: out to memory, and kept for the next step
      const double m = mt_cur + vl[tid];
      ml[tid] = m;
      a.M[(size_t)t * T + tid] = m;
    }
    // ---- C_t = (filtered C_t) + X J^T : the result stays in cn for the next step
    double* Ct = a.Cv + (size_t)t * tt;
    {
      const int I = wave >> 1, J0 = 3 * (wave & 1);
#pragma unroll
      for (int i = 0; i < 3; ++i) cn[i] = ct[i];
#pragma unroll 8
      for (int k = 0; k < kpad; k += 4) {
        const double av = Dl[(16 * I + c) * PITCH + k + g];
#pragma unroll
        for (int i = 0; i < 3; ++i) cn[i] = mfma(av, Jl[(16 * (J0 + i) + c) * PITCH + k + g], cn[i]);
      }
#pragma unroll
      for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = 16 * I + g + 4 * r, col = 16 * (J0 + i) + c;
          if (row < T && col < T) Ct[(size_t)row * T + col] = cn[i][r];
        }
      }
    }
    if (t > 0) load_tiles(a.Cv + (size_t)(t - 1) * tt, ct);          // consumed one whole step later
    __syncthreads();                         // LDS free for the next step; m_t visible
  }
}

}  // namespace

extern "C" {

int hgp_copy_list_f64(const hgp_copy_item* items_dev, int n_items, long max_n, void* stream) {
  if (n_items == 0) return 0;
  if (!items_dev || n_items < 0 || n_items > 65535 || max_n <= 0) return -1;
  const long blocks = std::min<long>(64, (max_n / 2 + 255) / 256 + 1);
  hipLaunchKernelGGL(k_copy_list, dim3((unsigned)blocks, (unsigned)n_items), dim3(256), 0, (hipStream_t)stream, items_dev);
  return launch_status();
}

int hgp_gemm_list_f64(const hgp_gemm_item* items_dev, int n_items, int total_tiles, void* stream) {
  if (n_items == 0) return 0;
  if (!items_dev || n_items < 0 || total_tiles <= 0) return -1;
  hipLaunchKernelGGL(k_gemm_list, dim3((total_tiles + WAVES - 1) / WAVES), dim3(64 * WAVES), 0, (hipStream_t)stream, items_dev, n_items,
                     (const uint32_t*)nullptr, total_tiles);
  return launch_status();
}

int hgp_gemm_list_mapped_f64(const hgp_gemm_item* items_dev, int n_items, const uint32_t* tile_map_dev, int total_tiles, void* stream) {
  if (n_items == 0) return 0;
  if (!items_dev || !tile_map_dev || n_items < 0 || n_items > 65535 || total_tiles <= 0) return -1;
  hipLaunchKernelGGL(k_gemm_list, dim3((total_tiles + WAVES - 1) / WAVES), dim3(64 * WAVES), 0, (hipStream_t)stream, items_dev, n_items,
                     tile_map_dev, total_tiles);
  return launch_status();
}

int hgp_lds_chain_gather2_batched_f64(const hgp_chain_gather_desc* descs_dev, int n_chains, int T, void* stream) {
  if (n_chains == 0) return 0;
  if (!descs_dev || n_chains < 0 || T <= 0) return -1;
  const long total = 8L * T * T + 2L * T;
  // a grid-stride loop per chain: every block pays the two diagonal means (2 T strided loads + a barrier) before it copies, so a
  // block per 256 elements (2 050 blocks per chain at T = 256) spent more time there than copying: 288 us for 23 chains
  const long blocks = std::min<long>((total + 255) / 256, n_chains >= 8 ? 64 : 256);
  hipLaunchKernelGGL(k_chain_gather2_b, dim3((unsigned)blocks, (unsigned)n_chains), dim3(256), 0, (hipStream_t)stream, descs_dev);
  return launch_status();
}

int hgp_lds_chain_finish2_batched_f64(const hgp_chain_finish_desc* descs_dev, int n_chains, int T, void* stream) {
  if (n_chains == 0) return 0;
  if (!descs_dev || n_chains < 0 || T <= 0) return -1;
  const long n2 = 2L * T * T;
  hipLaunchKernelGGL(k_chain_finish2_b, dim3((unsigned)std::min<long>(64, (n2 + 255) / 256), (unsigned)n_chains), dim3(256), 0,
                     (hipStream_t)stream, descs_dev);
  return launch_status();
}


int hgp_rts_chain_f64(const double* J, const double* P, const double* AM, double* M, double* Cv, int n, int T, void* stream) {
  if (!J || !P || !AM || !M || !Cv || n < 0 || T <= 0) return -1;
  if (T > 96) return -2;
  if (n < 2) return 0;
  RtsArgs a{J, P, AM, M, Cv, n, T};
  const size_t lds = RtsLds::BYTES;
  if (int rc_ = hgp_internal_ensure_dynamic_lds(reinterpret_cast<const void*>(&k_rts_chain), lds)) return rc_;
  hipLaunchKernelGGL(k_rts_chain, dim3(1), dim3(64 * RTS_WAVES), lds, (hipStream_t)stream, a);
  return launch_status();
}

}  // extern "C"
