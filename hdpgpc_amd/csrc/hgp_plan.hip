// The pairs plan: the per-cluster operators of the explicit-operator pair kernels (hgp_pairs.hip) and of the solve-based kernel
// (hgp_pairs_acc.hip), the layout of the plan's device buffer, the C-ABI of the plan and of hgp_loglik_pairs_f64 / hgp_loglik_pairs_ragged_f64, and the one driver of a pair-scoring call
// (hgp_internal_pairs_score: kernel arguments, launch order, the walk in slices of PAIRS_FB_CAP segments) behind every entry.
//
// hgp_pairs_plan_update, TP <= 128:  k_prep_build (K~, S, scalars) -> inverse factor Z = L^-1 (hgp_inverse.hip) -> k_plan_ops<NB>
// (M', a', ||K~^-1||_inf and the routing flags in ONE launch: every workgroup recomputes from Z the strips of Kinv = Z^T Z,
// P = S Kinv and the two tiles of Q = Kinv P its tile pair of M' needs; P and Q never reach memory) -> the operands of the
// solve-based kernel for the flagged clusters (hgp_internal_acc_prep).  K~, Z and Kinv of cluster k depend on the grid, theta and
// the jitter 1e-4 mean|diag Sigma_k| alone: a cluster for which k_prep_build finds all of them unchanged, bit for bit, keeps them
// (PlanReuse in hgp_internal.hpp) - no Gram build, its inverse workgroups leave at once, k_plan_ops reads its Kinv tiles from d_Kinv.
// TP = 192, 256:  k_prep_build -> cooperative factor + inverse -> 3 x k_gemm (Kinv, P, Q in memory) -> k_prep_final -> k_acc_flags
// -> operands (d_A holds L there, and the strips do not fit LDS).
#include <algorithm>
#include <new>

#include "../../include/hdpgpc_hip_ragged.h"
#include "hgp_internal.hpp"
#include "tile_f64.hpp"

using namespace hgp;

namespace {

// ------------------------------------------------------------------ per-cluster operators (plan)
// scal[k*8 + ..] : 0 c, 1 ell, 2 noise, 3 iso flag, 4 mean(diag Sigma), 5 jitter of K~, 6 ||K~^{-1}||_inf
struct PrepArgs {
  const double* xb;
  const double* mean;
  const double* Sigma;
  int T, TP, K;
  const double* theta;  // [K,3] device copy
  double* scal;         // [K,8]
  double* A;            // [K,TP,TP] K~ (identity padded)
  double* S;            // [K,TP,TP] 0.5 (Sigma + Sigma^T) (zero padded)
  double* xb_copy;      // [TP]
  // TP <= 128 (reuse.same != NULL): K~ of a cluster whose grid and jitter have the bits of the call that computed it is not rebuilt,
  // and xb_copy, only compared here, is written by k_plan_ops (no workgroup of this launch reads it while another writes it)
  PlanReuse reuse;
  int32_t* info;        // the caller's status array (or NULL): a kept cluster reports the status of the call that factored it
};

__global__ __launch_bounds__(256) void k_prep_build(PrepArgs a) {
  __shared__ double red[256];
  __shared__ int redi[256];
  const int k = blockIdx.x, tid = threadIdx.x;
  const int T = a.T, TP = a.TP;
  const double* Sg = a.Sigma + (size_t)k * T * T;
  const double c = a.theta[3 * k], ell = a.theta[3 * k + 1], noise = a.theta[3 * k + 2];
  double s_abs = 0.0, s_sgn = 0.0;
  for (int i = tid; i < T; i += 256) {
    double d = Sg[(size_t)i * T + i];
    s_abs += fabs(d);
    s_sgn += d;
  }
  red[tid] = s_abs;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  const double mean_abs = red[0] / T;
  __syncthreads();
  red[tid] = s_sgn;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  const double mS = red[0] / T;
  int bad = 0;
  for (int i = tid; i < T; i += 256) {
    double d = Sg[(size_t)i * T + i];
    if (!(fabs(d - mS) <= 1e-8 + 1e-5 * fabs(mS))) bad = 1;   // torch.isclose defaults (GPI.py:497)
  }
  const bool reuse = a.reuse.same != nullptr;
  if (reuse) {
    // bit 1: the incoming grid is not, bit for bit, the one the kept operators were computed for (compared as integers:
    // -0.0 differs from +0.0, a NaN pattern equals itself)
    const long long* xn = reinterpret_cast<const long long*>(a.xb);
    const long long* xo = reinterpret_cast<const long long*>(a.xb_copy);
    for (int i = tid; i < T; i += 256)
      if (xn[i] != xo[i]) bad |= 2;
  }
  redi[tid] = bad;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) redi[tid] |= redi[tid + o];
    __syncthreads();
  }
  const double jit = 1e-4 * fmax(mean_abs, F64_EPS);           // GPI.py:488
  // Every workgroup of the cluster takes the same decision from words that no workgroup of this launch changes under it: valid
  // is only ever cleared here, and only when the decision is "differs" whatever valid reads; key_jit and xb_copy belong to k_plan_ops.
  const bool same = reuse && (redi[0] & 2) == 0 && a.reuse.valid[k] != 0 && a.reuse.key_jit[k] == __double_as_longlong(jit);
  if (tid == 0 && blockIdx.y == 0) {
    double* sc = a.scal + 8 * k;
    sc[0] = c;
    sc[1] = ell;
    sc[2] = noise;
    sc[3] = (redi[0] & 1) ? 0.0 : 1.0;
    sc[4] = mS;
    sc[5] = jit;
    sc[6] = 0.0;   // ||K~^{-1}||_inf: accumulated by k_prep_final / k_plan_ops with an atomic maximum
    if (reuse) {
      a.reuse.same[k] = same ? 1 : 0;
      if (same) {
        if (a.info) a.info[k] = a.reuse.info[k];
      } else {
        a.reuse.valid[k] = 0;      // until the last workgroup of k_plan_ops has seen every store of this call
        a.reuse.factored[k] = 0;   // d_A is K~ again
      }
    }
  }
  if (!reuse && k == 0 && blockIdx.y == 0)
    for (int i = tid; i < TP; i += 256) a.xb_copy[i] = (i < T) ? a.xb[i] : 0.0;
  double* Ak = a.A + (size_t)k * TP * TP;
  double* Sk = a.S + (size_t)k * TP * TP;
  if (same) {   // K~ (or its factor, where k_acc_factor has run) stands: S alone
    for (int idx = blockIdx.y * 256 + tid; idx < TP * TP; idx += gridDim.y * 256) {
      int i = idx / TP, j = idx % TP;
      double sv = 0.0;
      if (i < T && j < T) sv = 0.5 * (Sg[(size_t)i * T + j] + Sg[(size_t)j * T + i]);
      Sk[idx] = sv;
    }
    return;
  }
  for (int idx = blockIdx.y * 256 + tid; idx < TP * TP; idx += gridDim.y * 256) {
    int i = idx / TP, j = idx % TP;
    double av, sv = 0.0;
    if (i < T && j < T) {
      double u = a.xb[i] / ell - a.xb[j] / ell;
      av = c * exp(-0.5 * (u * u));
      if (i == j) av += jit;
      sv = 0.5 * (Sg[(size_t)i * T + j] + Sg[(size_t)j * T + i]);
    } else {
      av = (i == j) ? 1.0 : 0.0;
    }
    Ak[idx] = av;
    Sk[idx] = sv;
  }
}

// M'[i][j] = c^2 (sym(Q) - sym(Kinv))[i][j], Q = Kinv S Kinv.  Stated once: k_prep_final and k_plan_ops compile the same expression.
__device__ __forceinline__ double plan_mp_value(double c, double qij, double qji, double kij, double kji) {
  return (c * c) * (0.5 * (qij + qji) - 0.5 * (kij + kji));
}
// Column order of M' (logical j -> physical jp).  The pairs kernel reads row k of M' as the A operands of the NH
// row tiles of one half h (tiles NH h .. NH h + NH - 1): inside a half, tiles are interleaved two by two so that ONE
// 16-byte load per lane (lane cc) yields the operands of tiles 2q and 2q + 1; an odd last tile stays contiguous.
__device__ __forceinline__ int plan_mp_col(int j, int NHh) {
  const int hh = j / (16 * NHh), tl = (j / 16) % NHh, cc = j % 16;
  const int loc = (tl < 2 * (NHh / 2)) ? 32 * (tl / 2) + 2 * cc + (tl & 1) : 16 * (NHh - 1) + cc;
  return 16 * NHh * hh + loc;
}

struct PrepFinalArgs {
  const double* Q;      // Kinv * S * Kinv
  const double* Kinv;
  const double* mean;   // [K,T]
  double* scal;
  int T, TP;
  double* Mp;           // [K,TP,TP]
  double* ap;           // [K,TP]
  int interleave;       // 1: tile-pair interleaved columns (fused pairs kernel); 0: plain row-major (cooperative pairs kernel)
  int32_t* fb;          // fall-back list of k_pairs: its two counters start every plan state at zero (a killed launch cannot leave them set)
};

__global__ __launch_bounds__(256) void k_prep_final(PrepFinalArgs a) {
  const int k = blockIdx.x, tid = threadIdx.x;
  if (a.fb && k == 0 && blockIdx.y == 0 && tid == 0) {
    a.fb[0] = 0;
    a.fb[1 + PAIRS_FB_CAP] = 0;
  }
  const int T = a.T, TP = a.TP;
  const double c = a.scal[8 * k];
  const double* Q = a.Q + (size_t)k * TP * TP;
  const double* Ki = a.Kinv + (size_t)k * TP * TP;
  double* Mp = a.Mp + (size_t)k * TP * TP;
  // M' = c^2 (sym(Q) - sym(Kinv)) by 32 x 32 tiles: tile (bi, bj) and its mirror (bj, bi) are both read row-wise
  // (coalesced) and the mirror is transposed through LDS (pitch 33).  Column order: plan_mp_col.
  __shared__ double tq[32][33], tk[32][33];
  const int NHh = (TP / 16) / 2, nt = TP / 32;
  const int tx = tid & 31, ty = tid >> 5;   // 32 x 8 threads, 4 rows each
  for (int t = blockIdx.y; t < nt * nt; t += gridDim.y) {
    const int bi = t / nt, bj = t % nt;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) {   // mirror tile, natural order: element (32 bj + y, 32 bi + tx)
      const int y = ty + 8 * r;
      tq[y][tx] = Q[(size_t)(32 * bj + y) * TP + 32 * bi + tx];
      tk[y][tx] = Ki[(size_t)(32 * bj + y) * TP + 32 * bi + tx];
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int y = ty + 8 * r;
      const int i = 32 * bi + y, j = 32 * bj + tx;
      double v = 0.0;
      if (i < T && j < T) v = plan_mp_value(c, Q[(size_t)i * TP + j], tq[tx][y], Ki[(size_t)i * TP + j], tk[tx][y]);
      const int jp = a.interleave ? plan_mp_col(j, NHh) : j;
      Mp[(size_t)i * TP + jp] = v;
    }
  }
  // a' = c Kinv mean and the row sums of |Kinv| (rows dealt to the gridDim.y blocks of the cluster)
  const double* mu = a.mean + (size_t)k * T;
  __shared__ double red[256];
  double rmax = 0.0;
  for (int i = blockIdx.y * 256 + tid; i < TP; i += gridDim.y * 256) {
    double s = 0.0, rs = 0.0;
    if (i < T) {
#pragma unroll 8
      for (int j = 0; j < T; ++j) {
        const double kij = Ki[(size_t)j * TP + i];   // K~^{-1} = Z^T Z is symmetric: read column-wise, coalesced
        s = fma(kij, mu[j], s);
        rs += fabs(kij);
      }
    }
    a.ap[(size_t)k * TP + i] = c * s;
    rmax = fmax(rmax, rs);
  }
  red[tid] = rmax;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) red[tid] = fmax(red[tid], red[tid + o]);
    __syncthreads();
  }
  // ||K~^{-1}||_inf >= ||K~^{-1}||_2: maximum over the blocks (non-negative doubles order like their bit patterns;
  // k_prep_build zeroes the slot)
  if (tid == 0) atomicMax(reinterpret_cast<unsigned long long*>(a.scal + 8 * k + 6), (unsigned long long)__double_as_longlong(red[0]));
}

// ------------------------------------------------------------------ one launch behind the inverse (TP <= 128)
// M', a', ||K~^-1||_inf and the routing flags from Z = L^-1, without P or Q in global memory (Kinv: written, not read).  One workgroup per
// (cluster k, tile pair I < J) recomputes what its two output tiles M'[I][J], M'[J][I] depend on:
//   Kinv[:, I], Kinv[:, J] (block columns) and Kinv[I, :], Kinv[J, :] (block rows) from Z   - the chains of Kinv = Z^T Z,
//   P[:, I] = S Kinv[:, I], P[:, J]                                                         - the chains of P = S Kinv,
//   Q_IJ = Kinv[I, :] P[:, J], Q_JI = Kinv[J, :] P[:, I]                                    - the chains of Q = Kinv P,
// every tile by ONE accumulator over ascending k-steps of 4 (exactly k_gemm's order: the operators keep their bits).  The
// redundant MFMAs cost nothing: the chip is otherwise idle.  A block row is never taken as the transpose of a block column
// (nothing here relies on Z^T Z being symmetric bit for bit).  The diagonal tile (I, I) needs the strips of block I only, so
// the workgroup of pair (I, I+1) makes it as well (one more Q tile), with a'[16 I ..] and the row sums of |Kinv|; the last
// pair also serves block NB-1.  K NB (NB-1)/2 workgroups: 224 at K = 8, NB = 8 - one round on 256 CUs.  The last of those
// workgroups to finish (an atomic counter behind a fence: nobody waits for anybody) computes the routing flags of all clusters
// and re-arms the counter and the two counters of the fall-back list.
struct PlanOpsArgs {
  const double* Z;      // [K,TP,TP] L^-1, zeros above the diagonal
  const double* S;      // [K,TP,TP] 0.5 (Sigma + Sigma^T)
  const double* mean;   // [K,T]
  double* scal;
  int T, K;
  double* Mp;           // [K,TP,TP], tile-pair interleaved columns
  double* ap;           // [K,TP]
  double tol;           // accuracy threshold of the routing flags (hgp_pairs_plan_set_accuracy)
  int32_t* acc_list;
  int32_t* fb;
  unsigned* done;       // finished workgroups, of those that serve a diagonal block, of this launch; zero between launches
  // Kinv of a cluster that k_prep_build found unchanged (reuse.same) is read from Kinv instead of being recomputed from Z; a cluster
  // that is computed leaves its Kinv there, with what the next call's comparison needs (grid copy, jitter bits, status)
  double* Kinv;         // [K][NB][NB] tiles (a, b) of K~^-1 in accumulator layout [lane][4]
  PlanReuse reuse;
  const double* xb;     // [T] the caller's grid
  double* xb_copy;      // [TP]
  const int32_t* info;  // the caller's status array (or NULL), written by the inverse launch
};

template <int NB>
struct PlanOpsLds {
  static constexpr int TILE = 256;        // acc layout [lane][4]: the B operand of k-step s is element s of the lane's d4
  static constexpr int TILE_T = 16 * 17;  // row-major, pitch 17: read as the A operand X[c][4 s + g] (and transposed for M')
  static constexpr int COL = 0, ROW = COL + 2 * NB * TILE, P = ROW + 2 * NB * TILE_T, END = P + 2 * NB * TILE;
  static constexpr int QT = END, DOUBLES = END + 4 * TILE_T;   // Q_IJ, Q_JI, Q_II, Q_JJ; NB = 8: 109 056 bytes
  static constexpr size_t BYTES = (size_t)DOUBLES * sizeof(double);
};

// routing flags of all clusters (scal[8k+7], acc_list = [count, ids...] ascending): one thread
__device__ inline void plan_acc_flags(double* scal, int K, double tol, int32_t* acc_list) {
  int n = 0;
  for (int k = 0; k < K; ++k) {
    // ||K~^-1||_inf was accumulated by atomics of other workgroups: read it past this CU's vector cache
    const double ninf = __longlong_as_double((long long)__hip_atomic_load(
        reinterpret_cast<unsigned long long*>(scal + 8 * k + 6), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    const double ck = scal[8 * k] * ninf;
    const double bound = F64_EPS * ck * ck;
    const bool flag = (tol == 0.0) || (tol > 0.0 && !(bound <= tol));   // NaN bound -> solve-based
    scal[8 * k + 7] = flag ? 1.0 : 0.0;
    if (flag) acc_list[1 + n++] = k;
  }
  acc_list[0] = n;
}

template <int NB>
__global__ __launch_bounds__(128 * NB) void k_plan_ops(PlanOpsArgs a) {
  using L = PlanOpsLds<NB>;
  constexpr int TP = 16 * NB, NK = 4 * NB, NOFF = NB * (NB - 1) / 2;
  constexpr int TRIP = (NB == 6) ? 12 : (NB == 2 ? 8 : 16);   // k-steps whose operand loads are issued together (NK % TRIP == 0)
  extern __shared__ __attribute__((aligned(16))) double smem[];
  __shared__ int last;
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, c = lane & 15;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // one workgroup per pair t of the strictly upper tiles of cluster k, by columns: (0,1), (0,2), (1,2), ...
  const int k = blockIdx.x / NOFF;
  int I, J = 1;
  {
    int t = blockIdx.x % NOFF;
    while (t >= J) t -= J++;
    I = t;
  }
  // the diagonal tiles need nothing but the strips of their own block, which every workgroup of that block holds anyway:
  // (I, I+1) also makes tile (I, I), and the last pair (NB-2, NB-1) also tile (NB-1, NB-1) - no second round of workgroups
  const bool dI = J == I + 1, dJ = dI && J == NB - 1;
  const int T = a.T;
  const double* Z = a.Z + (size_t)k * TP * TP;
  const double* S = a.S + (size_t)k * TP * TP;
  double* colS = smem + L::COL;   // [2][NB] tiles (a, I), (a, J) of Kinv
  double* rowS = smem + L::ROW;   // [2][NB] tiles (I, a), (J, a) of Kinv
  double* pS = smem + L::P;       // [2][NB] tiles (t, I), (t, J) of P
  double* qT = smem + L::QT;      // [4] Q_IJ, Q_JI, Q_II, Q_JJ
  const int q = wave / NB, wa = wave % NB;   // this wave's strip (0: I, 1: J) and tile index along it
  const int Bq = q ? J : I;

  // ---- Kinv strips: tile (wa, Bq) of the block column and tile (Bq, wa) of the block row, from the same two operand streams.
  // Tile (a, b) of Kinv is the chain mfma(Z[:, a], Z[:, b]) over ascending k-steps whoever runs it - as element of a block column
  // (ccol of the wave with wa = a, Bq = b) or of a block row (crow of the wave with Bq = a, wa = b): ONE value per tile, which the
  // workgroups of the pairs (B, B + 1) leave in a.Kinv, block column B each (the last pair also NB - 1): every tile written once.
  // An unchanged cluster (same: uniform over the workgroup) takes its two tiles from there, bits as computed; (a, b) is never
  // taken for (b, a).
  const bool same = a.reuse.same[k] != 0;
  {
    double* Kc = a.Kinv + (size_t)k * TP * TP + (wa * NB + Bq) * L::TILE + lane * 4;
    d4 ccol = (d4){0.0, 0.0, 0.0, 0.0}, crow = (d4){0.0, 0.0, 0.0, 0.0};
    if (same) {
      ccol = *reinterpret_cast<const d4*>(Kc);
      crow = *reinterpret_cast<const d4*>(a.Kinv + (size_t)k * TP * TP + (Bq * NB + wa) * L::TILE + lane * 4);
    } else {
      const double* Za = Z + 16 * wa + c;
      const double* Zb = Z + 16 * Bq + c;
#pragma unroll
      for (int k0 = 0; k0 < NK; k0 += TRIP) {
        double za[TRIP], zb[TRIP];
#pragma unroll
        for (int u = 0; u < TRIP; ++u) {
          const int kk = 4 * (k0 + u) + g;
          za[u] = Za[(size_t)kk * TP];
          zb[u] = Zb[(size_t)kk * TP];
        }
        // every load of the trip is in flight before its first MFMA: left alone, the scheduler trades them for occupancy this
        // kernel cannot use and exposes one L2 latency per k-step
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < TRIP; ++u) {
          ccol = mfma(za[u], zb[u], ccol);   // Kinv[16 wa + .][16 Bq + .]
          crow = mfma(zb[u], za[u], crow);   // Kinv[16 Bq + .][16 wa + .]
        }
      }
      if (q == 0 ? dI : dJ) *reinterpret_cast<d4*>(Kc) = ccol;
    }
    *reinterpret_cast<d4*>(colS + (q * NB + wa) * L::TILE + lane * 4) = ccol;
#pragma unroll
    for (int r = 0; r < 4; ++r) rowS[(q * NB + wa) * L::TILE_T + (g + 4 * r) * 17 + c] = crow[r];
  }
  __syncthreads();

  // ---- P strips: tile (wa, Bq) of P = S Kinv; A operand from S (L2), B operand from the block column in LDS
  {
    const double* Scol = S + (size_t)g * TP + 16 * wa + c;   // S[16 wa + c][4 u + g] = S[4 u + g][16 wa + c]: S is exactly symmetric,
                                                            // and rows of 16 lanes read 128 contiguous bytes this way
    const double* cs = colS + q * NB * L::TILE + lane * 4;
    d4 acc = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k0 = 0; k0 < NK; k0 += TRIP) {
      double sv[TRIP];
#pragma unroll
      for (int u = 0; u < TRIP; ++u) sv[u] = Scol[(size_t)(4 * (k0 + u)) * TP];
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < TRIP; ++u) acc = mfma(sv[u], cs[((k0 + u) >> 2) * L::TILE + ((k0 + u) & 3)], acc);
    }
    *reinterpret_cast<d4*>(pS + (q * NB + wa) * L::TILE + lane * 4) = acc;
  }
  __syncthreads();

  // ---- Q tiles (waves 0 .. 3) beside a' and the row sums of |Kinv| (two further waves; NB = 2 has none: waves 2, 3 do both)
  if (wave < 2 || (wave == 2 && dI) || (wave == 3 && dJ)) {
    // wave 0: Q_IJ = Kinv[I, :] P[:, J];  1: Q_JI = Kinv[J, :] P[:, I];  2: Q_II = Kinv[I, :] P[:, I];  3: Q_JJ = Kinv[J, :] P[:, J]
    const int sr = wave & 1, sp = (wave < 2) ? 1 - sr : sr;
    const double* rs_ = rowS + sr * NB * L::TILE_T + c * 17 + g;
    const double* ps = pS + sp * NB * L::TILE + lane * 4;
    d4 acc = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int u = 0; u < NK; ++u) acc = mfma(rs_[(u >> 2) * L::TILE_T + 4 * (u & 3)], ps[(u >> 2) * L::TILE + (u & 3)], acc);
#pragma unroll
    for (int r = 0; r < 4; ++r) qT[wave * L::TILE_T + (g + 4 * r) * 17 + c] = acc[r];
  }
  constexpr int WA = NB > 2 ? 4 : 2;   // waves WA, WA + 1: a' of block I, of block J
  if ((wave == WA && dI) || (wave == WA + 1 && dJ)) {
    // a'[i] = c sum_j Kinv[j][i] mean[j], row sums of |Kinv|: serially over j = 0 .. T-1, from the block column
    const int sq = wave - WA;
    const double* cs = colS + sq * NB * L::TILE;
    const double cc = a.scal[8 * k];
    const double* mu = a.mean + (size_t)k * T;
    const int i = 16 * (sq ? J : I) + c;
    double s = 0.0, rs = 0.0;
    if (g == 0 && i < T) {
#pragma unroll 8
      for (int j = 0; j < T; ++j) {
        const int jj = j & 15;
        const double kij = cs[(j >> 4) * L::TILE + (16 * (jj & 3) + c) * 4 + (jj >> 2)];   // Kinv[j][i]
        s = fma(kij, mu[j], s);
        rs += fabs(kij);
      }
    }
    if (g == 0) a.ap[(size_t)k * TP + i] = cc * s;
    const double rmax = wave_allreduce<true>(fmax(0.0, rs));
    // ||K~^{-1}||_inf >= ||K~^{-1}||_2: maximum over the blocks (non-negative doubles order like their bit patterns;
    // k_prep_build zeroes the slot)
    if (lane == 0) atomicMax(reinterpret_cast<unsigned long long*>(a.scal + 8 * k + 6), (unsigned long long)__double_as_longlong(rmax));
  }
  __syncthreads();

  // ---- M' tiles (I, J), (J, I) and the diagonal tiles this workgroup makes: zero outside T, tile-pair interleaved columns
  {
    const double cc = a.scal[8 * k];
    double* Mp = a.Mp + (size_t)k * TP * TP;
    constexpr int NHh = NB / 2;
    for (int e = tid; e < 1024; e += 128 * NB) {
      const int m = e >> 8, rr = (e >> 4) & 15, c2 = e & 15;   // m: 0 (I, J), 1 (J, I), 2 (I, I), 3 (J, J)
      if ((m == 2 && !dI) || (m == 3 && !dJ)) continue;
      const int sm = m & 1, so = (m < 2) ? 1 - sm : sm;        // strips holding row bi and row bj of tile (bi, bj)
      const int bi = sm ? J : I, bj = so ? J : I;
      const int qa = m, qb = (m < 2) ? 1 - m : m;              // Q tile (bi, bj) and its mirror (bj, bi)
      const int i = 16 * bi + rr, j = 16 * bj + c2;
      double v = 0.0;
      if (i < T && j < T)
        v = plan_mp_value(cc, qT[qa * L::TILE_T + rr * 17 + c2], qT[qb * L::TILE_T + c2 * 17 + rr],
                          rowS[(sm * NB + bj) * L::TILE_T + rr * 17 + c2], rowS[(so * NB + bi) * L::TILE_T + c2 * 17 + rr]);
      Mp[(size_t)i * TP + plan_mp_col(j, NHh)] = v;
    }
  }

  // ---- the last of the K (NB - 1) workgroups that accumulate ||K~^-1||_inf routes the clusters.  One fence per workgroup, by
  // the thread that counts, behind the barrier that orders the workgroup's atomic maxima before it (a fence in every wave of
  // every workgroup writes the L2 back thousands of times per launch: 108 us for this kernel at NB = 8).
  if (!dI) return;
  // what the next call compares with, by pair (0, 1) of a cluster that was computed: the jitter's bits and the status beside its
  // Kinv, and (cluster 0: a changed grid changes every cluster) the grid.  All of it, like the Kinv stores above, by workgroups
  // that count below, so the valid marks are written behind it.
  if (!same && I == 0) {
    if (tid == 0) {
      a.reuse.key_jit[k] = __double_as_longlong(a.scal[8 * k + 5]);
      a.reuse.info[k] = a.info ? a.info[k] : 0;
    }
    if (k == 0)
      for (int i = tid; i < TP; i += 128 * NB) a.xb_copy[i] = (i < T) ? a.xb[i] : 0.0;
  }
  __syncthreads();
  if (tid == 0) {
    __threadfence();
    last = atomicAdd(a.done, 1u) == (unsigned)(a.K * (NB - 1)) - 1u ? 1 : 0;
  }
  __syncthreads();
  if (last && tid == 0) {
    __threadfence();
    plan_acc_flags(a.scal, a.K, a.tol, a.acc_list);
    a.fb[0] = 0;                    // fall-back list of k_pairs: its two counters start every plan state at zero
    a.fb[1 + PAIRS_FB_CAP] = 0;     // (a killed launch cannot leave them set)
    *a.done = 0u;
    // every cluster is now either computed in full by this launch or was valid before it.  Written last: a launch that dies
    // earlier leaves the clusters it was computing marked invalid (k_prep_build cleared them), and the next call computes them.
    for (int kk = 0; kk < a.K; ++kk) a.reuse.valid[kk] = 1;
  }
}

template <int NB>
int launch_plan_ops(const PlanOpsArgs& a, hipStream_t st) {
  const size_t lds = PlanOpsLds<NB>::BYTES;
  if (int rc = hgp_internal_ensure_dynamic_lds(reinterpret_cast<const void*>(&k_plan_ops<NB>), lds)) return rc;
  hipLaunchKernelGGL(k_plan_ops<NB>, dim3(a.K * (NB * (NB - 1) / 2)), dim3(128 * NB), lds, st, a);
  return launch_status();
}

static int tp_for(int n) {   // padded size: wave kernels {32,64,96,128}, cooperative kernels {192,256}
  if (n <= HGP_MAX_T_WAVE) return 16 * nb_for(n);
  return n <= 192 ? 192 : 256;
}

// The plan's device buffer, stated once: every area in order, each rounded up to 256 bytes.  Sets the padded size and the sizing of
// the overflow areas in *p; with `base` the d_* members are pointed into the buffer.  Returns the bytes the buffer needs.
size_t plan_layout(hgp_pairs_plan* p, int T, int Ts_max, int K, char* base) {
  const size_t TP = (size_t)tp_for(std::max(T, Ts_max));
  const size_t mat = (size_t)K * TP * TP * sizeof(double);
  p->TP = (int)TP;
  p->NB = p->TP / 16;
  p->coop = p->TP > HGP_MAX_T_WAVE;
  size_t o = 0;
  auto take = [&](auto*& member, size_t bytes) {
    if (base) member = reinterpret_cast<std::remove_reference_t<decltype(member)>>(base + o);
    o += (bytes + 255) & ~(size_t)255;
  };
  take(p->d_theta, (size_t)K * 3 * sizeof(double));
  take(p->d_scal, (size_t)K * 8 * sizeof(double));
  take(p->d_A, mat);   // K~ then L
  take(p->d_S, mat);
  take(p->d_Z, mat);
  take(p->d_Kinv, mat);   // TP <= 128: Kinv by 16 x 16 tiles in accumulator layout, kept from call to call (k_plan_ops)
  take(p->d_P, mat);      // P, Q: cooperative sizes only.  TP <= 128: first word of P = completion counter of k_plan_ops,
  take(p->d_Q, mat);      // start of Q = PlanReuse; the areas keep their size
  take(p->d_Mp, mat);
  take(p->d_ap, (size_t)K * TP * sizeof(double));
  take(p->d_perm, (size_t)K * sizeof(int32_t));
  take(p->d_xb, TP * sizeof(double));
  if (p->coop) {   // cooperative kernel: overflow areas for dense grids
    const size_t nb = (size_t)p->NB;
    const size_t cap = (nb >= 12) ? 48 : (nb == 8 ? 24 : 16);
    const size_t over = nb * nb > cap ? nb * nb - cap : 0;
    p->nscr = over ? (nb >= 12 ? 512 : 1024) : 0;
    p->escr_stride = (long)(over * 256);
    take(p->d_escr, (size_t)p->nscr * over * 256 * sizeof(double));
    take(p->d_eflags, ((size_t)p->nscr + 1) * sizeof(int32_t));
  }
  size_t sz[6];   // solve-based kernel (hgp_pairs_acc.hip): packed operands of L, Sigma; mean copy; per-workgroup S areas; flag list
  hgp_internal_acc_bytes((int)TP, K, sz);
  take(p->d_Lop, sz[0]);
  take(p->d_LTop, sz[1]);
  take(p->d_Dop, sz[2]);
  take(p->d_Sop, sz[3]);
  take(p->d_mu, sz[4]);
  take(p->d_sscr, sz[5]);
  take(p->d_acc_list, (size_t)(K + 1) * sizeof(int32_t));
  take(p->d_fb, (size_t)(PAIRS_FB_CAP + 2) * sizeof(int32_t));   // fall-back list of k_pairs
  return o;
}

}  // namespace

#ifdef HGP_STAMPS
unsigned long long* hgp_internal_stamp_dev = nullptr;   // host-side handle of the diagnostic counters (8 x u64)
#endif

// ------------------------------------------------------------------------------------------------ one pair-scoring call
// The kernel arguments of call c for length-scale group gi of the plan, whole batch: the only place that names the fields of
// PairsArgs.  The ragged and the streamed kernels take the same with one pointer behind it (PairsRagArgs, PairsSegArgs).
static PairsArgs pairs_args(const hgp_pairs_plan* p, size_t gi, const PairsCall& c, bool generic) {
  PairsArgs a{};
  a.x = c.x; a.y = c.y; a.N = c.N; a.Ts = c.ld; a.first_noise = c.first_noise; a.sel = c.sel;   // the call
  a.out_quad = c.out_quad; a.out_logdet = c.out_logdet; a.out_info = c.out_info;
  a.xb = p->d_xb; a.T = p->T; a.K = p->K; a.Mp = p->d_Mp; a.ap = p->d_ap; a.scal = p->d_scal; a.perm = p->d_perm;   // the plan
  a.kbeg = p->grp_beg[gi]; a.kend = p->grp_end[gi]; a.ell = p->grp_ell[gi];                         // the group
  a.escr = p->d_escr; a.eflags = p->d_eflags; a.nscr = p->nscr; a.escr_stride = p->escr_stride; a.fb = p->d_fb;
  a.flags = generic ? 1 : 0;
  a.score_add = -0.5 * (double)c.ld * LOG_2PI; a.score_on = p->score_out;
#ifdef HGP_STAMPS
  a.stamps = hgp_internal_stamp_dev;
#endif
  return a;
}

// The generic kernel hands the fall-back list back empty; after a launch that failed, the host does
static void pairs_reset_list(int32_t* fb, hipStream_t st) {
  (void)hipMemsetAsync(fb, 0, sizeof(int32_t), st);
  (void)hipMemsetAsync(fb + 1 + PAIRS_FB_CAP, 0, sizeof(int32_t), st);
}

// KA = PairsArgs (every row has c.ld points) or PairsRagArgs (c.seg_len)
template <class KA>
static int pairs_score_as(const hgp_pairs_plan* p, const PairsCall& c, void* store, hipStream_t st) {
  const bool generic = pairs_generic_forced();
  const int NB = p->NB;
  for (size_t gi = 0; gi < p->grp_beg.size(); ++gi) {
    KA a{pairs_args(p, gi, c, generic)};
    if constexpr (pairs_ragged<KA>) a.seg_len = c.seg_len;
    if (p->coop || NB < 6 || generic) {   // one kernel takes every segment: no list, no slices
      if (int rc = hgp_internal_pairs_all(a, NB, p->coop, st)) return rc;
      continue;
    }
    for (int off = 0; off < c.N; off += PAIRS_FB_CAP) {   // the fall-back list holds PAIRS_FB_CAP segments
      const KA s = pairs_slice(a, off, std::min(PAIRS_FB_CAP, c.N - off));
      const int32_t* len = nullptr;
      if constexpr (pairs_ragged<KA>) len = s.seg_len;
      const int rc1 = store ? hgp_internal_pairs_streamed(s, len, store, gi * (size_t)c.N + off, NB, st)   // k_segops, k_pairs_seg
                            : hgp_internal_pairs_band(s, NB, st);
      const int rc2 = hgp_internal_pairs_listed(s, NB, st);
      if (rc1 || rc2) {
        pairs_reset_list(p->d_fb, st);
        return rc1 ? rc1 : rc2;
      }
    }
  }
  return hgp_internal_pairs_acc(p, c, std::bool_constant<pairs_ragged<KA>>{}, st);
}

int hgp_internal_pairs_score(const hgp_pairs_plan* p, const PairsCall& c, void* store, hipStream_t st) {
  if (c.ld > HGP_MAX_T_COOP) return -2;
  if (c.ld > p->TP) return -2;   // plan was created with a smaller Ts_max
  // the hand-out flags of the overflow areas start every call at "free": a launch that was killed mid-flight cannot leave the
  // next one spinning (a plan serves ONE stream at a time; see the header)
  if (p->coop && p->d_eflags && p->nscr > 0 &&
      hipMemsetAsync(p->d_eflags, 0, (p->nscr + 1) * sizeof(int32_t), st) != hipSuccess)
    return launch_status();
  return c.seg_len ? pairs_score_as<PairsRagArgs>(p, c, store, st) : pairs_score_as<PairsArgs>(p, c, store, st);
}

extern "C" {

size_t hgp_pairs_plan_device_bytes(int T, int Ts_max, int K) {
  if (T <= 0 || Ts_max <= 0 || K <= 0) return 0;
  hgp_pairs_plan sizing;
  return plan_layout(&sizing, T, Ts_max, K, nullptr);
}

int hgp_pairs_plan_create(hgp_pairs_plan** plan, int T, int Ts_max, int K, const double* theta_host, void* dev_buf,
                          size_t dev_bytes) {
  if (!plan || !theta_host || !dev_buf || T <= 0 || Ts_max <= 0 || K <= 0) return -1;
  if (T > HGP_MAX_T_COOP || Ts_max > HGP_MAX_T_COOP) return -2;
  if (dev_bytes < hgp_pairs_plan_device_bytes(T, Ts_max, K)) return -1;
  for (int k = 0; k < K; ++k)
    if (!(theta_host[3 * k] > 0.0) || !(theta_host[3 * k + 1] > 0.0)) return -1;
  hgp_pairs_plan* p = new (std::nothrow) hgp_pairs_plan();
  if (!p) return -1;
  p->T = T;
  p->K = K;
  p->theta.assign(theta_host, theta_host + 3 * (size_t)K);
  p->perm.resize(K);
  for (int k = 0; k < K; ++k) p->perm[k] = k;
  std::stable_sort(p->perm.begin(), p->perm.end(),
                   [&](int a, int b) { return p->theta[3 * a + 1] < p->theta[3 * b + 1]; });
  for (int i = 0; i < K;) {
    int j = i;
    double ell = p->theta[3 * p->perm[i] + 1];
    while (j < K && p->theta[3 * p->perm[j] + 1] == ell) ++j;
    p->grp_beg.push_back(i);
    p->grp_end.push_back(j);
    p->grp_ell.push_back(ell);
    i = j;
  }
  plan_layout(p, T, Ts_max, K, (char*)dev_buf);
  if (hipMemset(p->d_fb, 0, (size_t)(PAIRS_FB_CAP + 2) * sizeof(int32_t)) != hipSuccess) {
    delete p;
    return 1000 + (int)hipGetLastError();
  }
  // completion counter of k_plan_ops: first word of the P area, which the one-wave sizes do not use otherwise
  if (!p->coop && hipMemset(p->d_P, 0, 256) != hipSuccess) {
    delete p;
    return 1000 + (int)hipGetLastError();
  }
  // no cluster has operators yet (PlanReuse: start of the Q area; K 24 bytes of the K TP^2 8 it holds)
  if (!p->coop && hipMemset(p->d_Q, 0, (size_t)K * PlanReuse::BYTES_PER_CLUSTER) != hipSuccess) {
    delete p;
    return 1000 + (int)hipGetLastError();
  }
  if (p->coop && hipMemset(p->d_eflags, 0, (p->nscr + 1) * sizeof(int32_t)) != hipSuccess) {
    delete p;
    return 1000 + (int)hipGetLastError();
  }
  if (hipMemcpy(p->d_theta, p->theta.data(), sizeof(double) * 3 * K, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(p->d_perm, p->perm.data(), sizeof(int32_t) * K, hipMemcpyHostToDevice) != hipSuccess) {
    delete p;
    return 1000 + (int)hipGetLastError();
  }
  *plan = p;
  return 0;
}

void hgp_pairs_plan_destroy(hgp_pairs_plan* plan) { delete plan; }

const double* hgp_pairs_plan_scalars(const hgp_pairs_plan* plan) { return plan ? plan->d_scal : nullptr; }

int hgp_pairs_plan_update(hgp_pairs_plan* p, const double* x_basis, const double* mean, const double* Sigma,
                          int32_t* info, void* stream) {
  if (!p || !x_basis || !mean || !Sigma) return -1;
  hipStream_t st = (hipStream_t)stream;
  const int K = p->K, T = p->T, TP = p->TP;
  // TP <= 128: the device decides per cluster whether K~, Z and Kinv of an earlier call still hold (k_prep_build compares the grid
  // and the jitter bit for bit); the host never knows, and issues the same launches either way
  const PlanReuse reuse = p->coop ? PlanReuse{} : plan_reuse(p);
  PrepArgs pa{x_basis, mean, Sigma, T, TP, K, p->d_theta, p->d_scal, p->d_A, p->d_S, p->d_xb, reuse, info};
  hipLaunchKernelGGL(k_prep_build, dim3(K, 8), dim3(256), 0, st, pa);
  // Z = chol(K~)^{-1}  (the factor itself is not needed)
  // symmetric = 1: k_prep_build writes K~ from (x_i - x_j)^2, exactly symmetric
  InvArgs fa{p->d_A, TP, K, 0.0, 0.0, p->d_Z, info};
  fa.symmetric = 1;
  fa.keep = reuse.same;   // a kept cluster's workgroups leave at once
  if (int rc = hgp_internal_chol_inverse(fa, p->NB, p->d_A, st)) return rc;   // TP > 128: K~ is overwritten by its factor
  if (!p->coop) {
    // TP <= 128: M', a', ||K~^-1||_inf and the routing flags in one launch behind the inverse; P, Q never reach memory
    PlanOpsArgs oa{p->d_Z, p->d_S, mean, p->d_scal, T, K, p->d_Mp, p->d_ap, p->acc_tol, p->d_acc_list, p->d_fb,
                   reinterpret_cast<unsigned*>(p->d_P), p->d_Kinv, reuse, x_basis, p->d_xb, info};
    if (int rc = dispatch_nb_wave(TP, [&](auto nb) { return launch_plan_ops<decltype(nb)::value>(oa, st); })) return rc;
    // clusters whose explicit operator would lose digits take the solve-based kernel: packed operands of L, Sigma
    int rc = hgp_internal_acc_prep(p, mean, /*flags_done=*/true, st);
    return rc ? rc : launch_status();
  }
  const long sm = (long)TP * TP;
  GemmArgs g1{p->d_Z, p->d_Z, p->d_Kinv, TP, TP, TP, TP, TP, TP, sm, sm, sm, 1.0, 0.0, 1, 0};     // Kinv = Z^T Z
  GemmArgs g2{p->d_S, p->d_Kinv, p->d_P, TP, TP, TP, TP, TP, TP, sm, sm, sm, 1.0, 0.0, 0, 0};    // P = S Kinv
  GemmArgs g3{p->d_Kinv, p->d_P, p->d_Q, TP, TP, TP, TP, TP, TP, sm, sm, sm, 1.0, 0.0, 0, 0};    // Q = Kinv S Kinv
  hgp_internal_gemm(g1, K, st);
  hgp_internal_gemm(g2, K, st);
  hgp_internal_gemm(g3, K, st);
  PrepFinalArgs fin{p->d_Q, p->d_Kinv, mean, p->d_scal, T, TP, p->d_Mp, p->d_ap, p->coop ? 0 : 1, p->d_fb};
  hipLaunchKernelGGL(k_prep_final, dim3(K, 8), dim3(256), 0, st, fin);
  // overflow-area flags: a launch that was killed mid-flight must not leave areas marked busy for the next one
  if (p->d_eflags && p->nscr > 0 && hipMemsetAsync(p->d_eflags, 0, (p->nscr + 1) * sizeof(int32_t), st) != hipSuccess) return launch_status();
  // clusters whose explicit operator would lose digits take the solve-based kernel: flags + packed operands of L, Sigma
  int rc = hgp_internal_acc_prep(p, mean, /*flags_done=*/false, st);
  return rc ? rc : launch_status();
}

int hgp_pairs_plan_set_accuracy(hgp_pairs_plan* p, double tol) {
  if (!p || tol != tol) return -1;
  p->acc_tol = tol;
  return 0;
}

int hgp_pairs_plan_set_score_output(hgp_pairs_plan* p, int on) {
  if (!p) return -1;
  p->score_out = on ? 1 : 0;
  return 0;
}

int hgp_loglik_pairs_f64(const hgp_pairs_plan* p, const double* x, const double* y, int N, int Ts,
                         const double* first_noise, const int32_t* sel, double* out_quad, double* out_logdet,
                         int32_t* out_info, void* stream) {
  if (N == 0) return 0;   // an empty batch is a no-op (its pointers may legitimately be null)
  if (!p || !x || !y || !out_quad || N < 0 || Ts <= 0) return -1;
  return hgp_internal_pairs_score(p, PairsCall{x, y, N, Ts, nullptr, first_noise, sel, out_quad, out_logdet, out_info}, nullptr,
                                  (hipStream_t)stream);
}

int hgp_loglik_pairs_ragged_f64(const hgp_pairs_plan* p, const double* x, const double* y, int N, int ld, const int32_t* seg_len,
                                const double* first_noise, const int32_t* sel, double* out_quad, double* out_logdet,
                                int32_t* out_info, void* stream) {
  if (N == 0) return 0;
  if (!p || !x || !y || !seg_len || !out_quad || N < 0 || ld <= 0) return -1;
  return hgp_internal_pairs_score(p, PairsCall{x, y, N, ld, seg_len, first_noise, sel, out_quad, out_logdet, out_info}, nullptr,
                                  (hipStream_t)stream);
}

#ifdef HGP_STAMPS
// diagnostic build: read and reset the phase cycle sums (d/f*, sweep 1, K** init, sweep 2, regularise, factor, -, diag16)
int hgp_debug_stamps(unsigned long long* out8_host) {
  if (!hgp_internal_stamp_dev) {
    if (hipMalloc(&hgp_internal_stamp_dev, 128) != hipSuccess) return 1;
    (void)hipMemset(hgp_internal_stamp_dev, 0, 128);
  }
  if (hipMemcpy(out8_host, hgp_internal_stamp_dev, 128, hipMemcpyDeviceToHost) != hipSuccess) return 1;
  (void)hipMemset(hgp_internal_stamp_dev, 0, 128);
  return 0;
}
#endif

}  // extern "C"
