// The pairs plan: the per-cluster operators of the explicit-operator pair kernels (hgp_pairs.hip) and of the solve-based kernel
// (hgp_pairs_acc.hip), the layout of the plan's device buffer, and the C-ABI of the plan and of hgp_loglik_pairs_f64.
#include <algorithm>
#include <new>

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
  redi[tid] = bad;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) redi[tid] |= redi[tid + o];
    __syncthreads();
  }
  const double jit = 1e-4 * fmax(mean_abs, F64_EPS);           // GPI.py:488
  if (tid == 0 && blockIdx.y == 0) {
    double* sc = a.scal + 8 * k;
    sc[0] = c;
    sc[1] = ell;
    sc[2] = noise;
    sc[3] = redi[0] ? 0.0 : 1.0;
    sc[4] = mS;
    sc[5] = jit;
    sc[6] = 0.0;   // ||K~^{-1}||_inf: accumulated by k_prep_final with an atomic maximum
  }
  if (k == 0 && blockIdx.y == 0)
    for (int i = tid; i < TP; i += 256) a.xb_copy[i] = (i < T) ? a.xb[i] : 0.0;
  double* Ak = a.A + (size_t)k * TP * TP;
  double* Sk = a.S + (size_t)k * TP * TP;
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
  // (coalesced) and the mirror is transposed through LDS (pitch 33).
  // Column order of M' (logical j -> physical jp).  The pairs kernel reads row k of M' as the A operands of the NH
  // row tiles of one half h (tiles NH h .. NH h + NH - 1): inside a half, tiles are interleaved two by two so that ONE
  // 16-byte load per lane (lane cc) yields the operands of tiles 2q and 2q + 1; an odd last tile stays contiguous.
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
      if (i < T && j < T)
        v = (c * c) * (0.5 * (Q[(size_t)i * TP + j] + tq[tx][y]) - 0.5 * (Ki[(size_t)i * TP + j] + tk[tx][y]));
      int jp = j;
      if (a.interleave) {
        const int hh = j / (16 * NHh), tl = (j / 16) % NHh, cc = j % 16;
        const int loc = (tl < 2 * (NHh / 2)) ? 32 * (tl / 2) + 2 * cc + (tl & 1) : 16 * (NHh - 1) + cc;
        jp = 16 * NHh * hh + loc;
      }
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
  take(p->d_Kinv, mat);
  take(p->d_P, mat);
  take(p->d_Q, mat);
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
  PrepArgs pa{x_basis, mean, Sigma, T, TP, K, p->d_theta, p->d_scal, p->d_A, p->d_S, p->d_xb};
  hipLaunchKernelGGL(k_prep_build, dim3(K, 8), dim3(256), 0, st, pa);
  // Z = chol(K~)^{-1}  (the factor itself is not needed)
  PotrfArgs fa{p->d_A, TP, K, 0.0, 0.0, p->d_Z, nullptr, info};
  fa.inv_info = 1;
  fa.symmetric = 1;   // k_prep_build writes K~ from (x_i - x_j)^2: exactly symmetric
  if (int rc = hgp_internal_chol_inverse(fa, p->NB, st)) return rc;
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
  int rc = hgp_internal_acc_prep(p, mean, st);
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
  if (Ts > HGP_MAX_T_COOP) return -2;
  if (Ts > p->TP) return -2;   // plan was created with a smaller Ts_max
  hipStream_t st = (hipStream_t)stream;
  int rc = 0;
  // the hand-out flags of the overflow areas start every call at "free": a launch that was killed mid-flight cannot leave the
  // next one spinning (a plan serves ONE stream at a time; see the header)
  if (p->coop && p->d_eflags && p->nscr > 0 &&
      hipMemsetAsync(p->d_eflags, 0, (p->nscr + 1) * sizeof(int32_t), st) != hipSuccess)
    return launch_status();
  for (size_t gi = 0; gi < p->grp_beg.size() && rc == 0; ++gi) {
    PairsArgs a{x, y, N, Ts, p->d_xb, p->T, p->d_Mp, p->d_ap, p->d_scal, p->d_perm, p->grp_beg[gi], p->grp_end[gi],
                p->grp_ell[gi], first_noise, sel,
#ifdef HGP_STAMPS
                hgp_internal_stamp_dev,
#endif
                p->K, out_quad, out_logdet, out_info, p->d_escr, p->d_eflags, p->nscr, p->escr_stride,
                env_on("HGP_PAIRS_GENERIC") ? 1 : 0, -0.5 * (double)Ts * 1.8378770664093453, p->score_out, p->d_fb};
    rc = hgp_internal_pairs_fast(a, p->NB, p->coop, st);
  }
  if (rc == 0) rc = hgp_internal_pairs_acc(p, x, y, N, Ts, first_noise, sel, out_quad, out_logdet, out_info, st);
  return rc;
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
