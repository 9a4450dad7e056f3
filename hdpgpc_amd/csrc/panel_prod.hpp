// The [T, panel] product of the four-wave panel kernels (k_bands of hgp_bands.hip, k_sample of hgp_sample.hip): one workgroup of
// four waves multiplies a [T, T] operand that streams from L2 with a [T, 16 BN_CT] panel that sits in LDS in accumulator-tile
// order, on v_mfma_f64_16x16x4_f64.  Wave w owns the row tiles w, w + 4, ... of the result in accumulator registers; every
// element of the streamed operand feeds the BN_CT column tiles of the panel.  The sum over k runs k tile ascending, k-step
// ascending in every column slot: a column's result does not depend on its position in the panel.
#pragma once
#include "hgp_internal.hpp"
#include "tile_f64.hpp"

namespace hgp {

// 16-wide column tiles per panel (one A-operand element feeds that many MFMAs): four while a wave owns at most two row tiles
// (T <= 128), two above - two [row tiles][column tiles] accumulator sets are live at once, and 2 x 4 x 4 tiles are the whole
// register file
constexpr int bands_ct(int RT) { return RT <= 2 ? 4 : 2; }

// acc[i][ct] (+/-)= op(A)[row tile I = wave + 4 i][:] X[:][column tile ct], X in LDS as accumulator tiles (tile kt * BN_CT + ct).
// MODE 0: op(A) = A, lower block-triangular (k tiles <= I);  MODE 1: op(A) = A^T of such an A (k tiles >= I);
// MODE 2: op(A) = A^T, every k tile (used for symmetric operands: the transposed access is the coalesced one).
// TRI (MODE 0 only): the entries of A above the diagonal count as exact zeros whatever the memory holds there (the diagonal tile
// is masked in the loader).
template <int RT, int BN_CT, int MODE, bool SUB, bool TRI = false>
__device__ __forceinline__ void bands_prod(const double* __restrict__ A, int T, int nb, const double* Xs, int wave, int lane_in,
                                           d4 (&acc)[RT][BN_CT]) {
  static_assert(!TRI || MODE == 0, "the triangular mask belongs to the lower block-triangular product");
#pragma unroll
  for (int i = 0; i < RT; ++i) {
    const int I = wave + WAVES * i;
    if (I >= nb) continue;
    const int lane = launder(lane_in);
    const int g = lane >> 4, c = lane & 15;
    const int klo = (MODE == 1) ? I : 0, khi = (MODE == 0) ? I + 1 : nb;
    const int row = 16 * I + c;
    const bool rok = row < T;
    const int rowc = rok ? row : T - 1;
    auto load = [&](int kt, double (&a)[4]) {
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int k = 16 * kt + 4 * s + g;
        const int kc = k < T ? k : T - 1;
        const double v = (MODE == 0) ? A[(long)rowc * T + kc] : A[(long)kc * T + rowc];
        if constexpr (TRI) a[s] = (rok && k <= row) ? v : 0.0;   // k <= row < T
        else a[s] = (rok && k < T) ? v : 0.0;
      }
    };
    double an[4];
    load(klo, an);
    for (int kt = klo; kt < khi; ++kt) {
      double a[4];
#pragma unroll
      for (int s = 0; s < 4; ++s) a[s] = an[s];
      if (kt + 1 < khi) load(kt + 1, an);   // the next k tile travels while this one is multiplied
#pragma unroll
      for (int s = 0; s < 4; ++s) {
#pragma unroll
        for (int ct = 0; ct < BN_CT; ++ct) {
          const double b = Xs[((kt * BN_CT + ct) * 4 + s) * 64 + lane];
          acc[i][ct] = SUB ? mfma_sub(a[s], b, acc[i][ct]) : mfma(a[s], b, acc[i][ct]);
        }
      }
    }
  }
}

template <int RT, int BN_CT>
__device__ __forceinline__ void bands_zero(d4 (&acc)[RT][BN_CT]) {
#pragma unroll
  for (int i = 0; i < RT; ++i)
#pragma unroll
    for (int ct = 0; ct < BN_CT; ++ct) acc[i][ct] = d4{0.0, 0.0, 0.0, 0.0};
}

// the calling wave's row tiles of a panel into LDS, behind a barrier that ends every wave's reads of the previous panel
template <int RT, int BN_CT>
__device__ __forceinline__ void bands_publish(const d4 (&v)[RT][BN_CT], double* Xs, int nb, int wave, int lane) {
  __syncthreads();
#pragma unroll
  for (int i = 0; i < RT; ++i) {
    const int I = wave + WAVES * i;
    if (I >= nb) continue;
#pragma unroll
    for (int ct = 0; ct < BN_CT; ++ct) lds_tile_store(Xs, I * BN_CT + ct, lane, v[i][ct]);
  }
  __syncthreads();
}

}  // namespace hgp
