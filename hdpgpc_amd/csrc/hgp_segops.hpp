// The segment-operator store of hgp_loglik_pairs_segops_f64 (include/hdpgpc_hip_segops.h): what the band pair kernel
// builds per segment before it meets a cluster - the blocks of E, the K** tiles, the band decision - kept from call to call in a
// buffer of the caller.  Stated once here, for k_segops (writes it), the streamed band kernel (reads it) and the launcher (sizes it).
//
// The store is [length-scale group of the plan][segment] records of SegOps<NB>::REC doubles:
//   tiles  [NE + NK][16][16]  row-major 16 x 16 blocks, element (row, column) of the block at 16 row + column:
//            E tiles first, column panel by column panel: the blocks PairsBand<NB>::emask(J), Kt ascending  (e_block)
//            then the K** tiles PairsBand<NB>::kmask(J), column by column, I ascending, without the factor c   (k_tile)
//   keyx   [TP]   the x row the tiles were built from, bit for bit (the first `len` entries)
//   keyxb  [TP]   the basis grid (the first T entries)
//   words  16 doubles: int32 flag, len, T, ld, NB at W_*; the length-scale as a double at ELL
// A record is valid iff its flag word has SEG_VALID.  k_segops clears the flag before it rewrites a record and sets it LAST, so a
// launch that died leaves "differs"; a zero-filled store holds nothing valid.  Only the workgroup of segment n touches record n.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace hgp {

constexpr int SEG_VALID = 1;    // the record is complete and belongs to its key
constexpr int SEG_BAND = 2;     // masks of the segment = the block-tridiagonal pattern of the static sweeps: tiles are present
constexpr int SEG_BADLEN = 4;   // len outside [1, ld]: no tiles, the pairs of the row report NaN / info = -1

template <int NB>
struct SegOps {
  static constexpr int TP = 16 * NB, NH = NB / 2;
  static constexpr int NE = 3 * NB - 2, NK = 2 * NB - 1, NT = NE + NK, TILE = 256;
  static constexpr int TILES = 0, KEYX = NT * TILE, KEYXB = KEYX + TP, WORDS = KEYXB + TP, REC = WORDS + 16;   // doubles
  static constexpr int W_FLAG = 0, W_LEN = 1, W_T = 2, W_LD = 3, W_NB = 4;   // int32 words behind WORDS
  static constexpr int ELL = WORDS + 4;                                      // double
  static_assert(REC % 2 == 0, "records are read as 16-byte vectors");
  struct Block {
    int Kt, J;
  };
  // tile t < NE: block (Kt, J) of E
  __host__ __device__ static constexpr Block e_block(int t) { return Block{(t + 1) / 3 - 1 + (t + 1) % 3, (t + 1) / 3}; }
  // tile NE + k: tile (I, J) of K**, I <= J
  __host__ __device__ static constexpr Block k_tile(int k) { return Block{(k + 1) / 2 - 1 + (k + 1) % 2, (k + 1) / 2}; }
  // the inverses: slot of block (Kt, J), |Kt - J| <= 1, and of tile (I, J), J - 1 <= I <= J
  __host__ __device__ static constexpr int e_slot(int Kt, int J) { return 3 * J + (Kt - J + 1) - 1; }
  __host__ __device__ static constexpr int k_slot(int I, int J) { return NE + 2 * J + (I - J + 1) - 1; }
  // where a tile lies in the E array of the band kernel's LDS (PairsLds): K** tile (I, J) lives in block ((I + NH) % NB, J)
  __host__ __device__ static constexpr Block lds_block(int t) {
    return t < NE ? e_block(t) : Block{(k_tile(t - NE).Kt + NH) % NB, k_tile(t - NE).J};
  }
  static constexpr size_t BYTES = sizeof(double) * REC;
};

}  // namespace hgp
