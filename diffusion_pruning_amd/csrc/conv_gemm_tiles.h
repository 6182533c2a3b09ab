// The tiles of aptp_conv_gemm: ONE row per APTP_TILE_* id, in id order -- the only place that states a fact about a tile.  Derived
// from it: the host geometry (kTiles: workspace, arrival counters, statistics rows / slots, grids), the family predicates and the
// launch switches of conv_gemm.hip, lin_gemm.hip, conv_lean.hip and conv_gemm_sk.hip; tests/tiles.py parses the same rows.  A new
// tile is one row here plus its entry in the public enum (include/aptp_hip.h: the documented numbering, with what each group of
// tiles is for); the static_asserts below fail the build when the two disagree.
//   X(NAME, FAMILY, BM, BN, WM, WN, STAGES, KU, KS, LIN, C3)        NAME: the enum suffix (APTP_TILE_##NAME)
//   FAMILY   REG register-staged operands (conv_gemm_kernel, the only one with an fp32 parity instantiation) | DMA operands copied
//            global->LDS by LDS-DMA (conv_gemm_dma_kernel) | PP the same kernel, two wave groups alternating load and MFMA slots |
//            HALO input halo kept in LDS (conv3x3_halo_kernel) | SK persistent stream-K (conv_gemm_sk.hip) | SKL the same with a
//            phase's fragment reads in its own load slot instead of one phase ahead
//   BM, BN   tile extents; WM, WN: the wave grid of ONE compute grid (a wave owns BM / WM rows and BN / WN columns)
//   STAGES   depth of the LDS ring (REG: the two halves of its double buffer; SK / SKL: filled in half-tiles)
//   KU       64-wide K-tiles per barrier (2: an effective K-step of 128)
//   KS       copies of the compute grid in one workgroup (WM * WN * KS waves), each on its own 32-wide half of every K-tile, summed
//            through LDS before the epilogue (intra-workgroup split-K)
//   LIN, C3  lin_gemm.hip / conv_lean.hip has a lean instantiation: <BM, BN, 2, 2, min(STAGES, 4), KU> for plain linear layers,
//            the row's own <BM, BN, WM, WN, STAGES, PP, KU> for 3x3 convolutions
#pragma once
#define APTP_CONV_GEMM_TILES(X) \
  X(128x128,          REG,  128, 128, 2, 2, 2, 1, 1, 0, 0)  /* register-staged */ \
  X(128x160,          REG,  128, 160, 2, 2, 2, 1, 1, 0, 0) \
  X(64x128,           REG,   64, 128, 2, 2, 2, 1, 1, 0, 0) \
  X(64x160,           REG,   64, 160, 2, 2, 2, 1, 1, 0, 0) \
  X(128x64,           REG,  128,  64, 2, 2, 2, 1, 1, 0, 0) \
  X(64x64,            REG,   64,  64, 2, 2, 2, 1, 1, 0, 0) \
  X(DMA_128x128,      DMA,  128, 128, 2, 2, 2, 1, 1, 0, 0)  /* the same tiles through LDS-DMA, 2-deep ring */ \
  X(DMA_128x160,      DMA,  128, 160, 2, 2, 2, 1, 1, 0, 0) \
  X(DMA_64x128,       DMA,   64, 128, 2, 2, 2, 1, 1, 1, 0) \
  X(DMA_64x160,       DMA,   64, 160, 2, 2, 2, 1, 1, 0, 0) \
  X(DMA_128x64,       DMA,  128,  64, 2, 2, 2, 1, 1, 1, 0) \
  X(DMA_64x64,        DMA,   64,  64, 2, 2, 2, 1, 1, 1, 0) \
  X(DMA3_128x128,     DMA,  128, 128, 2, 2, 3, 1, 1, 0, 0)  /* 3-deep ring (DMA two K-steps ahead, counted vmcnt + raw barrier) */ \
  X(DMA3_128x160,     DMA,  128, 160, 2, 2, 3, 1, 1, 0, 0) \
  X(DMA3_64x128,      DMA,   64, 128, 2, 2, 3, 1, 1, 1, 0) \
  X(DMA3_64x160,      DMA,   64, 160, 2, 2, 3, 1, 1, 0, 0) \
  X(DMA3_128x64,      DMA,  128,  64, 2, 2, 3, 1, 1, 1, 0) \
  X(DMA3_64x64,       DMA,   64,  64, 2, 2, 3, 1, 1, 1, 1) \
  X(DMA8_128x160,     DMA,  128, 160, 4, 2, 2, 1, 1, 0, 0)  /* 8 waves: one weight tile shared by twice the rows */ \
  X(DMA8_256x160,     DMA,  256, 160, 4, 2, 2, 1, 1, 0, 0) \
  X(DMA8_128x128,     DMA,  128, 128, 2, 4, 2, 1, 1, 0, 0) \
  X(DMA8_256x128,     DMA,  256, 128, 4, 2, 2, 1, 1, 0, 0) \
  X(DMA4_64x160,      DMA,   64, 160, 2, 2, 4, 1, 1, 0, 0)  /* 4 waves, 4-stage ring (three operand tiles in flight) */ \
  X(DMA4_64x128,      DMA,   64, 128, 2, 2, 4, 1, 1, 1, 0) \
  X(DMA4_64x64,       DMA,   64,  64, 2, 2, 4, 1, 1, 1, 0) \
  X(DMA4_128x64,      DMA,  128,  64, 2, 2, 4, 1, 1, 1, 0) \
  X(DMA4_128x128,     DMA,  128, 128, 2, 2, 4, 1, 1, 0, 0) \
  X(DMA8R3_128x160,   DMA,  128, 160, 4, 2, 3, 1, 1, 0, 1)  /* 8 waves, 3- or 4-stage ring */ \
  X(DMA8R4_128x160,   DMA,  128, 160, 4, 2, 4, 1, 1, 0, 0) \
  X(DMA8R3_128x128,   DMA,  128, 128, 2, 4, 3, 1, 1, 0, 1) \
  X(DMA8R4_128x128,   DMA,  128, 128, 2, 4, 4, 1, 1, 0, 0) \
  X(DMA8R3_256x128,   DMA,  256, 128, 4, 2, 3, 1, 1, 0, 0) \
  X(PP3_128x160,      PP,   128, 160, 4, 2, 3, 1, 1, 0, 0)  /* ping-pong, 3- to 5-stage ring */ \
  X(PP4_128x160,      PP,   128, 160, 4, 2, 4, 1, 1, 0, 1) \
  X(PP3_128x128,      PP,   128, 128, 2, 4, 3, 1, 1, 0, 0) \
  X(PP4_128x128,      PP,   128, 128, 2, 4, 4, 1, 1, 0, 0) \
  X(PP4_64x160,       PP,    64, 160, 4, 2, 4, 1, 1, 0, 0) \
  X(PP4_64x128,       PP,    64, 128, 2, 4, 4, 1, 1, 0, 0) \
  X(PP5_64x160,       PP,    64, 160, 4, 2, 5, 1, 1, 0, 0) \
  X(PP4_128x64,       PP,   128,  64, 4, 2, 4, 1, 1, 0, 1) \
  X(PP3_256x128,      PP,   256, 128, 4, 2, 3, 1, 1, 0, 0) \
  X(PP3_128x256,      PP,   128, 256, 2, 4, 3, 1, 1, 0, 0) \
  X(HALO_128x160,     HALO, 128, 160, 4, 2, 4, 1, 1, 0, 0)  /* halo-in-LDS, 8 waves (4 x 2), weights through a 4-stage ring */ \
  X(HALO_128x128,     HALO, 128, 128, 4, 2, 4, 1, 1, 0, 0) \
  X(DMA6_64x64,       DMA,   64,  64, 2, 2, 6, 1, 1, 1, 0)  /* 6- or 8-stage ring: few workgroups, long K (latency-bound) */ \
  X(DMA8S_64x64,      DMA,   64,  64, 2, 2, 8, 1, 1, 1, 0) \
  X(DMA6_64x128,      DMA,   64, 128, 2, 2, 6, 1, 1, 1, 0) \
  X(DMA6_128x64,      DMA,  128,  64, 2, 2, 6, 1, 1, 1, 0) \
  X(KU2S4_64x64,      DMA,   64,  64, 2, 2, 4, 2, 1, 1, 0)  /* TWO K-tiles per barrier (KU = 2); the last two: 8 waves */ \
  X(KU2S6_64x64,      DMA,   64,  64, 2, 2, 6, 2, 1, 1, 0) \
  X(KU2S4_64x128,     DMA,   64, 128, 2, 2, 4, 2, 1, 1, 0) \
  X(KU2S6_64x128,     DMA,   64, 128, 2, 2, 6, 2, 1, 1, 0) \
  X(KU2S4_128x64,     DMA,  128,  64, 2, 2, 4, 2, 1, 1, 0) \
  X(KU2S4_128x128,    DMA,  128, 128, 2, 2, 4, 2, 1, 0, 0) \
  X(KU2S4_64x160,     DMA,   64, 160, 2, 2, 4, 2, 1, 0, 0) \
  X(KU2S4_128x160,    DMA,  128, 160, 4, 2, 4, 2, 1, 0, 1) \
  X(KU2S4_128x128W8,  DMA,  128, 128, 2, 4, 4, 2, 1, 0, 0) \
  X(KS2S3_64x64,      DMA,   64,  64, 2, 2, 3, 1, 2, 0, 0)  /* 8 waves as TWO copies of a 2 x 2 wave grid (KS = 2) */ \
  X(KS2S4_64x64,      DMA,   64,  64, 2, 2, 4, 1, 2, 0, 0) \
  X(KS2S3_64x128,     DMA,   64, 128, 2, 2, 3, 1, 2, 0, 0) \
  X(KS2S4_64x128,     DMA,   64, 128, 2, 2, 4, 1, 2, 0, 0) \
  X(KS2S3_128x64,     DMA,  128,  64, 2, 2, 3, 1, 2, 0, 0) \
  X(KS2S3_128x128,    DMA,  128, 128, 2, 2, 3, 1, 2, 0, 0) \
  X(SK_256x160,       SK,   256, 160, 4, 2, 3, 1, 1, 0, 0)  /* stream-K macro-tiles; split_k > 1 = K split on, 1 = whole tiles */ \
  X(SK_256x128,       SK,   256, 128, 4, 2, 3, 1, 1, 0, 0) \
  X(SK_128x256,       SK,   128, 256, 2, 4, 3, 1, 1, 0, 0) \
  X(SKL_256x160,      SKL,  256, 160, 4, 2, 3, 1, 1, 0, 0)  /* ... fragment reads in the load slot (tuner candidates) */ \
  X(SKL_256x128,      SKL,  256, 128, 4, 2, 3, 1, 1, 0, 0) \
  X(SKL_128x256,      SKL,  128, 256, 2, 4, 3, 1, 1, 0, 0) \
  X(SK_128x160,       SK,   128, 160, 4, 2, 3, 1, 1, 0, 0)  /* stream-K on 128-row tiles (SK_128x128: 4 x 2 waves, not 2 x 4) */ \
  X(SKL_128x160,      SKL,  128, 160, 4, 2, 3, 1, 1, 0, 0) \
  X(SK_128x128,       SK,   128, 128, 4, 2, 3, 1, 1, 0, 0) \
  X(SKL_128x128,      SKL,  128, 128, 4, 2, 3, 1, 1, 0, 0)

namespace aptp_cg {
enum class TileFamily { NONE, REG, DMA, PP, HALO, SK, SKL };      // (the stream-K pair last: is_sk_tile)
// tile extents, the wave grid's N extent and the waves of one compute grid (the KS = 2 tiles: 4, in a 512-thread workgroup)
struct TileCfg { int bm, bn, wn, nw; TileFamily family; bool lin, c3; };
#define X(NAME, FAMILY, BM, BN, WM, WN, STAGES, KU, KS, LIN, C3) {BM, BN, WN, WM * WN, TileFamily::FAMILY, LIN != 0, C3 != 0},
constexpr TileCfg kTiles[] = {{0, 0, 0, 0, TileFamily::NONE, false, false}, APTP_CONV_GEMM_TILES(X)};   // [0]: APTP_TILE_AUTO
#undef X
constexpr int kNumTiles = (int)(sizeof(kTiles) / sizeof(kTiles[0]));
// the public numbering is the row order
#define X(NAME, ...) r##NAME,
enum TileRow { rAUTO, APTP_CONV_GEMM_TILES(X) };
#undef X
#define X(NAME, ...) static_assert(APTP_TILE_##NAME == r##NAME, "include/aptp_hip.h: APTP_TILE_" #NAME " is not this row's index");
APTP_CONV_GEMM_TILES(X)
#undef X

inline bool tile_known(int t) { return t > 0 && t < kNumTiles; }
inline bool is_reg_tile(int t) { return tile_known(t) && kTiles[t].family == TileFamily::REG; }
inline bool is_sk_tile(int t) { return tile_known(t) && kTiles[t].family >= TileFamily::SK; }
// the LDS-DMA kernels that stream padding lanes from the 8 KiB zero page (the halo pair included, the stream-K tiles not)
inline bool is_dma_tile(int t) { return tile_known(t) && !is_reg_tile(t) && !is_sk_tile(t); }

}  // namespace aptp_cg
