// The GEMM / conv tile table and everything that is derived from it: the kernel argument block, the host plan, the
// launcher entry points of the kernel-family translation units and the table-driven dispatch they share.
//
// One row of kTiles states everything the host knows about a tile: its kernel family, its template arguments and the
// forms it is instantiated for.  The planner (gemm.hip) asks the row "is this form instantiated?", the family
// launchers instantiate exactly the kernels whose rows say so (dispatch() below reads the same bits in an
// `if constexpr`), and dd_gemm_kernel_name prints the row — so a plan never names a kernel the library does not hold.
// Adding or removing a tile is a one-line change here.
#pragma once
#include "dd_common.h"
#include <utility>

namespace ddg {

constexpr int BK = 64;  // K elements per pipeline step (8 chunks of 16 B per tile row)
constexpr int kNumCU = 256;

struct GemmParams {
  const void* a; const void* a2; int64_t lda, lda2; int k1;
  int rows, n, k;
  const void* w; const void* bias; const void* rowvec; int rows_per_inst, ld_rowvec;
  const void* res; int64_t ldres;
  void* out; int64_t ldc;
  float alpha; int accumulate; int act;
  int hin, win, cin, hv, wv, hout, wout, stride, upsample;
  float scale_h, scale_w;
  int k_per_split;
  float* partial;
  int tiles_m, tiles_n;
  uint32_t a_bytes, a2_bytes, w_bytes;   // buffer extents for the descriptor-based DMA path
  uint32_t out_bytes, res_bytes;         // dd_gemm3_kernel's fast epilogue: extents of out / res (0 = take the general epilogue)
  int g_per_tile, chunks_per_split;      // direct small-image conv (dd_conv3s_kernel)
  int band_rows, bands; float inv_bands; // ... its BAND form: output pixels per band, bands per instance
  const float* ln_colsum; const float* ln_bias; float ln_eps;   // LayerNorm fold (dd_gemm2_kernel, dense)
  int out_f32;                           // store fp32 instead of T
  float* stat_out;                       // [rows][n/32][2] row sum / sum of squares of the fp32 values before their rounding to T, or NULL
  const float* stat_in;                  // LayerNorm fold: [rows][k/32][2] table of the `a` rows, or NULL
  int hm_d, hm_planes; float hm_scale;   // head-major output: plane width D, scaled planes, their factor
  int persist;                           // dd_gemm2_kernel: the grid is smaller than the tile count (see the kernel)
  uint64_t* dbg_stamps;                  // DD_DBG_STAMP builds only
  float inv_hw, inv_wout, inv_rpi;       // 1 / (hout*wout), 1 / wout, 1 / rows_per_inst for dd_fdiv
  void* ln_out; int64_t ld_ln_out;       // LayerNorm EMITTED by the epilogue of the 80x320 tile (second output)
  const void* lno_gamma; const void* lno_beta;
  float inv_tiles_n, inv_hm_d;           // dd_gemm4_kernel: 1 / tiles_n, 1 / hm_d for dd_fdiv
  uint32_t ln_out_bytes;                 // ... extent of ln_out for its buffer stores
};

// Folded-upsample conv (dd_gemm2u_kernel): the output pixels of a nearest-upsample + 3x3 conv, enumerated class by class.
// Per axis a coordinate o with s = src(o) is of class 0 (taps read s-1 | s s), 1 (s s | s+1) or 2 (s-1 | s, tap +1 outside
// the output: the last coordinate of an odd size); a pixel's class is 3 * row class + column class, each class has its own
// [n][4 * cin] weight matrix (the tap slices that read one source pixel summed ahead of time) and starts on a tile boundary.
constexpr int kUpfoldMax = 64;             // largest output height / width the coordinate lists hold
struct UpfoldTab {
  uint16_t tile0[10];                      // first row tile of class c; [9] = all row tiles
  uint8_t widx[9];                         // weight matrix of class c (the non-empty classes, in order)
  uint8_t ny[3], nx[3], y0[3], x0[3];      // per axis class: coordinates, and where its list starts in y[] / x[]
  float inv_plane[9], inv_nx[3];           // 1 / (ny * nx), 1 / nx for dd_fdiv
  int m;                                   // instances
  uint8_t y[kUpfoldMax], x[kUpfoldMax];    // output coordinates, class by class
};

enum Family {
  FAM_REG,      // register-staged software pipeline: dd_gemm_kernel / dd_gemm_pad0_kernel (gemm1.hip)
  FAM_RING,     // LDS-DMA ring: dd_gemm2_kernel (gemm2_kernel.h)
  FAM_PIPE,     // pipelined LDS-DMA ring, dense only: dd_gemm3_kernel, and dd_gemm4_kernel as its persistent form
  FAM_DIRECT,   // direct small-image conv: dd_conv3s_kernel; stride 1 / no resize / Cin % 64 == 0 only
};

// what a tile is instantiated for
enum Form : unsigned {
  F_DENSE = 1,
  F_CONV = 2,
  F_GEGLU = 4,      // dense with the GEGLU gate in the epilogue: the h / gate halves need four 16-column blocks per wave
  F_PAD0 = 8,       // conv with pad_lo = 0 (dd_gemm_conv_pad): dd_gemm_pad0_kernel
  F_LN_OUT = 16,    // the whole-row tile whose epilogue can emit LayerNorm(out) as a second tensor (dd_gemm_desc.ln_out)
  F_PERSIST = 32,   // persistent walk over the tiles: inside dd_gemm2_kernel (FAM_RING), dd_gemm4_kernel (FAM_PIPE)
  F_UPFOLD = 64,    // folded-upsample conv (dd_gemm_desc.upfold): dd_gemm2u_kernel, the CONV ring with 2 x 2 summed taps
};

struct TileCfg {
  int id; const char* name; Family family;
  int wm, wn, tm, tn;       // waves of the workgroup, 16-row / 16-column blocks per wave
  unsigned forms;
  int depth = 0;            // slots of the LDS ring (FAM_RING, FAM_PIPE), of the weight ring (FAM_DIRECT: the kernel's NSW)
  int grp = 1;              // FAM_DIRECT: taps per barrier (GRP)
  bool band = false;        // FAM_DIRECT: the BAND form
};

constexpr unsigned REG_ALL = F_DENSE | F_CONV | F_GEGLU | F_PAD0, REG_TN2 = F_DENSE | F_CONV | F_PAD0;
constexpr unsigned RING_ALL = F_DENSE | F_CONV | F_GEGLU | F_PERSIST, RING_TN2 = F_DENSE | F_CONV | F_PERSIST;
constexpr unsigned RING_DENSE = F_DENSE | F_PERSIST;
constexpr unsigned UPF = F_UPFOLD;
constexpr unsigned PIPE = F_DENSE | F_PERSIST;

// {id, name, family, waves, blocks per wave, forms[, ring slots[, GRP[, BAND]]]}
constexpr TileCfg kTiles[] = {
    {1, "128x128", FAM_REG, 2, 2, 4, 4, REG_ALL},
    {2, "128x64", FAM_REG, 2, 2, 4, 2, REG_TN2},
    {3, "64x128", FAM_REG, 2, 2, 2, 4, REG_ALL},
    {4, "64x64", FAM_REG, 2, 2, 2, 2, REG_TN2},
    {5, "256x128", FAM_REG, 4, 2, 4, 4, REG_ALL},
    {11, "128x128/dma2", FAM_RING, 2, 2, 4, 4, RING_ALL, 2},
    {12, "128x128/dma3", FAM_RING, 2, 2, 4, 4, RING_ALL | UPF, 3},
    {13, "128x64/dma3", FAM_RING, 2, 2, 4, 2, RING_TN2 | UPF, 3},
    {14, "64x128/dma3", FAM_RING, 2, 2, 2, 4, RING_ALL | UPF, 3},
    {15, "64x64/dma3", FAM_RING, 2, 2, 2, 2, RING_TN2 | UPF, 3},
    {16, "256x128/dma2", FAM_RING, 4, 2, 4, 4, RING_ALL, 2},
    {20, "256x128/dma3", FAM_RING, 4, 2, 4, 4, RING_ALL | UPF, 3},
    {23, "128x64/dma4", FAM_RING, 2, 2, 4, 2, RING_TN2, 4},
    {24, "64x128/dma4", FAM_RING, 2, 2, 2, 4, RING_ALL, 4},
    // 160-wide tiles (10 waves = 2 x 5): every channel count of this network (320, 640, 960, 1280, 1920, 2560) is
    // a multiple of 160, so no column of the tile multiplies padding (a 128-wide tile wastes 1/6 of its MFMAs at
    // N = 320 and 16800 rows / 160 = 105 row tiles x 2 = 210 workgroups fill the chip in ONE generation)
    {27, "160x160/dma2", FAM_RING, 2, 5, 5, 2, RING_TN2, 2},
    {28, "160x160/dma3", FAM_RING, 2, 5, 5, 2, RING_TN2 | UPF, 3},
    // 80 WHOLE rows of a 320-wide output per workgroup (1 x 10 waves): the only tile whose epilogue can emit
    // LayerNorm(out) as a second tensor (dd_gemm_desc.ln_out); 16800 rows -> 210 workgroups, one generation
    {40, "80x320/dma2", FAM_RING, 1, 10, 5, 2, RING_DENSE | F_LN_OUT, 2},
    // 1092 x 1280 outputs over 256 CUs = 5460 per CU: 96x64 -> 12 x 20 = 240 workgroups (one generation, nearly every
    // CU busy) staging 410 KB each where the 64x128 tile stages 491 KB on 180 CUs.  Challenged against the tracked table
    // (bench.py --challenge-tiles 52, cold weights, 3 % to win): takes 28 of the dense shapes per dtype, ~1 us each
    // (1092x1280x1280 15.4 -> 14.4, 336x1280x1280 14.8 -> 13.8 and no split-K, 4200x640x1920 27.1 -> 21.7); 96x128
    // tiles won nothing (profiles/r03_tile_challenge.txt)
    {52, "96x64/dma3", FAM_RING, 2, 2, 3, 2, RING_TN2 | UPF, 3},
    // 32-row tiles for the few-row GEMMs (time / box / text embeddings: 12-240 rows; 336 x 1280 -> 11 x 20 workgroups):
    // 1-2 us each in the same challenge; 96x64 with 2 / 4 slots, 96x128 and 192x64 tiles won nothing and were removed
    {59, "32x64/dma3", FAM_RING, 2, 2, 1, 2, RING_DENSE, 3},
    {60, "32x64/dma6", FAM_RING, 2, 2, 1, 2, RING_DENSE, 6},
    // 192 rows: 1092 rows -> 6 row tiles (180 workgroups at N = 3840 where 256x128 has 150): the per-CU staging rate,
    // not the tile's arithmetic intensity, bounds a launch that leaves CUs without a workgroup (1092x3840x1280:
    // 26.5 -> 23.2 us cold, 1092x1280x6400: 41.4 -> 37.6)
    {44, "192x128/dma3", FAM_RING, 4, 2, 3, 4, RING_ALL | UPF, 3},
    {46, "192x128/dma2", FAM_RING, 4, 2, 3, 4, RING_ALL, 2},
    // 256x256 (round 3): the tiled family is bound by L2 -> LDS staging, and staged bytes per flop go with
    // (BM + BN) / (BM * BN): 0.0078 B/flop against 0.0117 for 256x128.  8 waves of 128 x 64 (32 accumulator blocks per
    // wave: one wave per SIMD pair, 2 stages of 64 KB).  Candidates for the wide GEGLU projections and the big convs.
    {50, "256x256/dma2", FAM_RING, 2, 4, 8, 4, RING_ALL, 2},
    // pipelined LDS-DMA family (round 5; dense only)
    {72, "96x64/p3", FAM_PIPE, 2, 2, 3, 2, PIPE, 3},             // 60 KB: two workgroups per CU
    {73, "96x64/p5", FAM_PIPE, 2, 2, 3, 2, PIPE, 5},             // deeper rings: one workgroup per CU, cold weights 3-4 K-steps ahead
    {75, "192x128/p3", FAM_PIPE, 4, 2, 3, 4, PIPE | F_GEGLU, 3},
    {76, "32x64/p4", FAM_PIPE, 2, 2, 1, 2, F_DENSE, 4},
    {77, "32x64/p6", FAM_PIPE, 2, 2, 1, 2, F_DENSE, 6},
    {78, "160x160/p3", FAM_PIPE, 2, 5, 5, 2, PIPE, 3},
    {74, "80x320/p3", FAM_PIPE, 1, 10, 5, 2, PIPE | F_LN_OUT, 3},   // the LayerNorm-emitting tile (tile 40) on the pipelined loop
    // direct small-image conv
    {31, "conv3s 384x64", FAM_DIRECT, 4, 2, 6, 2, F_CONV, 5},
    {39, "conv3s band 384x64", FAM_DIRECT, 4, 2, 6, 2, F_CONV, 5, 1, true},   // BAND form (images larger than the tile: 28x50 level)
    // (round 5: the same 384 x 64 tile on FOUR waves of 96 x 64, one per SIMD — 10 fragment reads per 24 MFMAs instead of
    //  8 per 12 — was built, bit-identical, and 12-16 % SLOWER on every level (28x50: 40.5 vs 35.2 us): without a partner
    //  wave the step's chain barrier -> weight reads -> MFMAs is exposed; profiles/r05_conv3s_ab.txt.  Removed.)
    {34, "conv3s 192x64/w4", FAM_DIRECT, 2, 2, 6, 2, F_CONV, 4},
    {35, "conv3s 128x64/w3", FAM_DIRECT, 2, 2, 4, 2, F_CONV, 3},     // 72 KB of LDS: two workgroups per CU
    {37, "conv3s 192x64/g3", FAM_DIRECT, 2, 2, 6, 2, F_CONV, 6, 3},     // taps in groups of three: one barrier per 72 MFMAs
    // (Round 5 removed what no entry of the tracked table used: 64x64 rings of 2 / 4 / 6 / 8 slots, 128x64 / 128x128 with
    //  2 / 4, 384x64, the GEGLU-only 160x320, three direct-conv variants, and the round-2 row-panel family.)
};
constexpr int kNumTiles = sizeof(kTiles) / sizeof(kTiles[0]);

// the tiles the planner chooses on purpose: the auto heuristic's candidates (biggest first) and the two LayerNorm-emitting tiles
constexpr int kTile128x128 = 1, kTile128x64 = 2, kTile64x128 = 3, kTile64x64 = 4;
constexpr int kAutoTiles[] = {kTile128x128, kTile128x64, kTile64x128, kTile64x64};
constexpr int kTileLnRing = 40, kTileLnPipe = 74;

constexpr int tile_bm(const TileCfg& t) { return t.wm * t.tm * 16; }
constexpr int tile_bn(const TileCfg& t) { return t.wn * t.tn * 16; }
constexpr int tile_index(int id) {
  for (int i = 0; i < kNumTiles; ++i) if (kTiles[i].id == id) return i;
  return -1;
}

constexpr bool tiles_consistent() {          // what the kernels' own static_asserts do not say
  for (const TileCfg& t : kTiles)
    if (((t.forms & F_PAD0) && t.family != FAM_REG) || ((t.forms & F_CONV) && t.family == FAM_PIPE) ||
        ((t.forms & F_LN_OUT) && tile_bn(t) != 320) || ((t.forms & F_UPFOLD) && (t.family != FAM_RING || !(t.forms & F_CONV))) || (t.family == FAM_DIRECT) != (t.forms == F_CONV)) return false;
  for (int id : kAutoTiles) if (tile_index(id) < 0 || kTiles[tile_index(id)].family != FAM_REG) return false;
  return tile_index(kTileLnRing) >= 0 && tile_index(kTileLnPipe) >= 0;
}
static_assert(tiles_consistent(), "kTiles");

// Workgroups of a pipelined tile that are resident per CU — decided from the tile alone (ring bytes and waves), not from an
// occupancy query, so that dd_gemm_kernel_name reports the launcher's choice without a device: two 4-wave workgroups
// where two rings fit the 160 KB of LDS (the 60 KB 96x64 ring; its kernels need <= 128 registers), else one.
constexpr int gemm4_resident(const TileCfg& t) {
  const int ring = t.depth * (tile_bm(t) + tile_bn(t)) * BK * 2;
  return (t.wm * t.wn == 4 && 2 * ring <= 160 * 1024) ? 2 : 1;
}

struct Plan { int tile_idx; int split; int tiles_m, tiles_n; int k_per_split; int g_per_tile, chunks_per_split; bool unsupported; bool persist_ok; int band_rows, bands; bool persist3_ok; UpfoldTab upf; };

// ---- launcher entry points of the family translation units: launch the kernel of tile pl.tile_idx in one form for
// dtype DD_F16 / DD_BF16, or return DD_ERR_UNSUPPORTED where the tile's row holds no such instantiation
using LaunchFn = int(int dtype, unsigned form, const GemmParams& p, const Plan& pl, hipStream_t s);
__attribute__((visibility("hidden"))) LaunchFn launch_gemm1, launch_gemm2_dense, launch_gemm2_geglu, launch_gemm2_conv, launch_gemm2_upfold, launch_gemm3,
    launch_gemm4, launch_conv3s;

// launch KERN; a kernel with more than 64 KB of dynamic LDS has its limit raised on each device's first launch
template <auto KERN>
void raise_lds_limit(size_t smem) {
  static std::atomic<uint64_t> attr_done{0};
  dd_ensure_dyn_lds(reinterpret_cast<const void*>(KERN), smem, attr_done);
}
template <auto KERN>
int launch_kernel(dim3 grid, int threads, size_t smem, hipStream_t s, const GemmParams& p) {
  raise_lds_limit<KERN>(smem);
  hipLaunchKernelGGL(KERN, grid, dim3(threads), smem, s, p);
  return dd_check_launch();
}

// ---- table-driven dispatch: L::run<T, I, FORM>(p, pl, s) for row I = pl.tile_idx, compiled for exactly the rows of family
// L::family whose forms hold FORM (and L::needs) — the bits the planner asked before it chose the tile
template <typename L, typename T, unsigned FORM, size_t I>
int launch_row(const GemmParams& p, const Plan& pl, hipStream_t s) {
  if constexpr (kTiles[I].family == L::family && (kTiles[I].forms & (FORM | L::needs)) == (FORM | L::needs))
    return L::template run<T, I, FORM>(p, pl, s);
  else return DD_ERR_UNSUPPORTED;
}
template <typename L, typename T, unsigned FORM, size_t... I>
int launch_rows(const GemmParams& p, const Plan& pl, hipStream_t s, std::index_sequence<I...>) {
  int rc = DD_ERR_UNSUPPORTED;
  (void)((pl.tile_idx == (int)I && ((rc = launch_row<L, T, FORM, I>(p, pl, s)), true)) || ...);
  return rc;
}
template <typename L, unsigned... FORMS>          // FORMS: the forms this translation unit instantiates
int dispatch(int dtype, unsigned form, const GemmParams& p, const Plan& pl, hipStream_t s) {
  constexpr auto rows = std::make_index_sequence<kNumTiles>{};
  int rc = DD_ERR_UNSUPPORTED;
  (void)((form == FORMS && ((rc = dtype == DD_F16 ? launch_rows<L, _Float16, FORMS>(p, pl, s, rows)
                                                  : launch_rows<L, __bf16, FORMS>(p, pl, s, rows)), true)) || ...);
  return rc;
}

}  // namespace ddg
