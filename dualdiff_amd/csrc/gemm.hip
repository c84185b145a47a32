// GEMM / conv host side: the planner over the tile table (gemm_tiles.h), the split-K reduce, and the C entry points.
// The kernels are in the family translation units (gemm1.hip, gemm23.hip, gemm2_geglu.hip, gemm2_conv.hip, gemm2_upfold.hip, gemm4.hip, conv3s.hip).
#include "gemm_device.h"
#include <algorithm>
#include <cmath>

namespace {

template <typename T>
__global__ __launch_bounds__(256)
void dd_splitk_reduce_kernel(const GemmParams p, int nsplit) {
  const int64_t groups_per_row = p.n / 8;
  const int64_t total = (int64_t)p.rows * groups_per_row;
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total;
       g += (int64_t)gridDim.x * blockDim.x) {
    const int row = (int)(g / groups_per_row);
    const int col = (int)(g - (int64_t)row * groups_per_row) * 8;
    float v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int z = 0; z < nsplit; ++z) {
      const float* src = p.partial + ((int64_t)z * p.rows + row) * p.n + col;
      const f32x4 a = *reinterpret_cast<const f32x4*>(src);
      const f32x4 b = *reinterpret_cast<const f32x4*>(src + 4);
      v[0] += a[0]; v[1] += a[1]; v[2] += a[2]; v[3] += a[3];
      v[4] += b[0]; v[5] += b[1]; v[6] += b[2]; v[7] += b[3];
    }
    epilogue_store8<T>(p, row, col, v);
  }
}

int ceil_div(int a, int b) { return (a + b - 1) / b; }

// The LDS-DMA family wants a K structure in whole 64-element steps (no step straddles a conv tap or
// the a/a2 seam) and buffers below 2^31 bytes (32-bit lane offsets, DD_OOB out of range for all).
bool dma_ok(const dd_gemm_desc* d) {
  const int64_t lim = (int64_t)1 << 30;              // elements
  const int64_t nw = (d->epilogue == DD_EPI_GEGLU ? 2 : 1) * (int64_t)d->n;
  bool ok = (d->k % BK) == 0 && nw * d->k < lim;
  if (d->conv) {
    ok = ok && (d->cin % BK) == 0 && (int64_t)d->rows / (d->hout * d->wout) * d->hin * d->win * d->cin < lim;
  } else {
    ok = ok && (int64_t)d->rows * d->lda < lim;
    if (d->a2) ok = ok && (d->k1 % BK) == 0 && (int64_t)d->rows * d->lda2 < lim;
  }
  return ok;
}

// ---- folded-upsample conv (dd_gemm_desc.upfold): the classes of the output coordinates of one axis -------------------
// torch nearest, as the 9-tap kernels compute it: min(floor(dst * (float)(in / out)), in - 1)
int upfold_src(int o, int in, int out) { return std::min((int)floorf((float)o * ((float)in / (float)out)), in - 1); }

// Class of output coordinate o (UpfoldTab), or -1 where no class reproduces its three taps.  Slot 0 / 1 of class 0 and 2
// reads source s - 1 / s and of class 1 s / s + 1, s = src(o); the taps go to slots (0 | 1 1), (0 0 | 1), (0 | 1 | dropped).
// A tap inside the output must find its own source in its slot; a tap outside it (zero padding) must be dropped or sit in a
// slot outside the source image, which the DMA fills with zeros.
int upfold_class(int o, int in, int out) {
  const int s = upfold_src(o, in, out);
  for (int c = 0; c < 3; ++c) {
    bool ok = true;
    for (int t = -1; t <= 1 && ok; ++t) {
      const bool tap_in = o + t >= 0 && o + t < out;
      if (c == 2 && t == 1) { ok = !tap_in; continue; }
      const int src = (c == 1 ? s : s - 1) + (c == 1 ? t == 1 : t >= 0);
      const bool src_in = src >= 0 && src < in;
      ok = tap_in ? src_in && upfold_src(o + t, in, out) == src : !src_in;
    }
    if (ok) return c;
  }
  return -1;
}

// the coordinates of an axis class by class; false where the fold does not apply
bool upfold_axis(int in, int out, uint8_t* list, uint8_t* n, uint8_t* start) {
  if (in <= 0 || out <= in || out > kUpfoldMax) return false;
  int pos = 0;
  for (int c = 0; c < 3; ++c) {
    start[c] = (uint8_t)pos;
    for (int o = 0; o < out; ++o) {
      const int k = upfold_class(o, in, out);
      if (k < 0) return false;
      if (k == c) list[pos++] = (uint8_t)o;
    }
    n[c] = (uint8_t)(pos - start[c]);
  }
  return true;
}

// the class table of a descriptor for row tiles of bm rows; false where the fold does not apply
bool upfold_tab(const dd_gemm_desc* d, int bm, UpfoldTab* t, int* tiles_m, int* ncls) {
  *t = UpfoldTab{};
  if (!d->conv || d->stride != 1 || d->hout != d->hv || d->wout != d->wv || d->hout <= 0 || d->wout <= 0) return false;
  if (!upfold_axis(d->hin, d->hv, t->y, t->ny, t->y0) || !upfold_axis(d->win, d->wv, t->x, t->nx, t->x0)) return false;
  t->m = d->rows / (d->hout * d->wout);
  int tiles = 0, w = 0;
  for (int c = 0; c < 9; ++c) {
    const int plane = t->ny[c / 3] * t->nx[c % 3];
    t->tile0[c] = (uint16_t)tiles;
    t->widx[c] = (uint8_t)w;
    t->inv_plane[c] = plane ? 1.0f / (float)plane : 1.0f;
    if (plane) ++w;
    tiles += (t->m * plane + bm - 1) / bm;
    if (tiles > 65535) return false;
  }
  t->tile0[9] = (uint16_t)tiles;
  for (int c = 0; c < 3; ++c) t->inv_nx[c] = t->nx[c] ? 1.0f / (float)t->nx[c] : 1.0f;
  *tiles_m = tiles;
  *ncls = w;
  return true;
}

// DD_PERSIST=0 / DD_PERSIST3=0: the A/B switches of the two persistent forms, read once
bool env_is_zero(const char* name) { const char* v = getenv(name); return v && atoi(v) == 0; }
bool persist_off() { static const bool off = env_is_zero("DD_PERSIST"); return off; }
bool persist3_off() { static const bool off = env_is_zero("DD_PERSIST3"); return off; }

// bytes of a [rows][ld] matrix of T whose rows hold n elements; buffer descriptors address extents below 2^31
int64_t extent_bytes(const dd_gemm_desc* d, int64_t ld) { return (((int64_t)d->rows - 1) * ld + d->n) * 2; }
constexpr int64_t kExtentLimit = (int64_t)1 << 31;

// the first tile of a family with the wave / block shape of `like`, or -1
int twin(const TileCfg& like, Family family) {
  for (int i = 0; i < kNumTiles; ++i)
    if (kTiles[i].family == family && kTiles[i].wm == like.wm && kTiles[i].wn == like.wn && kTiles[i].tm == like.tm &&
        kTiles[i].tn == like.tn) return i;
  return -1;
}

Plan unsupported() { Plan pl{}; pl.unsupported = true; return pl; }

// direct small-image conv, and its BAND form on row bands with a halo (images larger than the tile)
Plan plan_direct(const dd_gemm_desc* d, int ti, unsigned form) {
  const TileCfg& t = kTiles[ti];
  const int hw = d->hout * d->wout, W = d->wout;
  const int arows = tile_bm(t) + 88;               // = the BAND kernel's AROWS
  const int R = W > 0 ? std::min(tile_bm(t), arows - 16 - 2 * (W + 1)) / W : 0;      // whole image rows per band
  const bool ok = form == F_CONV && d->stride == 1 && d->hv == d->hin && d->wv == d->win && d->hout == d->hin &&
                  d->wout == d->win && (d->cin % BK) == 0 && hw > 0 && d->rows % hw == 0 && dma_ok(d) &&
                  (t.band ? hw > tile_bm(t) && R >= 1 : hw <= tile_bm(t) && tile_bm(t) < 65535);
  if (!ok) return unsupported();
  const int m_inst = d->rows / hw;
  Plan pl{};
  pl.tile_idx = ti;
  if (t.band) {
    pl.band_rows = R * W;
    pl.bands = ceil_div(d->hout, R);
    pl.g_per_tile = 1;
    pl.tiles_m = m_inst * pl.bands;
  } else {
    pl.g_per_tile = std::min(tile_bm(t) / hw, m_inst);
    pl.tiles_m = ceil_div(m_inst, pl.g_per_tile);
  }
  const int nchunks = d->cin / BK;                 // split-K is over channel chunks
  const int split = std::min(d->split_k > 0 ? d->split_k : 1, nchunks);
  pl.chunks_per_split = ceil_div(nchunks, split);
  pl.tiles_n = ceil_div(d->n, tile_bn(t));
  pl.split = ceil_div(nchunks, pl.chunks_per_split);
  pl.k_per_split = pl.chunks_per_split * BK;
  return pl;
}

// the form a descriptor asks for; pad_lo == 0 is F_PAD0 (validate_pad: conv, stride 2, no upsample, no GEGLU)
unsigned form_of(const dd_gemm_desc* d, int pad_lo) {
  return pad_lo == 0 ? F_PAD0 : d->conv && d->upfold ? F_UPFOLD : d->conv ? F_CONV : d->epilogue == DD_EPI_GEGLU ? F_GEGLU : F_DENSE;
}

Plan make_plan(const dd_gemm_desc* d, int pad_lo) {
  const bool geglu = d->epilogue == DD_EPI_GEGLU;
  const unsigned form = form_of(d, pad_lo);
  int ti = d->tile > 0 ? tile_index(d->tile) : -1;
  if (ti < 0) {
    // heuristic: biggest tile that still yields >= ~1.5 waves of blocks; else the smallest one that has the form
    for (int id : kAutoTiles) {
      const TileCfg& t = kTiles[tile_index(id)];
      if (!(t.forms & form)) continue;
      ti = tile_index(id);
      const int bn_out = geglu ? tile_bn(t) / 2 : tile_bn(t);
      if ((long)ceil_div(d->rows, tile_bm(t)) * ceil_div(d->n, bn_out) >= (long)kNumCU * 3 / 2) break;
    }
  }
  if (ti < 0) {
    if (form != F_UPFOLD) return unsupported();
    // no tile named (a direct caller with the tuner off): the model folds only shapes of the tracked table, with their tile
    ti = tile_index(d->rows >= 8192 ? 28 : 52);
  }
  if (d->ln_colsum) {                                // LayerNorm fold lives in the LDS-DMA family only
    // heuristic picked a register-staged tile: take its LDS-DMA twin (round 5 removed the 2-slot 128x64 / 64x64 tiles the
    // old table {11, 17, 14, 18} pointed at, so the twin is looked up by shape)
    const int ring = twin(kTiles[ti], FAM_RING);
    if (d->tile <= 0 && ring >= 0) ti = ring;
    if (kTiles[ti].family != FAM_RING || !dma_ok(d)) return unsupported();
  }
  if (kTiles[ti].family == FAM_PIPE && d->conv) return unsupported();   // dense only, and no fall-back from it
  if (d->ln_out) {                                   // LayerNorm-emitting epilogue: the 80x320 tiles, one column tile
    if (d->tile > 0 && !(kTiles[ti].forms & F_LN_OUT)) return unsupported();
    // auto: the pipelined form — one tile per workgroup while its row tiles are one residency generation (153 KB of LDS: one
    // workgroup per CU), the persistent walk of dd_gemm4_kernel beyond (round 6: 67200 x 320 x 320 46.5 us against 56.4 for
    // the dd_gemm2 form's walk, x 1280 112.7 against 143.7: profiles/r06_gemm3_bound.txt); with DD_PERSIST3=0 the round-5
    // rule (beyond one generation the dd_gemm2 form)
    if (d->tile <= 0) {
      const int pipe = tile_index(kTileLnPipe);
      ti = (!persist3_off() || ceil_div(d->rows, tile_bm(kTiles[pipe])) <= kNumCU) ? pipe : tile_index(kTileLnRing);
    }
    if (d->n != 320 || !dma_ok(d)) return unsupported();
  }
  if (kTiles[ti].family == FAM_DIRECT) return plan_direct(d, ti, form);
  // the folded-upsample conv: no other family has the form, and its epilogue is the plain T store
  if (form == F_UPFOLD && (kTiles[ti].family != FAM_RING || !dma_ok(d) || d->ln_stats_out || d->out_f32)) return unsupported();
  if (kTiles[ti].family != FAM_REG && !dma_ok(d)) {  // same tile shape, register-staged family
    const int reg = twin(kTiles[ti], FAM_REG);       // no twin: 128x128 (GEGLU-capable) / 64x64
    ti = reg >= 0 ? reg : tile_index(geglu ? kTile128x128 : kTile64x64);
  }
  const TileCfg& t = kTiles[ti];
  // forms the tile's launcher instantiates no kernel for (the same bits gate its `if constexpr`): GEGLU on a tile whose waves
  // hold two 16-column blocks, a convolution on the 32-row and whole-row tiles, pad_lo = 0 outside the register-staged family
  if (!(t.forms & form)) return unsupported();
  Plan pl{};
  const int bn_out = geglu ? tile_bn(t) / 2 : tile_bn(t);
  pl.tile_idx = ti;
  pl.tiles_m = ceil_div(d->rows, tile_bm(t));
  pl.tiles_n = ceil_div(d->n, bn_out);
  if (form == F_UPFOLD) {                            // row tiles class by class; one [n][k] weight matrix per class
    int ncls = 0;
    if (!upfold_tab(d, tile_bm(t), &pl.upf, &pl.tiles_m, &ncls) || (int64_t)ncls * d->n * d->k >= ((int64_t)1 << 30))
      return unsupported();
  }
  int split = d->split_k;
  const int nkt = ceil_div(d->k, BK);
  if (split <= 0) {                                  // auto: two waves of workgroups, at least 4 K-steps each, at most 32 slabs
    const long blocks = (long)pl.tiles_m * pl.tiles_n;
    const bool deep = !geglu && blocks < kNumCU && nkt >= 16;
    split = deep ? (int)std::max(1L, std::min({(2L * kNumCU + blocks - 1) / blocks, (long)nkt / 4, 32L})) : 1;
  }
  if (geglu || d->ln_colsum || d->ln_stats_out || d->out_headmajor_d || d->ln_out) split = 1;
  if (split > nkt) split = nkt;
  int kts = ceil_div(nkt, split);
  split = ceil_div(nkt, kts);
  pl.split = split;
  pl.k_per_split = kts * BK;
  const bool walk = (t.forms & F_PERSIST) && !d->conv && split == 1 && !d->ln_colsum && nkt >= t.depth;
  // persistent walk with cross-tile prefetch (dd_gemm2_kernel): dense, one K range per tile, no epilogue that uses
  // LDS or per-tile LDS state, and a K loop at least as long as the ring
  pl.persist_ok = walk && t.family == FAM_RING && !persist_off() && !d->ln_out;
  // persistent walk of the PIPELINED family (dd_gemm4_kernel, round 6): split == 1, K in whole steps and at least as long
  // as the ring, an epilogue with a fixed number of memory operations (plain / head-major / GEGLU / the LayerNorm tile),
  // buffer-descriptor addressing (31-bit extents)
  const bool ln_tile = (t.forms & F_LN_OUT) != 0;
  const bool pre_acc = !geglu && !ln_tile && t.tm * (t.tn / 2) <= 4;
  pl.persist3_ok = walk && t.family == FAM_PIPE && !persist3_off() && (d->k % BK) == 0 && !d->out_f32 && !d->ln_stats_out &&
                   !d->rowvec && (!d->accumulate || pre_acc) && ln_tile == (d->ln_out != nullptr) &&
                   extent_bytes(d, d->ldc) < kExtentLimit && (!d->res || extent_bytes(d, d->ldres) < kExtentLimit) &&
                   (!d->ln_out || extent_bytes(d, d->ld_ln_out) < kExtentLimit);
  return pl;
}

inline bool gemm4_takes(const Plan& pl) {          // the persistent form: more tiles than one residency generation
  return pl.persist3_ok && pl.tiles_m * pl.tiles_n > kNumCU * gemm4_resident(kTiles[pl.tile_idx]);
}

LaunchFn* launcher(const Plan& pl, unsigned form) {     // the translation unit that holds the tile's kernel in this form
  switch (kTiles[pl.tile_idx].family) {
    case FAM_REG: return launch_gemm1;
    case FAM_RING: return form == F_UPFOLD ? launch_gemm2_upfold : form == F_CONV ? launch_gemm2_conv : form == F_GEGLU ? launch_gemm2_geglu : launch_gemm2_dense;
    case FAM_PIPE: return gemm4_takes(pl) ? launch_gemm4 : launch_gemm3;
    default: return launch_conv3s;
  }
}

// pad_lo: top / left padding of a conv (dd_gemm_conv_pad); the output size is that of the (pad_lo, 1) padded image
int validate(const dd_gemm_desc* d, int pad_lo = 1) {
  if (!d || !d->a || !d->w || !d->out) return DD_ERR_BAD_ARG;
  if (d->ln_colsum) {                                  // LayerNorm fold
    if (!d->ln_bias || d->conv || d->a2 || d->bias) return DD_ERR_BAD_ARG;
    if (d->k != 320 && d->k != 640 && d->k != 1280) return DD_ERR_UNSUPPORTED;
    if (!dd_aligned16(d->ln_colsum) || !dd_aligned16(d->ln_bias) || (d->lda & 7)) return DD_ERR_BAD_ARG;
  }
  if (d->ln_out) {                                     // LayerNorm emitted by the epilogue (80x320 tile)
    if (!d->lno_gamma || !d->lno_beta || d->conv || d->epilogue != DD_EPI_NONE || d->rowvec || d->accumulate ||
        d->out_f32 || d->out_headmajor_d || d->ln_stats_out || d->ln_colsum)
      return DD_ERR_UNSUPPORTED;
    if (d->n != 320) return DD_ERR_UNSUPPORTED;
    if (!dd_aligned16(d->ln_out) || !dd_aligned16(d->lno_gamma) || !dd_aligned16(d->lno_beta) || (d->ld_ln_out & 7))
      return DD_ERR_BAD_ARG;
  }
  if (d->rows <= 0 || d->n <= 0 || d->k <= 0) return DD_ERR_BAD_ARG;
  if (d->rows >= (1 << 22)) return DD_ERR_UNSUPPORTED;         // dd_fdiv's exactness bound (largest real case: 1.08 M)
  if ((d->k & 7) || (d->n & 7) || (d->ldc & 7)) return DD_ERR_BAD_ARG;
  if (d->dtype != DD_F16 && d->dtype != DD_BF16) return DD_ERR_BAD_ARG;
  if (!dd_aligned16(d->a) || !dd_aligned16(d->w) || !dd_aligned16(d->out)) return DD_ERR_BAD_ARG;
  if (d->bias && !dd_aligned16(d->bias)) return DD_ERR_BAD_ARG;
  if (d->res && (!dd_aligned16(d->res) || (d->ldres & 7))) return DD_ERR_BAD_ARG;
  if (d->rowvec && (!dd_aligned16(d->rowvec) || (d->ld_rowvec & 7) || d->rows_per_inst <= 0)) return DD_ERR_BAD_ARG;
  if (d->conv) {
    if (d->a2) return DD_ERR_UNSUPPORTED;
    if (d->cin <= 0 || (d->cin & 7) || d->k != (d->upfold ? 4 : 9) * d->cin) return DD_ERR_BAD_ARG;
    if (d->hin <= 0 || d->win <= 0 || d->hout <= 0 || d->wout <= 0) return DD_ERR_BAD_ARG;
    if (d->stride != 1 && d->stride != 2) return DD_ERR_UNSUPPORTED;
    if (d->hv <= 0 || d->wv <= 0) return DD_ERR_BAD_ARG;
    if (d->rows % (d->hout * d->wout) != 0) return DD_ERR_BAD_ARG;
    if ((d->hv + pad_lo + 1 - 3) / d->stride + 1 != d->hout || (d->wv + pad_lo + 1 - 3) / d->stride + 1 != d->wout)
      return DD_ERR_BAD_ARG;
  } else {
    if (d->lda & 7) return DD_ERR_BAD_ARG;
    if (d->a2) {
      if (!dd_aligned16(d->a2) || (d->lda2 & 7) || (d->k1 & 7) || d->k1 <= 0 || d->k1 >= d->k) return DD_ERR_BAD_ARG;
    }
  }
  if (d->epilogue != DD_EPI_NONE && d->epilogue != DD_EPI_GEGLU && d->epilogue != DD_EPI_SILU) return DD_ERR_BAD_ARG;
  if (d->out_f32 && (d->epilogue == DD_EPI_GEGLU || d->accumulate)) return DD_ERR_UNSUPPORTED;
  if (d->ln_stats_out && ((d->n & 31) || d->epilogue == DD_EPI_GEGLU || d->out_f32 || !dd_aligned16(d->ln_stats_out)))
    return DD_ERR_UNSUPPORTED;
  if (d->ln_stats_in && (!d->ln_colsum || !dd_aligned16(d->ln_stats_in))) return DD_ERR_BAD_ARG;
  if (d->out_headmajor_d) {
    if (d->out_headmajor_d < 8 || (d->out_headmajor_d & 7) || d->n % d->out_headmajor_d) return DD_ERR_BAD_ARG;
    if (d->conv || d->epilogue == DD_EPI_GEGLU || d->accumulate || d->out_f32 || d->ln_stats_out) return DD_ERR_UNSUPPORTED;
  }
  if (d->epilogue == DD_EPI_GEGLU && (d->res || d->rowvec || d->accumulate || d->alpha != 1.0f)) return DD_ERR_UNSUPPORTED;
  if (d->epilogue == DD_EPI_GEGLU && d->conv) return DD_ERR_UNSUPPORTED;      // no tile carries a conv + GEGLU kernel
  if (d->upfold && (!d->conv || pad_lo != 1)) return DD_ERR_BAD_ARG;         // (whether the map folds is the planner's answer)
  return DD_OK;
}

// pad_lo = 0 exists for one layer: Downsample2D(padding=0) — conv, stride 2, no upsample, plain or SiLU epilogue.
// hout = (hin - 2) / 2 + 1 needs hin >= 2 (a 1-pixel image padded to 2 has no 3x3 window).
int validate_pad(const dd_gemm_desc* d, int pad_lo) {
  if (pad_lo != 0 && pad_lo != 1) return DD_ERR_BAD_ARG;
  if (pad_lo == 1) return validate(d);
  if (!d || !d->conv) return DD_ERR_BAD_ARG;
  if (d->stride != 2 || d->hv != d->hin || d->wv != d->win || d->epilogue == DD_EPI_GEGLU) return DD_ERR_UNSUPPORTED;
  if (d->hin < 2 || d->win < 2) return DD_ERR_BAD_ARG;
  return validate(d, 0);
}

thread_local char g_kname[160];

}  // namespace

extern "C" int dd_gemm_num_tiles(void) { return kNumTiles; }
extern "C" int dd_gemm_tile_id(int index) { return (index >= 0 && index < kNumTiles) ? kTiles[index].id : -1; }

// Split-K workspace layout: [DD_COUNTER_BYTES, reserved][split fp32 slabs].  The reserved head held the arrival counters
// of the in-launch reduction (round 3, removed in round 5: slower than the reduce launch on every split-K shape of the
// step); the slab offset is kept because dd_groupnorm_splitk's callers address the slabs behind it.
constexpr int64_t DD_COUNTER_BYTES = 65536;

namespace {

int64_t workspace_bytes(const dd_gemm_desc* d, int pad_lo) {
  if (validate_pad(d, pad_lo) != DD_OK) return 0;
  const Plan pl = make_plan(d, pad_lo);
  if (pl.unsupported || pl.split <= 1) return 0;
  return DD_COUNTER_BYTES + (int64_t)pl.split * d->rows * d->n * (int64_t)sizeof(float);
}

const char* kernel_name(const dd_gemm_desc* d, int pad_lo) {
  const int vc = validate_pad(d, pad_lo);
  if (vc != DD_OK) return (pad_lo == 0 && vc == DD_ERR_UNSUPPORTED) ? "unsupported" : "invalid";
  const Plan pl = make_plan(d, pad_lo);
  if (pl.unsupported) return "unsupported";
  const TileCfg& t = kTiles[pl.tile_idx];
  // demangled template-argument form, as rocprofv3 prints the kernel symbol: the row's arguments behind <T, WM, WN, TM, TN
  const char* conv = d->conv ? "true" : "false";
  const char* geglu = d->epilogue == DD_EPI_GEGLU ? "true" : "false";
  const char* kern = "dd_gemm_pad0_kernel";
  char args[48] = "";
  if (pad_lo == 0) {
  } else if (t.family == FAM_DIRECT) {
    kern = "dd_conv3s_kernel";
    snprintf(args, sizeof(args), ", %d, %d, %s", t.depth, t.grp, t.band ? "true" : "false");
  } else if (t.family == FAM_PIPE) {
    kern = gemm4_takes(pl) ? "dd_gemm4_kernel" : "dd_gemm3_kernel";
    snprintf(args, sizeof(args), ", %d, %s", t.depth, geglu);
  } else if (t.family == FAM_RING && d->upfold) {
    kern = "dd_gemm2u_kernel";
    snprintf(args, sizeof(args), ", %d", t.depth);
  } else if (t.family == FAM_RING) {
    kern = "dd_gemm2_kernel";
    snprintf(args, sizeof(args), ", %d, %s, %s", t.depth, conv, geglu);
  } else {
    kern = "dd_gemm_kernel";
    snprintf(args, sizeof(args), ", %s, %s", conv, geglu);
  }
  snprintf(g_kname, sizeof(g_kname), "%s<%s, %d, %d, %d, %d%s> split=%d grid=%dx%d tile=%s", kern,
           d->dtype == DD_F16 ? "_Float16" : "__bf16", t.wm, t.wn, t.tm, t.tn, args, pl.split, pl.tiles_m, pl.tiles_n, t.name);
  return g_kname;
}

int gemm_run(const dd_gemm_desc* d, int pad_lo, dd_stream_t stream) {
  const int vc = validate_pad(d, pad_lo);
  if (vc != DD_OK) return vc;
  const Plan pl = make_plan(d, pad_lo);
  if (pl.unsupported) return DD_ERR_UNSUPPORTED;
  GemmParams p{};
  p.g_per_tile = pl.g_per_tile; p.chunks_per_split = pl.chunks_per_split;
  p.ln_colsum = reinterpret_cast<const float*>(d->ln_colsum);
  p.ln_bias = reinterpret_cast<const float*>(d->ln_bias);
  p.ln_eps = d->ln_eps;
  p.ln_out = d->ln_out; p.ld_ln_out = d->ld_ln_out; p.lno_gamma = d->lno_gamma; p.lno_beta = d->lno_beta;
  p.a = d->a; p.a2 = d->a2; p.lda = d->lda; p.lda2 = d->lda2;
  p.k1 = d->a2 ? d->k1 : d->k;
  p.rows = d->rows; p.n = d->n; p.k = d->k;
  p.w = d->w; p.bias = d->bias; p.rowvec = d->rowvec;
  p.rows_per_inst = d->rows_per_inst > 0 ? d->rows_per_inst : 1; p.ld_rowvec = d->ld_rowvec;
  p.res = d->res; p.ldres = d->ldres; p.out = d->out; p.ldc = d->ldc;
  p.alpha = d->alpha; p.accumulate = d->accumulate; p.out_f32 = d->out_f32;
  p.stat_out = reinterpret_cast<float*>(d->ln_stats_out);
  p.stat_in = reinterpret_cast<const float*>(d->ln_stats_in);
  p.hm_d = d->out_headmajor_d; p.hm_planes = d->hm_scaled_planes; p.hm_scale = d->hm_scale;
  p.act = d->epilogue == DD_EPI_SILU ? DD_EPI_SILU : DD_EPI_NONE;
  p.hin = d->hin; p.win = d->win; p.cin = d->cin; p.hv = d->hv; p.wv = d->wv;
  p.hout = d->hout; p.wout = d->wout; p.stride = d->stride;
  p.upsample = d->conv && (d->hv != d->hin || d->wv != d->win);
  // torch nearest: src = min(floor(dst * (in/out)), in-1) with a float scale
  p.scale_h = d->conv ? (float)d->hin / (float)d->hv : 1.f;
  p.scale_w = d->conv ? (float)d->win / (float)d->wv : 1.f;
  p.k_per_split = pl.k_per_split;
  p.tiles_m = pl.tiles_m; p.tiles_n = pl.tiles_n;
  p.band_rows = pl.band_rows; p.bands = pl.bands; p.inv_bands = pl.bands > 0 ? 1.0f / (float)pl.bands : 1.0f;
  p.inv_hw = d->conv ? 1.0f / (float)(d->hout * d->wout) : 1.0f;
  p.inv_wout = d->conv ? 1.0f / (float)d->wout : 1.0f;
  p.inv_rpi = 1.0f / (float)p.rows_per_inst;
  {
    const int64_t nw = (d->epilogue == DD_EPI_GEGLU ? 2 : 1) * (int64_t)d->n;
    p.w_bytes = (uint32_t)(nw * d->k * 2);
    if (d->upfold) {                                   // one matrix per non-empty class
      int ncls = 0;
      for (int c = 0; c < 9; ++c) ncls += pl.upf.tile0[c + 1] > pl.upf.tile0[c];
      p.w_bytes = (uint32_t)(ncls * nw * d->k * 2);
    }
    if (d->conv) {
      p.a_bytes = (uint32_t)((int64_t)d->rows / (d->hout * d->wout) * d->hin * d->win * d->cin * 2);
      p.a2_bytes = 0;
    } else {
      p.a_bytes = (uint32_t)((((int64_t)d->rows - 1) * d->lda + p.k1) * 2);
      p.a2_bytes = d->a2 ? (uint32_t)((((int64_t)d->rows - 1) * d->lda2 + (d->k - d->k1)) * 2) : 0u;
    }
  }
  {
    // extents for the buffer-descriptor epilogue of the pipelined family (T output; 32-bit byte offsets)
    const int64_t ob = extent_bytes(d, d->ldc), rb = extent_bytes(d, d->ldres);
    const bool fits = ob < kExtentLimit && (!d->res || rb < kExtentLimit);
    p.out_bytes = fits ? (uint32_t)ob : 0u;
    p.res_bytes = fits && d->res ? (uint32_t)rb : 0u;
  }
  p.persist = 0;
  p.inv_tiles_n = 1.0f / (float)(pl.tiles_n > 0 ? pl.tiles_n : 1);
  p.inv_hm_d = d->out_headmajor_d > 0 ? 1.0f / (float)d->out_headmajor_d : 1.0f;
  p.ln_out_bytes = d->ln_out ? (uint32_t)extent_bytes(d, d->ld_ln_out) : 0u;
  p.partial = nullptr;
  p.dbg_stamps = nullptr;
  DD_STAMP_HOST(p, d);
  if (pl.split > 1) {
    const int64_t need = DD_COUNTER_BYTES + (int64_t)pl.split * d->rows * d->n * (int64_t)sizeof(float);
    if (!d->ws || d->ws_bytes < need) return DD_ERR_WORKSPACE;
    p.partial = reinterpret_cast<float*>(reinterpret_cast<char*>(d->ws) + DD_COUNTER_BYTES);
  }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  dd_clear_error();
  if (d->phase != 2) {                      // phase 2: the reduce launch only (per-launch timing of a split-K GEMM)
    const int rc = launcher(pl, form_of(d, pad_lo))(d->dtype, form_of(d, pad_lo), p, pl, s);
    if (rc != DD_OK) return rc;
  }
  if (pl.split > 1 && d->phase != 1) {
    const int blocks = (int)std::min<int64_t>(((int64_t)p.rows * (p.n / 8) + 255) / 256, 2048);
    if (d->dtype == DD_F16) hipLaunchKernelGGL(dd_splitk_reduce_kernel<_Float16>, dim3(blocks), dim3(256), 0, s, p, pl.split);
    else hipLaunchKernelGGL(dd_splitk_reduce_kernel<__bf16>, dim3(blocks), dim3(256), 0, s, p, pl.split);
    return dd_check_launch();
  }
  return DD_OK;
}

}  // namespace

extern "C" int64_t dd_gemm_workspace_bytes(const dd_gemm_desc* d) { return workspace_bytes(d, 1); }
extern "C" const char* dd_gemm_kernel_name(const dd_gemm_desc* d) { return kernel_name(d, 1); }
extern "C" int dd_gemm(const dd_gemm_desc* d, dd_stream_t stream) { return gemm_run(d, 1, stream); }

extern "C" int dd_gemm_conv_pad(const dd_gemm_desc* d, int32_t pad_lo, dd_stream_t stream) {
  return gemm_run(d, pad_lo, stream);
}
extern "C" int64_t dd_gemm_conv_pad_workspace_bytes(const dd_gemm_desc* d, int32_t pad_lo) {
  return workspace_bytes(d, pad_lo);
}
extern "C" const char* dd_gemm_conv_pad_kernel_name(const dd_gemm_desc* d, int32_t pad_lo) {
  return kernel_name(d, pad_lo);
}
