// JPEG output: uint8 frames (m, H, W, 3) in device memory -> the .jpg files the reference saves, byte for byte.
//
// The reference hands every generated view to PIL's `Image.save(<name>.jpg)` with no options
// (perception/data_prepare/val_set_gen.py:44, tools/downstream_v3_batched.py:244-252): libjpeg's baseline encoder at
// quality 75, 4:2:0 chroma, the standard Huffman tables, the `islow` integer DCT.  All of it is integer arithmetic, so the
// bytes are reproduced exactly.  Six launches on the caller's stream, none of which depends on m or on the content:
//
//   blocks    one wave per MCU (16 x 16 pixels): colour conversion, edge replication per component, 2 x 2 chroma
//             downsampling, the forward DCT of the 4 Y + Cb + Cr blocks, quantisation, libjpeg's dummy blocks; int16
//             coefficients in zigzag order to the workspace.
//   count     one wave per MCU, one lane per coefficient: the Huffman bit count of every block, summed per MCU.
//   scan      one workgroup per frame: exclusive prefix sum of the MCU bit counts = every MCU's bit offset in the frame's
//             unstuffed stream, the frame's bit total, and zeroes in the stream words that two MCUs share.
//   emit      one wave per MCU: the same codes again, assembled MSB-first in LDS and written to the stream; words that
//             belong to one MCU alone are stored, the (zeroed) words it shares with a neighbour take an atomicOr.  The
//             last MCU fills the last byte with 1-bits.
//   ffcount   0xFF bytes per 4 KB chunk of the stream.
//   assemble  header + stream with a 0x00 behind every 0xFF + FF D9 into the frame's output row, every store bounded by
//             the row's capacity, and the frame's true length.
//
// The tables (quantisation values in zigzag order as the header's DQT segments hold them, and the Huffman codes) come
// from the caller, built once per quality on the host (pipeline/image_output.py).  A lane's code is at most 16 + 15 bits
// and a block holds at most three ZRL codes, so a block is at most 64 * 31 + 48 bits: the stream is sized at 64 words per
// block, and every stream access is bounded by that size as well, whatever the tables hold.
#include "dd_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / DD_WAVE;     // MCUs per workgroup
constexpr int kMcuWords = 6 * 64;              // stream words an MCU can fill
constexpr int kBufWords = kMcuWords + 4;       // + the bits before its offset in the first word, + the final padding
constexpr int kChunk = 4096;                   // bytes of the unstuffed stream per workgroup of the last two launches
constexpr int kScanThreads = 1024;
constexpr int64_t kMaxMcus = 262144;           // bit offsets are 32-bit: 262144 * 6 * 64 * 32 < 2^32

// natural (row-major) index of the i-th coefficient of the zigzag scan
__device__ const uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                        41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                        30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct Geom {
  int32_t h, w;
  int32_t mw, nmcu;                            // MCUs per row, per frame
  int32_t ybw, ybh;                            // real Y blocks per row / column: ceil(w / 8), ceil(h / 8)
  int32_t chh;                                 // real chroma rows: ceil(h / 2)
  int32_t nchunk;                              // chunks the stream of a frame can hold
  int64_t stream_words;                        // per frame, a multiple of 4
};

// Workspace, every part 16-byte aligned:
//   int16 coef[m][nmcu][6][64] | uint32 mcu_bits[m][nmcu] | uint32 mcu_off[m][nmcu] | uint32 frame_bits[m] |
//   uint32 chunk_ff[m][nchunk] | uint32 stream[m][stream_words]
struct Layout {
  int64_t coef, mcu_bits, mcu_off, frame_bits, chunk_ff, stream, total;
};

static inline int64_t up16(int64_t v) { return (v + 15) & ~(int64_t)15; }

static inline bool geometry(int32_t m, int32_t h, int32_t w, Geom* g, Layout* l) {
  const int64_t mw = (w + 15) / 16, mh = (h + 15) / 16, nmcu = mw * mh;
  if (nmcu > kMaxMcus) return false;
  g->h = h; g->w = w; g->mw = (int32_t)mw; g->nmcu = (int32_t)nmcu;
  g->ybw = (w + 7) / 8; g->ybh = (h + 7) / 8; g->chh = (h + 1) / 2;
  g->stream_words = (nmcu * kMcuWords + 4 + 3) & ~(int64_t)3;
  g->nchunk = (int32_t)((g->stream_words * 4 + kChunk - 1) / kChunk);
  int64_t at = 0;
  l->coef = at; at += up16((int64_t)m * nmcu * 6 * 64 * 2);
  l->mcu_bits = at; at += up16((int64_t)m * nmcu * 4);
  l->mcu_off = at; at += up16((int64_t)m * nmcu * 4);
  l->frame_bits = at; at += up16((int64_t)m * 4);
  l->chunk_ff = at; at += up16((int64_t)m * g->nchunk * 4);
  l->stream = at; at += up16((int64_t)m * g->stream_words * 4);
  l->total = at;
  return true;
}

// ---- blocks -------------------------------------------------------------------------------------------------------------

// One pass of jfdctint.c over p[0], p[stride], ..., p[7 * stride], in place.  PASS 1 (rows): outputs 0 and 4 are scaled up
// by PASS1_BITS = 2, the others descaled by CONST_BITS - PASS1_BITS = 11; PASS 2 (columns): descaled by 2 and by 15.
template <int PASS>
__device__ __forceinline__ void dd_fdct8(int32_t* p, int stride) {
  constexpr int N = PASS == 1 ? 11 : 15;
  constexpr int32_t R = 1 << (N - 1);
  const int32_t d0 = p[0], d1 = p[stride], d2 = p[2 * stride], d3 = p[3 * stride];
  const int32_t d4 = p[4 * stride], d5 = p[5 * stride], d6 = p[6 * stride], d7 = p[7 * stride];
  const int32_t t0 = d0 + d7, t7 = d0 - d7, t1 = d1 + d6, t6 = d1 - d6;
  const int32_t t2 = d2 + d5, t5 = d2 - d5, t3 = d3 + d4, t4 = d3 - d4;
  const int32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  if (PASS == 1) {
    p[0] = (t10 + t11) * 4;
    p[4 * stride] = (t10 - t11) * 4;
  } else {
    p[0] = (t10 + t11 + 2) >> 2;
    p[4 * stride] = (t10 - t11 + 2) >> 2;
  }
  const int32_t y1 = (t12 + t13) * 4433;
  p[2 * stride] = (y1 + t13 * 6270 + R) >> N;
  p[6 * stride] = (y1 - t12 * 15137 + R) >> N;
  const int32_t z5 = (t4 + t6 + t5 + t7) * 9633;
  const int32_t z1 = (t4 + t7) * -7373, z2 = (t5 + t6) * -20995;
  const int32_t z3 = (t4 + t6) * -16069 + z5, z4 = (t5 + t7) * -3196 + z5;
  p[7 * stride] = (t4 * 2446 + z1 + z3 + R) >> N;
  p[5 * stride] = (t5 * 16819 + z2 + z4 + R) >> N;
  p[3 * stride] = (t6 * 25172 + z2 + z3 + R) >> N;
  p[1 * stride] = (t7 * 12299 + z1 + z4 + R) >> N;
}

__global__ __launch_bounds__(kThreads)
void dd_jpeg_blocks_kernel(const uint8_t* __restrict__ frames, const uint32_t* __restrict__ tables,
                           int16_t* __restrict__ coef, const Geom g) {
  __shared__ int32_t s_blk[kWaves][6][64];     // samples - 128, then DCT coefficients, natural order
  __shared__ int32_t s_c[kWaves][2][256];      // Cb, Cr of the MCU's 16 x 16 pixels
  __shared__ __attribute__((aligned(4))) int16_t s_q[kWaves][6][64];   // quantised, zigzag order
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t img = blockIdx.y;
  const int mcu_raw = blockIdx.x * kWaves + wave;
  const bool active = mcu_raw < g.nmcu;
  const int mcu = active ? mcu_raw : g.nmcu - 1;             // an idle wave works on a valid MCU and stores nothing
  const int my = mcu / g.mw, mx = mcu - my * g.mw;

  // pixels, edges replicated: Y into its four blocks, Cb / Cr at full size
  const uint8_t* f = frames + img * g.h * g.w * 3;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int p = lane + 64 * i, py = p >> 4, px = p & 15;
    const int y = min(my * 16 + py, g.h - 1), x = min(mx * 16 + px, g.w - 1);
    const uint8_t* s = f + ((int64_t)y * g.w + x) * 3;
    const int32_t r = s[0], gg = s[1], b = s[2];
    const int32_t yy = (19595 * r + 38470 * gg + 7471 * b + 32768) >> 16;
    const int32_t cb = (-11059 * r - 21709 * gg + 32768 * b + (128 << 16) + 32767) >> 16;
    const int32_t cr = (32768 * r - 27439 * gg - 5329 * b + (128 << 16) + 32767) >> 16;
    s_blk[wave][(py >> 3) * 2 + (px >> 3)][(py & 7) * 8 + (px & 7)] = yy - 128;
    s_c[wave][0][p] = cb;
    s_c[wave][1][p] = cr;
  }
  __syncthreads();
  // chroma: rows are replicated on the DOWNSAMPLED plane (chroma row chh - 1 repeats), columns on the full-size one
  {
    const int cr = lane >> 3, cc = lane & 7;
    const int rc = min(my * 8 + cr, g.chh - 1);
    const int r0 = min(2 * rc, g.h - 1) - my * 16, r1 = min(2 * rc + 1, g.h - 1) - my * 16;       // both in [0, 16)
    const int bias = 1 + (cc & 1);
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int32_t* pl = s_c[wave][c];
      s_blk[wave][4 + c][lane] = ((pl[r0 * 16 + 2 * cc] + pl[r0 * 16 + 2 * cc + 1] + pl[r1 * 16 + 2 * cc] +
                                   pl[r1 * 16 + 2 * cc + 1] + bias) >> 2) - 128;
    }
  }
  __syncthreads();
  if (lane < 48) dd_fdct8<1>(&s_blk[wave][lane >> 3][(lane & 7) * 8], 1);
  __syncthreads();
  if (lane < 48) dd_fdct8<2>(&s_blk[wave][lane >> 3][lane & 7], 8);
  __syncthreads();
  // quantise by 8 q, rounding half away from zero; a Y block outside the image is a dummy block: no AC, DC below
  const int nat = kZigzag[lane];
#pragma unroll
  for (int b = 0; b < 6; ++b) {
    const int32_t q = (int32_t)min(max(tables[(b >= 4 ? 64 : 0) + lane], 1u), 65535u) * 8;
    const int32_t c = s_blk[wave][b][nat];
    int32_t v = (abs(c) + (q >> 1)) / q;
    v = c < 0 ? -v : v;
    const bool real = b >= 4 || (2 * my + (b >> 1) < g.ybh && 2 * mx + (b & 1) < g.ybw);
    s_q[wave][b][lane] = (int16_t)(real ? v : 0);
  }
  __syncthreads();
  // dummy blocks take the DC of the block before them in their row, a dummy bottom row that of block 1
  if (lane == 0) {
    const bool right = 2 * mx + 1 >= g.ybw, bottom = 2 * my + 1 >= g.ybh;
    if (right) s_q[wave][1][0] = s_q[wave][0][0];
    if (bottom) {
      s_q[wave][2][0] = s_q[wave][1][0];
      s_q[wave][3][0] = s_q[wave][1][0];
    } else if (right) {
      s_q[wave][3][0] = s_q[wave][2][0];
    }
  }
  __syncthreads();
  if (active) {
    uint32_t* dst = reinterpret_cast<uint32_t*>(coef + (img * g.nmcu + mcu) * 6 * 64);
    const uint32_t* src = reinterpret_cast<const uint32_t*>(&s_q[wave][0][0]);
#pragma unroll
    for (int i = 0; i < 3; ++i) dst[lane + 64 * i] = src[lane + 64 * i];
  }
}

// ---- codes --------------------------------------------------------------------------------------------------------------

struct LaneCode {
  uint32_t zrl;                                // ZRL codes in front (0..3)
  uint32_t bits, nbits;                        // Huffman code and magnitude bits, nbits <= 31
};

__device__ __forceinline__ uint32_t dd_huff_len(uint32_t e) { return min(e & 255u, 16u); }
__device__ __forceinline__ uint32_t dd_huff_code(uint32_t e) { return (e >> 8) & ((1u << dd_huff_len(e)) - 1u); }

// What lane `lane` of a wave contributes to a block whose zigzag coefficient `lane` is v (lane 0: the DC difference).
// nz: ballot of v != 0.  dc / ac: the component's tables.
__device__ __forceinline__ LaneCode dd_jpeg_lane_code(int32_t v, int lane, uint64_t nz, const uint32_t* dc,
                                                      const uint32_t* ac) {
  LaneCode c = {0u, 0u, 0u};
  const uint32_t a = (uint32_t)abs(v);
  const uint32_t size = min(a ? 32u - (uint32_t)__builtin_clz(a) : 0u, 15u);
  const uint32_t mag = (uint32_t)(v < 0 ? v - 1 : v) & ((1u << size) - 1u);
  if (lane == 0) {
    const uint32_t e = dc[size];
    c.bits = (dd_huff_code(e) << size) | mag;
    c.nbits = dd_huff_len(e) + size;
  } else if (v != 0) {
    const uint64_t before = nz & ((1ull << lane) - 1ull) & ~1ull;             // non-zero AC coefficients in front
    const int prev = before ? 63 - __builtin_clzll(before) : 0;
    const uint32_t run = (uint32_t)(lane - 1 - prev);
    const uint32_t e = ac[((run & 15u) << 4) | size];
    c.zrl = run >> 4;
    c.bits = (dd_huff_code(e) << size) | mag;
    c.nbits = dd_huff_len(e) + size;
  } else if (lane == 63) {                                                   // the block ends in zeros: EOB
    c.bits = dd_huff_code(ac[0]);
    c.nbits = dd_huff_len(ac[0]);
  }
  return c;
}

// Coefficient `lane` of block b of an MCU, the DC as its difference from the previous block of the component in scan
// order (Y00 Y01 Y10 Y11 Cb Cr per MCU, predictors 0 at the first MCU).  cm: the MCU's coefficients.
__device__ __forceinline__ int32_t dd_jpeg_value(const int16_t* cm, int b, int lane, int mcu) {
  int32_t v = cm[b * 64 + lane];
  if (lane == 0) {
    int32_t pred = 0;
    if (b >= 1 && b <= 3) pred = cm[(b - 1) * 64];
    else if (mcu > 0) pred = cm[-6 * 64 + (b == 0 ? 3 : b) * 64];
    v -= pred;
  }
  return v;
}

__device__ __forceinline__ void dd_load_huff(uint32_t* s_tab, const uint32_t* tables) {
  for (int i = threadIdx.x; i < 32 + 512; i += kThreads) s_tab[i] = tables[128 + i];      // tables: q[2][64] | dc[2][16] | ac[2][256]
}

__global__ __launch_bounds__(kThreads)
void dd_jpeg_count_kernel(const int16_t* __restrict__ coef, const uint32_t* __restrict__ tables,
                          uint32_t* __restrict__ mcu_bits, const Geom g) {
  __shared__ uint32_t s_tab[32 + 512];
  dd_load_huff(s_tab, tables);
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t img = blockIdx.y;
  const int mcu = blockIdx.x * kWaves + wave;
  if (mcu >= g.nmcu) return;
  const int16_t* cm = coef + (img * g.nmcu + mcu) * 6 * 64;
  const uint32_t zlen = dd_huff_len(s_tab[32 + 0xF0]), zlen_c = dd_huff_len(s_tab[32 + 256 + 0xF0]);
  uint32_t bits = 0;
#pragma unroll
  for (int b = 0; b < 6; ++b) {
    const int32_t v = dd_jpeg_value(cm, b, lane, mcu);
    const uint64_t nz = __ballot(v != 0);
    const int t = b >= 4;
    const LaneCode c = dd_jpeg_lane_code(v, lane, nz, s_tab + 16 * t, s_tab + 32 + 256 * t);
    bits += c.zrl * (t ? zlen_c : zlen) + c.nbits;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) bits += __shfl_xor(bits, o, 64);
  if (lane == 0) mcu_bits[img * g.nmcu + mcu] = bits;
}

// One workgroup per frame: thread t owns the `per` consecutive MCUs from t * per.
__global__ __launch_bounds__(kScanThreads)
void dd_jpeg_scan_kernel(const uint32_t* __restrict__ mcu_bits, uint32_t* __restrict__ mcu_off,
                         uint32_t* __restrict__ frame_bits, uint32_t* __restrict__ stream, const Geom g) {
  __shared__ uint32_t s_sum[kScanThreads];
  const int tid = threadIdx.x;
  const int64_t img = blockIdx.x;
  const uint32_t* in = mcu_bits + img * g.nmcu;
  uint32_t* off = mcu_off + img * g.nmcu;
  uint32_t* st = stream + img * g.stream_words;
  const int per = (g.nmcu + kScanThreads - 1) / kScanThreads;
  const int i0 = min(tid * per, g.nmcu), i1 = min(i0 + per, g.nmcu);
  uint32_t mine = 0;
  for (int i = i0; i < i1; ++i) mine += in[i];
  s_sum[tid] = mine;
  __syncthreads();
  for (int d = 1; d < kScanThreads; d <<= 1) {               // inclusive scan of the threads' sums
    const uint32_t add = tid >= d ? s_sum[tid - d] : 0u;
    __syncthreads();
    s_sum[tid] += add;
    __syncthreads();
  }
  uint32_t at = s_sum[tid] - mine;
  for (int i = i0; i < i1; ++i) {
    off[i] = at;
    if ((int64_t)(at >> 5) < g.stream_words) st[at >> 5] = 0u;                // the word an MCU may share with the one before
    at += in[i];
  }
  if (tid == kScanThreads - 1) frame_bits[img] = s_sum[tid];
}

// `nbits` <= 32 bits of `value` at bit `pos` of the MSB-first stream image in LDS
__device__ __forceinline__ void dd_put_bits(uint32_t* buf, uint32_t pos, uint32_t value, uint32_t nbits) {
  if (nbits == 0) return;
  const uint32_t sh = pos & 31u, w = pos >> 5;
  if (w + 1 >= (uint32_t)kBufWords) return;                                  // cannot happen: see the size of a block above
  const uint64_t v = (uint64_t)value << (64u - sh - nbits);
  atomicOr(&buf[w], (uint32_t)(v >> 32));
  if ((uint32_t)v) atomicOr(&buf[w + 1], (uint32_t)v);
}

__global__ __launch_bounds__(kThreads)
void dd_jpeg_emit_kernel(const int16_t* __restrict__ coef, const uint32_t* __restrict__ tables,
                         const uint32_t* __restrict__ mcu_off, uint32_t* __restrict__ stream, const Geom g) {
  __shared__ uint32_t s_tab[32 + 512];
  __shared__ uint32_t s_buf[kWaves][kBufWords];
  dd_load_huff(s_tab, tables);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  uint32_t* buf = s_buf[wave];
  for (int i = lane; i < kBufWords; i += DD_WAVE) buf[i] = 0u;
  __syncthreads();
  const int64_t img = blockIdx.y;
  const int mcu_raw = blockIdx.x * kWaves + wave;
  const bool active = mcu_raw < g.nmcu;
  const int mcu = active ? mcu_raw : g.nmcu - 1;             // an idle wave repeats the last MCU in its own LDS, stores nothing
  const int16_t* cm = coef + (img * g.nmcu + mcu) * 6 * 64;
  const uint32_t off = mcu_off[img * g.nmcu + mcu];
  uint32_t pos = off & 31u;                                                  // bit position in buf
#pragma unroll
  for (int b = 0; b < 6; ++b) {
    const int32_t v = dd_jpeg_value(cm, b, lane, mcu);
    const uint64_t nz = __ballot(v != 0);
    const int t = b >= 4;
    const uint32_t* ac = s_tab + 32 + 256 * t;
    const LaneCode c = dd_jpeg_lane_code(v, lane, nz, s_tab + 16 * t, ac);
    const uint32_t zcode = dd_huff_code(ac[0xF0]), zlen = dd_huff_len(ac[0xF0]);
    const uint32_t len = c.zrl * zlen + c.nbits;
    uint32_t incl = len;                                                     // inclusive prefix sum over the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t up = __shfl_up(incl, o, 64);
      if (lane >= o) incl += up;
    }
    uint32_t at = pos + incl - len;
    for (uint32_t z = 0; z < c.zrl; ++z) {
      dd_put_bits(buf, at, zcode, zlen);
      at += zlen;
    }
    dd_put_bits(buf, at, c.bits, c.nbits);
    pos += __shfl(incl, 63, 64);
  }
  const bool last = mcu == g.nmcu - 1;
  const uint32_t end = pos;                                                  // before the padding
  if (last) {                                                                // fill the frame's last byte with 1-bits
    const uint32_t pad = (8u - (pos & 7u)) & 7u;
    if (lane == 0) dd_put_bits(buf, pos, (1u << pad) - 1u, pad);
    pos += pad;
  }
  __syncthreads();
  if (!active) return;
  // Word 0 may hold the end of the MCU before (the scan zeroed it), the last word the start of the next one: atomicOr.
  // Every other word is this MCU's alone and is stored whole, as is the frame's last word.
  uint32_t* st = stream + img * g.stream_words;
  const int64_t base = off >> 5;
  const int nw = (int)((pos + 31u) >> 5);
  for (int j = lane; j < nw; j += DD_WAVE) {
    const int64_t k = base + j;
    if (k >= g.stream_words) break;
    const uint32_t word = __builtin_bswap32(buf[j]);                         // MSB-first bits as bytes in memory order
    const bool shared = j == 0 || (j == nw - 1 && !last && (end & 31u) != 0u);
    if (shared) atomicOr(&st[k], word);
    else st[k] = word;
  }
}

// ---- stuffing and assembly ----------------------------------------------------------------------------------------------

__device__ __forceinline__ uint32_t dd_block_sum(uint32_t v, uint32_t* s_red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  uint32_t t = 0;
#pragma unroll
  for (int i = 0; i < kWaves; ++i) t += s_red[i];
  return t;
}

__device__ __forceinline__ int64_t dd_stream_bytes(const uint32_t* frame_bits, int64_t img, const Geom& g) {
  const int64_t n = ((int64_t)frame_bits[img] + 7) >> 3;
  return min(n, g.stream_words * 4);
}

// this thread's 16 bytes of the chunk, and how many of them are stream bytes
__device__ __forceinline__ int dd_load16(const uint32_t* st, int64_t first, int64_t nbytes, uint8_t (&b)[16]) {
  const int n = (int)max((int64_t)0, min((int64_t)16, nbytes - first));
  if (n > 0) {
    const u32x4 v = dd_ld16(reinterpret_cast<const uint8_t*>(st) + first);   // a frame's stream is a multiple of 16 bytes
    __builtin_memcpy(b, &v, 16);
  }
  return n;
}

__global__ __launch_bounds__(kThreads)
void dd_jpeg_ffcount_kernel(const uint32_t* __restrict__ stream, const uint32_t* __restrict__ frame_bits,
                            uint32_t* __restrict__ chunk_ff, const Geom g) {
  __shared__ uint32_t s_red[kWaves];
  const int64_t img = blockIdx.y;
  const int64_t nbytes = dd_stream_bytes(frame_bits, img, g);
  const int64_t c0 = (int64_t)blockIdx.x * kChunk;
  if (c0 >= nbytes) return;
  uint8_t b[16];
  const int n = dd_load16(stream + img * g.stream_words, c0 + threadIdx.x * 16, nbytes, b);
  uint32_t ff = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) ff += (i < n && b[i] == 0xFF) ? 1u : 0u;
  ff = dd_block_sum(ff, s_red);
  if (threadIdx.x == 0) chunk_ff[img * g.nchunk + blockIdx.x] = ff;
}

__global__ __launch_bounds__(kThreads)
void dd_jpeg_assemble_kernel(const uint32_t* __restrict__ stream, const uint32_t* __restrict__ frame_bits,
                             const uint32_t* __restrict__ chunk_ff, const uint8_t* __restrict__ header,
                             int32_t header_len, uint8_t* __restrict__ out, int64_t capacity,
                             int32_t* __restrict__ lengths, const Geom g) {
  __shared__ uint32_t s_red[kWaves];
  __shared__ uint32_t s_scan[kThreads];
  const int tid = threadIdx.x;
  const int64_t img = blockIdx.y;
  const int64_t nbytes = dd_stream_bytes(frame_bits, img, g);
  const int chunk = blockIdx.x;
  const bool tail = chunk == g.nchunk;                       // the extra workgroup: header, FF D9, length
  const int64_t c0 = (int64_t)chunk * kChunk;
  if (!tail && c0 >= nbytes) return;
  // 0xFF bytes in the chunks before this one (tail: in all of them)
  const int before = tail ? (int)((nbytes + kChunk - 1) / kChunk) : chunk;
  uint32_t ffs = 0;
  for (int i = tid; i < before; i += kThreads) ffs += chunk_ff[img * g.nchunk + i];
  ffs = dd_block_sum(ffs, s_red);
  uint8_t* row = out + img * capacity;
  if (tail) {
    for (int i = tid; i < header_len && i < capacity; i += kThreads) row[i] = header[i];
    const int64_t len = (int64_t)header_len + nbytes + ffs + 2;
    if (tid == 0) {
      if (len - 2 < capacity) row[len - 2] = 0xFF;
      if (len - 1 < capacity) row[len - 1] = 0xD9;
      lengths[img] = (int32_t)len;
    }
    return;
  }
  uint8_t b[16];
  const int n = dd_load16(stream + img * g.stream_words, c0 + tid * 16, nbytes, b);
  uint32_t ff = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) ff += (i < n && b[i] == 0xFF) ? 1u : 0u;
  s_scan[tid] = ff;
  __syncthreads();
  for (int d = 1; d < kThreads; d <<= 1) {                   // inclusive scan of the threads' counts
    const uint32_t add = tid >= d ? s_scan[tid - d] : 0u;
    __syncthreads();
    s_scan[tid] += add;
    __syncthreads();
  }
  int64_t at = (int64_t)header_len + c0 + tid * 16 + ffs + (s_scan[tid] - ff);
  for (int i = 0; i < n; ++i) {
    if (at < capacity) row[at] = b[i];
    ++at;
    if (b[i] == 0xFF) {
      if (at < capacity) row[at] = 0x00;
      ++at;
    }
  }
}

}  // namespace

extern "C" int64_t dd_jpeg_workspace_bytes(int32_t m, int32_t h, int32_t w) {
  if (m <= 0 || m > 65535 || h <= 0 || w <= 0 || h > 65535 || w > 65535) return -1;
  Geom g;
  Layout l;
  if (!geometry(m, h, w, &g, &l)) return -1;
  return l.total;
}

extern "C" int dd_jpeg_encode_u8(const uint8_t* frames, int32_t m, int32_t h, int32_t w, const uint8_t* header,
                                 int32_t header_len, const uint32_t* tables, void* workspace, int64_t workspace_bytes,
                                 uint8_t* out, int64_t capacity, int32_t* lengths, dd_stream_t stream) {
  if (!frames || !header || !tables || !workspace || !out || !lengths) return DD_ERR_BAD_ARG;
  if (m <= 0 || h <= 0 || w <= 0 || h > 65535 || w > 65535 || header_len <= 0) return DD_ERR_BAD_ARG;
  if (capacity < (int64_t)header_len + 2) return DD_ERR_BAD_ARG;
  if (!dd_aligned16(workspace) || (reinterpret_cast<uintptr_t>(tables) & 3u) || (reinterpret_cast<uintptr_t>(lengths) & 3u))
    return DD_ERR_BAD_ARG;
  Geom g;
  Layout l;
  if (!geometry(m, h, w, &g, &l) || m > 65535) return DD_ERR_UNSUPPORTED;
  if (workspace_bytes < l.total) return DD_ERR_BAD_ARG;
  uint8_t* ws = reinterpret_cast<uint8_t*>(workspace);
  int16_t* coef = reinterpret_cast<int16_t*>(ws + l.coef);
  uint32_t* mcu_bits = reinterpret_cast<uint32_t*>(ws + l.mcu_bits);
  uint32_t* mcu_off = reinterpret_cast<uint32_t*>(ws + l.mcu_off);
  uint32_t* frame_bits = reinterpret_cast<uint32_t*>(ws + l.frame_bits);
  uint32_t* chunk_ff = reinterpret_cast<uint32_t*>(ws + l.chunk_ff);
  uint32_t* bits = reinterpret_cast<uint32_t*>(ws + l.stream);
  const dim3 per_mcu((unsigned)((g.nmcu + kWaves - 1) / kWaves), (unsigned)m);
  hipStream_t s = dd_stream(stream);
  dd_clear_error();
  hipLaunchKernelGGL(dd_jpeg_blocks_kernel, per_mcu, dim3(kThreads), 0, s, frames, tables, coef, g);
  hipLaunchKernelGGL(dd_jpeg_count_kernel, per_mcu, dim3(kThreads), 0, s, coef, tables, mcu_bits, g);
  hipLaunchKernelGGL(dd_jpeg_scan_kernel, dim3((unsigned)m), dim3(kScanThreads), 0, s, mcu_bits, mcu_off, frame_bits, bits, g);
  hipLaunchKernelGGL(dd_jpeg_emit_kernel, per_mcu, dim3(kThreads), 0, s, coef, tables, mcu_off, bits, g);
  hipLaunchKernelGGL(dd_jpeg_ffcount_kernel, dim3((unsigned)g.nchunk, (unsigned)m), dim3(kThreads), 0, s, bits, frame_bits,
                     chunk_ff, g);
  hipLaunchKernelGGL(dd_jpeg_assemble_kernel, dim3((unsigned)g.nchunk + 1, (unsigned)m), dim3(kThreads), 0, s, bits,
                     frame_bits, chunk_ff, header, header_len, out, capacity, lengths, g);
  return dd_check_launch();
}
