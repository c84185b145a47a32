// JPEG input, the decode core: everything of csrc/jpeg_decode.hip that touches the bit stream or a coefficient, as plain
// functions that compile for the device and for the host.  The kernels call them one lane at a time; the stand-alone host
// program tools/jpeg_decode_host_check.cpp runs the same functions in the same order under the address and undefined-
// behaviour sanitizers, over good and over broken streams, so that the bounds below are checked without a GPU.
//
// The stream these functions read is the entropy-coded segment with the FF 00 stuffing already removed (the kernels'
// count / compact passes do that), as 32-bit words in memory order.  A position is a bit index into it.
//
// What holds whatever the stream and the tables contain:
//   - a read touches words [0, nwords) only; bits at and behind `nbits` read as 1 (the filler);
//   - a symbol consumes at least one bit, so a loop over symbols ends after at most `limit - pos` turns;
//   - a coefficient is written at block < total_blocks, index < 64 only;
//   - table entries are never trusted: lengths are clamped to 1..16, value indices masked to 0..255, selectors to 0..1.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DD_JD_HD __host__ __device__ __forceinline__
#else
#define DD_JD_HD inline
#endif

#ifndef DD_JD_SUB_BITS
#define DD_JD_SUB_BITS 1024                    // S: bits of the stream per subsequence (one lane each); profiles/jpeg_input.txt
#endif

// per-frame status bits
#define DD_JD_EXHAUSTED 1                      // the stream ended before the frame's last block
#define DD_JD_BAD_CODE 2                       // a bit pattern that is in no Huffman table, or a symbol baseline does not have
#define DD_JD_BAD_RUN 4                        // a run of zeros that passes coefficient 63
#define DD_JD_TRAILING 8                       // a byte or more of the stream is left behind the frame's last block

// One Huffman table, built by the host from the file's (bits, values) (pipeline/jpeg_input.py: huffman_block).
struct DdJdHuff {
  uint16_t lut[256];                           // the next 8 bits -> (length << 8) | symbol; 0: the code is longer than 8 bits
  int32_t lim[17];                             // lim[l]: the next 16 bits are a code of length <= l iff they are below it
  int32_t off[17];                             // the symbol of a code of length l is vals[off[l] + (next 16 bits >> (16 - l))]
  uint8_t vals[256];
};

// The table block of one frame.
struct DdJdTables {
  uint16_t q[3][64];                           // quantisation values per component, natural (row-major) order
  uint8_t tdc[3], tac[3];                      // DC / AC table selector per component
  uint8_t pad[2];
  DdJdHuff huff[4];                            // DC 0, DC 1, AC 0, AC 1
  uint8_t tail[8];                             // to a multiple of 16 bytes
};
static_assert(sizeof(DdJdHuff) == 904, "table layout");
static_assert(sizeof(DdJdTables) == 4016, "table layout");

// Where a decoder stands: at bit `pos`, in block `blk` of the MCU, before coefficient `idx` of it (0: the DC symbol is
// next); nblk counts the blocks completed since the entry it started from.
struct DdJdState {
  int32_t pos, blk, idx, nblk;
};

// the entry states of two decoders agree (nblk is relative and takes no part)
DD_JD_HD bool dd_jd_same(const DdJdState& a, const DdJdState& b) {
  return a.pos == b.pos && a.blk == b.blk && a.idx == b.idx;
}

DD_JD_HD uint32_t dd_jd_bswap(uint32_t v) { return __builtin_bswap32(v); }

// The 32 bits at `pos` (0 <= pos < nbits), MSB first; bits at and behind nbits are 1.
DD_JD_HD uint32_t dd_jd_peek32(const uint32_t* words, int32_t nwords, int32_t nbits, int32_t pos) {
  const int32_t w = pos >> 5, sh = pos & 31;
  const int32_t w0 = w < nwords ? w : nwords - 1, w1 = w + 1 < nwords ? w + 1 : nwords - 1;
  const uint32_t hi = dd_jd_bswap(words[w0]), lo = dd_jd_bswap(words[w1]);
  uint32_t v = sh ? (hi << sh) | (lo >> (32 - sh)) : hi;
  const int32_t valid = nbits - pos;
  if (valid < 32) v |= valid <= 0 ? 0xFFFFFFFFu : 0xFFFFFFFFu >> valid;
  return v;
}

// The symbol at the top of v -> its value, *len = its code length (1..16).  A pattern in no table: symbol 0, length 16, flag.
DD_JD_HD uint32_t dd_jd_symbol(const DdJdHuff* t, uint32_t v, int32_t* len, uint32_t* flags) {
  const uint32_t c = v >> 16;
  const uint32_t e = t->lut[c >> 8];
  int32_t l = (int32_t)(e >> 8);
  uint32_t sym = e & 255u;
  if (l == 0) {
    for (l = 9; l <= 16; ++l)
      if ((int32_t)c < t->lim[l]) break;
    if (l > 16) {
      *flags |= DD_JD_BAD_CODE;
      l = 16;
      sym = 0;
    } else {
      sym = t->vals[((uint32_t)t->off[l] + (c >> (16 - l))) & 255u];
    }
  }
  *len = l < 1 ? 1 : (l > 16 ? 16 : l);
  return sym;
}

// block of the MCU -> component: 4:2:0 (6 blocks) Y Y Y Y Cb Cr, 4:4:4 (3 blocks) Y Cb Cr
DD_JD_HD int32_t dd_jd_component(int32_t blk, int32_t bpm) { return bpm == 6 ? (blk < 4 ? 0 : blk - 3) : blk; }

// Decodes the symbols that start in [s.pos, limit) from entry state s and returns the exit state.  limit <= nbits.
// WRITE: the non-zero coefficients (zigzag order) and, at index 0, the DC differences go to coef[block * 64 + index] of
// the blocks from first_block on; decoding stops at total_blocks, what is left of the stream is padding.  Flags are
// raised in both modes; only the WRITE pass, which starts from a true entry, reports them.
template <bool WRITE>
DD_JD_HD DdJdState dd_jd_decode_sub(const uint32_t* words, int32_t nwords, int32_t nbits, int32_t limit, DdJdState s,
                                    const DdJdTables* t, int32_t bpm, int16_t* coef, int32_t first_block,
                                    int32_t total_blocks, uint32_t* flags) {
  s.nblk = 0;
  if (limit > nbits) limit = nbits;
  if (s.blk < 0 || s.blk >= bpm) s.blk = 0;
  if (s.idx < 0 || s.idx > 63) s.idx = 0;
  while (s.pos >= 0 && s.pos < limit) {
    const int32_t block = first_block + s.nblk;
    if (WRITE && (block < 0 || block >= total_blocks)) break;
    const int32_t comp = dd_jd_component(s.blk, bpm);
    const bool dc = s.idx == 0;
    const DdJdHuff* tab = &t->huff[dc ? (t->tdc[comp] & 1) : 2 + (t->tac[comp] & 1)];
    const uint32_t v = dd_jd_peek32(words, nwords, nbits, s.pos);
    int32_t len;
    const uint32_t sym = dd_jd_symbol(tab, v, &len, flags);
    const int32_t size = (int32_t)(sym & 15u), run = (int32_t)(sym >> 4);
    int32_t value = 0;
    if (size) {
      const int32_t extra = (int32_t)((v << len) >> (32 - size));            // len + size <= 31
      value = extra < (1 << (size - 1)) ? extra - (1 << size) + 1 : extra;
    }
    s.pos += len + size;
    if (WRITE && s.pos > nbits) *flags |= DD_JD_EXHAUSTED;
    bool end = false;
    if (dc) {
      if (sym > 11u) *flags |= DD_JD_BAD_CODE;                               // baseline: DC sizes 0..11
      if (WRITE) coef[(int64_t)block * 64] = (int16_t)value;
      s.idx = 1;
    } else if (size == 0) {
      if (run == 15) {                                                       // ZRL: sixteen zeros
        s.idx += 16;
        if (s.idx > 63) {
          *flags |= DD_JD_BAD_RUN;
          end = true;
        }
      } else {                                                               // EOB (a run with it belongs to progressive files)
        if (run) *flags |= DD_JD_BAD_CODE;
        end = true;
      }
    } else {
      s.idx += run;
      if (s.idx > 63) {
        *flags |= DD_JD_BAD_RUN;
        end = true;
      } else {
        if (WRITE) coef[(int64_t)block * 64 + s.idx] = (int16_t)value;
        end = ++s.idx == 64;
      }
    }
    if (end) {
      if (WRITE && block + 1 == total_blocks && nbits - s.pos >= 8) *flags |= DD_JD_TRAILING;   // more than padding
      s.idx = 0;
      s.blk = s.blk + 1 == bpm ? 0 : s.blk + 1;
      ++s.nblk;
    }
  }
  return s;
}

// ---- from coefficients to pixels ----------------------------------------------------------------------------------------

// zigzag position of the natural (row-major) index
DD_JD_HD int32_t dd_jd_zigzag_of(int32_t natural) {
  const uint8_t z[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30,
                         41, 43, 9,  11, 18, 24, 31, 40, 44, 53, 10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38,
                         46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};
  return z[natural & 63];
}

// One pass of libjpeg's jidctint.c (`islow`) over d[0..7]: CONST_BITS 13, PASS1_BITS 2; descale by `shift` (11 in the
// column pass, 18 in the row pass).  The sums are taken modulo 2^32, which is libjpeg's int arithmetic wherever that does
// not overflow, and defined for any input.
DD_JD_HD void dd_jd_idct8(int32_t* d, int32_t shift) {
  typedef uint32_t u;
  const u i0 = (u)d[0], i1 = (u)d[1], i2 = (u)d[2], i3 = (u)d[3], i4 = (u)d[4], i5 = (u)d[5], i6 = (u)d[6], i7 = (u)d[7];
  u z1 = (i2 + i6) * 4433u;
  const u e2 = z1 + i6 * (u)-15137, e3 = z1 + i2 * 6270u;
  const u e0 = (i0 + i4) * 8192u, e1 = (i0 - i4) * 8192u;
  const u t10 = e0 + e3, t13 = e0 - e3, t11 = e1 + e2, t12 = e1 - e2;
  u o0 = i7, o1 = i5, o2 = i3, o3 = i1;
  z1 = o0 + o3;
  u z2 = o1 + o2, z3 = o0 + o2, z4 = o1 + o3;
  const u z5 = (z3 + z4) * 9633u;
  o0 *= 2446u; o1 *= 16819u; o2 *= 25172u; o3 *= 12299u;
  z1 *= (u)-7373; z2 *= (u)-20995;
  z3 = z3 * (u)-16069 + z5;
  z4 = z4 * (u)-3196 + z5;
  o0 += z1 + z3; o1 += z2 + z4; o2 += z2 + z3; o3 += z1 + z4;
  const u r = 1u << (shift - 1);
  d[0] = (int32_t)(t10 + o3 + r) >> shift;
  d[7] = (int32_t)(t10 - o3 + r) >> shift;
  d[1] = (int32_t)(t11 + o2 + r) >> shift;
  d[6] = (int32_t)(t11 - o2 + r) >> shift;
  d[2] = (int32_t)(t12 + o1 + r) >> shift;
  d[5] = (int32_t)(t12 - o1 + r) >> shift;
  d[3] = (int32_t)(t13 + o0 + r) >> shift;
  d[4] = (int32_t)(t13 - o0 + r) >> shift;
}

DD_JD_HD int32_t dd_jd_clamp255(int32_t v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// Column `col` of block `coef` (zigzag order) dequantised by q (natural order) through the column pass -> ws[row * 8 + col]
DD_JD_HD void dd_jd_idct_column(const int16_t* coef, const uint16_t* q, int32_t col, int32_t* ws) {
  int32_t d[8];
  for (int r = 0; r < 8; ++r) {
    const int32_t n = r * 8 + col;
    d[r] = (int32_t)coef[dd_jd_zigzag_of(n)] * (int32_t)q[n];
  }
  dd_jd_idct8(d, 11);
  for (int r = 0; r < 8; ++r) ws[r * 8 + col] = d[r];
}

// Row `row` of ws through the row pass, + 128, clamped -> out[0..7]
DD_JD_HD void dd_jd_idct_row(const int32_t* ws, int32_t row, uint8_t* out) {
  int32_t d[8];
  for (int c = 0; c < 8; ++c) d[c] = ws[row * 8 + c];
  dd_jd_idct8(d, 18);
  for (int c = 0; c < 8; ++c) out[c] = (uint8_t)dd_jd_clamp255(d[c] + 128);
}

// libjpeg's h2v2 upsampling of plane p (stride `stride`, true size tch x tcw) at output pixel (y, x): the "fancy" triangle
// filter, each edge replicating its own row / column — but, as jdsample.c chooses it, only for a chroma plane more than two
// columns wide; a narrower one (frames of width 1..4) is replicated 2 x 2 in both directions.
DD_JD_HD int32_t dd_jd_upsample(const uint8_t* p, int32_t stride, int32_t tch, int32_t tcw, int32_t y, int32_t x) {
  if (tcw <= 2) return (int32_t)p[(int64_t)(y >> 1) * stride + (x >> 1)];
  const int32_t cy = y >> 1, cx = x >> 1;
  int32_t fy = (y & 1) ? cy + 1 : cy - 1, fx = (x & 1) ? cx + 1 : cx - 1;
  fy = fy < 0 ? 0 : (fy > tch - 1 ? tch - 1 : fy);
  fx = fx < 0 ? 0 : (fx > tcw - 1 ? tcw - 1 : fx);
  const int32_t s = 3 * (int32_t)p[(int64_t)cy * stride + cx] + (int32_t)p[(int64_t)fy * stride + cx];
  const int32_t o = 3 * (int32_t)p[(int64_t)cy * stride + fx] + (int32_t)p[(int64_t)fy * stride + fx];
  return (3 * s + o + ((x & 1) ? 7 : 8)) >> 4;
}

// jdcolor.c's 16-bit fixed point: FIX(1.402) 91881, FIX(1.772) 116130, FIX(0.34414) 22554, FIX(0.71414) 46802
DD_JD_HD void dd_jd_rgb(int32_t y, int32_t cb, int32_t cr, uint8_t* rgb) {
  cb -= 128;
  cr -= 128;
  rgb[0] = (uint8_t)dd_jd_clamp255(y + ((91881 * cr + 32768) >> 16));
  rgb[1] = (uint8_t)dd_jd_clamp255(y + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
  rgb[2] = (uint8_t)dd_jd_clamp255(y + ((116130 * cb + 32768) >> 16));
}
