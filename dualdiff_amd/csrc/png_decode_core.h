// PNG input, the decode core: everything of csrc/png_decode.hip that reads the deflate stream or has a bound to get wrong
// — the bit reader, the code-length to decode-table construction, symbol decode, the length / distance arithmetic, the
// stored-block header, the block walk itself and the Paeth predictor — as plain functions that compile for the device and
// for the host.  The kernels run the walk with all 64 lanes of one wave in step (every lane computes the same values from
// the same bytes; a `Ctx` says where the output goes and which lane writes the tables); the stand-alone host program
// tools/png_decode_host_check.cpp runs the same functions with a plain array behind them under the address and undefined-
// behaviour sanitizers, over good and over broken streams, so that the bounds below are checked without a GPU.
//
// What holds whatever the stream contains:
//   - a read touches bytes [0, n) of the stream only; bytes at and behind n read as 0, and consuming one of their bits is
//     DD_PD_TRUNCATED at the next check, which follows every symbol, every header and every stored block;
//   - a block header consumes at least 3 bits and a symbol at least 1, so the walk ends after at most 8 n + 3 turns;
//   - an output position never passes `limit`: the token that would pass it is DD_PD_TOO_LONG and is not written;
//   - a match never starts before output position 0 (DD_PD_BAD_DISTANCE);
//   - code lengths are 0..15 by construction, a table index is checked against the table's size, and a table is used only
//     after dd_pd_build accepted its lengths (not oversubscribed; incomplete only as zlib's inflate allows it: no code at
//     all, or one code of one bit — the one-code distance tree of RFC 1951 3.2.7, which csrc/png.hip writes).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DD_PD_HD __host__ __device__ __forceinline__
#else
#define DD_PD_HD inline
#endif

// per-frame status bits (include/dualdiff_hip.h: DD_PNG_*)
#define DD_PD_TRUNCATED 1                      // the stream ends inside a block, or before the four Adler-32 bytes
#define DD_PD_BAD_BLOCK 2                      // block type 3
#define DD_PD_BAD_STORED 4                     // a stored block whose LEN is not the complement of NLEN
#define DD_PD_BAD_LENGTHS 8                    // code lengths that are oversubscribed, incomplete, too many, or without symbol 256
#define DD_PD_BAD_SYMBOL 16                    // symbol 286 / 287, distance code 30 / 31, a repeat with nothing to repeat, a bit pattern in no code
#define DD_PD_BAD_DISTANCE 32                  // a match that starts before the first byte of the output
#define DD_PD_TOO_LONG 64                      // more bytes than the frame's filtered size
#define DD_PD_TOO_SHORT 128                    // the final block ends with fewer
#define DD_PD_BAD_ADLER 256                    // the Adler-32 of the filtered bytes is not the stream's
#define DD_PD_BAD_ZLIB 512                     // the two zlib header bytes: CM, CINFO, FCHECK or FDICT
#define DD_PD_BAD_FILTER 1024                  // a row's filter type byte above 4

#define DD_PD_LUT_BITS 9
#define DD_PD_MAX_LIT 288                      // the fixed code lists 288 literal / length symbols, a dynamic one at most 286
#define DD_PD_ADLER 65521u

// ---- the bit reader: LSB first (RFC 1951 3.1.1) ---------------------------------------------------------------------------

struct DdPdBits {
  const uint8_t* p;
  int64_t n;                                   // bytes of the stream
  int64_t at;                                  // the byte `ahead` starts at
  int64_t used;                                // bits consumed
  uint64_t buf;                                // the next `cnt` bits, the first one in bit 0
  int32_t cnt;
  uint32_t ahead;                              // the four bytes at `at`, loaded before they are needed
};

DD_PD_HD uint32_t dd_pd_byte(const DdPdBits& b, int64_t i) { return (i >= 0 && i < b.n) ? b.p[i] : 0u; }

// the four bytes from byte i on, the first one in the low bits; zeros outside the stream
DD_PD_HD uint32_t dd_pd_word(const DdPdBits& b, int64_t i) {
  if (i >= 0 && i + 4 <= b.n)
    return (uint32_t)b.p[i] | ((uint32_t)b.p[i + 1] << 8) | ((uint32_t)b.p[i + 2] << 16) | ((uint32_t)b.p[i + 3] << 24);
  return dd_pd_byte(b, i) | (dd_pd_byte(b, i + 1) << 8) | (dd_pd_byte(b, i + 2) << 16) | (dd_pd_byte(b, i + 3) << 24);
}

DD_PD_HD void dd_pd_seek(DdPdBits& b, int64_t byte) {
  b.at = byte;
  b.used = byte * 8;
  b.buf = 0;
  b.cnt = 0;
  b.ahead = dd_pd_word(b, byte);
}

DD_PD_HD void dd_pd_open(DdPdBits& b, const uint8_t* p, int64_t n) {
  b.p = p;
  b.n = n > 0 ? n : 0;
  dd_pd_seek(b, 0);
}

// at least 32 bits in the buffer; the word behind them is requested now and used by the next call, so that its way from
// memory overlaps the symbols in between
DD_PD_HD void dd_pd_fill(DdPdBits& b) {
  if (b.cnt >= 32) return;
  b.buf |= (uint64_t)b.ahead << b.cnt;
  b.cnt += 32;
  b.at += 4;
  b.ahead = dd_pd_word(b, b.at);
}

// the next k <= 24 bits, not consumed
DD_PD_HD uint32_t dd_pd_peek(DdPdBits& b, int k) {
  dd_pd_fill(b);
  return (uint32_t)b.buf & ((1u << k) - 1u);
}

DD_PD_HD void dd_pd_skip(DdPdBits& b, int k) {
  b.buf >>= k;
  b.cnt -= k;
  b.used += k;
}

DD_PD_HD uint32_t dd_pd_take(DdPdBits& b, int k) {
  const uint32_t v = dd_pd_peek(b, k);
  dd_pd_skip(b, k);
  return v;
}

// a bit behind the stream's end has been consumed
DD_PD_HD bool dd_pd_over(const DdPdBits& b) { return b.used > b.n * 8; }

DD_PD_HD void dd_pd_align(DdPdBits& b) { dd_pd_seek(b, (b.used + 7) >> 3); }

// ---- Huffman decode tables ------------------------------------------------------------------------------------------------

struct DdPdHuff {
  uint16_t lut[1 << DD_PD_LUT_BITS];           // the next 9 bits -> (length << 9) | symbol; 0: a longer code, or none
  uint16_t count[16];                          // codes per length
  uint16_t sym[DD_PD_MAX_LIT];                 // symbols in canonical order
};

DD_PD_HD uint32_t dd_pd_reverse(uint32_t code, int len) {
  uint32_t r = 0;
  for (int i = 0; i < len; ++i) r |= ((code >> i) & 1u) << (len - 1 - i);
  return r;
}

// lens[0..n) (each 0..15, n <= 288) -> h; false: the lengths are oversubscribed, or incomplete in a way zlib refuses.
// strict: not even the one-code form is let through (the code-length code, zlib's CODES).
DD_PD_HD bool dd_pd_build(DdPdHuff& h, const uint8_t* lens, int n, bool strict) {
  if (n > DD_PD_MAX_LIT) n = DD_PD_MAX_LIT;
  for (int i = 0; i < (1 << DD_PD_LUT_BITS); ++i) h.lut[i] = 0;
  for (int l = 0; l < 16; ++l) h.count[l] = 0;
  for (int s = 0; s < n; ++s) h.count[lens[s] & 15] += 1;
  const int used = n - h.count[0];
  int left = 1, maxlen = 0;
  for (int l = 1; l < 16; ++l) {
    left <<= 1;
    left -= h.count[l];
    if (left < 0) return false;                // oversubscribed
    if (h.count[l]) maxlen = l;
  }
  if (left > 0 && used != 0 && (strict || maxlen != 1)) return false;
  if (left > 0 && used == 0 && strict) return false;
  uint16_t offs[16], next[16];
  offs[0] = 0;
  offs[1] = 0;
  for (int l = 1; l < 15; ++l) offs[l + 1] = (uint16_t)(offs[l] + h.count[l]);
  uint32_t code = 0;
  next[0] = 0;
  for (int l = 1; l < 16; ++l) {
    code = (code + (l > 1 ? h.count[l - 1] : 0)) << 1;
    next[l] = (uint16_t)code;
  }
  for (int s = 0; s < n; ++s) {
    const int l = lens[s] & 15;
    if (!l) continue;
    const int at = offs[l]++;
    if (at < DD_PD_MAX_LIT) h.sym[at] = (uint16_t)s;
    if (l <= DD_PD_LUT_BITS) {
      const uint32_t c = next[l]++;            // < 2^l: the lengths are not oversubscribed
      for (uint32_t k = dd_pd_reverse(c, l); k < (1u << DD_PD_LUT_BITS); k += 1u << l) h.lut[k] = (uint16_t)((l << 9) | s);
    }
  }
  return true;
}

// the next symbol, its bits consumed; -1 (nothing consumed): the bits are in no code of the table
DD_PD_HD int dd_pd_decode(DdPdBits& b, const DdPdHuff& h) {
  const uint32_t v = dd_pd_peek(b, 15);
  const uint32_t e = h.lut[v & ((1u << DD_PD_LUT_BITS) - 1u)];
  if (e) {
    dd_pd_skip(b, (int)(e >> 9));
    return (int)(e & 511u);
  }
  int code = 0, first = 0, index = 0;
  for (int len = 1; len <= 15; ++len) {
    code |= (int)((v >> (len - 1)) & 1u);
    const int count = h.count[len];
    if (code - count < first) {
      const int i = index + (code - first);
      if (i < 0 || i >= DD_PD_MAX_LIT) return -1;
      dd_pd_skip(b, len);
      return h.sym[i];
    }
    index += count;
    first += count;
    first <<= 1;
    code <<= 1;
  }
  return -1;
}

// ---- lengths and distances (RFC 1951 3.2.5), arithmetic ------------------------------------------------------------------

// symbol 257..285 -> the base length 3..258 and its extra bits 0..5
DD_PD_HD void dd_pd_length(int sym, int* base, int* extra) {
  const int s = sym - 257;
  if (s < 8) {
    *base = 3 + s;
    *extra = 0;
  } else if (s == 28) {
    *base = 258;
    *extra = 0;
  } else {
    const int eb = (s - 4) >> 2;
    *base = 3 + ((4 + (s & 3)) << eb);
    *extra = eb;
  }
}

// code 0..29 -> the base distance 1..24577 and its extra bits 0..13
DD_PD_HD void dd_pd_distance(int code, int* base, int* extra) {
  if (code < 4) {
    *base = 1 + code;
    *extra = 0;
  } else {
    const int eb = (code >> 1) - 1;
    *base = 1 + ((2 + (code & 1)) << eb);
    *extra = eb;
  }
}

// ---- blocks -------------------------------------------------------------------------------------------------------------------

struct DdPdShared {                            // one per decoder: LDS on the device
  DdPdHuff lit, dist;
  uint8_t lens[DD_PD_MAX_LIT + 32];
  DdPdBits br;                                 // the leader's reader behind a block header
  int32_t err, final_block, btype;
  uint32_t stored_len;
};

// the order in which a dynamic block's header lists the code-length code's lengths (RFC 1951 3.2.7)
DD_PD_HD int dd_pd_cl_order(int i) {
  const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  return order[i < 19 ? i : 18];
}

// The stored-block header behind the 3 header bits: to the byte boundary, LEN, NLEN.  -> status
DD_PD_HD uint32_t dd_pd_stored_head(DdPdBits& b, uint32_t* len) {
  dd_pd_align(b);
  const uint32_t l = dd_pd_take(b, 16), nl = dd_pd_take(b, 16);
  if (dd_pd_over(b)) return DD_PD_TRUNCATED;
  if ((l ^ nl) != 0xFFFFu) return DD_PD_BAD_STORED;
  *len = l;
  return 0;
}

// A block's header, by ONE thread: BFINAL, BTYPE and for the Huffman types both decode tables in `sh`.  -> status
DD_PD_HD uint32_t dd_pd_block_head(DdPdBits& b, DdPdShared* sh) {
  sh->final_block = (int32_t)dd_pd_take(b, 1);
  sh->btype = (int32_t)dd_pd_take(b, 2);
  sh->stored_len = 0;
  if (dd_pd_over(b)) return DD_PD_TRUNCATED;
  if (sh->btype == 3) return DD_PD_BAD_BLOCK;
  if (sh->btype == 0) return dd_pd_stored_head(b, &sh->stored_len);
  int nlit, ndist;
  if (sh->btype == 1) {
    nlit = 288;
    ndist = 32;
    for (int i = 0; i < 288; ++i) sh->lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
    for (int i = 0; i < 32; ++i) sh->lens[288 + i] = 5;
  } else {
    nlit = 257 + (int)dd_pd_take(b, 5);
    ndist = 1 + (int)dd_pd_take(b, 5);
    const int ncl = 4 + (int)dd_pd_take(b, 4);
    if (dd_pd_over(b)) return DD_PD_TRUNCATED;
    if (nlit > 286 || ndist > 30) return DD_PD_BAD_LENGTHS;
    uint8_t cl[19];
    for (int i = 0; i < 19; ++i) cl[i] = 0;
    for (int i = 0; i < ncl; ++i) cl[dd_pd_cl_order(i)] = (uint8_t)dd_pd_take(b, 3);
    if (dd_pd_over(b)) return DD_PD_TRUNCATED;
    if (!dd_pd_build(sh->lit, cl, 19, true)) return DD_PD_BAD_LENGTHS;
    const int total = nlit + ndist;            // <= 316
    int i = 0;
    while (i < total) {                        // every turn consumes a bit or ends the walk
      const int s = dd_pd_decode(b, sh->lit);
      if (dd_pd_over(b)) return DD_PD_TRUNCATED;
      if (s < 0 || s > 18) return DD_PD_BAD_SYMBOL;
      if (s < 16) {
        sh->lens[i++] = (uint8_t)s;
        continue;
      }
      int rep, val = 0;
      if (s == 16) {
        if (i == 0) return DD_PD_BAD_SYMBOL;   // nothing to repeat
        val = sh->lens[i - 1];
        rep = 3 + (int)dd_pd_take(b, 2);
      } else if (s == 17) {
        rep = 3 + (int)dd_pd_take(b, 3);
      } else {
        rep = 11 + (int)dd_pd_take(b, 7);
      }
      if (dd_pd_over(b)) return DD_PD_TRUNCATED;
      if (i + rep > total) return DD_PD_BAD_LENGTHS;
      for (int k = 0; k < rep; ++k) sh->lens[i++] = (uint8_t)val;
    }
    if (sh->lens[256] == 0) return DD_PD_BAD_LENGTHS;        // no end-of-block symbol
    // the distance lengths behind a fixed place, so that both builds read from `lens`
    for (int k = ndist - 1; k >= 0; --k) sh->lens[288 + k] = sh->lens[nlit + k];
  }
  if (!dd_pd_build(sh->lit, sh->lens, nlit, false)) return DD_PD_BAD_LENGTHS;
  if (!dd_pd_build(sh->dist, sh->lens + 288, ndist, false)) return DD_PD_BAD_LENGTHS;
  return 0;
}

// The walk over the blocks of a deflate stream from the reader's position.  Ctx:
//   bool leader()                                   one caller per decoder says true: it reads the headers into `sh`
//   void sync()                                     everything the callers wrote to `sh` or to the output is visible behind it
//   void lit(uint32_t pos, uint32_t byte)
//   void copy(uint32_t pos, uint32_t len, uint32_t dist)      len 3..258, 1 <= dist <= pos, pos + len <= limit
//   void stored(const uint8_t* src, uint32_t pos, uint32_t n) n bytes of the stream, inside it, pos + n <= limit
//   void advance(uint32_t pos)                      behind every token
// The walk ends behind the final block, or behind a block that ends at or after bit `stop_bits` (< 0: never), or at the
// first error.  *pos: the output position, in and out; *final_seen: the final block was walked.  -> status
template <typename Ctx>
DD_PD_HD uint32_t dd_pd_inflate(DdPdBits& br, DdPdShared* sh, Ctx& ctx, uint32_t limit, int64_t stop_bits, uint32_t* pos_io,
                                int* final_seen) {
  uint32_t pos = *pos_io, err = 0;
  *final_seen = 0;
  for (;;) {                                   // a turn consumes at least the 3 header bits, or ends the walk
    ctx.sync();
    if (ctx.leader()) {
      const uint32_t e = dd_pd_block_head(br, sh);
      sh->br = br;
      sh->err = (int32_t)e;
    }
    ctx.sync();
    br = sh->br;
    err = (uint32_t)sh->err;
    const int final_block = sh->final_block, btype = sh->btype;
    const uint32_t slen = sh->stored_len;
    if (err) break;
    if (btype == 0) {
      const int64_t off = br.used >> 3, avail = br.n - off;    // >= 0: the header was inside the stream
      if ((uint64_t)pos + slen > limit) {
        err = DD_PD_TOO_LONG;
        break;
      }
      const uint32_t take = (int64_t)slen <= avail ? slen : (uint32_t)avail;
      if (take) ctx.stored(br.p + off, pos, take);
      pos += take;
      dd_pd_seek(br, off + slen);
      if (take < slen) {
        err = DD_PD_TRUNCATED;
        break;
      }
      ctx.advance(pos);
    } else {
      for (;;) {                               // a turn consumes at least one bit, or ends the walk
        const int s = dd_pd_decode(br, sh->lit);
        if (dd_pd_over(br)) { err = DD_PD_TRUNCATED; break; }
        if (s < 0 || s > 285) { err = DD_PD_BAD_SYMBOL; break; }
        if (s == 256) break;
        if (s < 256) {
          if (pos >= limit) { err = DD_PD_TOO_LONG; break; }
          ctx.lit(pos, (uint32_t)s);
          pos += 1;
        } else {
          int base, extra;
          dd_pd_length(s, &base, &extra);
          const uint32_t len = (uint32_t)base + dd_pd_take(br, extra);
          const int d = dd_pd_decode(br, sh->dist);
          if (dd_pd_over(br)) { err = DD_PD_TRUNCATED; break; }
          if (d < 0 || d > 29) { err = DD_PD_BAD_SYMBOL; break; }
          dd_pd_distance(d, &base, &extra);
          const uint32_t dist = (uint32_t)base + dd_pd_take(br, extra);
          if (dd_pd_over(br)) { err = DD_PD_TRUNCATED; break; }
          if (dist > pos) { err = DD_PD_BAD_DISTANCE; break; }
          if ((uint64_t)pos + len > limit) { err = DD_PD_TOO_LONG; break; }
          ctx.copy(pos, len, dist);
          pos += len;
        }
        ctx.advance(pos);
      }
      if (err) break;
    }
    if (final_block) {
      *final_seen = 1;
      break;
    }
    if (stop_bits >= 0 && br.used >= stop_bits) break;
  }
  *pos_io = pos;
  return err;
}

// the two zlib header bytes (RFC 1950 2.2): deflate, a window of at most 32 KiB, the check bits, no preset dictionary
DD_PD_HD bool dd_pd_zlib_header_ok(uint32_t cmf, uint32_t flg) {
  return (cmf & 15u) == 8u && (cmf >> 4) <= 7u && ((cmf << 8) | flg) % 31u == 0u && (flg & 32u) == 0u;
}

// the Adler-32 behind the final block: to the byte boundary, four bytes, the most significant first.  -> status
DD_PD_HD uint32_t dd_pd_trailer(DdPdBits& b, uint32_t* adler) {
  dd_pd_align(b);
  uint32_t v = 0;
  for (int i = 0; i < 4; ++i) v = (v << 8) | dd_pd_take(b, 8);
  if (dd_pd_over(b)) return DD_PD_TRUNCATED;
  *adler = v;
  return 0;
}

// Adler-32 of segments: a segment of n bytes x[0..n) has a = sum x[k], b = sum (n - k) x[k], both mod 65521; a segment
// moves the running (A, B) to (A + a, B + n A + b).  (A, B) starts at (1, 0).
DD_PD_HD void dd_pd_adler_sums(const uint8_t* x, int64_t n, uint32_t* a_out, uint32_t* b_out) {
  uint64_t a = 0, b = 0;
  for (int64_t k = 0; k < n; ++k) {
    a += x[k];
    b += (uint64_t)(n - k) % DD_PD_ADLER * x[k];
    if ((k & 0xFFFF) == 0xFFFF) {
      a %= DD_PD_ADLER;
      b %= DD_PD_ADLER;
    }
  }
  *a_out = (uint32_t)(a % DD_PD_ADLER);
  *b_out = (uint32_t)(b % DD_PD_ADLER);
}

DD_PD_HD void dd_pd_adler_join(uint32_t* A, uint32_t* B, uint32_t a, uint32_t b, int64_t n) {
  *B = (uint32_t)((*B + (uint64_t)(n % DD_PD_ADLER) * *A + b) % DD_PD_ADLER);
  *A = (*A + a) % DD_PD_ADLER;
}

// ---- unfilter (PNG specification, 9: Filtering) -------------------------------------------------------------------------------

DD_PD_HD int dd_pd_paeth(int a, int b, int c) {
  const int p = a + b - c;
  const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

// the byte that filter `type` (0..4) turned into x; a: left, b: above, c: above left, 0 outside the image
DD_PD_HD uint32_t dd_pd_unfilter(int type, uint32_t x, uint32_t a, uint32_t b, uint32_t c) {
  uint32_t pred = 0;
  if (type == 1) pred = a;
  else if (type == 2) pred = b;
  else if (type == 3) pred = (a + b) >> 1;
  else if (type == 4) pred = (uint32_t)dd_pd_paeth((int)a, (int)b, (int)c);
  return (x + pred) & 255u;
}

// bytes per pixel of colour type 0 / 2 / 6 at depth 8; 0: not built
DD_PD_HD int dd_pd_bpp(int colour_type) { return colour_type == 0 ? 1 : colour_type == 2 ? 3 : colour_type == 6 ? 4 : 0; }
