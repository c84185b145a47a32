// PNG output: uint8 frames (m, H, W, 3) — or (m, H, W, 4), RGBA: dd_png_encode_u8c — in device memory -> lossless .png
// files, one per frame.
//
// The reference's demo and validation path saves every result as .png (tools/test.py:74-97: `{n}_gen{ti}.png`,
// `{n}_ori.png`, `{n}_map.png`, the view grids of runner/img_utils.py:5-40).  PIL's bytes are zlib's lazy-match parse, one
// sequential chain, and are not reproduced.  What is produced is a valid PNG that decodes to exactly the input pixels, in a
// format every step of which is local to a row, to a run of equal bytes or to a 16 KiB chunk:
//
//   signature, IHDR (W, H, depth 8, colour type 2 — 6 for RGBA —, no interlace), one IDAT per chunk, IEND;
//   the IDAT payloads concatenate to one zlib stream: 78 01, one deflate block (pair) per chunk, the Adler-32;
//   per row the filter type 0..4 with the smallest sum of min(b, 256 - b) over its filtered bytes, ties to the lowest type;
//   the filtered stream cut into chunks of 16384 bytes; per chunk literals and distance-1 matches of length 3..258 by
//   zlib Z_RLE's rule (one literal, then matches of 258, then a match of the rest if it is at least 3, else literals; runs
//   end at the chunk's end), coded as one dynamic-Huffman block, or as a stored block where that is shorter.
//
// The choices the format leaves open:
//   * Every chunk ends on a byte boundary: a dynamic block is followed by an empty stored block (3 bits, padding, 00 00 FF
//     FF).  The dynamic block never carries BFINAL; the stored block of the last chunk does.  So a chunk's bytes depend on
//     nothing but its own 16384 bytes and on whether it is the last one.
//   * One IDAT per chunk: the workgroup that copies a chunk computes the CRC of its own IDAT, no combine across chunks.
//     The first IDAT starts with the two zlib header bytes, the last one ends with the Adler-32.
//   * Code lengths: Huffman's algorithm by two queues over the used symbols sorted by (count, symbol), the leaf taken before
//     the internal node on equal weight (Moffat and Katajainen's in-place form); the leaves per depth are then limited as in
//     the well-known Kraft-sum repair: depths above the limit fold into the limit, and while the Kraft sum is too large one
//     code of the limit is dropped and the deepest shorter code is split in two.  Lengths go to the sorted symbols, longest
//     first.  Limit 15 for the literal / length code, 7 for the code-length code.
//   * The block header lists HLIT + 257 literal / length code lengths and ONE distance code length as one sequence, with
//     the repeat codes 16..18 by a rule local to a run of equal lengths (stated where the deflate kernel applies it).  Distance
//     code 0 always has length 1 (an incomplete one-code distance tree, which RFC 1951 3.2.7 allows), whether the chunk
//     has a match or not.
//   * A chunk is stored when its dynamic form (with the aligning block) has more bytes than 5 + its length.
//
// Four launches on the caller's stream, none of which depends on m or on the content:
//
//   filter    one workgroup per row: the five sums, the choice, the filtered row to the workspace.
//   deflate   one workgroup per chunk: runs by two scans over the boundaries of equal bytes, the symbol histogram, both
//             Huffman codes, the size of both forms, the chosen form assembled LSB-first in LDS and written to the chunk's
//             slot; the chunk's byte count and its two Adler sums.
//   scan      one workgroup per frame: every IDAT's offset in the file, the file's length, the Adler-32 of the whole
//             stream from the chunks' sums.
//   assemble  one workgroup per chunk: the IDAT (length, type, payload, CRC) into the frame's output row, the CRC from 256
//             partial remainders combined by multiplication with x^(8 n) mod P; one more workgroup per frame for the
//             signature, IHDR, IEND and the length.  Every store is bounded by the row's capacity.
//
// No table comes from the host: length codes are arithmetic, the CRC is bitwise, its shift constants are compile-time.
#include "dd_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / DD_WAVE;
constexpr int kChunk = 16384;                  // filtered bytes per deflate chunk
constexpr int kSeg = kChunk / kThreads;        // consecutive bytes a thread owns
constexpr int kSlot = 16400;                   // bytes a chunk's deflate form can take (5 + 16384), rounded up to 16
constexpr int kOutWords = kSlot / 4 + 2;
constexpr int kLit = 286, kCl = 19;
constexpr int kScanThreads = 1024;
constexpr int kCrcSeg = 72;                    // 256 x 72 >= "IDAT" + 2 + 16389 + 4
constexpr int kHead = 33;                      // signature + IHDR
constexpr int kFileFixed = 51;                 // signature, IHDR, IEND, zlib header, Adler-32
constexpr int kChunkFixed = 17;                // IDAT length / type / CRC, the stored block's five bytes
constexpr uint32_t kAdler = 65521u;
constexpr uint32_t kPoly = 0xEDB88320u;

// CRC-32 remainders as polynomials over GF(2), reflected: bit 31 is x^0, a step of one zero bit multiplies by x.
__host__ __device__ constexpr uint32_t dd_crc_mul(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (int i = 0; i < 32; ++i) {
    if (a & (0x80000000u >> i)) p ^= b;
    b = (b >> 1) ^ ((b & 1u) ? kPoly : 0u);
  }
  return p;
}
constexpr uint32_t dd_crc_xpow(int bits) {
  uint32_t v = 0x80000000u;
  for (int i = 0; i < bits; ++i) v = (v >> 1) ^ ((v & 1u) ? kPoly : 0u);
  return v;
}
constexpr uint32_t kS0 = dd_crc_xpow(8 * kCrcSeg), kS1 = dd_crc_mul(kS0, kS0), kS2 = dd_crc_mul(kS1, kS1),
                   kS3 = dd_crc_mul(kS2, kS2), kS4 = dd_crc_mul(kS3, kS3), kS5 = dd_crc_mul(kS4, kS4),
                   kS6 = dd_crc_mul(kS5, kS5), kS7 = dd_crc_mul(kS6, kS6);
// x^(8 * kCrcSeg * 2^k) mod P: what moves a remainder past 2^k segments
__device__ const uint32_t kCrcShift[8] = {kS0, kS1, kS2, kS3, kS4, kS5, kS6, kS7};
// the order in which a dynamic block's header lists the code-length code's lengths (RFC 1951 3.2.7)
__device__ const uint8_t kClOrder[kCl] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

struct Geom {
  int32_t h, w;
  int32_t bpp;                                 // bytes per pixel: 3 (RGB, colour type 2) or 4 (RGBA, colour type 6)
  int32_t row;                                 // filtered bytes per row: 1 + bpp w
  int32_t nchunk;                              // chunks per frame
  int64_t len;                                 // filtered bytes per frame
  int64_t stride;                              // ... rounded up to 16: a frame's place in the workspace
};

// Workspace, every part 16-byte aligned:
//   uint8 filt[m][stride] | uint8 slot[m][nchunk][kSlot] | uint32 info[m][nchunk][4] (bytes, Adler a, Adler b, -) |
//   uint32 off[m][nchunk] | uint32 frame[m][2] (file length, Adler-32)
struct Layout {
  int64_t filt, slot, info, off, frame, total;
};

static inline int64_t up16(int64_t v) { return (v + 15) & ~(int64_t)15; }

// false: the frame's worst-case file does not fit the int32 lengths
static inline bool geometry(int32_t m, int32_t h, int32_t w, int32_t bpp, Geom* g, Layout* l) {
  const int64_t row = 1 + bpp * (int64_t)w, len = row * h, nchunk = (len + kChunk - 1) / kChunk;
  if (kFileFixed + kChunkFixed * nchunk + len > 0x7fffffff) return false;
  g->h = h; g->w = w; g->bpp = bpp; g->row = (int32_t)row; g->nchunk = (int32_t)nchunk; g->len = len; g->stride = up16(len);
  int64_t at = 0;
  l->filt = at; at += (int64_t)m * g->stride;
  l->slot = at; at += (int64_t)m * nchunk * kSlot;
  l->info = at; at += (int64_t)m * nchunk * 16;
  l->off = at; at += up16((int64_t)m * nchunk * 4);
  l->frame = at; at += up16((int64_t)m * 8);
  l->total = at;
  return true;
}

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

// ---- filter -------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ int dd_paeth(int a, int b, int c) {
  const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

// x filtered by `type`; a: left, b: above, c: above left (PNG specification, 9: Filtering)
__device__ __forceinline__ uint32_t dd_png_filter(int type, int x, int a, int b, int c) {
  int pred = 0;
  if (type == 1) pred = a;
  else if (type == 2) pred = b;
  else if (type == 3) pred = (a + b) >> 1;
  else if (type == 4) pred = dd_paeth(a, b, c);
  return (uint32_t)(x - pred) & 255u;
}

__global__ __launch_bounds__(kThreads)
void dd_png_filter_kernel(const uint8_t* __restrict__ frames, uint8_t* __restrict__ filt, const Geom g) {
  __shared__ uint32_t s_red[kWaves];
  const int tid = threadIdx.x;
  const int y = blockIdx.x;
  const int64_t img = blockIdx.y;
  const int nb = g.bpp * g.w, bpp = g.bpp;
  const uint8_t* cur = frames + (img * g.h + y) * (int64_t)nb;
  const uint8_t* up = cur - nb;                              // read for y > 0 only
  uint32_t sums[5] = {0u, 0u, 0u, 0u, 0u};
  for (int k = tid; k < nb; k += kThreads) {
    const int x = cur[k], a = k >= bpp ? cur[k - bpp] : 0, b = y > 0 ? up[k] : 0, c = (y > 0 && k >= bpp) ? up[k - bpp] : 0;
#pragma unroll
    for (int t = 0; t < 5; ++t) {
      const uint32_t v = dd_png_filter(t, x, a, b, c);
      sums[t] += v < 128u ? v : 256u - v;
    }
  }
  int type = 0;
  uint32_t best = 0;
#pragma unroll
  for (int t = 0; t < 5; ++t) {
    const uint32_t s = dd_block_sum(sums[t], s_red);
    if (t == 0 || s < best) {
      best = s;
      type = t;
    }
  }
  uint8_t* dst = filt + img * g.stride + (int64_t)y * g.row;
  if (tid == 0) dst[0] = (uint8_t)type;
  for (int k = tid; k < nb; k += kThreads) {
    const int x = cur[k], a = k >= bpp ? cur[k - bpp] : 0, b = y > 0 ? up[k] : 0, c = (y > 0 && k >= bpp) ? up[k - bpp] : 0;
    dst[1 + k] = (uint8_t)dd_png_filter(type, x, a, b, c);
  }
}

// ---- deflate ------------------------------------------------------------------------------------------------------------

// The tokens of the positions [lo, hi) of a chunk, in order: f(symbol, extra bits, extra value, is a match).  start: where
// the run that holds `lo` begins if `lo` itself is no boundary; next: the first boundary at or behind `hi` (the chunk's
// length if there is none).  A run is a maximal stretch of equal bytes inside the chunk.
template <typename F>
__device__ __forceinline__ void dd_png_walk(const uint8_t* in, int lo, int hi, int start, int next, F&& f) {
  int s = start, e = 0;
  bool have = false;
  for (int i = lo; i < hi; ++i) {
    const bool bnd = i == 0 || in[i] != in[i - 1];
    if (bnd) s = i;
    if (bnd || !have) {                                      // the end of the run that holds i
      int j = i + 1;
      while (j < hi && in[j] == in[j - 1]) ++j;
      e = j < hi ? j : next;
      have = true;
    }
    const int p = i - s;
    int len = 0;
    if (p > 0) {
      const int j = p - 1, rest = e - s - 1, q = (rest / 258) * 258, r = rest - q;
      if (j < q) {
        if (j % 258 != 0) continue;
        len = 258;
      } else if (r >= 3) {
        if (j != q) continue;
        len = r;
      }
    }
    if (len == 0) {
      f((int)in[i], 0, 0, 0);
    } else if (len == 258) {
      f(285, 0, 0, 1);
    } else {
      const int l = len - 3;                                 // 0..254
      if (l < 8) {
        f(257 + l, 0, 0, 1);
      } else {
        const int eb = 29 - __builtin_clz((uint32_t)l);      // floor(log2 l) - 2: 1..5
        f(261 + 4 * eb + ((l >> eb) & 3), eb, l & ((1 << eb) - 1), 1);
      }
    }
  }
}

struct CodeScratch {
  uint32_t w[kLit + 2];                        // sorted weights, then depths
  uint16_t order[kLit + 2];                    // the symbol of a sorted position
  int32_t bl[16], next[16];
  int32_t n;
};

// Code lengths (<= maxlen) and bit-reversed canonical codes of the symbols with hist > 0; the whole workgroup calls it.
__device__ void dd_png_build_code(const uint32_t* hist, int nsym, int maxlen, uint8_t* lens, uint16_t* codes, CodeScratch* cs) {
  const int tid = threadIdx.x;
  if (tid == 0) cs->n = 0;
  __syncthreads();
  for (int s = tid; s < nsym; s += kThreads) {
    const uint32_t f = hist[s];
    lens[s] = 0;
    codes[s] = 0;
    if (f) {
      int rank = 0;
      for (int o = 0; o < nsym; ++o) {
        const uint32_t fo = hist[o];
        rank += (fo && (fo < f || (fo == f && o < s))) ? 1 : 0;
      }
      cs->w[rank] = f;
      cs->order[rank] = (uint16_t)s;
      atomicAdd(&cs->n, 1);
    }
  }
  __syncthreads();
  if (tid == 0) {
    const int n = cs->n;
    uint32_t* A = cs->w;
    if (n == 1) {
      A[0] = 1;
    } else if (n >= 2) {
      // Moffat and Katajainen, "In-place calculation of minimum-redundancy codes": weights -> parents -> depths
      A[0] += A[1];
      int root = 0, leaf = 2;
      for (int nx = 1; nx < n - 1; ++nx) {
        if (leaf >= n || A[root] < A[leaf]) { A[nx] = A[root]; A[root++] = (uint32_t)nx; } else A[nx] = A[leaf++];
        if (leaf >= n || (root < nx && A[root] < A[leaf])) { A[nx] += A[root]; A[root++] = (uint32_t)nx; } else A[nx] += A[leaf++];
      }
      A[n - 2] = 0;
      for (int nx = n - 3; nx >= 0; --nx) A[nx] = A[A[nx]] + 1;
      int avbl = 1, used = 0, dpth = 0, rt = n - 2, nx = n - 1;
      while (avbl > 0) {
        while (rt >= 0 && (int)A[rt] == dpth) { ++used; --rt; }
        while (avbl > used) { A[nx--] = (uint32_t)dpth; --avbl; }
        avbl = 2 * used;
        ++dpth;
        used = 0;
      }
    }
    for (int d = 0; d < 16; ++d) cs->bl[d] = 0;
    for (int i = 0; i < n; ++i) cs->bl[min((int)A[i], maxlen)] += 1;
    uint32_t total = 0;
    for (int d = 1; d <= maxlen; ++d) total += (uint32_t)cs->bl[d] << (maxlen - d);
    while (total > (1u << maxlen)) {
      cs->bl[maxlen] -= 1;
      for (int d = maxlen - 1; d > 0; --d) {
        if (cs->bl[d]) {
          cs->bl[d] -= 1;
          cs->bl[d + 1] += 2;
          break;
        }
      }
      --total;
    }
    int i = 0;
    for (int d = maxlen; d >= 1; --d)
      for (int k = 0; k < cs->bl[d] && i < n; ++k) lens[cs->order[i++]] = (uint8_t)d;
    uint32_t code = 0;
    cs->bl[0] = 0;
    for (int d = 1; d <= maxlen; ++d) {
      code = (code + (uint32_t)cs->bl[d - 1]) << 1;
      cs->next[d] = (int32_t)code;
    }
    for (int s = 0; s < nsym; ++s) {
      const int l = lens[s];
      if (l) {
        const uint32_t c = (uint32_t)cs->next[l]++;
        codes[s] = (uint16_t)(__builtin_bitreverse32(c) >> (32 - l));       // Huffman codes go in MSB first
      }
    }
  }
  __syncthreads();
}

// `nbits` <= 32 bits of `value` at bit `pos` of the LSB-first stream image in LDS
__device__ __forceinline__ void dd_png_put(uint32_t* buf, uint32_t pos, uint32_t value, uint32_t nbits) {
  if (nbits == 0) return;
  const uint32_t sh = pos & 31u, w = pos >> 5;
  if (w + 1 >= (uint32_t)kOutWords) return;                  // cannot happen: a dynamic form is written only if it fits
  const uint64_t v = (uint64_t)value << sh;
  atomicOr(&buf[w], (uint32_t)v);
  if ((uint32_t)(v >> 32)) atomicOr(&buf[w + 1], (uint32_t)(v >> 32));
}

__global__ __launch_bounds__(kThreads)
void dd_png_deflate_kernel(const uint8_t* __restrict__ filt, uint8_t* __restrict__ slots, uint32_t* __restrict__ info,
                           const Geom g) {
  __shared__ __attribute__((aligned(16))) uint8_t s_in[kChunk];
  __shared__ __attribute__((aligned(16))) uint32_t s_out[kOutWords];
  __shared__ uint32_t s_hist[kLit + 2], s_clhist[kCl + 1];
  __shared__ uint8_t s_rl_sym[kLit + 2], s_rl_ext[kLit + 2]; // the code lengths as the header lists them: symbols 0..18
  __shared__ int32_t s_rl_n;
  __shared__ uint8_t s_len[kLit + 2], s_cllen[kCl + 1];
  __shared__ uint16_t s_code[kLit + 2], s_clcode[kCl + 1];
  __shared__ int32_t s_a[kThreads], s_b[kThreads];
  __shared__ uint32_t s_red[kWaves];
  __shared__ CodeScratch s_cs;
  const int tid = threadIdx.x;
  const int c = blockIdx.x;
  const int64_t img = blockIdx.y;
  const int n = (int)min((int64_t)kChunk, g.len - (int64_t)c * kChunk);
  const bool last = c == g.nchunk - 1;
  const uint8_t* src = filt + img * g.stride + (int64_t)c * kChunk;          // 16-byte aligned
  for (int k = tid * 16; k < n; k += kThreads * 16) dd_st16(s_in + k, dd_ld16(src + k));   // inside the frame's stride
  for (int k = tid; k < kLit + 2; k += kThreads) s_hist[k] = 0u;
  if (tid < kCl + 1) s_clhist[tid] = 0u;
  __syncthreads();
  const int lo = min(tid * kSeg, n), hi = min(lo + kSeg, n);

  // boundaries of runs: the last one at or before every segment's start, the first one behind its end
  int lastb = -1, firstb = n;
  uint32_t ad_a = 0, ad_b = 0;
  for (int i = lo; i < hi; ++i) {
    if (i == 0 || s_in[i] != s_in[i - 1]) {
      if (firstb == n) firstb = i;
      lastb = i;
    }
    ad_a += s_in[i];
    ad_b += (uint32_t)(n - i) * s_in[i];
  }
  s_a[tid] = lastb;
  s_b[tid] = firstb;
  __syncthreads();
  for (int d = 1; d < kThreads; d <<= 1) {                   // inclusive max scan / inclusive suffix min scan
    const int va = tid >= d ? s_a[tid - d] : -1, vb = tid + d < kThreads ? s_b[tid + d] : n;
    __syncthreads();
    s_a[tid] = max(s_a[tid], va);
    s_b[tid] = min(s_b[tid], vb);
    __syncthreads();
  }
  const int start = tid > 0 ? max(s_a[tid - 1], 0) : 0;
  const int next = tid + 1 < kThreads ? s_b[tid + 1] : n;

  // pass 1: the histogram of the literal / length symbols, the extra and distance bits
  uint32_t xbits = 0;
  dd_png_walk(s_in, lo, hi, start, next, [&](int sym, int eb, int, int match) {
    atomicAdd(&s_hist[sym], 1u);
    xbits += (uint32_t)(eb + match);
  });
  if (tid == 0) s_hist[256] = 1u;
  const uint32_t adler_a = dd_block_sum(ad_a % kAdler, s_red) % kAdler;
  const uint32_t adler_b = dd_block_sum(ad_b % kAdler, s_red) % kAdler;      // ends in a barrier: the histogram is complete
  __syncthreads();
  dd_png_build_code(s_hist, kLit, 15, s_len, s_code, &s_cs);
  int top = 0;
  for (int s = tid; s < kLit; s += kThreads) top = s_hist[s] ? max(top, s + 1) : top;
  s_a[tid] = top;
  __syncthreads();
  for (int d = kThreads / 2; d > 0; d >>= 1) {
    if (tid < d) s_a[tid] = max(s_a[tid], s_a[tid + d]);
    __syncthreads();
  }
  const int nlit = max(s_a[0], 257);
  __syncthreads();
  // The nlit literal / length code lengths and the one distance code length (1) as one sequence, run by run: a run of
  // zeros as repeats of 138 (symbol 18, 11..138) while 3 or more are left, the last of them symbol 17 when below 11, then
  // single zeros; a run of another length as the length, repeats of 6 (symbol 16, 3..6) while 3 or more are left, then
  // the length itself.
  if (tid == 0) {
    const int total = nlit + 1;
    int nt = 0, i = 0;
    while (i < total) {
      const int v = i < nlit ? s_len[i] : 1;
      int r = 1;
      while (i + r < total && (i + r < nlit ? s_len[i + r] : 1) == v) ++r;
      i += r;
      if (v != 0) {
        s_rl_sym[nt] = (uint8_t)v; s_rl_ext[nt++] = 0;
        --r;
      }
      while (r >= 3) {
        const int t = min(r, v ? 6 : 138);
        s_rl_sym[nt] = (uint8_t)(v ? 16 : (t >= 11 ? 18 : 17));
        s_rl_ext[nt++] = (uint8_t)(v ? t - 3 : (t >= 11 ? t - 11 : t - 3));
        r -= t;
      }
      for (; r > 0; --r) {
        s_rl_sym[nt] = (uint8_t)v; s_rl_ext[nt++] = 0;
      }
    }
    s_rl_n = nt;
    for (int k = 0; k < nt; ++k) s_clhist[s_rl_sym[k]] += 1u;
  }
  __syncthreads();
  dd_png_build_code(s_clhist, kCl, 7, s_cllen, s_clcode, &s_cs);
  uint32_t tok = xbits, clb = 0;
  for (int s = tid; s < kLit; s += kThreads) {
    tok += s_hist[s] * s_len[s];
  }
  for (int k = tid; k < s_rl_n; k += kThreads) {
    const int sym = s_rl_sym[k];
    clb += s_cllen[sym] + (sym == 16 ? 2u : sym == 17 ? 3u : sym == 18 ? 7u : 0u);
  }
  const uint32_t tokbits = dd_block_sum(tok, s_red);         // tokens and the end-of-block symbol
  int hclen = 4;
  for (int k = 4; k < kCl; ++k) hclen = s_cllen[kClOrder[k]] ? k + 1 : hclen;
  const uint32_t headbits = 17u + 3u * hclen + dd_block_sum(clb, s_red);
  const uint32_t dynbits = headbits + tokbits;
  const uint32_t dyn_bytes = (dynbits + 3u + 7u) / 8u + 4u, stored_bytes = 5u + (uint32_t)n;
  const bool dyn = dyn_bytes <= stored_bytes;
  uint8_t* slot = slots + (img * g.nchunk + c) * (int64_t)kSlot;
  if (tid == 0) {
    uint32_t* o = info + (img * g.nchunk + c) * 4;
    o[0] = dyn ? dyn_bytes : stored_bytes;
    o[1] = adler_a;
    o[2] = adler_b;
    o[3] = 0u;
  }
  if (!dyn) {
    if (tid == 0) {
      slot[0] = last ? 1 : 0;
      slot[1] = (uint8_t)(n & 255);
      slot[2] = (uint8_t)(n >> 8);
      slot[3] = (uint8_t)(~n & 255);
      slot[4] = (uint8_t)((~n >> 8) & 255);
    }
    for (int i = tid; i < n; i += kThreads) slot[5 + i] = s_in[i];
    return;
  }
  for (int k = tid; k < kOutWords; k += kThreads) s_out[k] = 0u;
  // pass 2: every thread's bits, their prefix sum
  uint32_t mine = 0;
  dd_png_walk(s_in, lo, hi, start, next, [&](int sym, int eb, int, int match) { mine += (uint32_t)(s_len[sym] + eb + match); });
  __syncthreads();
  s_a[tid] = (int32_t)mine;
  __syncthreads();
  for (int d = 1; d < kThreads; d <<= 1) {
    const int add = tid >= d ? s_a[tid - d] : 0;
    __syncthreads();
    s_a[tid] += add;
    __syncthreads();
  }
  uint32_t pos = headbits + (uint32_t)s_a[tid] - mine;
  // pass 3: the tokens; thread 0 also writes the header, the end of the block and the aligning stored block
  dd_png_walk(s_in, lo, hi, start, next, [&](int sym, int eb, int ev, int match) {
    const uint32_t l = s_len[sym];
    dd_png_put(s_out, pos, (uint32_t)s_code[sym] | ((uint32_t)ev << l), l + (uint32_t)eb + (uint32_t)match);   // distance code 0: a 0 bit
    pos += l + (uint32_t)eb + (uint32_t)match;
  });
  if (tid == 0) {
    uint32_t at = 0;
    dd_png_put(s_out, at, 4u, 3); at += 3;                   // BFINAL 0, BTYPE 2
    dd_png_put(s_out, at, (uint32_t)(nlit - 257), 5); at += 5;
    at += 5;                                                 // HDIST 0: one distance code
    dd_png_put(s_out, at, (uint32_t)(hclen - 4), 4); at += 4;
    for (int k = 0; k < hclen; ++k) {
      dd_png_put(s_out, at, s_cllen[kClOrder[k]], 3);
      at += 3;
    }
    for (int k = 0; k < s_rl_n; ++k) {
      const int sym = s_rl_sym[k];
      dd_png_put(s_out, at, s_clcode[sym], s_cllen[sym]);
      at += s_cllen[sym];
      const uint32_t xb = sym == 16 ? 2u : sym == 17 ? 3u : sym == 18 ? 7u : 0u;
      dd_png_put(s_out, at, s_rl_ext[k], xb);
      at += xb;
    }
    dd_png_put(s_out, dynbits - s_len[256], s_code[256], s_len[256]);
    dd_png_put(s_out, dynbits, last ? 1u : 0u, 3);          // an empty stored block: BFINAL, BTYPE 0, padding, LEN 0, NLEN
    dd_png_put(s_out, ((dynbits + 3u + 7u) / 8u) * 8u, 0xFFFF0000u, 32);
  }
  __syncthreads();
  uint32_t* dst = reinterpret_cast<uint32_t*>(slot);
  const int nw = (int)((dyn_bytes + 3u) / 4u);               // <= kSlot / 4
  for (int k = tid; k < nw; k += kThreads) dst[k] = s_out[k];
}

// ---- offsets and the Adler-32 -------------------------------------------------------------------------------------------

__device__ __forceinline__ uint32_t dd_scan1024(uint32_t v, uint32_t* s) {   // inclusive
  const int tid = threadIdx.x;
  __syncthreads();
  s[tid] = v;
  __syncthreads();
  for (int d = 1; d < kScanThreads; d <<= 1) {
    const uint32_t add = tid >= d ? s[tid - d] : 0u;
    __syncthreads();
    s[tid] += add;
    __syncthreads();
  }
  return s[tid];
}

__device__ __forceinline__ uint32_t dd_idat_bytes(const uint32_t* info, int i, const Geom& g) {
  return 12u + min(info[4 * i], (uint32_t)kSlot) + (i == 0 ? 2u : 0u) + (i == g.nchunk - 1 ? 4u : 0u);
}

// One workgroup per frame: thread t owns the `per` consecutive chunks from t * per.
__global__ __launch_bounds__(kScanThreads)
void dd_png_scan_kernel(const uint32_t* __restrict__ info, uint32_t* __restrict__ off, uint32_t* __restrict__ frame,
                        const Geom g) {
  __shared__ uint32_t s_sum[kScanThreads];
  const int tid = threadIdx.x;
  const int64_t img = blockIdx.x;
  const uint32_t* in = info + img * g.nchunk * 4;
  uint32_t* o = off + img * g.nchunk;
  const int per = (g.nchunk + kScanThreads - 1) / kScanThreads;
  const int i0 = (int)min((int64_t)tid * per, (int64_t)g.nchunk), i1 = min(i0 + per, g.nchunk);
  uint32_t bytes = 0, a = 0;
  for (int i = i0; i < i1; ++i) {
    bytes += dd_idat_bytes(in, i, g);
    a = (a + in[4 * i + 1]) % kAdler;
  }
  const uint32_t bytes_incl = dd_scan1024(bytes, s_sum);
  const uint32_t total = s_sum[kScanThreads - 1];
  const uint32_t a_incl = dd_scan1024(a, s_sum);             // < 1024 * 65521
  const uint32_t a_total = s_sum[kScanThreads - 1];
  // Adler-32: A = 1 + sum of bytes, B = sum of the A's; a chunk of n bytes with sums (a, b) moves (A, B) to
  // (A + a, B + n A + b)
  uint32_t at = kHead + bytes_incl - bytes, A = (1u + a_incl - a) % kAdler, B = 0;
  for (int i = i0; i < i1; ++i) {
    o[i] = at;
    at += dd_idat_bytes(in, i, g);
    const uint32_t n = (uint32_t)min((int64_t)kChunk, g.len - (int64_t)i * kChunk);
    B = (B + (n * A) % kAdler + in[4 * i + 2] % kAdler) % kAdler;
    A = (A + in[4 * i + 1]) % kAdler;
  }
  dd_scan1024(B, s_sum);
  if (tid == kScanThreads - 1) {
    frame[img * 2] = kHead + total + 12u;
    frame[img * 2 + 1] = ((s_sum[tid] % kAdler) << 16) | ((1u + a_total) % kAdler);
  }
}

// ---- assembly -----------------------------------------------------------------------------------------------------------

__device__ __forceinline__ uint32_t dd_crc_byte(uint32_t r, uint32_t byte) {
  r ^= byte;
#pragma unroll
  for (int i = 0; i < 8; ++i) r = (r >> 1) ^ (kPoly & (0u - (r & 1u)));
  return r;
}

__device__ __forceinline__ void dd_put_be32(uint8_t* row, int64_t at, int64_t capacity, uint32_t v) {
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (at + i < capacity) row[at + i] = (uint8_t)(v >> (24 - 8 * i));
}

__global__ __launch_bounds__(kThreads)
void dd_png_assemble_kernel(const uint8_t* __restrict__ slots, const uint32_t* __restrict__ info,
                            const uint32_t* __restrict__ off, const uint32_t* __restrict__ frame, uint8_t* __restrict__ out,
                            int64_t capacity, int32_t* __restrict__ lengths, const Geom g) {
  __shared__ uint32_t s_crc[kThreads];
  __shared__ uint8_t s_head[kHead + 12];
  const int tid = threadIdx.x;
  const int64_t img = blockIdx.y;
  const int c = blockIdx.x;
  uint8_t* row = out + img * capacity;
  if (c == g.nchunk) {                                       // the extra workgroup: signature, IHDR, IEND, length
    const int64_t len = frame[img * 2];
    if (tid == 0) {
      const uint8_t sig[16] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A, 0, 0, 0, 13, 'I', 'H', 'D', 'R'};
      for (int i = 0; i < 16; ++i) s_head[i] = sig[i];
      for (int i = 0; i < 4; ++i) {
        s_head[16 + i] = (uint8_t)((uint32_t)g.w >> (24 - 8 * i));
        s_head[20 + i] = (uint8_t)((uint32_t)g.h >> (24 - 8 * i));
      }
      s_head[24] = 8; s_head[25] = g.bpp == 4 ? 6 : 2; s_head[26] = 0; s_head[27] = 0; s_head[28] = 0;
      uint32_t r = 0xFFFFFFFFu;
      for (int i = 12; i < 29; ++i) r = dd_crc_byte(r, s_head[i]);
      r ^= 0xFFFFFFFFu;
      for (int i = 0; i < 4; ++i) s_head[29 + i] = (uint8_t)(r >> (24 - 8 * i));
      const uint8_t iend[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xAE, 0x42, 0x60, 0x82};
      for (int i = 0; i < 12; ++i) s_head[kHead + i] = iend[i];
      lengths[img] = (int32_t)len;
    }
    __syncthreads();
    if (tid < kHead + 12) {
      const int64_t at = tid < kHead ? tid : len - 12 + (tid - kHead);
      if (at < capacity) row[at] = s_head[tid];
    }
    return;
  }
  const bool last = c == g.nchunk - 1;
  const uint32_t nb = min(info[(img * g.nchunk + c) * 4], (uint32_t)kSlot);
  const int pre = c == 0 ? 2 : 0, post = last ? 4 : 0;
  const int plen = pre + (int)nb + post, msg = 4 + plen;     // the CRC covers the type and the payload
  const uint32_t adler = frame[img * 2 + 1];
  const uint8_t* slot = slots + (img * g.nchunk + c) * (int64_t)kSlot;
  const int64_t base = off[img * g.nchunk + c];
  // The message right-aligned in 256 segments of kCrcSeg bytes: leading zeros leave a zero remainder as it is.  Its first
  // four bytes are complemented, which is what the initial value 0xFFFFFFFF of the CRC does.
  const int pad = kThreads * kCrcSeg - msg;
  uint32_t r = 0;
  for (int k = 0; k < kCrcSeg; ++k) {
    int j = tid * kCrcSeg + k - pad;
    if (j < 0) continue;
    const int64_t at = base + 4 + j;
    uint32_t byte;
    if (j < 4) {
      byte = (0x54414449u >> (8 * j)) & 255u;                // "IDAT"
    } else if (j < 4 + pre) {
      byte = j == 4 ? 0x78u : 0x01u;                         // zlib: deflate, 32 K window, no dictionary, level 0
    } else if (j < 4 + pre + (int)nb) {
      byte = slot[j - 4 - pre];
    } else {
      byte = (adler >> (24 - 8 * (j - 4 - pre - (int)nb))) & 255u;
    }
    if (at < capacity) row[at] = (uint8_t)byte;
    r = dd_crc_byte(r, j < 4 ? byte ^ 255u : byte);
  }
  s_crc[tid] = r;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int stride = 1 << k;
    if ((tid & (2 * stride - 1)) == 0) s_crc[tid] = dd_crc_mul(s_crc[tid], kCrcShift[k]) ^ s_crc[tid + stride];
    __syncthreads();
  }
  if (tid == 0) {
    dd_put_be32(row, base, capacity, (uint32_t)plen);
    dd_put_be32(row, base + 4 + msg, capacity, s_crc[0] ^ 0xFFFFFFFFu);
  }
}

}  // namespace

extern "C" int64_t dd_png_workspace_bytes_c(int32_t m, int32_t h, int32_t w, int32_t channels) {
  if (m <= 0 || m > 65535 || h <= 0 || w <= 0 || (channels != 3 && channels != 4)) return -1;
  Geom g;
  Layout l;
  if (!geometry(m, h, w, channels, &g, &l)) return -1;
  return l.total;
}

extern "C" int64_t dd_png_workspace_bytes(int32_t m, int32_t h, int32_t w) { return dd_png_workspace_bytes_c(m, h, w, 3); }

extern "C" int dd_png_encode_u8c(const uint8_t* frames, int32_t m, int32_t h, int32_t w, int32_t channels, void* workspace,
                                 int64_t workspace_bytes, uint8_t* out, int64_t capacity, int32_t* lengths,
                                 dd_stream_t stream) {
  if (!frames || !workspace || !out || !lengths) return DD_ERR_BAD_ARG;
  if (m <= 0 || h <= 0 || w <= 0 || (channels != 3 && channels != 4)) return DD_ERR_BAD_ARG;
  if (capacity < kFileFixed) return DD_ERR_BAD_ARG;
  if (!dd_aligned16(workspace) || (reinterpret_cast<uintptr_t>(lengths) & 3u)) return DD_ERR_BAD_ARG;
  Geom g;
  Layout l;
  if (!geometry(m, h, w, channels, &g, &l) || m > 65535) return DD_ERR_UNSUPPORTED;
  if (workspace_bytes < l.total) return DD_ERR_BAD_ARG;
  uint8_t* ws = reinterpret_cast<uint8_t*>(workspace);
  uint8_t* filt = ws + l.filt;
  uint8_t* slots = ws + l.slot;
  uint32_t* info = reinterpret_cast<uint32_t*>(ws + l.info);
  uint32_t* off = reinterpret_cast<uint32_t*>(ws + l.off);
  uint32_t* frame = reinterpret_cast<uint32_t*>(ws + l.frame);
  hipStream_t s = dd_stream(stream);
  dd_clear_error();
  hipLaunchKernelGGL(dd_png_filter_kernel, dim3((unsigned)h, (unsigned)m), dim3(kThreads), 0, s, frames, filt, g);
  hipLaunchKernelGGL(dd_png_deflate_kernel, dim3((unsigned)g.nchunk, (unsigned)m), dim3(kThreads), 0, s, filt, slots, info, g);
  hipLaunchKernelGGL(dd_png_scan_kernel, dim3((unsigned)m), dim3(kScanThreads), 0, s, info, off, frame, g);
  hipLaunchKernelGGL(dd_png_assemble_kernel, dim3((unsigned)g.nchunk + 1, (unsigned)m), dim3(kThreads), 0, s, slots, info, off,
                     frame, out, capacity, lengths, g);
  return dd_check_launch();
}

extern "C" int dd_png_encode_u8(const uint8_t* frames, int32_t m, int32_t h, int32_t w, void* workspace,
                                int64_t workspace_bytes, uint8_t* out, int64_t capacity, int32_t* lengths,
                                dd_stream_t stream) {
  return dd_png_encode_u8c(frames, m, h, w, 3, workspace, workspace_bytes, out, capacity, lengths, stream);
}
