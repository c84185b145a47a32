// JPEG input: the entropy-coded segments of m baseline .jpg files of one geometry -> uint8 frames (m, H, W, 3) in device
// memory, byte for byte what PIL's `Image.open(f).convert("RGB")` returns (libjpeg: Huffman decoding, the `islow` integer
// inverse DCT, "fancy" chroma upsampling, 16-bit fixed-point colour conversion; all of it integer arithmetic).
//
// A frame's segment is one sequential bit stream.  It is cut into subsequences of S = DD_JD_SUB_BITS bits, one lane each,
// and decoded by the self-synchronising scheme: every lane first decodes from its own start as if a block began there,
// then, `rounds` times, again from the state its left neighbour ended in.  Huffman streams re-synchronise on their own,
// so after a few rounds nearly every lane has started from its true state — but nothing rests on that: a lane's entry is
// true if it equals its neighbour's exit and the neighbour's entry is true, the first lane's entry is known, and the repair
// pass decodes again, in order, every lane for which that chain breaks (a flat frame is a periodic stream on which a
// misaligned decoder can stay misaligned for ever).  The launches, on the caller's stream, whatever the content is:
//
//   (memset)  the coefficients to zero
//   ffcount   FF 00 pairs per 4 KB chunk of the file's segment (at whatever byte offset it lies); status = 0
//   unstuff   the segment without its stuffing bytes into the workspace, and its length in bits
//   spec      one lane per subsequence: decode from (start, block 0, coefficient 0), keep the exit state
//   round     x rounds: decode from the left neighbour's exit state, unless that is the entry already used
//   repair    one wave per frame: 64 entries checked at a time against their neighbours' exits; the first that differs
//             is decoded again by its lane, then the ones behind it are compared with the new exit, and so on
//   blocks    one workgroup per frame: exclusive prefix sum of the blocks each subsequence completes; fewer than the
//             frame has: status EXHAUSTED
//   emit      one lane per subsequence, from its true entry: the non-zero coefficients and the DC differences, status bits
//   dc        one workgroup per frame and component: prefix sum of the DC differences
//   idct      eight lanes per block: dequantisation, column pass, row pass, + 128, clamp -> the component planes
//   colour    one lane per pixel: chroma upsampling (triangle filter; replication for a plane of one or two columns),
//             YCbCr -> RGB, rows below H and columns below W only
//
// Phases are ordered by the kernel boundaries alone; no workgroup waits for another.  The decode core — bit reader,
// Huffman lookup, one subsequence from an entry state, the arithmetic from coefficients to pixels — is jpeg_decode_core.h,
// shared with the host program that runs it under the sanitizers; its header lists the bounds.  Here, every read of the
// caller's bytes is clamped to the frame's range and to the upload's size, and every per-subsequence array is indexed
// below the count derived from the frame's own bit length, which is at most the one the workspace was sized for.
#include "dd_common.h"
#ifndef DD_JD_SUB_BITS                         // an A/B build of the library sets another S (DD_HIP_DEFINES, tools/jpeg_input_timing.py)
#define DD_JD_SUB_BITS DD_JPEG_SUB_BITS
#endif
#include "jpeg_decode_core.h"

static_assert(DD_JD_EXHAUSTED == DD_JPEG_EXHAUSTED && DD_JD_BAD_CODE == DD_JPEG_BAD_CODE && DD_JD_BAD_RUN == DD_JPEG_BAD_RUN &&
                  DD_JD_TRAILING == DD_JPEG_TRAILING,
              "the core's status bits are the header's");

namespace {

constexpr int kThreads = 256;                  // lanes (subsequences) per workgroup of spec / round / emit
constexpr int kScanThreads = 1024;             // the two prefix sums
constexpr int kChunk = 4096;                   // bytes of the stuffed segment per workgroup of ffcount / unstuff
constexpr int kSub = DD_JD_SUB_BITS;
constexpr int64_t kMaxMcus = 262144;
constexpr int64_t kMaxScanBytes = (int64_t)1 << 27;      // bit positions are int32
static_assert(kSub >= 64 && kSub % 32 == 0, "a subsequence holds at least one symbol and starts on a word");

struct Geom {
  int32_t h, w;
  int32_t bpm;                                 // blocks per MCU: 6 (4:2:0) or 3 (4:4:4)
  int32_t mw, nmcu, nblk;                      // MCUs per row, per frame; blocks per frame
  int32_t yw, yh, cw, ch;                      // padded planes: Y, and Cb / Cr
  int32_t tcw, tch;                            // true chroma size: ceil(w / 2), ceil(h / 2) (4:2:0)
  int32_t cap;                                 // bytes of a frame's segment, at most
  int32_t nchunk, nsub;                        // chunks and subsequences a segment of `cap` bytes has
  int32_t stream_words;                        // per frame
  int64_t plane_bytes;                         // per frame: Y | Cb | Cr
  int64_t c_off, c_size;                       // Cb's offset in it; Cr follows c_size bytes behind
};

// Workspace, every part 16-byte aligned:
//   int16 coef[m][nblk][64] | uint8 planes[m][plane_bytes] | uint32 stream[m][stream_words] | uint32 chunk_ff[m][nchunk] |
//   int32 nbits[m] | State ent[m][nsub] | State ex[2][m][nsub] | int32 first[m][nsub]
struct Layout {
  int64_t coef, planes, stream, chunk_ff, nbits, ent, ex0, ex1, first, total;
};

static inline int64_t up16(int64_t v) { return (v + 15) & ~(int64_t)15; }

static inline bool geometry(int32_t m, int32_t h, int32_t w, int32_t sampling, int64_t cap, Geom* g, Layout* l) {
  const int mcu = sampling == 420 ? 16 : 8;
  const int64_t mw = (w + mcu - 1) / mcu, mh = (h + mcu - 1) / mcu, nmcu = mw * mh;
  if (nmcu > kMaxMcus || cap > kMaxScanBytes) return false;
  g->h = h; g->w = w; g->bpm = sampling == 420 ? 6 : 3;
  g->mw = (int32_t)mw; g->nmcu = (int32_t)nmcu; g->nblk = (int32_t)(nmcu * g->bpm);
  g->yw = (int32_t)(mw * mcu); g->yh = (int32_t)(mh * mcu); g->cw = (int32_t)(mw * 8); g->ch = (int32_t)(mh * 8);
  g->tcw = sampling == 420 ? (w + 1) / 2 : w; g->tch = sampling == 420 ? (h + 1) / 2 : h;
  g->cap = (int32_t)cap;
  g->nchunk = (int32_t)((cap + kChunk - 1) / kChunk);
  g->nsub = (int32_t)((cap * 8 + kSub - 1) / kSub);
  g->stream_words = (int32_t)(up16(cap + 8) / 4);
  g->c_off = up16((int64_t)g->yw * g->yh);
  g->c_size = up16((int64_t)g->cw * g->ch);
  g->plane_bytes = g->c_off + 2 * g->c_size;
  int64_t at = 0;
  l->coef = at; at += up16((int64_t)m * g->nblk * 64 * 2);
  l->planes = at; at += up16((int64_t)m * g->plane_bytes);
  l->stream = at; at += up16((int64_t)m * g->stream_words * 4);
  l->chunk_ff = at; at += up16((int64_t)m * g->nchunk * 4);
  l->nbits = at; at += up16((int64_t)m * 4);
  l->ent = at; at += (int64_t)m * g->nsub * 16;
  l->ex0 = at; at += (int64_t)m * g->nsub * 16;
  l->ex1 = at; at += (int64_t)m * g->nsub * 16;
  l->first = at; at += up16((int64_t)m * g->nsub * 4);
  l->total = at;
  return true;
}

// What the caller uploaded: m segments somewhere in `scan`.
struct Upload {
  const uint8_t* scan;
  int64_t scan_bytes;
  const int32_t* offsets;
  const int32_t* lengths;
};

// frame f's segment, clamped to the upload and to the capacity the workspace was sized for
__device__ __forceinline__ const uint8_t* dd_jd_range(const Upload& u, int64_t f, int32_t cap, int32_t* len) {
  const int64_t off = min(max((int64_t)u.offsets[f], (int64_t)0), u.scan_bytes);
  *len = (int32_t)min(max((int64_t)u.lengths[f], (int64_t)0), min((int64_t)cap, u.scan_bytes - off));
  return u.scan + off;
}

__device__ __forceinline__ uint32_t dd_jd_block_sum(uint32_t v, uint32_t* s_red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  uint32_t t = 0;
#pragma unroll
  for (int i = 0; i < kThreads / DD_WAVE; ++i) t += s_red[i];
  return t;
}

// ---- stuffing -----------------------------------------------------------------------------------------------------------

// this thread's 16 bytes of the chunk, the byte in front of them, and how many of them lie in the segment
__device__ __forceinline__ int dd_jd_load16(const uint8_t* src, int32_t len, int64_t first, uint8_t (&b)[16], uint8_t* prev) {
  const int n = (int)max((int64_t)0, min((int64_t)16, (int64_t)len - first));
  *prev = (n > 0 && first > 0) ? src[first - 1] : (uint8_t)0;
#pragma unroll
  for (int i = 0; i < 16; ++i) b[i] = i < n ? src[first + i] : (uint8_t)0;
  return n;
}

__global__ __launch_bounds__(kThreads)
void dd_jpegd_ffcount_kernel(const Upload u, uint32_t* __restrict__ chunk_ff, int32_t* __restrict__ status, const Geom g) {
  __shared__ uint32_t s_red[kThreads / DD_WAVE];
  const int64_t f = blockIdx.y;
  if (blockIdx.x == 0 && threadIdx.x == 0) status[f] = 0;
  int32_t len;
  const uint8_t* src = dd_jd_range(u, f, g.cap, &len);
  const int64_t c0 = (int64_t)blockIdx.x * kChunk;
  if (c0 >= len) return;
  uint8_t b[16], prev;
  const int n = dd_jd_load16(src, len, c0 + threadIdx.x * 16, b, &prev);
  uint32_t ff = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    ff += (i < n && b[i] == 0 && prev == 0xFF) ? 1u : 0u;
    prev = b[i];
  }
  ff = dd_jd_block_sum(ff, s_red);
  if (threadIdx.x == 0) chunk_ff[f * g.nchunk + blockIdx.x] = ff;
}

__global__ __launch_bounds__(kThreads)
void dd_jpegd_unstuff_kernel(const Upload u, const uint32_t* __restrict__ chunk_ff, uint32_t* __restrict__ stream,
                             int32_t* __restrict__ nbits, const Geom g) {
  __shared__ uint32_t s_red[kThreads / DD_WAVE];
  __shared__ uint32_t s_scan[kThreads];
  const int tid = threadIdx.x;
  const int64_t f = blockIdx.y;
  int32_t len;
  const uint8_t* src = dd_jd_range(u, f, g.cap, &len);
  const int chunk = blockIdx.x;
  const bool tail = chunk == g.nchunk;                       // the extra workgroup: the segment's length without stuffing
  const int64_t c0 = (int64_t)chunk * kChunk;
  if (!tail && c0 >= len) return;
  const int before = tail ? (len + kChunk - 1) / kChunk : chunk;
  uint32_t ffs = 0;
  for (int i = tid; i < before; i += kThreads) ffs += chunk_ff[f * g.nchunk + i];
  ffs = dd_jd_block_sum(ffs, s_red);
  if (tail) {
    if (tid == 0) nbits[f] = (int32_t)(((int64_t)len - (int64_t)min(ffs, (uint32_t)len)) * 8);
    return;
  }
  uint8_t b[16], prev;
  const int n = dd_jd_load16(src, len, c0 + tid * 16, b, &prev);
  uint32_t drop = 0;                                         // bit i: byte i is a stuffing byte
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    drop |= (i < n && b[i] == 0 && prev == 0xFF) ? 1u << i : 0u;
    prev = b[i];
  }
  const uint32_t ff = (uint32_t)__builtin_popcount(drop);
  s_scan[tid] = ff;
  __syncthreads();
  for (int d = 1; d < kThreads; d <<= 1) {                   // inclusive scan of the threads' counts
    const uint32_t add = tid >= d ? s_scan[tid - d] : 0u;
    __syncthreads();
    s_scan[tid] += add;
    __syncthreads();
  }
  uint8_t* dst = reinterpret_cast<uint8_t*>(stream + f * g.stream_words);
  int64_t at = c0 + tid * 16 - (int64_t)ffs - (int64_t)(s_scan[tid] - ff);
  const int64_t room = (int64_t)g.stream_words * 4;
  for (int i = 0; i < n; ++i) {
    if (drop >> i & 1u) continue;
    if (at >= 0 && at < room) dst[at] = b[i];
    ++at;
  }
}

// ---- the self-synchronising decode --------------------------------------------------------------------------------------

__device__ __forceinline__ void dd_jd_load_tables(DdJdTables* s_t, const DdJdTables* t) {
  const uint32_t* src = reinterpret_cast<const uint32_t*>(t);
  uint32_t* dst = reinterpret_cast<uint32_t*>(s_t);
  for (int i = threadIdx.x; i < (int)(sizeof(DdJdTables) / 4); i += blockDim.x) dst[i] = src[i];
}

__device__ __forceinline__ int32_t dd_jd_subs(int32_t nb, const Geom& g) {
  return min((int32_t)(((int64_t)max(nb, 0) + kSub - 1) / kSub), g.nsub);
}

// first != 0: the speculative pass.  Otherwise one round: ex_prev holds every lane's exit of the pass before.
__global__ __launch_bounds__(kThreads)
void dd_jpegd_spec_kernel(const uint32_t* __restrict__ stream, const int32_t* __restrict__ nbits,
                          const DdJdTables* __restrict__ tables, DdJdState* __restrict__ ent,
                          const DdJdState* __restrict__ ex_prev, DdJdState* __restrict__ ex_next, const Geom g,
                          const int first) {
  __shared__ DdJdTables s_t;
  const int64_t f = blockIdx.y;
  dd_jd_load_tables(&s_t, tables + f);
  __syncthreads();
  const int32_t nb = nbits[f];
  const int32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= dd_jd_subs(nb, g)) return;
  const int64_t at = f * g.nsub + i;
  DdJdState e = {i * kSub, 0, 0, 0};
  if (!first) {
    if (i > 0) e = ex_prev[at - 1];
    if (dd_jd_same(ent[at], e)) {                            // the exit of the pass before still stands
      ex_next[at] = ex_prev[at];
      return;
    }
  }
  ent[at] = e;
  uint32_t flags = 0;
  ex_next[at] = dd_jd_decode_sub<false>(stream + f * g.stream_words, g.stream_words, nb, (i + 1) * kSub, e, &s_t, g.bpm,
                                        nullptr, 0, 0, &flags);
}

__device__ __forceinline__ DdJdState dd_jd_shfl_up1(const DdJdState& s) {
  DdJdState r;
  r.pos = __shfl_up(s.pos, 1, 64);
  r.blk = __shfl_up(s.blk, 1, 64);
  r.idx = __shfl_up(s.idx, 1, 64);
  r.nblk = 0;
  return r;
}

// One wave per frame.  Entry 0 is true; entry i is true if it equals exit i - 1 and entry i - 1 is true.  The wave looks at
// 64 entries at a time; the first one that differs from its neighbour's exit takes that exit as its entry and is decoded
// again, which may change its own exit, so the entries behind it are compared again, from there on only.
__global__ __launch_bounds__(DD_WAVE)
void dd_jpegd_repair_kernel(const uint32_t* __restrict__ stream, const int32_t* __restrict__ nbits,
                            const DdJdTables* __restrict__ tables, DdJdState* __restrict__ ent, DdJdState* __restrict__ ex,
                            const Geom g) {
  __shared__ DdJdTables s_t;
  const int64_t f = blockIdx.x;
  dd_jd_load_tables(&s_t, tables + f);
  __syncthreads();
  const int lane = threadIdx.x;
  const int32_t nb = nbits[f];
  const int32_t nsub = dd_jd_subs(nb, g);
  const uint32_t* words = stream + f * g.stream_words;
  DdJdState carry = {0, 0, 0, 0};                            // the exit in front of the group: the stream's true start
  for (int32_t base = 0; base < nsub; base += DD_WAVE) {
    const int32_t i = base + lane;
    const bool active = i < nsub;
    const int64_t at = f * g.nsub + (active ? i : base);
    DdJdState e = ent[at], x = ex[at];
    int start = 0;
    for (int turn = 0; turn < DD_WAVE; ++turn) {
      DdJdState p = dd_jd_shfl_up1(x);
      if (lane == 0) p = carry;
      const bool bad = active && lane >= start && !dd_jd_same(e, p);
      const uint64_t mask = __ballot(bad);
      if (!mask) break;
      const int j = __builtin_ctzll(mask);
      if (lane == j) {
        e = p;
        e.nblk = 0;
        uint32_t flags = 0;
        x = dd_jd_decode_sub<false>(words, g.stream_words, nb, (i + 1) * kSub, e, &s_t, g.bpm, nullptr, 0, 0, &flags);
        ent[at] = e;
        ex[at] = x;
      }
      start = j + 1;
    }
    carry.pos = __shfl(x.pos, DD_WAVE - 1, 64);
    carry.blk = __shfl(x.blk, DD_WAVE - 1, 64);
    carry.idx = __shfl(x.idx, DD_WAVE - 1, 64);
  }
}

// One workgroup per frame: thread t owns the `per` consecutive subsequences from t * per.
__global__ __launch_bounds__(kScanThreads)
void dd_jpegd_blocks_kernel(const int32_t* __restrict__ nbits, const DdJdState* __restrict__ ex, int32_t* __restrict__ first,
                            int32_t* __restrict__ status, const Geom g) {
  __shared__ uint32_t s_sum[kScanThreads];
  const int tid = threadIdx.x;
  const int64_t f = blockIdx.x;
  const int32_t nsub = dd_jd_subs(nbits[f], g);
  const int per = (nsub + kScanThreads - 1) / kScanThreads;
  const int i0 = min(tid * per, nsub), i1 = min(i0 + per, nsub);
  uint32_t mine = 0;
  for (int i = i0; i < i1; ++i) mine += (uint32_t)max(ex[f * g.nsub + i].nblk, 0);
  s_sum[tid] = mine;
  __syncthreads();
  for (int d = 1; d < kScanThreads; d <<= 1) {
    const uint32_t add = tid >= d ? s_sum[tid - d] : 0u;
    __syncthreads();
    s_sum[tid] += add;
    __syncthreads();
  }
  uint32_t at = s_sum[tid] - mine;
  for (int i = i0; i < i1; ++i) {
    first[f * g.nsub + i] = (int32_t)min(at, (uint32_t)g.nblk);
    at += (uint32_t)max(ex[f * g.nsub + i].nblk, 0);
  }
  if (tid == kScanThreads - 1 && s_sum[tid] < (uint32_t)g.nblk) atomicOr(&status[f], DD_JD_EXHAUSTED);
}

__global__ __launch_bounds__(kThreads)
void dd_jpegd_emit_kernel(const uint32_t* __restrict__ stream, const int32_t* __restrict__ nbits,
                          const DdJdTables* __restrict__ tables, const DdJdState* __restrict__ ent,
                          const int32_t* __restrict__ first, int16_t* __restrict__ coef, int32_t* __restrict__ status,
                          const Geom g) {
  __shared__ DdJdTables s_t;
  const int64_t f = blockIdx.y;
  dd_jd_load_tables(&s_t, tables + f);
  __syncthreads();
  const int32_t nb = nbits[f];
  const int32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= dd_jd_subs(nb, g)) return;
  const int64_t at = f * g.nsub + i;
  uint32_t flags = 0;
  dd_jd_decode_sub<true>(stream + f * g.stream_words, g.stream_words, nb, (i + 1) * kSub, ent[at], &s_t, g.bpm,
                         coef + f * g.nblk * 64, first[at], g.nblk, &flags);
  if (flags) atomicOr(&status[f], (int32_t)flags);
}

// ---- from coefficients to pixels ----------------------------------------------------------------------------------------

// the j-th block of component c in scan order
__device__ __forceinline__ int32_t dd_jd_comp_block(int32_t j, int c, int bpm) {
  if (bpm == 3) return j * 3 + c;
  return c == 0 ? (j >> 2) * 6 + (j & 3) : j * 6 + 3 + c;
}

// One workgroup per frame and component: the DC differences become DC values, in place (modulo 2^16, as they are stored).
__global__ __launch_bounds__(kScanThreads)
void dd_jpegd_dc_kernel(int16_t* __restrict__ coef, const Geom g) {
  __shared__ uint32_t s_sum[kScanThreads];
  const int tid = threadIdx.x, c = blockIdx.x;
  int16_t* cf = coef + (int64_t)blockIdx.y * g.nblk * 64;
  const int n = g.nmcu * ((g.bpm == 6 && c == 0) ? 4 : 1);
  const int per = (n + kScanThreads - 1) / kScanThreads;
  const int i0 = min(tid * per, n), i1 = min(i0 + per, n);
  uint32_t mine = 0;
  for (int i = i0; i < i1; ++i) mine += (uint32_t)(int32_t)cf[(int64_t)dd_jd_comp_block(i, c, g.bpm) * 64];
  s_sum[tid] = mine;
  __syncthreads();
  for (int d = 1; d < kScanThreads; d <<= 1) {
    const uint32_t add = tid >= d ? s_sum[tid - d] : 0u;
    __syncthreads();
    s_sum[tid] += add;
    __syncthreads();
  }
  uint32_t at = s_sum[tid] - mine;
  for (int i = i0; i < i1; ++i) {
    int16_t* p = cf + (int64_t)dd_jd_comp_block(i, c, g.bpm) * 64;
    at += (uint32_t)(int32_t)*p;
    *p = (int16_t)(uint16_t)at;
  }
}

// Eight lanes per block, 32 blocks per workgroup: lane c of a block takes column c, then row c.
__global__ __launch_bounds__(kThreads)
void dd_jpegd_idct_kernel(const int16_t* __restrict__ coef, const DdJdTables* __restrict__ tables,
                          uint8_t* __restrict__ planes, const Geom g) {
  __shared__ int32_t s_ws[kThreads / 8][64];
  const int64_t f = blockIdx.y;
  const int slot = threadIdx.x >> 3, c = threadIdx.x & 7;
  const int32_t raw = blockIdx.x * (kThreads / 8) + slot;
  const bool active = raw < g.nblk;
  const int32_t b = active ? raw : g.nblk - 1;               // an idle slot works on a valid block and stores nothing
  const int32_t mcu = b / g.bpm, k = b - mcu * g.bpm;
  const int32_t comp = dd_jd_component(k, g.bpm);
  dd_jd_idct_column(coef + (f * g.nblk + b) * 64, tables[f].q[comp], c, s_ws[slot]);
  __syncthreads();
  uint8_t px[8];
  dd_jd_idct_row(s_ws[slot], c, px);
  if (!active) return;
  const int32_t my = mcu / g.mw, mx = mcu - my * g.mw;
  uint8_t* pl = planes + f * g.plane_bytes;
  int64_t at;
  if (comp == 0 && g.bpm == 6) at = (int64_t)((2 * my + (k >> 1)) * 8 + c) * g.yw + (2 * mx + (k & 1)) * 8;
  else if (comp == 0) at = (int64_t)(my * 8 + c) * g.yw + mx * 8;
  else at = g.c_off + (comp - 1) * g.c_size + (int64_t)(my * 8 + c) * g.cw + mx * 8;
  u32x2 v;
  __builtin_memcpy(&v, px, 8);
  *reinterpret_cast<u32x2*>(pl + at) = v;                    // plane bases are multiples of 16, strides and columns of 8
}

__global__ __launch_bounds__(kThreads)
void dd_jpegd_colour_kernel(const uint8_t* __restrict__ planes, uint8_t* __restrict__ out, const Geom g) {
  const int64_t f = blockIdx.y;
  const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (p >= (int64_t)g.h * g.w) return;
  const int32_t y = (int32_t)(p / g.w), x = (int32_t)(p - (int64_t)y * g.w);
  const uint8_t* pl = planes + f * g.plane_bytes;
  const uint8_t* pcb = pl + g.c_off;
  const uint8_t* pcr = pcb + g.c_size;
  const int32_t yy = pl[(int64_t)y * g.yw + x];
  int32_t cb, cr;
  if (g.bpm == 6) {
    cb = dd_jd_upsample(pcb, g.cw, g.tch, g.tcw, y, x);
    cr = dd_jd_upsample(pcr, g.cw, g.tch, g.tcw, y, x);
  } else {
    cb = pcb[(int64_t)y * g.cw + x];
    cr = pcr[(int64_t)y * g.cw + x];
  }
  uint8_t rgb[3];
  dd_jd_rgb(yy, cb, cr, rgb);
  uint8_t* o = out + (f * g.h * g.w + p) * 3;
  o[0] = rgb[0];
  o[1] = rgb[1];
  o[2] = rgb[2];
}

static inline bool sizes_ok(int32_t m, int32_t h, int32_t w, int32_t sampling, int64_t max_scan_bytes) {
  return m > 0 && h > 0 && w > 0 && h <= 65535 && w <= 65535 && (sampling == 420 || sampling == 444) && max_scan_bytes > 0;
}

}  // namespace

extern "C" int64_t dd_jpeg_decode_workspace_bytes(int32_t m, int32_t h, int32_t w, int32_t sampling, int64_t max_scan_bytes) {
  if (!sizes_ok(m, h, w, sampling, max_scan_bytes) || m > 65535) return -1;
  Geom g;
  Layout l;
  if (!geometry(m, h, w, sampling, max_scan_bytes, &g, &l)) return -1;
  return l.total;
}

extern "C" int dd_jpeg_decode_u8(const uint8_t* scan, int64_t scan_bytes, const int32_t* offsets, const int32_t* lengths,
                                 int64_t max_scan_bytes, const void* tables, int32_t m, int32_t h, int32_t w,
                                 int32_t sampling, uint8_t* out, int32_t* status, void* workspace, int64_t workspace_bytes,
                                 int32_t rounds, dd_stream_t stream) {
  if (!scan || !offsets || !lengths || !tables || !out || !status || !workspace) return DD_ERR_BAD_ARG;
  if (!sizes_ok(m, h, w, sampling, max_scan_bytes) || scan_bytes <= 0 || rounds < -1 || rounds > 64) return DD_ERR_BAD_ARG;
  if (!dd_aligned16(workspace) || (reinterpret_cast<uintptr_t>(tables) & 3u) || (reinterpret_cast<uintptr_t>(offsets) & 3u) ||
      (reinterpret_cast<uintptr_t>(lengths) & 3u) || (reinterpret_cast<uintptr_t>(status) & 3u))
    return DD_ERR_BAD_ARG;
  Geom g;
  Layout l;
  if (!geometry(m, h, w, sampling, max_scan_bytes, &g, &l) || m > 65535) return DD_ERR_UNSUPPORTED;
  if (workspace_bytes < l.total) return DD_ERR_BAD_ARG;
  if (rounds < 0) rounds = DD_JPEG_DECODE_ROUNDS;
  uint8_t* ws = reinterpret_cast<uint8_t*>(workspace);
  int16_t* coef = reinterpret_cast<int16_t*>(ws + l.coef);
  uint8_t* planes = ws + l.planes;
  uint32_t* bits = reinterpret_cast<uint32_t*>(ws + l.stream);
  uint32_t* chunk_ff = reinterpret_cast<uint32_t*>(ws + l.chunk_ff);
  int32_t* nbits = reinterpret_cast<int32_t*>(ws + l.nbits);
  DdJdState* ent = reinterpret_cast<DdJdState*>(ws + l.ent);
  DdJdState* ex[2] = {reinterpret_cast<DdJdState*>(ws + l.ex0), reinterpret_cast<DdJdState*>(ws + l.ex1)};
  int32_t* first = reinterpret_cast<int32_t*>(ws + l.first);
  const DdJdTables* tab = reinterpret_cast<const DdJdTables*>(tables);
  const Upload u = {scan, scan_bytes, offsets, lengths};
  const dim3 per_sub((unsigned)((g.nsub + kThreads - 1) / kThreads), (unsigned)m);
  hipStream_t s = dd_stream(stream);
  dd_clear_error();
  if (hipMemsetAsync(coef, 0, (size_t)m * g.nblk * 64 * 2, s) != hipSuccess) return DD_ERR_LAUNCH;
  hipLaunchKernelGGL(dd_jpegd_ffcount_kernel, dim3((unsigned)g.nchunk, (unsigned)m), dim3(kThreads), 0, s, u, chunk_ff, status, g);
  hipLaunchKernelGGL(dd_jpegd_unstuff_kernel, dim3((unsigned)g.nchunk + 1, (unsigned)m), dim3(kThreads), 0, s, u, chunk_ff, bits,
                     nbits, g);
  int cur = 0;
  hipLaunchKernelGGL(dd_jpegd_spec_kernel, per_sub, dim3(kThreads), 0, s, bits, nbits, tab, ent, ex[1], ex[0], g, 1);
  for (int r = 0; r < rounds; ++r) {
    hipLaunchKernelGGL(dd_jpegd_spec_kernel, per_sub, dim3(kThreads), 0, s, bits, nbits, tab, ent, ex[cur], ex[cur ^ 1], g, 0);
    cur ^= 1;
  }
  hipLaunchKernelGGL(dd_jpegd_repair_kernel, dim3((unsigned)m), dim3(DD_WAVE), 0, s, bits, nbits, tab, ent, ex[cur], g);
  hipLaunchKernelGGL(dd_jpegd_blocks_kernel, dim3((unsigned)m), dim3(kScanThreads), 0, s, nbits, ex[cur], first, status, g);
  hipLaunchKernelGGL(dd_jpegd_emit_kernel, per_sub, dim3(kThreads), 0, s, bits, nbits, tab, ent, first, coef, status, g);
  hipLaunchKernelGGL(dd_jpegd_dc_kernel, dim3(3, (unsigned)m), dim3(kScanThreads), 0, s, coef, g);
  hipLaunchKernelGGL(dd_jpegd_idct_kernel, dim3((unsigned)((g.nblk + kThreads / 8 - 1) / (kThreads / 8)), (unsigned)m),
                     dim3(kThreads), 0, s, coef, tab, planes, g);
  hipLaunchKernelGGL(dd_jpegd_colour_kernel, dim3((unsigned)(((int64_t)h * w + kThreads - 1) / kThreads), (unsigned)m),
                     dim3(kThreads), 0, s, planes, out, g);
  return dd_check_launch();
}
