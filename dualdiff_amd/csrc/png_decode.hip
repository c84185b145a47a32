// PNG input: the IDAT payloads of m .png files of one geometry -> uint8 frames (m, H, W, 3) in device memory, byte for byte
// `np.asarray(Image.open(f).convert("RGB"))`; and the collate step of the image-mode ORS condition on top of them.
//
// The reference's default ORS condition is one RGBA panorama .png per sample, opened with PIL on the host
// (magicdrive/dataset/dataset_wrapper.py:62-81, misc/test_utils.py:218-222) and cropped per view in collate_fn
// (dataset/utils.py:348-408).  Here the host walks the chunks (pipeline/png_input.py: parse_png) and uploads the
// concatenated IDAT payloads; everything behind that is on the device, in four launches and one memset whatever m and the
// content are:
//
//   chunks    one workgroup (one wave) per 16 KiB slot of a file that has the SHAPE of csrc/png.hip's own format: it inflates
//             its IDAT from bit 0 of the payload into its slot and verifies what makes that equal to the sequential decode —
//             it consumed exactly its payload, produced exactly its slot, no match reached before its slot, and BFINAL came
//             exactly at the end of the last chunk.  Anything else sets the file's fallback flag.
//   stream    one workgroup (one wave) per file, launched unconditionally: the zlib header; then, unless every chunk of the
//             file verified, the whole stream block by block — stored, fixed and dynamic blocks, a 32 KiB window in LDS —
//             into the workspace; then the Adler-32 trailer.  Sets the frame's status.
//   adler     one workgroup per 16 KiB segment of the filtered bytes: its two Adler sums.
//   unfilter  one workgroup per file: the segments' sums joined and compared with the trailer; then the rows unfiltered,
//             1024 of them side by side with thread r on row y0 + r one pixel behind thread r - 1 (left and above-left are
//             the thread's own registers, above comes from the thread before by a shuffle, across waves by a word in
//             LDS), and written as RGB.
//
// How one wave inflates: all 64 lanes walk the stream in step (csrc/png_decode_core.h: dd_pd_inflate) — the same bytes, the
// same tables in LDS, the same values, so control flow never diverges.  Lane 0 reads a block's header and builds its tables;
// literals go to the window by lane 0, a match is copied by all lanes at once (byte i of it is window[pos - dist + i % dist],
// all of which stand before the match), and the window goes to global memory 4 KiB at a time.
//
// The condition is one launch on top: dd_png_condition_kernel (stack and per-view crop), or, for image_size [192, 384],
// dd_png_condition_resize_kernel (crop_drivewm: per view a zero row on top, a bilinear resize, a crop).
#include "dd_common.h"
#include "png_decode_core.h"

namespace {

constexpr int kThreads = 256;
constexpr int kSeg = 16384;                    // csrc/png.hip's chunk: filtered bytes per IDAT of our own files
constexpr int kWindow = 32768;
constexpr int kFlush = 4096;
constexpr int kRows = 1024;                    // rows that are unfiltered side by side, one thread each
constexpr int kWaves = kRows / DD_WAVE;
constexpr int kStep = 8;                       // pixels a thread makes between its loads and its stores

struct Geom {
  int32_t m, h, w;
  int32_t nseg;                                // 16 KiB segments of the longest (RGBA) filtered frame
  int64_t stride;                              // a frame's place in the workspace: h (1 + 4 w) rounded up to 16
};

// Workspace, every part 16-byte aligned:
//   uint32 flag[m] (a chunk of the file did not verify; cleared by the memset) | uint32 trailer[m] (the stream's
//   Adler-32) | uint32 sums[m][nseg][2] | uint8 filt[m][stride]
struct Layout {
  int64_t flag, trailer, sums, filt, total;
};

static inline int64_t up16(int64_t v) { return (v + 15) & ~(int64_t)15; }

static inline bool sizes_ok(int32_t m, int32_t h, int32_t w) { return m > 0 && h > 0 && w > 0; }

// false: more than one call takes (positions in a frame are 32-bit)
static inline bool geometry(int32_t m, int32_t h, int32_t w, Geom* g, Layout* l) {
  const int64_t len = (int64_t)h * (1 + 4 * (int64_t)w);
  if (len > 0x7fffffff - kSeg || m > 65535) return false;
  g->m = m; g->h = h; g->w = w;
  g->nseg = (int32_t)((len + kSeg - 1) / kSeg);
  g->stride = up16(len);
  int64_t at = 0;
  l->flag = at; at += up16((int64_t)m * 4);
  l->trailer = at; at += up16((int64_t)m * 4);
  l->sums = at; at += up16((int64_t)m * g->nseg * 8);
  l->filt = at; at += (int64_t)m * g->stride;
  l->total = at;
  return true;
}

// files: int32 [m][4]: the stream's offset in `streams`, its length, the colour type, the index in `tab` of the file's
// nchunk + 1 IDAT boundaries (relative to the stream's start) or -1
struct Upload {
  const uint8_t* streams;
  int64_t streams_bytes;
  const int32_t* files;
  const int32_t* tab;
  int32_t ntab;
};

struct File {
  const uint8_t* p;
  int64_t n;
  int32_t bpp, tab;
  uint32_t len;                                // filtered bytes of the frame
};

// whatever the tables hold, the stream lies inside `streams`
__device__ __forceinline__ File dd_pngd_file(const Upload& u, int f, const Geom& g) {
  const int32_t* e = u.files + 4 * (int64_t)f;
  int64_t off = e[0], n = e[1];
  off = off < 0 ? 0 : (off > u.streams_bytes ? u.streams_bytes : off);
  n = n < 0 ? 0 : (n > u.streams_bytes - off ? u.streams_bytes - off : n);
  File r;
  r.p = u.streams + off;
  r.n = n;
  const int bpp = dd_pd_bpp(e[2]);
  r.bpp = bpp ? bpp : 3;
  r.tab = e[3];
  r.len = (uint32_t)g.h * (1u + (uint32_t)r.bpp * (uint32_t)g.w);
  return r;
}

// the chunk count of a file of our own format, and whether its boundaries lie inside the table
__device__ __forceinline__ int dd_pngd_nchunk(const Upload& u, const File& f) {
  if (f.bpp != 3 || f.tab < 0) return 0;
  const int64_t n = ((int64_t)f.len + kSeg - 1) / kSeg;
  return (int64_t)f.tab + n + 1 <= (int64_t)u.ntab ? (int)n : 0;
}

// LDS stores of one lane, seen by the other lanes of the wave: the DS queue is in order, the compiler must not reorder
__device__ __forceinline__ void dd_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Where one wave's inflate goes: a window of `mask + 1` bytes in LDS (a power of two, at least every distance the walk
// lets through), and dst[0, limit) in global memory behind it; dst is 4-byte aligned.
struct WaveCtx {
  uint8_t* win;
  uint32_t mask;
  uint8_t* dst;
  uint32_t flushed;
  int lane;

  __device__ __forceinline__ bool leader() const { return lane == 0; }
  __device__ __forceinline__ void sync() const { __syncthreads(); }
  __device__ __forceinline__ void lit(uint32_t pos, uint32_t byte) {
    if (lane == 0) win[pos & mask] = (uint8_t)byte;
  }
  // Source and destination may share window slots only when dist + len passes the window's size, and then slot of
  // destination byte i is the slot of source byte i - (size - dist), an earlier one: read in this step or a step before.
  __device__ __forceinline__ void copy(uint32_t pos, uint32_t len, uint32_t dist) {
    dd_wave_sync();
    for (uint32_t i0 = 0; i0 < len; i0 += DD_WAVE) {
      const uint32_t i = i0 + (uint32_t)lane;
      uint8_t v = 0;
      if (i < len) v = win[(pos - dist + i % dist) & mask];
      dd_wave_sync();
      if (i < len) win[(pos + i) & mask] = v;
    }
  }
  // the window's bytes [flushed, upto) to global memory
  __device__ __forceinline__ void flush(uint32_t upto) {
    dd_wave_sync();
    while ((flushed & 3u) && flushed < upto) {
      if (lane == 0) dst[flushed] = win[flushed & mask];
      flushed += 1;
    }
    const uint32_t nw = (upto - flushed) >> 2;
    for (uint32_t k = (uint32_t)lane; k < nw; k += DD_WAVE) {
      const uint32_t at = flushed + 4u * k;
      *reinterpret_cast<uint32_t*>(dst + at) = *reinterpret_cast<const uint32_t*>(win + (at & mask));
    }
    flushed += 4u * nw;
    const uint32_t rest = upto - flushed;      // < 4
    if ((uint32_t)lane < rest) dst[flushed + lane] = win[(flushed + lane) & mask];
    flushed = upto;
  }
  __device__ __forceinline__ void stored(const uint8_t* src, uint32_t pos, uint32_t n) {
    flush(pos);
    for (uint32_t i = (uint32_t)lane; i < n; i += DD_WAVE) {
      const uint8_t v = src[i];
      dst[pos + i] = v;
      if (n - i <= mask + 1u) win[(pos + i) & mask] = v;     // the last window's worth: one writer per slot
    }
    flushed = pos + n;
  }
  __device__ __forceinline__ void advance(uint32_t pos) {
    if (pos - flushed >= (uint32_t)kFlush) flush(pos & ~3u);
  }
};

// ---- chunks ---------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(DD_WAVE)
void dd_pngd_chunk_kernel(const Upload u, uint8_t* __restrict__ filt, uint32_t* __restrict__ flag, const Geom g) {
  __shared__ __attribute__((aligned(16))) uint8_t s_win[kSeg];
  __shared__ DdPdShared s_sh;
  const int f = blockIdx.y, c = blockIdx.x;
  const File file = dd_pngd_file(u, f, g);
  const int nchunk = dd_pngd_nchunk(u, file);
  if (c >= nchunk) return;                                   // the whole workgroup: nothing here depends on the thread
  const bool last = c == nchunk - 1;
  const int64_t t0 = u.tab[file.tab + c], t1 = u.tab[file.tab + c + 1];
  const int64_t lo = t0 + (c == 0 ? 2 : 0), hi = t1 - (last ? 4 : 0);
  const uint32_t want = (uint32_t)min((int64_t)kSeg, (int64_t)file.len - (int64_t)c * kSeg);
  bool ok = t0 >= 0 && t1 <= file.n && lo <= hi;
  uint32_t pos = 0;
  if (ok) {                                                  // uniform
    DdPdBits br;
    dd_pd_open(br, file.p + lo, hi - lo);
    WaveCtx ctx = {s_win, (uint32_t)kSeg - 1u, filt + (int64_t)f * g.stride + (int64_t)c * kSeg, 0u, (int)threadIdx.x};
    int final_seen = 0;
    const uint32_t err = dd_pd_inflate(br, &s_sh, ctx, want, (hi - lo) * 8, &pos, &final_seen);
    ctx.flush(pos);
    ok = err == 0 && pos == want && br.used == (hi - lo) * 8 && (final_seen != 0) == last;
  }
  if (!ok && threadIdx.x == 0) atomicOr(&flag[f], 1u);
}

// ---- the stream -----------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(DD_WAVE)
void dd_pngd_stream_kernel(const Upload u, uint8_t* __restrict__ filt, const uint32_t* __restrict__ flag,
                           uint32_t* __restrict__ trailer, int32_t* __restrict__ status, int32_t* __restrict__ paths,
                           const Geom g, const int use_chunks) {
  __shared__ __attribute__((aligned(16))) uint8_t s_win[kWindow];
  __shared__ DdPdShared s_sh;
  const int f = blockIdx.x;
  const File file = dd_pngd_file(u, f, g);
  const bool chunked = use_chunks && dd_pngd_nchunk(u, file) > 0 && flag[f] == 0u;
  DdPdBits br;
  dd_pd_open(br, file.p, file.n);
  uint32_t err = 0, adler = 0;
  const uint32_t cmf = dd_pd_take(br, 8), flg = dd_pd_take(br, 8);
  if (dd_pd_over(br)) err = DD_PD_TRUNCATED;
  else if (!dd_pd_zlib_header_ok(cmf, flg)) err = DD_PD_BAD_ZLIB;
  if (!err && chunked) {
    dd_pd_seek(br, file.n - 4);                              // >= 2: the chunks verified
  } else if (!err) {                                         // uniform: every lane holds the same values
    WaveCtx ctx = {s_win, (uint32_t)kWindow - 1u, filt + (int64_t)f * g.stride, 0u, (int)threadIdx.x};
    uint32_t pos = 0;
    int final_seen = 0;
    err = dd_pd_inflate(br, &s_sh, ctx, file.len, -1, &pos, &final_seen);
    ctx.flush(pos);
    if (!err && pos < file.len) err = DD_PD_TOO_SHORT;
  }
  if (!err) err = dd_pd_trailer(br, &adler);
  if (threadIdx.x == 0) {
    paths[f] = chunked ? 1 : 0;
    trailer[f] = adler;
    status[f] = (int32_t)err;
  }
}

// ---- Adler-32 -------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kThreads)
void dd_pngd_adler_kernel(const Upload u, const uint8_t* __restrict__ filt, const int32_t* __restrict__ status,
                          uint32_t* __restrict__ sums, const Geom g) {
  __shared__ uint32_t s_a[kThreads], s_b[kThreads];
  const int f = blockIdx.y, seg = blockIdx.x, tid = threadIdx.x;
  const File file = dd_pngd_file(u, f, g);
  const int64_t start = (int64_t)seg * kSeg;
  if (start >= (int64_t)file.len || status[f] != 0) return;  // the whole workgroup
  const int n = (int)min((int64_t)kSeg, (int64_t)file.len - start);
  const uint8_t* x = filt + (int64_t)f * g.stride + start;
  constexpr int per = kSeg / kThreads;                       // 64 consecutive bytes per thread
  const int lo = min(tid * per, n), hi = min(lo + per, n);
  uint32_t a = 0, b = 0;                                     // < 64 * 255, < 16384 * 64 * 255
  for (int k = lo; k < hi; ++k) {
    a += x[k];
    b += (uint32_t)(n - k) * x[k];
  }
  s_a[tid] = a;
  s_b[tid] = b % DD_PD_ADLER;
  __syncthreads();
  for (int d = kThreads / 2; d > 0; d >>= 1) {
    if (tid < d) {
      s_a[tid] += s_a[tid + d];                              // < 16384 * 255
      s_b[tid] = (s_b[tid] + s_b[tid + d]) % DD_PD_ADLER;
    }
    __syncthreads();
  }
  if (tid == 0) {
    uint32_t* o = sums + ((int64_t)f * g.nseg + seg) * 2;
    o[0] = s_a[0] % DD_PD_ADLER;
    o[1] = s_b[0];
  }
}

// ---- unfilter and convert -------------------------------------------------------------------------------------------------

template <int BPP>
__device__ __forceinline__ uint32_t dd_pngd_load_px(const uint8_t* p) {
  uint32_t v = p[0];
  if (BPP >= 3) v |= ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
  if (BPP == 4) v |= (uint32_t)p[3] << 24;
  return v;
}

// The rows of one frame unfiltered, thread r of a sweep on row y0 + r, one pixel behind thread r - 1: at step t it makes
// pixel x = t - r from its own last pixel (left), the pixel thread r - 1 made one step ago (above: a shuffle inside a
// wave, a word in LDS from the last lane of the wave before, two words in turn so that one barrier per step orders them)
// and what that was a step earlier (above left).  kStep steps at a time between the loads of the filtered bytes and the
// stores of the RGB pixels, so that a barrier waits for memory once per kStep pixels.  The last row of a sweep is also
// written back to the workspace: thread 0 of the next sweep reads it as the row above.
template <int BPP>
__device__ __forceinline__ void dd_pngd_unfilter_rows(uint8_t* base, uint8_t* o, int h, int w, uint32_t* s_edge, uint32_t* s_bad) {
  const int tid = threadIdx.x, lane = tid & (DD_WAVE - 1), wave = tid / DD_WAVE;
  const int64_t row = 1 + (int64_t)BPP * w;
  for (int y0 = 0; y0 < h; y0 += kRows) {
    const int y = y0 + tid;
    const bool rowok = y < h;
    uint8_t* cur = base + (int64_t)(rowok ? y : 0) * row;
    int type = rowok ? cur[0] : 0;
    if (type > 4) {
      atomicOr(s_bad, 1u);
      type = 0;
    }
    const bool keep = tid == kRows - 1 && y + 1 < h;         // the row above the next sweep
    const int steps = w + min(kRows, h - y0) - 1;
    uint32_t last = 0, above_left = 0;
    for (int t0 = 0; t0 < steps; t0 += kStep) {              // every thread takes every turn: the barriers are uniform
      uint32_t v[kStep], first[kStep], r[kStep];
#pragma unroll
      for (int j = 0; j < kStep; ++j) {
        const int x = t0 + j - tid;
        const bool ok = rowok && x >= 0 && x < w;
        const uint8_t* p = cur + 1 + (int64_t)(ok ? x : 0) * BPP;
        v[j] = ok ? dd_pngd_load_px<BPP>(p) : 0u;
        first[j] = (ok && tid == 0 && y > 0) ? dd_pngd_load_px<BPP>(p - row) : 0u;     // the sweep before is complete
      }
#pragma unroll
      for (int j = 0; j < kStep; ++j) {
        const int t = t0 + j, x = t - tid;
        uint32_t up = __shfl_up(last, 1, DD_WAVE);
        if (lane == 0 && wave > 0) up = s_edge[((t + 1) & 1) * kWaves + wave - 1];     // written one step ago
        if (tid == 0) up = first[j];
        r[j] = 0u;
        if (rowok && x >= 0 && x < w) {
          const uint32_t a = x > 0 ? last : 0u, c = x > 0 ? above_left : 0u;
          uint32_t q = 0;
#pragma unroll
          for (int k = 0; k < BPP; ++k)
            q |= dd_pd_unfilter(type, (v[j] >> (8 * k)) & 255u, (a >> (8 * k)) & 255u, (up >> (8 * k)) & 255u,
                                (c >> (8 * k)) & 255u) << (8 * k);
          r[j] = q;
          last = q;
          above_left = up;
        }
        if (lane == DD_WAVE - 1) s_edge[(t & 1) * kWaves + wave] = last;
        __syncthreads();
      }
#pragma unroll
      for (int j = 0; j < kStep; ++j) {
        const int x = t0 + j - tid;
        if (rowok && x >= 0 && x < w) {
          uint8_t* d = o + ((int64_t)y * w + x) * 3;
          d[0] = (uint8_t)r[j];
          d[1] = (uint8_t)(BPP == 1 ? r[j] : r[j] >> 8);
          d[2] = (uint8_t)(BPP == 1 ? r[j] : r[j] >> 16);
          if (keep) {
            uint8_t* p = cur + 1 + (int64_t)x * BPP;
#pragma unroll
            for (int k = 0; k < BPP; ++k) p[k] = (uint8_t)(r[j] >> (8 * k));
          }
        }
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kRows)
void dd_pngd_unfilter_kernel(const Upload u, uint8_t* __restrict__ filt, const uint32_t* __restrict__ trailer,
                             const uint32_t* __restrict__ sums, uint8_t* __restrict__ out, int32_t* __restrict__ status,
                             const Geom g) {
  __shared__ uint32_t s_stop, s_bad;
  __shared__ uint32_t s_edge[2 * kWaves];
  const int f = blockIdx.x, tid = threadIdx.x;
  const File file = dd_pngd_file(u, f, g);
  if (tid == 0) {
    uint32_t stop = status[f] != 0 ? 1u : 0u;
    if (!stop) {
      uint32_t A = 1, B = 0;
      const int nseg = (int)(((int64_t)file.len + kSeg - 1) / kSeg);         // <= g.nseg
      for (int s = 0; s < nseg; ++s) {
        const uint32_t* o = sums + ((int64_t)f * g.nseg + s) * 2;
        dd_pd_adler_join(&A, &B, o[0], o[1], min((int64_t)kSeg, (int64_t)file.len - (int64_t)s * kSeg));
      }
      if (((B << 16) | A) != trailer[f]) {
        status[f] = DD_PD_BAD_ADLER;
        stop = 1u;
      }
    }
    s_stop = stop;
    s_bad = 0u;
  }
  __syncthreads();
  if (s_stop) return;                                        // the whole workgroup, on the flag in LDS
  uint8_t* base = filt + (int64_t)f * g.stride;
  uint8_t* o = out + (int64_t)f * g.h * g.w * 3;
  if (file.bpp == 1) dd_pngd_unfilter_rows<1>(base, o, g.h, g.w, s_edge, &s_bad);            // uniform: one file, one type
  else if (file.bpp == 3) dd_pngd_unfilter_rows<3>(base, o, g.h, g.w, s_edge, &s_bad);
  else dd_pngd_unfilter_rows<4>(base, o, g.h, g.w, s_edge, &s_bad);
  if (tid == 0 && s_bad) status[f] = DD_PD_BAD_FILTER;
}

// ---- the ORS condition ----------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kThreads)
void dd_png_condition_kernel(const uint8_t* __restrict__ frames, float* __restrict__ out, const float* __restrict__ lut,
                             int64_t total, int h, int w, int views, int top, int left, int oh, int ow) {
  const int pw = w / views;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kThreads) {
    const int ox = (int)(i % ((int64_t)views * ow));
    int64_t r = i / ((int64_t)views * ow);
    const int oy = (int)(r % oh);
    r /= oh;
    const int c = (int)(r % 3);
    const int64_t b = r / 3;
    const int v = ox / ow, x = v * pw + left + ox % ow, y = top + oy;
    out[i] = lut[frames[((b * h + y) * w + x) * 3 + c]];
  }
}

// crop_drivewm's pad, resize and crop (dataset/utils.py:355-358, 374-388) per view: what the kernel below is told
struct Resize {
  int h, w, pw;                                // the frames; pw = w / views
  int pad;                                     // zero rows above every view
  int top, left, oh, ow;                       // the crop of the resized view
  int row;                                     // views * ow: one row of the output
};

// One output element: the bilinear sample of the padded view at resized row top + oy, column left + ox % ow.  The taps and
// weights of both axes come from the host's float32 tables; the combination is spelled out operation by operation — the
// horizontal pair of each row first, products rounded on their own, the sums fused — so that the compiler's contraction has
// nothing to decide.  A tap is clamped to the padded view whatever the tables hold.
__device__ __forceinline__ float dd_pngc_sample(const uint8_t* __restrict__ frames, const float* __restrict__ lut,
                                                const int32_t* __restrict__ ridx, const float* __restrict__ rlam,
                                                const int32_t* __restrict__ cidx, const float* __restrict__ clam,
                                                const Resize& g, int64_t b, int c, int oy, int ox) {
  const int v = ox / g.ow, x = g.left + ox - v * g.ow, y = g.top + oy;
  const int y0 = min(max(ridx[2 * y], 0), g.h + g.pad - 1), y1 = min(max(ridx[2 * y + 1], 0), g.h + g.pad - 1);
  const int x0 = min(max(cidx[2 * x], 0), g.pw - 1), x1 = min(max(cidx[2 * x + 1], 0), g.pw - 1);
  const float a0 = rlam[2 * y], a1 = rlam[2 * y + 1], b0 = clam[2 * x], b1 = clam[2 * x + 1];
  const uint8_t* view = frames + (b * g.h * g.w + (int64_t)v * g.pw) * 3 + c;
  float A = 0.0f, B = 0.0f, C = 0.0f, D = 0.0f;              // a padded row is 0.0f
  if (y0 >= g.pad) {
    const uint8_t* r = view + (int64_t)(y0 - g.pad) * g.w * 3;
    A = lut[r[x0 * 3]];
    B = lut[r[x1 * 3]];
  }
  if (y1 >= g.pad) {
    const uint8_t* r = view + (int64_t)(y1 - g.pad) * g.w * 3;
    C = lut[r[x0 * 3]];
    D = lut[r[x1 * 3]];
  }
  const float t = __fmaf_rn(b0, A, __fmul_rn(b1, B));
  const float u = __fmaf_rn(b0, C, __fmul_rn(b1, D));
  return __fmaf_rn(a0, t, __fmul_rn(a1, u));
}

// element i of the output [b][3][oh][row] -> its sample, plane, row and column
template <typename T>
__device__ __forceinline__ void dd_pngc_place(T i, const Resize& g, int* ox, int* oy, int* c, int64_t* b) {
  *ox = (int)(i % (T)g.row);
  T r = i / (T)g.row;
  *oy = (int)(r % (T)g.oh);
  r /= (T)g.oh;
  *c = (int)(r % 3);
  *b = (int64_t)(r / 3);
}

// One thread per four consecutive floats of the output taken as one flat array, so that every store but the last is a
// full 16-byte store whatever views * ow is (a run may cross from one output row into the next); the last run of a total
// that is no multiple of four is stored float by float.
__global__ __launch_bounds__(kThreads)
void dd_png_condition_resize_kernel(const uint8_t* __restrict__ frames, float* __restrict__ out, const float* __restrict__ lut,
                                    const int32_t* __restrict__ ridx, const float* __restrict__ rlam,
                                    const int32_t* __restrict__ cidx, const float* __restrict__ clam, int64_t total,
                                    Resize g) {
  const int64_t runs = (total + 3) / 4;
  for (int64_t run = (int64_t)blockIdx.x * kThreads + threadIdx.x; run < runs; run += (int64_t)gridDim.x * kThreads) {
    const int64_t i = run * 4;
    int ox, oy, c;
    int64_t b;
    if (total <= 0x7fffffff) dd_pngc_place<uint32_t>((uint32_t)i, g, &ox, &oy, &c, &b);      // uniform: 32-bit divisions
    else dd_pngc_place<int64_t>(i, g, &ox, &oy, &c, &b);
    const int n = (int)min((int64_t)4, total - i);
    float val[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k < n) {
        val[k] = dd_pngc_sample(frames, lut, ridx, rlam, cidx, clam, g, b, c, oy, ox);
        if (++ox == g.row) {                                 // on to the next row, plane, sample
          ox = 0;
          if (++oy == g.oh) {
            oy = 0;
            if (++c == 3) {
              c = 0;
              ++b;
            }
          }
        }
      }
    }
    if (n == 4) {
      *reinterpret_cast<float4*>(out + i) = make_float4(val[0], val[1], val[2], val[3]);
    } else {
#pragma unroll
      for (int k = 0; k < 3; ++k)
        if (k < n) out[i + k] = val[k];
    }
  }
}

}  // namespace

extern "C" int64_t dd_png_decode_workspace_bytes(int32_t m, int32_t h, int32_t w) {
  if (!sizes_ok(m, h, w)) return -1;
  Geom g;
  Layout l;
  if (!geometry(m, h, w, &g, &l)) return -1;
  return l.total;
}

extern "C" int dd_png_decode_u8(const uint8_t* streams, int64_t streams_bytes, const int32_t* files, const int32_t* tab,
                                int32_t ntab, const int32_t* colour_types, int32_t m, int32_t h, int32_t w, int32_t chunked,
                                uint8_t* out, int32_t* status, int32_t* paths, void* workspace, int64_t workspace_bytes,
                                dd_stream_t stream) {
  if (!streams || !files || !colour_types || !out || !status || !paths || !workspace) return DD_ERR_BAD_ARG;
  if (!sizes_ok(m, h, w) || streams_bytes <= 0 || ntab < 0 || (ntab > 0 && !tab)) return DD_ERR_BAD_ARG;
  if (chunked != 0 && chunked != 1) return DD_ERR_BAD_ARG;
  if (!dd_aligned16(workspace) || (reinterpret_cast<uintptr_t>(files) & 3u) || (reinterpret_cast<uintptr_t>(tab) & 3u) ||
      (reinterpret_cast<uintptr_t>(status) & 3u) || (reinterpret_cast<uintptr_t>(paths) & 3u))
    return DD_ERR_BAD_ARG;
  Geom g;
  Layout l;
  if (!geometry(m, h, w, &g, &l)) return DD_ERR_UNSUPPORTED;
  for (int32_t i = 0; i < m; ++i)
    if (!dd_pd_bpp(colour_types[i])) return DD_ERR_BAD_ARG;  // host memory: what parse_png found
  if (workspace_bytes < l.total) return DD_ERR_BAD_ARG;
  uint8_t* ws = reinterpret_cast<uint8_t*>(workspace);
  uint32_t* flag = reinterpret_cast<uint32_t*>(ws + l.flag);
  uint32_t* trailer = reinterpret_cast<uint32_t*>(ws + l.trailer);
  uint32_t* sums = reinterpret_cast<uint32_t*>(ws + l.sums);
  uint8_t* filt = ws + l.filt;
  const Upload u = {streams, streams_bytes, files, tab, ntab};
  // the chunks of an RGB frame: never more than g.nseg, which counts four bytes per pixel
  const int64_t nchunk = ((int64_t)h * (1 + 3 * (int64_t)w) + kSeg - 1) / kSeg;
  hipStream_t s = dd_stream(stream);
  dd_clear_error();
  if (hipMemsetAsync(flag, 0, (size_t)m * 4, s) != hipSuccess) return DD_ERR_LAUNCH;
  if (chunked && ntab > 0)
    hipLaunchKernelGGL(dd_pngd_chunk_kernel, dim3((unsigned)nchunk, (unsigned)m), dim3(DD_WAVE), 0, s, u, filt, flag, g);
  hipLaunchKernelGGL(dd_pngd_stream_kernel, dim3((unsigned)m), dim3(DD_WAVE), 0, s, u, filt, flag, trailer, status, paths, g,
                     (int)chunked);
  hipLaunchKernelGGL(dd_pngd_adler_kernel, dim3((unsigned)g.nseg, (unsigned)m), dim3(kThreads), 0, s, u, filt, status, sums, g);
  hipLaunchKernelGGL(dd_pngd_unfilter_kernel, dim3((unsigned)m), dim3(kRows), 0, s, u, filt, trailer, sums, out, status, g);
  return dd_check_launch();
}

extern "C" int dd_png_condition(const uint8_t* frames, float* out, const float* lut, int32_t b, int32_t h, int32_t w,
                                int32_t views, int32_t top, int32_t left, int32_t oh, int32_t ow, dd_stream_t stream) {
  if (!frames || !out || !lut) return DD_ERR_BAD_ARG;
  if (b <= 0 || h <= 0 || w <= 0 || views <= 0 || oh <= 0 || ow <= 0 || top < 0 || left < 0) return DD_ERR_BAD_ARG;
  if (w % views != 0 || (int64_t)top + oh > h || (int64_t)left + ow > w / views) return DD_ERR_BAD_ARG;
  if (reinterpret_cast<uintptr_t>(out) & 3u || reinterpret_cast<uintptr_t>(lut) & 3u) return DD_ERR_BAD_ARG;
  const int64_t total = (int64_t)b * 3 * oh * views * ow;
  if ((int64_t)b * h * w * 3 > ((int64_t)1 << 40)) return DD_ERR_UNSUPPORTED;
  const int64_t blocks = (total + kThreads - 1) / kThreads;
  dd_clear_error();
  hipLaunchKernelGGL(dd_png_condition_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(kThreads), 0,
                     dd_stream(stream), frames, out, lut, total, (int)h, (int)w, (int)views, (int)top, (int)left, (int)oh,
                     (int)ow);
  return dd_check_launch();
}

extern "C" int dd_png_condition_resize(const uint8_t* frames, float* out, const float* lut, const int32_t* row_taps,
                                       const float* row_weights, const int32_t* col_taps, const float* col_weights,
                                       int32_t b, int32_t h, int32_t w, int32_t views, int32_t pad_top, int32_t rh,
                                       int32_t rw, int32_t top, int32_t left, int32_t oh, int32_t ow, dd_stream_t stream) {
  if (!frames || !out || !lut || !row_taps || !row_weights || !col_taps || !col_weights) return DD_ERR_BAD_ARG;
  if (b <= 0 || h <= 0 || w <= 0 || views <= 0 || rh <= 0 || rw <= 0 || oh <= 0 || ow <= 0) return DD_ERR_BAD_ARG;
  if (pad_top < 0 || top < 0 || left < 0) return DD_ERR_BAD_ARG;
  if (w % views != 0 || (int64_t)top + oh > rh || (int64_t)left + ow > rw) return DD_ERR_BAD_ARG;
  if (!dd_aligned16(out) || reinterpret_cast<uintptr_t>(lut) & 3u || reinterpret_cast<uintptr_t>(row_taps) & 3u ||
      reinterpret_cast<uintptr_t>(row_weights) & 3u || reinterpret_cast<uintptr_t>(col_taps) & 3u ||
      reinterpret_cast<uintptr_t>(col_weights) & 3u)
    return DD_ERR_BAD_ARG;
  // 32-bit positions inside a frame and inside an output row; 64-bit ones across the batch
  if ((int64_t)h + pad_top > 0x7fffffff || (int64_t)h * w * 3 > 0x7fffffff || (int64_t)views * ow > 0x7fffffff)
    return DD_ERR_UNSUPPORTED;
  if ((int64_t)b * h * w * 3 > ((int64_t)1 << 40) || (int64_t)b * 3 * oh * views * ow > ((int64_t)1 << 40))
    return DD_ERR_UNSUPPORTED;
  const int64_t total = (int64_t)b * 3 * oh * views * ow;
  const int64_t blocks = ((total + 3) / 4 + kThreads - 1) / kThreads;
  const Resize g = {(int)h, (int)w, (int)(w / views), (int)pad_top, (int)top, (int)left, (int)oh, (int)ow, (int)(views * ow)};
  dd_clear_error();
  hipLaunchKernelGGL(dd_png_condition_resize_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(kThreads), 0,
                     dd_stream(stream), frames, out, lut, row_taps, row_weights, col_taps, col_weights, total, g);
  return dd_check_launch();
}
