// Attention-map pictures: the per-token heat-map sheets the reference's analysis script makes of `gather_layer`
// (tools/explore_attn.py:114-151, view_images :25-53).
//
//  * dd_attn_heat: the selected context columns of a (views, h * w, n) map -> one coloured h x w tile per (view, column) as
//    an fp32 NCHW image holding colour / 255.  Per column the min-max normalisation in float64 (:118-122, :138-142) and
//    matplotlib's colour-map index k = min(int(X * 256), 255), NaN -> the "bad" colour (:123-128, :143-148).  The image
//    goes into dd_image_resample_u8, whose quantiser returns the colour byte for colour / 255 (the table holds the
//    quotient, built on the host), so PIL's resize (:129, :149) runs on the bytes the reference colours.
//  * dd_attn_sheet_u8: view_images' canvas (:25-53): tiles in row-major cells with 255 in the gutters and in the cells
//    without a tile, and text_under_image's strip (:13-23) pasted over the bottom rows of a tile.
//
// dd_attn_heat: a workgroup owns 16 columns of one view, as 16 x 16 threads: lanes along the COLUMNS (the key axis, the
// contiguous one of `maps`: a wave reads four rows of 16 consecutive floats), thread rows along the queries.  Pass 1: the
// exact minimum and maximum of each column, on the ORDERED BIT PATTERN of the floats (integer compares: no instruction
// whose result depends on the float mode, so a subnormal is never flushed), through LDS, no atomics.  Pass 2: the same
// rows again (1400 x 16 floats: they sit in L2), X and k per element, the k of 64 rows x 16 columns transposed through
// LDS, then lanes along the PIXELS of a tile: a wave stores 64 consecutive floats of each colour plane.  The double is
// built from the float's bits (dd_f32_bits_to_f64), not by v_cvt_f64_f32, for the same reason as the integer compares;
// the subtraction and the division are IEEE fp64 (this unit is built without any fast-math flag), which is what makes
// the index equal numpy's.
// dd_attn_sheet_u8: one lane per output pixel, lanes along the output row, every byte of `out` written exactly once.
#include "dd_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kCols = 16;                 // columns of a workgroup
constexpr int kRowLanes = kThreads / kCols;
constexpr int kChunk = 64;                // rows per transposed chunk: one wave's pixels
constexpr int kTableRows = 257;           // 256 colours and the NaN colour

// Order-preserving map of float bits to unsigned: a < b as floats (finite or infinite, -0 below +0) <=> key(a) < key(b).
__device__ __forceinline__ uint32_t dd_f32_key(uint32_t bits) { return (bits & 0x80000000u) ? ~bits : bits | 0x80000000u; }
__device__ __forceinline__ uint32_t dd_f32_unkey(uint32_t key) { return (key & 0x80000000u) ? key & 0x7fffffffu : ~key; }

// The double with the value of the float whose bits are `b`, exactly, by integer arithmetic: subnormals are normalised,
// zeros keep their sign, infinities and NaNs stay what they are.
__device__ __forceinline__ double dd_f32_bits_to_f64(uint32_t b) {
  const uint64_t sign = (uint64_t)(b >> 31) << 63;
  const uint32_t e = (b >> 23) & 0xffu;
  const uint32_t m = b & 0x7fffffu;
  uint64_t d;
  if (e == 0xffu) {
    d = sign | 0x7ff0000000000000ull | ((uint64_t)m << 29);
  } else if (e != 0u) {
    d = sign | ((uint64_t)(e + (1023u - 127u)) << 52) | ((uint64_t)m << 29);
  } else if (m == 0u) {
    d = sign;
  } else {
    const int p = 31 - __clz((int)m);                               // m * 2^-149 = 1.f * 2^(p - 149), p in [0, 22]
    d = sign | ((uint64_t)(p - 149 + 1023) << 52) | (((uint64_t)m << (52 - p)) & 0x000fffffffffffffull);
  }
  return __longlong_as_double((long long)d);
}

__global__ __launch_bounds__(kThreads)
void dd_attn_heat_kernel(const float* __restrict__ maps, const int32_t* __restrict__ cols,
                         const float* __restrict__ table, float* __restrict__ img, int32_t q, int32_t n, int32_t t,
                         int64_t ldm, int64_t vs) {
  __shared__ uint32_t red_lo[kRowLanes][kCols];
  __shared__ uint32_t red_hi[kRowLanes][kCols];
  __shared__ uint16_t kk[kCols][kChunk + 2];
  __shared__ float tab[kTableRows * 3];

  const int tid = threadIdx.x;
  const int cl = tid & (kCols - 1);
  const int rl = tid / kCols;
  const int view = blockIdx.y;
  const int c0 = blockIdx.x * kCols;
  const int ci = c0 + cl;                                           // which of the t selected columns
  const bool cok = ci < t;
  const int col = cok ? min(max(cols[ci], 0), n - 1) : 0;           // the contract is [0, n): nothing else is ever read
  const uint32_t* src = reinterpret_cast<const uint32_t*>(maps) + (int64_t)view * vs + col;

  for (int i = tid; i < kTableRows * 3; i += kThreads) tab[i] = table[(i / 3) * 4 + i % 3];

  uint32_t lo = 0xffffffffu, hi = 0u;
  if (cok) {
#pragma unroll 8                                                    // independent loads in flight: the pass is latency-bound
    for (int r = rl; r < q; r += kRowLanes) {
      const uint32_t key = dd_f32_key(src[(int64_t)r * ldm]);
      lo = min(lo, key);
      hi = max(hi, key);
    }
  }
  red_lo[rl][cl] = lo;
  red_hi[rl][cl] = hi;
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kRowLanes; ++j) {
    lo = min(lo, red_lo[j][cl]);
    hi = max(hi, red_hi[j][cl]);
  }
  const double dmin = dd_f32_bits_to_f64(dd_f32_unkey(lo));
  const double den = dd_f32_bits_to_f64(dd_f32_unkey(hi)) - dmin;

  const int wave = tid / DD_WAVE, lane = tid & (DD_WAVE - 1);
  for (int r0 = 0; r0 < q; r0 += kChunk) {
    if (cok) {
#pragma unroll
      for (int j = 0; j < kChunk / kRowLanes; ++j) {
        const int rr = rl + j * kRowLanes;
        const int r = r0 + rr;
        if (r < q) {
          const double x = (dd_f32_bits_to_f64(src[(int64_t)r * ldm]) - dmin) / den;
          const double y = x * 256.0;
          int k = 256;                                              // NaN: the "bad" colour
          if (y == y) k = (int)fmin(fmax(y, 0.0), 255.0);           // a non-finite input is clamped, never an index outside
          kk[cl][rr] = (uint16_t)k;
        }
      }
    }
    __syncthreads();
    const int r = r0 + lane;
    if (r < q) {
      for (int c = wave; c < kCols && c0 + c < t; c += kThreads / DD_WAVE) {
        const int k = kk[c][lane];
        float* o = img + ((int64_t)view * t + c0 + c) * 3 * q + r;
        o[0] = tab[3 * k];
        o[q] = tab[3 * k + 1];
        o[2 * (int64_t)q] = tab[3 * k + 2];
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kThreads)
void dd_attn_sheet_kernel(const uint8_t* __restrict__ tiles, const int32_t* __restrict__ index,
                          const uint8_t* __restrict__ labels, uint8_t* __restrict__ out, int32_t m, int32_t cells,
                          int32_t cols, int32_t th, int32_t tw, int32_t lh, int32_t gap, int32_t oh, int32_t ow) {
  const int64_t s = blockIdx.y;
  const int64_t px = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (px >= (int64_t)oh * ow) return;
  const int r = (int)(px / ow), c = (int)(px % ow);
  const int cr = r / (th + gap), y = r % (th + gap);
  const int cc = c / (tw + gap), x = c % (tw + gap);
  uint32_t b0 = 255u, b1 = 255u, b2 = 255u;
  if (y < th && x < tw) {                                           // else a gutter
    const int i = index[s * cells + cr * cols + cc];
    if (i >= 0 && i < m) {                                          // -1 (or anything that is no tile): an all-255 cell
      const uint8_t* p = y < th - lh ? tiles + (((int64_t)i * th + y) * tw + x) * 3
                                     : labels + (((int64_t)i * lh + (y - (th - lh))) * tw + x) * 3;
      b0 = p[0]; b1 = p[1]; b2 = p[2];
    }
  }
  uint8_t* o = out + (s * oh * ow + px) * 3;
  o[0] = (uint8_t)b0;
  o[1] = (uint8_t)b1;
  o[2] = (uint8_t)b2;
}

inline bool mis4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) != 0; }

}  // namespace

extern "C" int dd_attn_heat(const float* maps, const int32_t* cols, const float* table, float* img, int32_t views,
                            int32_t h, int32_t w, int32_t n, int32_t t, int64_t ldm, int64_t view_stride,
                            dd_stream_t stream) {
  if (!maps || !cols || !table || !img) return DD_ERR_BAD_ARG;
  if (views <= 0 || h <= 0 || w <= 0 || n <= 0 || t <= 0) return DD_ERR_BAD_ARG;
  if (ldm < n || view_stride < 0) return DD_ERR_BAD_ARG;
  if (mis4(maps) || mis4(cols) || mis4(table) || mis4(img)) return DD_ERR_BAD_ARG;
  if ((int64_t)views * t > 65535 || (int64_t)h * w >= ((int64_t)1 << 31)) return DD_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)((t + kCols - 1) / kCols), (unsigned)views);
  dd_clear_error();
  hipLaunchKernelGGL(dd_attn_heat_kernel, grid, dim3(kThreads), 0, dd_stream(stream), maps, cols, table, img, h * w, n, t,
                     ldm, view_stride);
  return dd_check_launch();
}

extern "C" int dd_attn_sheet_u8(const uint8_t* tiles, const int32_t* index, const uint8_t* labels, uint8_t* out, int32_t m,
                                int32_t sheets, int32_t rows, int32_t cols, int32_t th, int32_t tw, int32_t lh,
                                int32_t gap, dd_stream_t stream) {
  if (!tiles || !index || !out) return DD_ERR_BAD_ARG;
  if (m <= 0 || sheets <= 0 || rows <= 0 || cols <= 0 || th <= 0 || tw <= 0 || lh < 0 || gap < 0) return DD_ERR_BAD_ARG;
  if ((labels != nullptr) != (lh > 0) || lh > th) return DD_ERR_BAD_ARG;
  if (mis4(index)) return DD_ERR_BAD_ARG;
  const int64_t oh = (int64_t)rows * th + (int64_t)gap * (rows - 1), ow = (int64_t)cols * tw + (int64_t)gap * (cols - 1);
  const int64_t lim = (int64_t)1 << 31;                             // 32-bit pixel and cell indices, th + gap included
  if (sheets > 65535 || (int64_t)rows * cols >= lim || oh >= lim || ow >= lim || oh * ow >= lim ||
      (int64_t)th + gap >= lim || (int64_t)tw + gap >= lim)
    return DD_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)((oh * ow + kThreads - 1) / kThreads), (unsigned)sheets);
  dd_clear_error();
  hipLaunchKernelGGL(dd_attn_sheet_kernel, grid, dim3(kThreads), 0, dd_stream(stream), tiles, index, labels, out, m,
                     rows * cols, cols, th, tw, lh, gap, (int32_t)oh, (int32_t)ow);
  return dd_check_launch();
}
