// InceptionV3 feature extractor of the FID evaluation (the reference's tools/fid_score.py -> magicdrive/misc/inception.py,
// pytorch-fid's network): general implicit-GEMM convolution with the eval-mode BatchNorm + ReLU epilogue, the three 3 x 3
// pools, the global average and the input resize — everything that network needs beyond what dd_gemm's 3 x 3 / pad 1
// conv mode expresses (1 x 7, 7 x 1, 5 x 5, 1 x 3, 3 x 1, unpadded stride 2).
//
// dd_conv2d_kernel<T, BM, BN>: a workgroup of four waves owns BM output pixels x BN output channels.  K = kh kw cin is
// walked in steps of 32 (one MFMA 16x16x32); a step's operands are staged as 16-byte chunks of 8 channels — cin % 8 == 0
// keeps a chunk inside one tap, so a chunk is one bounds-checked gather (taps outside the image, rows past the last
// pixel, channels past cout and k >= K all read zero: K = 720 and 1200 end in a partly-zero step).  The gather of step
// t + 1 is issued to registers before the MFMAs of step t and lands in the other half of a double-buffered LDS image,
// one barrier per step.  An LDS row is the 64 bytes of one pixel's (or output channel's) K-step; its four chunks are
// permuted by the row's quad index ((4 - (row >> 2)) & 3, XOR) so that the sixteen lanes ds_read_b128 serves per cycle
// ({0-3, 12-15, 20-27}, ...) hit sixteen distinct 16-byte bank groups.
// The weights are the MFMA's A operand and the pixels its B operand, so a lane ends with four consecutive output
// channels of one pixel: the epilogue out = relu(acc * scale[n] + shift[n]) (fp32, BatchNorm never folded into the 16-bit
// weights) is stored as one 8-byte vector at out[pixel * ldc + c_off + n] — a branch of an Inception block writes its
// slice of the concatenated tensor directly.
#include "dd_common.h"

namespace {

struct dd_conv2d_args {
  const void* x; const void* w; const float* scale; const float* shift; void* out;
  int64_t ldc, rows;
  int32_t c_off, h, w_, cin, cout, kh, kw, stride, pad_h, pad_w, hout, wout, K, relu;
};

__device__ __forceinline__ int dd_c2_lds_off(int row, int kc) {
  return row * 64 + ((kc ^ ((4 - (row >> 2)) & 3)) << 4);
}

template <typename T, int BM, int BN>
__global__ __launch_bounds__(256)
void dd_conv2d_kernel(const dd_conv2d_args a) {
  using V8 = typename dd_vec<T>::v8;
  using V4 = typename dd_vec<T>::v4;
  constexpr int RA = BM / 64, RB = BN / 64;          // rows of the pixel / weight image one thread stages per K-step
  constexpr int WM = BM / 2, WN = BN / 2;            // a wave's share: 2 x 2 waves
  constexpr int FM = WM / 16, FN = WN / 16;
  constexpr int BUF = (BM + BN) * 64;
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * BUF];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave & 1, wn = wave >> 1;
  const int64_t row0 = (int64_t)blockIdx.x * BM;
  const int n0 = blockIdx.y * BN;
  const T* x = reinterpret_cast<const T*>(a.x);
  const T* wt = reinterpret_cast<const T*>(a.w);
  const int K = a.K, cin = a.cin, kw = a.kw, h = a.h, w = a.w_;

  // ---- staging role: row srow (+ 64 i) of either image, chunk skc of the K-step ----------------------------------------
  const int srow = tid >> 2, skc = tid & 3;
  const T* xb[RA];
  int iy0[RA], ix0[RA];
  bool rok[RA];
#pragma unroll
  for (int i = 0; i < RA; ++i) {
    const int64_t r = row0 + srow + 64 * i;
    rok[i] = r < a.rows;
    const int64_t rr = rok[i] ? r : 0;
    const int hw = a.hout * a.wout;
    const int img = (int)(rr / hw);
    const int rem = (int)(rr - (int64_t)img * hw);
    const int oy = rem / a.wout, ox = rem - oy * a.wout;
    iy0[i] = oy * a.stride - a.pad_h;
    ix0[i] = ox * a.stride - a.pad_w;
    xb[i] = x + (int64_t)img * h * w * cin;
  }
  int k = skc * 8;                                   // this thread's position in K: (ky, kx, ci)
  int tap = k / cin;
  int ci = k - tap * cin;
  int ky = tap / kw, kx = tap - ky * kw;

  u32x4 ra[RA], rb[RB];
  auto gload = [&]() __attribute__((always_inline)) {
    const bool kin = k < K;
#pragma unroll
    for (int i = 0; i < RA; ++i) {
      u32x4 v = {0u, 0u, 0u, 0u};
      const int iy = iy0[i] + ky, ix = ix0[i] + kx;
      if (kin && rok[i] && (unsigned)iy < (unsigned)h && (unsigned)ix < (unsigned)w)
        v = dd_ld16(xb[i] + ((int64_t)iy * w + ix) * cin + ci);
      ra[i] = v;
    }
#pragma unroll
    for (int j = 0; j < RB; ++j) {
      u32x4 v = {0u, 0u, 0u, 0u};
      const int n = n0 + srow + 64 * j;
      if (kin && n < a.cout) v = dd_ld16(wt + (int64_t)n * K + k);
      rb[j] = v;
    }
  };
  auto advance = [&]() __attribute__((always_inline)) {
    k += 32;
    ci += 32;
    while (ci >= cin) {                              // at most 4 rounds (cin >= 8), one when cin >= 32
      ci -= cin;
      if (++kx == kw) { kx = 0; ++ky; }
    }
  };
  auto lstore = [&](unsigned char* buf) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < RA; ++i) dd_st16(buf + dd_c2_lds_off(srow + 64 * i, skc), ra[i]);
#pragma unroll
    for (int j = 0; j < RB; ++j) dd_st16(buf + BM * 64 + dd_c2_lds_off(srow + 64 * j, skc), rb[j]);
  };

  f32x4 acc[FN][FM];
#pragma unroll
  for (int j = 0; j < FN; ++j)
#pragma unroll
    for (int i = 0; i < FM; ++i) acc[j][i] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int fr = lane & 15, fk = lane >> 4;          // fragment role: row fr of a 16-row block, chunk fk
  const int nk = (K + 31) >> 5;
  gload();
  lstore(lds);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    unsigned char* cur = lds + (kt & 1) * BUF;
    const bool more = kt + 1 < nk;                   // uniform
    if (more) {
      advance();
      gload();
    }
    V8 wf[FN], xf[FM];
#pragma unroll
    for (int j = 0; j < FN; ++j) wf[j] = dd_as_v8<T>(dd_ld16(cur + BM * 64 + dd_c2_lds_off(wn * WN + j * 16 + fr, fk)));
#pragma unroll
    for (int i = 0; i < FM; ++i) xf[i] = dd_as_v8<T>(dd_ld16(cur + dd_c2_lds_off(wm * WM + i * 16 + fr, fk)));
#pragma unroll
    for (int j = 0; j < FN; ++j)
#pragma unroll
      for (int i = 0; i < FM; ++i) acc[j][i] = dd_mfma16(wf[j], xf[i], acc[j][i]);
    if (more) lstore(lds + ((kt + 1) & 1) * BUF);
    __syncthreads();
  }

  // ---- epilogue: lane = pixel fr of block i, channels 4 fk .. 4 fk + 3 of block j ----------------------------------------
  T* out = reinterpret_cast<T*>(a.out);
#pragma unroll
  for (int j = 0; j < FN; ++j) {
    const int n = n0 + wn * WN + j * 16 + fk * 4;
    if (n >= a.cout) continue;                       // cout % 4 == 0: a lane's four channels are all in or all out
    float sc[4], sh[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      sc[r] = a.scale[n + r];
      sh[r] = a.shift[n + r];
    }
#pragma unroll
    for (int i = 0; i < FM; ++i) {
      const int64_t p = row0 + wm * WM + i * 16 + fr;
      if (p >= a.rows) continue;
      V4 o;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float v = fmaf(acc[j][i][r], sc[r], sh[r]);
        if (a.relu) v = fmaxf(v, 0.f);
        o[r] = (T)v;
      }
      *reinterpret_cast<V4*>(out + p * a.ldc + a.c_off + n) = o;
    }
  }
}

// tile ids of dd_conv2d_nhwc's `tile`: 0 = by shape
enum { C2_AUTO = 0, C2_64x64 = 1, C2_128x64 = 2 };

int conv2d_pick_tile(int64_t rows, int32_t cout, int32_t tile) {
  if (tile != C2_AUTO) return tile;
  // the 128-row tile halves the weight re-reads and LDS traffic per MFMA; it is taken while it still gives every CU two
  // workgroups (256 CUs), the 64-row tile otherwise
  const int64_t wgs = ((rows + 127) / 128) * ((cout + 63) / 64);
  return wgs >= 512 ? C2_128x64 : C2_64x64;
}

// ---- 3 x 3 pools --------------------------------------------------------------------------------------------------------
// One thread per output pixel and 8-channel vector.  mode 0: max, stride 2, pad 0; 1: max, stride 1, pad 1 (only in-image
// taps take part: padding never wins); 2: average, stride 1, pad 1, divided by the number of in-image taps.
template <typename T>
__global__ __launch_bounds__(256)
void dd_pool3x3_kernel(const T* __restrict__ x, T* __restrict__ out, int64_t total, int32_t h, int32_t w, int32_t c8,
                       int32_t hout, int32_t wout, int32_t mode, int64_t ldc, int32_t c_off) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const int cv = (int)(t % c8);
  const int64_t p = t / c8;
  const int ox = (int)(p % wout);
  const int64_t q = p / wout;
  const int oy = (int)(q % hout);
  const int64_t img = q / hout;
  const int stride = mode == 0 ? 2 : 1, pad = mode == 0 ? 0 : 1;
  const T* xin = x + img * h * w * (int64_t)(c8 * 8) + cv * 8;
  float r[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) r[e] = mode == 2 ? 0.f : -INFINITY;
  int cnt = 0;
  for (int dy = 0; dy < 3; ++dy) {
    const int iy = oy * stride - pad + dy;
    if ((unsigned)iy >= (unsigned)h) continue;
    for (int dx = 0; dx < 3; ++dx) {
      const int ix = ox * stride - pad + dx;
      if ((unsigned)ix >= (unsigned)w) continue;
      float v[8];
      dd_unpack8<T>(dd_ld16(xin + ((int64_t)iy * w + ix) * (c8 * 8)), v);
#pragma unroll
      for (int e = 0; e < 8; ++e) r[e] = mode == 2 ? r[e] + v[e] : fmaxf(r[e], v[e]);
      ++cnt;
    }
  }
  if (mode == 2) {
    const float n = (float)cnt;
#pragma unroll
    for (int e = 0; e < 8; ++e) r[e] = r[e] / n;
  }
  dd_st16(out + p * ldc + c_off + cv * 8, dd_pack8<T>(r));
}

// ---- global average: [m][hw][c] -> fp32 [m][c], one thread per (image, channel), summed in pixel order ------------------
template <typename T>
__global__ __launch_bounds__(256)
void dd_global_avgpool_kernel(const T* __restrict__ x, float* __restrict__ out, int64_t total, int32_t hw, int32_t c) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const int64_t img = t / c;
  const int ch = (int)(t - img * c);
  const T* p = x + img * hw * (int64_t)c + ch;
  float s = 0.f;
  for (int i = 0; i < hw; ++i) s += (float)p[(int64_t)i * c];
  out[t] = s / (float)hw;
}

// ---- network input: F.interpolate(bilinear, align_corners=False) and 2 x - 1, NCHW [0, 1] -> channel-padded NHWC --------
// torch's own arithmetic (aten UpSampleBilinear2d: area_pixel_compute_source_index and the two-level lerp) in fp32.
template <typename TI, typename T>
__global__ __launch_bounds__(256)
void dd_inception_input_kernel(const TI* __restrict__ x, T* __restrict__ out, int64_t total, int32_t h, int32_t w,
                               int32_t oh, int32_t ow, int32_t c_pad, int32_t resize, int32_t normalize) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const int ox = (int)(t % ow);
  const int64_t q = t / ow;
  const int oy = (int)(q % oh);
  const int64_t img = q / oh;
  const TI* xin = x + img * 3 * (int64_t)h * w;
  float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (resize) {
    const float sy = (float)h / (float)oh, sx = (float)w / (float)ow;
    const float fy = fmaxf(sy * ((float)oy + 0.5f) - 0.5f, 0.f), fx = fmaxf(sx * ((float)ox + 0.5f) - 0.5f, 0.f);
    const int y0 = min((int)fy, h - 1), x0 = min((int)fx, w - 1);
    const int y1 = y0 + (y0 < h - 1 ? 1 : 0), x1 = x0 + (x0 < w - 1 ? 1 : 0);
    const float ly1 = fy - (float)y0, lx1 = fx - (float)x0;
    const float ly0 = 1.f - ly1, lx0 = 1.f - lx1;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const TI* pc = xin + (int64_t)ch * h * w;
      const float v00 = (float)pc[(int64_t)y0 * w + x0], v01 = (float)pc[(int64_t)y0 * w + x1];
      const float v10 = (float)pc[(int64_t)y1 * w + x0], v11 = (float)pc[(int64_t)y1 * w + x1];
      v[ch] = ly0 * (lx0 * v00 + lx1 * v01) + ly1 * (lx0 * v10 + lx1 * v11);
    }
  } else {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) v[ch] = (float)xin[((int64_t)ch * h + oy) * w + ox];
  }
  if (normalize) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) v[ch] = 2.f * v[ch] - 1.f;
  }
  T* o = out + t * c_pad;
  dd_st16(o, dd_pack8<T>(v));
  const u32x4 z = {0u, 0u, 0u, 0u};
  for (int cv = 1; cv < c_pad / 8; ++cv) dd_st16(o + cv * 8, z);
}

}  // namespace

extern "C" int dd_conv2d_nhwc(const void* x, const void* w, const float* scale, const float* shift, void* out,
                              int64_t ldc, int32_t c_off, int32_t m, int32_t h, int32_t wd, int32_t cin, int32_t cout,
                              int32_t kh, int32_t kw, int32_t stride, int32_t pad_h, int32_t pad_w, int32_t relu,
                              int32_t tile, int32_t dtype, dd_stream_t stream) {
  if (!x || !w || !scale || !shift || !out || m <= 0 || h <= 0 || wd <= 0 || cin <= 0 || cout <= 0) return DD_ERR_BAD_ARG;
  if (dtype != DD_F16 && dtype != DD_BF16) return DD_ERR_BAD_ARG;
  if (kh < 1 || kh > 7 || kw < 1 || kw > 7 || (stride != 1 && stride != 2)) return DD_ERR_UNSUPPORTED;
  if (pad_h < 0 || pad_h > kh / 2 || pad_w < 0 || pad_w > kw / 2) return DD_ERR_UNSUPPORTED;
  if (cin % 8 != 0 || cout % 4 != 0) return DD_ERR_UNSUPPORTED;
  if (tile != C2_AUTO && tile != C2_64x64 && tile != C2_128x64) return DD_ERR_UNSUPPORTED;
  if (c_off < 0 || c_off % 4 != 0 || ldc % 4 != 0 || ldc < (int64_t)c_off + cout) return DD_ERR_BAD_ARG;
  if (!dd_aligned16(x) || !dd_aligned16(w) || (reinterpret_cast<uintptr_t>(out) & 7u)) return DD_ERR_BAD_ARG;
  if (h + 2 * pad_h < kh || wd + 2 * pad_w < kw) return DD_ERR_BAD_ARG;       // no output pixel
  const int32_t hout = (h + 2 * pad_h - kh) / stride + 1, wout = (wd + 2 * pad_w - kw) / stride + 1;
  const int64_t rows = (int64_t)m * hout * wout;
  if (rows >= ((int64_t)1 << 31) || (int64_t)h * wd >= ((int64_t)1 << 31) || (int64_t)hout * wout >= ((int64_t)1 << 31))
    return DD_ERR_UNSUPPORTED;
  dd_conv2d_args a;
  a.x = x; a.w = w; a.scale = scale; a.shift = shift; a.out = out;
  a.ldc = ldc; a.rows = rows; a.c_off = c_off; a.h = h; a.w_ = wd; a.cin = cin; a.cout = cout; a.kh = kh; a.kw = kw;
  a.stride = stride; a.pad_h = pad_h; a.pad_w = pad_w; a.hout = hout; a.wout = wout; a.K = kh * kw * cin;
  a.relu = relu ? 1 : 0;
  const int t = conv2d_pick_tile(rows, cout, tile);
  const int bm = t == C2_128x64 ? 128 : 64;
  const dim3 grid((unsigned)((rows + bm - 1) / bm), (unsigned)((cout + 63) / 64));
  dd_clear_error();
  return dd_dispatch16(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    if (t == C2_128x64)
      hipLaunchKernelGGL((dd_conv2d_kernel<T, 128, 64>), grid, dim3(256), 0, dd_stream(stream), a);
    else
      hipLaunchKernelGGL((dd_conv2d_kernel<T, 64, 64>), grid, dim3(256), 0, dd_stream(stream), a);
    return dd_check_launch();
  });
}

extern "C" const char* dd_conv2d_kernel_name(int64_t rows, int32_t cout, int32_t tile, int32_t dtype) {
  if (rows <= 0 || cout <= 0 || (dtype != DD_F16 && dtype != DD_BF16)) return "";
  if (tile != C2_AUTO && tile != C2_64x64 && tile != C2_128x64) return "";
  const bool big = conv2d_pick_tile(rows, cout, tile) == C2_128x64;
  if (dtype == DD_F16) return big ? "dd_conv2d_kernel<_Float16, 128, 64>" : "dd_conv2d_kernel<_Float16, 64, 64>";
  return big ? "dd_conv2d_kernel<__bf16, 128, 64>" : "dd_conv2d_kernel<__bf16, 64, 64>";
}

extern "C" int dd_pool3x3_nhwc(const void* x, void* out, int64_t ldc, int32_t c_off, int32_t m, int32_t h, int32_t wd,
                               int32_t c, int32_t mode, int32_t dtype, dd_stream_t stream) {
  if (!x || !out || m <= 0 || h <= 0 || wd <= 0 || c <= 0) return DD_ERR_BAD_ARG;
  if (dtype != DD_F16 && dtype != DD_BF16) return DD_ERR_BAD_ARG;
  if (mode < 0 || mode > 2 || c % 8 != 0) return DD_ERR_UNSUPPORTED;
  if (c_off < 0 || c_off % 8 != 0 || ldc % 8 != 0 || ldc < (int64_t)c_off + c) return DD_ERR_BAD_ARG;
  if (!dd_aligned16(x) || !dd_aligned16(out)) return DD_ERR_BAD_ARG;
  if (mode == 0 && (h < 3 || wd < 3)) return DD_ERR_BAD_ARG;                  // no output pixel
  const int32_t hout = mode == 0 ? (h - 3) / 2 + 1 : h, wout = mode == 0 ? (wd - 3) / 2 + 1 : wd;
  const int64_t total = (int64_t)m * hout * wout * (c / 8);
  if ((total + 255) / 256 >= ((int64_t)1 << 31)) return DD_ERR_UNSUPPORTED;
  dd_clear_error();
  return dd_dispatch16(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL((dd_pool3x3_kernel<T>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, dd_stream(stream),
                       (const T*)x, (T*)out, total, h, wd, c / 8, hout, wout, mode, ldc, c_off);
    return dd_check_launch();
  });
}

extern "C" int dd_global_avgpool_nhwc(const void* x, float* out, int32_t m, int32_t hw, int32_t c, int32_t dtype,
                                      dd_stream_t stream) {
  if (!x || !out || m <= 0 || hw <= 0 || c <= 0) return DD_ERR_BAD_ARG;
  if (dtype != DD_F16 && dtype != DD_BF16) return DD_ERR_BAD_ARG;
  const int64_t total = (int64_t)m * c;
  if ((total + 255) / 256 >= ((int64_t)1 << 31)) return DD_ERR_UNSUPPORTED;
  dd_clear_error();
  return dd_dispatch16(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL((dd_global_avgpool_kernel<T>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                       dd_stream(stream), (const T*)x, out, total, hw, c);
    return dd_check_launch();
  });
}

extern "C" int dd_inception_input(const void* x, void* out, int32_t m, int32_t h, int32_t wd, int32_t oh, int32_t ow,
                                  int32_t c_pad, int32_t resize, int32_t normalize, int32_t in_dtype, int32_t dtype,
                                  dd_stream_t stream) {
  if (!x || !out || m <= 0 || h <= 0 || wd <= 0 || oh <= 0 || ow <= 0) return DD_ERR_BAD_ARG;
  if (dtype != DD_F16 && dtype != DD_BF16) return DD_ERR_BAD_ARG;
  if (in_dtype != DD_F16 && in_dtype != DD_BF16 && in_dtype != DD_F32) return DD_ERR_BAD_ARG;
  if (c_pad < 8 || c_pad % 8 != 0) return DD_ERR_UNSUPPORTED;
  if (!resize && (oh != h || ow != wd)) return DD_ERR_BAD_ARG;
  if (!dd_aligned16(out)) return DD_ERR_BAD_ARG;
  const int64_t total = (int64_t)m * oh * ow;
  if ((total + 255) / 256 >= ((int64_t)1 << 31) || (int64_t)h * wd >= ((int64_t)1 << 31)) return DD_ERR_UNSUPPORTED;
  dd_clear_error();
  return dd_dispatch32(in_dtype, [&](auto ti) {
    using TI = typename decltype(ti)::type;
    return dd_dispatch16(dtype, [&](auto tag) {
      using T = typename decltype(tag)::type;
      hipLaunchKernelGGL((dd_inception_input_kernel<TI, T>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                         dd_stream(stream), (const TI*)x, (T*)out, total, h, wd, oh, ow, c_pad, resize ? 1 : 0,
                         normalize ? 1 : 0);
      return dd_check_launch();
    });
  });
}
