// Image output: the decoded views as the uint8 frames the reference saves.
//
//  * dd_image_quantize_u8: diffusers' numpy_to_pil arithmetic, (images * 255).round().astype("uint8"), NCHW -> NHWC bytes
//    (pipeline/pipeline_bev_controlnet.py:112,540; numpy_to_pil_double :72-80).
//  * dd_image_resample_u8: the same quantisation on load, then PIL's Image.resize(BICUBIC) on 8-bit pixels and
//    torchvision's Pad (perception/data_prepare/val_set_gen.py:147-159), one launch, byte for byte.
// Image input, further down: dd_image_load_u8, uint8 camera frames to the normalised pixel values the VAE encoder takes.
//
// PIL resamples 8-bit images in integer arithmetic: per output coordinate a row of 22-bit fixed-point coefficients and
// the window {xmin, count} it applies to; a horizontal pass over every input row, rounded and clipped to a byte, then a
// vertical pass over that.  The tables come from the caller (include/dualdiff_hip.h says how PIL builds them), so the
// kernel holds no floating point beyond the quantisation.
//
// A workgroup owns a tile of the PADDED output, tw x th pixels.  It stages the coefficient rows of its tile and the
// quantised input window of its footprint in LDS, runs the horizontal pass for the input rows of its vertical footprint
// (by[first row].xmin .. by[last row].xmin + count) into LDS as bytes, runs the vertical pass out of LDS four bytes of
// an output row per lane (one ds_read_b32 per tap), and leaves the finished tile — pad pixels included — in LDS.  The
// store phase then walks the 4-byte ALIGNED dwords of every row segment in global memory: a dword that lies inside the
// segment is funnel-shifted out of two LDS dwords and stored whole (64 lanes = 256 contiguous bytes), the up to three
// head and tail bytes of a segment go out as bytes.  A row is 3 * width bytes, so segments start at any alignment
// (1466 * 3 = 4398); no lane writes a byte outside its own segment, and neighbouring tiles never share a dword store.
#include "dd_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kPB = 22;                      // PIL's PRECISION_BITS for 8-bit pixels: 32 - 8 - 2

template <typename T>
__device__ __forceinline__ uint32_t dd_quant_u8(T x, int m11) {
  float v = (float)x;
  if (m11) v = v * 0.5f + 0.5f;              // v / 2 is exact, so the sum rounds once, fused or not
  v = fminf(fmaxf(v, 0.0f), 1.0f);
  return (uint32_t)(int)rintf(v * 255.0f);   // round to nearest even, as numpy's round
}

__device__ __forceinline__ uint32_t dd_clip8(int32_t acc) {
  return (uint32_t)min(max(acc >> kPB, 0), 255);
}

__device__ __forceinline__ int dd_clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

template <typename T>
__global__ __launch_bounds__(kThreads)
void dd_image_quantize_kernel(const T* __restrict__ x, uint8_t* __restrict__ out, int32_t hw, int32_t m11) {
  const int64_t img = blockIdx.y;
  const T* p = x + img * 3 * hw;
  uint8_t* g = out + img * 3 * hw;
  const int64_t i4 = ((int64_t)blockIdx.x * kThreads + threadIdx.x) * 4;       // first of this lane's 4 pixels
  if (i4 >= hw) return;
  const int n = (int)min((int64_t)4, hw - i4);
  uint32_t b[12];
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int c = 0; c < 3; ++c) b[k * 3 + c] = k < n ? dd_quant_u8<T>(p[(int64_t)c * hw + i4 + k], m11) : 0u;
  uint8_t* dst = g + i4 * 3;
  if (n == 4 && (reinterpret_cast<uintptr_t>(g) & 3u) == 0) {                  // 12 bytes at a multiple of 12 from g
    uint32_t* d32 = reinterpret_cast<uint32_t*>(dst);
#pragma unroll
    for (int j = 0; j < 3; ++j) d32[j] = b[4 * j] | (b[4 * j + 1] << 8) | (b[4 * j + 2] << 16) | (b[4 * j + 3] << 24);
  } else {
#pragma unroll
    for (int j = 0; j < 12; ++j)
      if (j < 3 * n) dst[j] = (uint8_t)b[j];
  }
}

struct ResampleArgs {
  const void* x;
  uint8_t* out;
  const int32_t *kx, *bx, *ky, *by;
  int32_t h, w, oh, ow, ksx, ksy, pad_l, pad_t;
  int32_t ht, wt;                            // padded output size
  int32_t tw, th;                            // tile of the padded output, pixels; tw % 4 == 0
  int32_t capw, caph;                        // input columns / rows the LDS slice holds
  int32_t qp;                                // pitch of the quantised input window, bytes (multiple of 4)
  int32_t fill, m11;
};

// LDS image of a workgroup, in this order (every part a multiple of 4 bytes):
//   int32 lkx[tw * ksx], lbx[tw * 2], lky[th * ksy], lby[th * 2]   coefficient rows and {first, count} RELATIVE to the slice
//   uint8 o[th][tw * 3 + 4] (+ 4)                                   the finished tile
//   uint8 t[caph][tw * 3]                                           horizontal pass, tile byte columns
//   uint8 q[caph][qp]                                               quantised input window, pixel-interleaved
static inline size_t resample_lds_bytes(int tw, int th, int ksx, int ksy, int capw, int caph, int* qp) {
  *qp = (capw * 3 + 3) & ~3;
  return (size_t)4 * (tw * ksx + tw * 2 + th * ksy + th * 2) + (size_t)th * (tw * 3 + 4) + 4 + (size_t)caph * tw * 3 +
         (size_t)caph * *qp;
}

template <typename T>
__global__ __launch_bounds__(kThreads)
void dd_image_resample_kernel(const ResampleArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t dd_img_lds[];
  const int tid = threadIdx.x;
  const int tw = a.tw, th = a.th, ksx = a.ksx, ksy = a.ksy;
  const int X0 = blockIdx.x * tw, Y0 = blockIdx.y * th;
  const int64_t img = blockIdx.z;
  // the image columns / rows (of the resized, unpadded image) this tile holds
  const int ox0 = max(X0 - a.pad_l, 0), ox1 = min(X0 + tw - a.pad_l, a.ow);
  const int oy0 = max(Y0 - a.pad_t, 0), oy1 = min(Y0 + th - a.pad_t, a.oh);
  const int ncol = max(ox1 - ox0, 0), nrow = max(oy1 - oy0, 0);
  const bool has = ncol > 0 && nrow > 0;

  int32_t* lkx = reinterpret_cast<int32_t*>(dd_img_lds);
  int32_t* lbx = lkx + tw * ksx;
  int32_t* lky = lbx + tw * 2;
  int32_t* lby = lky + th * ksy;
  const int op = tw * 3 + 4, tp = tw * 3, qp = a.qp;
  uint8_t* o = reinterpret_cast<uint8_t*>(lby + th * 2);
  uint8_t* t = o + th * op + 4;
  uint8_t* q = t + a.caph * tp;

  int c0 = 0, nc = 0, r0 = 0, nr = 0;        // the input window of the tile: columns [c0, c0 + nc), rows [r0, r0 + nr)
  if (has) {
    c0 = dd_clampi(a.bx[2 * ox0], 0, a.w);
    const int ce = dd_clampi(a.bx[2 * (ox1 - 1)], 0, a.w) + dd_clampi(a.bx[2 * (ox1 - 1) + 1], 0, ksx);
    nc = dd_clampi(min(ce, a.w) - c0, 0, a.capw);
    r0 = dd_clampi(a.by[2 * oy0], 0, a.h);
    const int re = dd_clampi(a.by[2 * (oy1 - 1)], 0, a.h) + dd_clampi(a.by[2 * (oy1 - 1) + 1], 0, ksy);
    nr = dd_clampi(min(re, a.h) - r0, 0, a.caph);
    // the tables of the tile; windows clamped to the slice, so that no table can index outside it
    for (int i = tid; i < ncol; i += kThreads) {
      const int rel = dd_clampi(dd_clampi(a.bx[2 * (ox0 + i)], 0, a.w) - c0, 0, nc);
      lbx[2 * i] = rel;
      lbx[2 * i + 1] = min(dd_clampi(a.bx[2 * (ox0 + i) + 1], 0, ksx), nc - rel);
    }
    for (int i = tid; i < ncol * ksx; i += kThreads) lkx[i] = a.kx[(int64_t)ox0 * ksx + i];
    for (int i = tid; i < nrow; i += kThreads) {
      const int rel = dd_clampi(dd_clampi(a.by[2 * (oy0 + i)], 0, a.h) - r0, 0, nr);
      lby[2 * i] = rel;
      lby[2 * i + 1] = min(dd_clampi(a.by[2 * (oy0 + i) + 1], 0, ksy), nr - rel);
    }
    for (int i = tid; i < nrow * ksy; i += kThreads) lky[i] = a.ky[(int64_t)oy0 * ksy + i];
    // quantise the window: consecutive lanes read consecutive columns of one plane
    const T* x = reinterpret_cast<const T*>(a.x) + img * 3 * a.h * a.w;
    for (int i = tid; i < 3 * nr * nc; i += kThreads) {
      const int c = i % nc, rr = i / nc;
      const int r = rr % nr, ch = rr / nr;
      q[r * qp + c * 3 + ch] = (uint8_t)dd_quant_u8<T>(x[((int64_t)ch * a.h + r0 + r) * a.w + c0 + c], a.m11);
    }
  }
  __syncthreads();

  // horizontal pass: one (input row, output column) per lane, three channels share the coefficient loads
  const int tcol0 = ox0 + a.pad_l - X0;      // tile column of image column ox0
  if (has) {
    for (int i = tid; i < nr * ncol; i += kThreads) {
      const int oc = i % ncol, r = i / ncol;
      const int rel = lbx[2 * oc], cnt = lbx[2 * oc + 1];
      const int32_t* kk = lkx + oc * ksx;
      const uint8_t* p = q + r * qp + rel * 3;
      int32_t a0 = 1 << (kPB - 1), a1 = a0, a2 = a0;
      for (int j = 0; j < cnt; ++j) {
        const int32_t k = kk[j];
        a0 += (int32_t)p[3 * j] * k;
        a1 += (int32_t)p[3 * j + 1] * k;
        a2 += (int32_t)p[3 * j + 2] * k;
      }
      uint8_t* d = t + r * tp + (tcol0 + oc) * 3;
      d[0] = (uint8_t)dd_clip8(a0);
      d[1] = (uint8_t)dd_clip8(a1);
      d[2] = (uint8_t)dd_clip8(a2);
    }
  }
  __syncthreads();

  // vertical pass: four bytes of an output row per lane; bytes outside the image are the fill
  const int ndw = tp >> 2;
  const int ib0 = tcol0 * 3, ib1 = (tcol0 + ncol) * 3;       // the image's bytes of a tile row
  const int trow0 = oy0 + a.pad_t - Y0;                       // tile row of image row oy0
  const uint32_t fill4 = (uint32_t)a.fill * 0x01010101u;
  const uint32_t* t32 = reinterpret_cast<const uint32_t*>(t);
  uint32_t* o32 = reinterpret_cast<uint32_t*>(o);
  for (int i = tid; i < th * ndw; i += kThreads) {
    const int d = i % ndw, y = i / ndw;
    const int yy = y - trow0;
    uint32_t res = fill4;
    if (has && yy >= 0 && yy < nrow && 4 * d + 4 > ib0 && 4 * d < ib1) {
      const int rel = lby[2 * yy], cnt = lby[2 * yy + 1];
      const int32_t* kk = lky + yy * ksy;
      const uint32_t* p = t32 + rel * ndw + d;
      int32_t a0 = 1 << (kPB - 1), a1 = a0, a2 = a0, a3 = a0;
      for (int j = 0; j < cnt; ++j) {
        const int32_t k = kk[j];
        const uint32_t v = p[j * ndw];
        a0 += (int32_t)(v & 255u) * k;
        a1 += (int32_t)((v >> 8) & 255u) * k;
        a2 += (int32_t)((v >> 16) & 255u) * k;
        a3 += (int32_t)(v >> 24) * k;
      }
      const uint32_t val = dd_clip8(a0) | (dd_clip8(a1) << 8) | (dd_clip8(a2) << 16) | (dd_clip8(a3) << 24);
      uint32_t mask = 0;                                      // bytes of this dword inside the image
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (4 * d + k >= ib0 && 4 * d + k < ib1) mask |= 0xffu << (8 * k);
      res = (val & mask) | (fill4 & ~mask);
    }
    o32[y * (op >> 2) + d] = res;
  }
  __syncthreads();

  // store: per tile row the segment [g, g + nb) of the output; slot s is the aligned dword at g - mis + 4 s
  const int rows = min(th, a.ht - Y0);
  const int nb = min(tw, a.wt - X0) * 3;
  const int slots = ((nb + 3) >> 2) + 1;
  for (int i = tid; i < rows * slots; i += kThreads) {
    const int s = i % slots, y = i / slots;
    uint8_t* g = a.out + ((img * a.ht + Y0 + y) * a.wt + X0) * 3;
    const int mis = (int)(reinterpret_cast<uintptr_t>(g) & 3u);
    const int off = 4 * s - mis;                              // tile byte of the dword's first byte
    const uint8_t* orow = o + y * op;
    if (off >= 0 && off + 4 <= nb) {
      const uint32_t* w32 = reinterpret_cast<const uint32_t*>(orow) + (off >> 2);
      const uint64_t two = (uint64_t)w32[0] | ((uint64_t)w32[1] << 32);       // the pitch keeps w32[1] inside the row
      *reinterpret_cast<uint32_t*>(g + off) = (uint32_t)(two >> (8 * (off & 3)));
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (off + k >= 0 && off + k < nb) g[off + k] = orow[off + k];
    }
  }
}

// Tiles from the widest down: the first whose LDS image fits 64 KB.  An upscale takes the first (10 KB at 4x).
const int kTiles[][2] = {{64, 32}, {64, 16}, {32, 16}, {32, 8}, {16, 8}, {16, 4}};

static inline int cap_of(int tile, int in, int out, int ks) {
  const int64_t span = ((int64_t)(tile - 1) * in + out - 1) / out + ks + 1;    // include/dualdiff_hip.h: PIL's bound
  return (int)(span < in ? span : in);
}

// ---- image input: uint8 HWC frames -> normalised float pixel values --------------------------------------------------
//
// dd_image_load_u8 is the resample the other way round: the input is already pixel-interleaved bytes, so staging the
// window is a copy (aligned dwords of every row segment, bytes at its ends; a row keeps its global address mod 4 in LDS so
// that the dwords stay aligned on both sides), the two passes are the ones above, and the vertical pass of a pixel ends in
// three look-ups of the caller's float[3][256] table and goes straight to global memory: one element per channel plane
// with lanes along x (layout 0), or the pixel's 8 channels-last elements as 16-byte stores (layout 1).  A crop is a slice
// of the tables, so a workgroup's tile is a tile of the crop and nothing outside it is staged or computed.

struct LoadArgs {
  const uint8_t* in;
  void* out;
  const int32_t *kx, *bx, *ky, *by;
  const float* lut;
  int32_t h, w, oh, ow, ksx, ksy;
  int32_t tw, th;                            // tile of the output, pixels; tw % 4 == 0
  int32_t capw, caph;                        // input columns / rows the LDS slice holds
  int32_t qp;                                // pitch of the input window, bytes (multiple of 4, >= capw * 3 + 3)
};

// LDS image of a workgroup, in this order (every part a multiple of 4 bytes):
//   int32 lkx[tw * ksx], lbx[tw * 2], lky[th * ksy], lby[th * 2]   as in dd_image_resample_kernel
//   float llut[3 * 256]                                             the normalisation table
//   uint8 t[caph][tw * 3]                                           horizontal pass, tile byte columns
//   uint8 q[caph][qp]                                               input window; row r starts at byte (its address & 3)
static inline size_t load_lds_bytes(int tw, int th, int ksx, int ksy, int capw, int caph, int* qp) {
  *qp = (capw * 3 + 3 + 3) & ~3;
  return (size_t)4 * (tw * ksx + tw * 2 + th * ksy + th * 2 + 768) + (size_t)caph * tw * 3 + (size_t)caph * *qp;
}

// The kernel sees a slice of the tables and not the size of the resized image, so the slice is sized from ksize alone:
// ksize = 2 ceil(2 max(in / out, 1)) + 1 gives in / out <= max(ksize - 1, 4) / 4, and with it PIL's bound of cap_of.  The
// image's own size does not enter, so that a small image takes the tile a large one takes at the same ratio.
static inline int load_cap_of(int tile, int ks) {
  const int num = ks - 1 > 4 ? ks - 1 : 4;
  return ((tile - 1) * num + 3) / 4 + ks + 1;
}

template <typename T, int LAYOUT>
__global__ __launch_bounds__(kThreads)
void dd_image_load_kernel(const LoadArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t dd_img_lds[];
  const int tid = threadIdx.x;
  const int tw = a.tw, th = a.th, ksx = a.ksx, ksy = a.ksy;
  const int X0 = blockIdx.x * tw, Y0 = blockIdx.y * th;
  const int64_t img = blockIdx.z;
  const int ncol = min(tw, a.ow - X0), nrow = min(th, a.oh - Y0);           // >= 1 by the grid

  int32_t* lkx = reinterpret_cast<int32_t*>(dd_img_lds);
  int32_t* lbx = lkx + tw * ksx;
  int32_t* lky = lbx + tw * 2;
  int32_t* lby = lky + th * ksy;
  float* llut = reinterpret_cast<float*>(lby + th * 2);
  const int tp = tw * 3, qp = a.qp;
  uint8_t* t = reinterpret_cast<uint8_t*>(llut + 768);
  uint8_t* q = t + a.caph * tp;

  // the input window of the tile: columns [c0, c0 + nc), rows [r0, r0 + nr)
  const int c0 = dd_clampi(a.bx[2 * X0], 0, a.w);
  const int ce = dd_clampi(a.bx[2 * (X0 + ncol - 1)], 0, a.w) + dd_clampi(a.bx[2 * (X0 + ncol - 1) + 1], 0, ksx);
  const int nc = dd_clampi(min(ce, a.w) - c0, 0, a.capw);
  const int r0 = dd_clampi(a.by[2 * Y0], 0, a.h);
  const int re = dd_clampi(a.by[2 * (Y0 + nrow - 1)], 0, a.h) + dd_clampi(a.by[2 * (Y0 + nrow - 1) + 1], 0, ksy);
  const int nr = dd_clampi(min(re, a.h) - r0, 0, a.caph);
  // the tables of the tile; windows clamped to the slice, so that no table can index outside it
  for (int i = tid; i < ncol; i += kThreads) {
    const int rel = dd_clampi(dd_clampi(a.bx[2 * (X0 + i)], 0, a.w) - c0, 0, nc);
    lbx[2 * i] = rel;
    lbx[2 * i + 1] = min(dd_clampi(a.bx[2 * (X0 + i) + 1], 0, ksx), nc - rel);
  }
  for (int i = tid; i < ncol * ksx; i += kThreads) lkx[i] = a.kx[(int64_t)X0 * ksx + i];
  for (int i = tid; i < nrow; i += kThreads) {
    const int rel = dd_clampi(dd_clampi(a.by[2 * (Y0 + i)], 0, a.h) - r0, 0, nr);
    lby[2 * i] = rel;
    lby[2 * i + 1] = min(dd_clampi(a.by[2 * (Y0 + i) + 1], 0, ksy), nr - rel);
  }
  for (int i = tid; i < nrow * ksy; i += kThreads) lky[i] = a.ky[(int64_t)Y0 * ksy + i];
  for (int i = tid; i < 768; i += kThreads) llut[i] = a.lut[i];
  // copy the window: per row the segment [g, g + nb); slot s is the aligned dword at g - mis + 4 s, kept at q + 4 s
  const int64_t rowb = (int64_t)a.w * 3;
  const uint8_t* src = a.in + ((img * a.h + r0) * a.w + c0) * 3;
  const int nb = nc * 3;
  const int slots = ((nb + 3) >> 2) + 1;
  for (int i = tid; i < nr * slots; i += kThreads) {
    const int s = i % slots, r = i / slots;
    const uint8_t* g = src + r * rowb;
    const int mis = (int)(reinterpret_cast<uintptr_t>(g) & 3u);
    const int off = 4 * s - mis;                              // segment byte of the dword's first byte
    uint8_t* qrow = q + r * qp + mis;                         // where segment byte 0 goes
    if (off >= 0 && off + 4 <= nb) {
      *reinterpret_cast<uint32_t*>(qrow + off) = *reinterpret_cast<const uint32_t*>(g + off);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (off + k >= 0 && off + k < nb) qrow[off + k] = g[off + k];
    }
  }
  __syncthreads();

  // horizontal pass: one (input row, output column) per lane, three channels share the coefficient loads
  for (int i = tid; i < nr * ncol; i += kThreads) {
    const int oc = i % ncol, r = i / ncol;
    const int rel = lbx[2 * oc], cnt = lbx[2 * oc + 1];
    const int32_t* kk = lkx + oc * ksx;
    const int mis = (int)(reinterpret_cast<uintptr_t>(src + r * rowb) & 3u);
    const uint8_t* p = q + r * qp + mis + rel * 3;
    int32_t a0 = 1 << (kPB - 1), a1 = a0, a2 = a0;
    for (int j = 0; j < cnt; ++j) {
      const int32_t k = kk[j];
      a0 += (int32_t)p[3 * j] * k;
      a1 += (int32_t)p[3 * j + 1] * k;
      a2 += (int32_t)p[3 * j + 2] * k;
    }
    uint8_t* d = t + r * tp + oc * 3;
    d[0] = (uint8_t)dd_clip8(a0);
    d[1] = (uint8_t)dd_clip8(a1);
    d[2] = (uint8_t)dd_clip8(a2);
  }
  __syncthreads();

  // vertical pass: one pixel per lane, lanes along x; the three bytes index the table and go out in T
  for (int i = tid; i < nrow * tw; i += kThreads) {
    const int x = i % tw, y = i / tw;
    if (x >= ncol) continue;
    const int rel = lby[2 * y], cnt = lby[2 * y + 1];
    const int32_t* kk = lky + y * ksy;
    const uint8_t* p = t + rel * tp + x * 3;
    int32_t a0 = 1 << (kPB - 1), a1 = a0, a2 = a0;
    for (int j = 0; j < cnt; ++j) {
      const int32_t k = kk[j];
      a0 += (int32_t)p[j * tp] * k;
      a1 += (int32_t)p[j * tp + 1] * k;
      a2 += (int32_t)p[j * tp + 2] * k;
    }
    const T v0 = (T)llut[dd_clip8(a0)], v1 = (T)llut[256 + dd_clip8(a1)], v2 = (T)llut[512 + dd_clip8(a2)];
    if (LAYOUT == 0) {
      const int64_t plane = (int64_t)a.oh * a.ow;
      T* o = reinterpret_cast<T*>(a.out) + img * 3 * plane + (int64_t)(Y0 + y) * a.ow + X0 + x;
      o[0] = v0;
      o[plane] = v1;
      o[2 * plane] = v2;
    } else {
      const T zero = (T)0.0f;
      const T px[8] = {v0, v1, v2, zero, zero, zero, zero, zero};
      u32x4 u[sizeof(T) / 2];
      __builtin_memcpy(u, px, sizeof(px));
      uint8_t* o = reinterpret_cast<uint8_t*>(a.out) + ((img * a.oh + Y0 + y) * a.ow + X0 + x) * (int64_t)sizeof(px);
#pragma unroll
      for (int k = 0; k < (int)(sizeof(T) / 2); ++k) dd_st16(o + 16 * k, u[k]);
    }
  }
}

}  // namespace

extern "C" int dd_image_quantize_u8(const void* x, uint8_t* out, int32_t m, int32_t h, int32_t w, int32_t m11,
                                    int32_t dtype, dd_stream_t stream) {
  if (!x || !out || m <= 0 || h <= 0 || w <= 0) return DD_ERR_BAD_ARG;
  if (dtype != DD_F16 && dtype != DD_BF16 && dtype != DD_F32) return DD_ERR_BAD_ARG;
  const int64_t hw = (int64_t)h * w;
  if (m > 65535 || hw >= ((int64_t)1 << 31)) return DD_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)((hw + 4 * kThreads - 1) / (4 * kThreads)), (unsigned)m);
  dd_clear_error();
  return dd_dispatch32(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(dd_image_quantize_kernel<T>, grid, dim3(kThreads), 0, dd_stream(stream), (const T*)x, out,
                       (int32_t)hw, m11);
    return dd_check_launch();
  });
}

extern "C" int dd_image_resample_u8(const void* x, uint8_t* out, int32_t m, int32_t h, int32_t w, int32_t oh, int32_t ow,
                                    const int32_t* kx, const int32_t* bx, int32_t ksx, const int32_t* ky,
                                    const int32_t* by, int32_t ksy, int32_t pad_l, int32_t pad_t, int32_t pad_r,
                                    int32_t pad_b, int32_t fill, int32_t m11, int32_t dtype, dd_stream_t stream) {
  if (!x || !out || !kx || !bx || !ky || !by) return DD_ERR_BAD_ARG;
  if (m <= 0 || h <= 0 || w <= 0 || oh <= 0 || ow <= 0 || ksx <= 0 || ksy <= 0) return DD_ERR_BAD_ARG;
  if (pad_l < 0 || pad_t < 0 || pad_r < 0 || pad_b < 0 || fill < 0 || fill > 255) return DD_ERR_BAD_ARG;
  if (dtype != DD_F16 && dtype != DD_BF16 && dtype != DD_F32) return DD_ERR_BAD_ARG;
  if (ksx > DD_IMAGE_MAX_KSIZE || ksy > DD_IMAGE_MAX_KSIZE || m > 65535) return DD_ERR_UNSUPPORTED;
  const int64_t ht = (int64_t)pad_t + oh + pad_b, wt = (int64_t)pad_l + ow + pad_r;
  if (ht >= ((int64_t)1 << 24) || wt >= ((int64_t)1 << 24) || h >= (1 << 24) || w >= (1 << 24)) return DD_ERR_UNSUPPORTED;
  ResampleArgs a;
  a.x = x; a.out = out; a.kx = kx; a.bx = bx; a.ky = ky; a.by = by;
  a.h = h; a.w = w; a.oh = oh; a.ow = ow; a.ksx = ksx; a.ksy = ksy; a.pad_l = pad_l; a.pad_t = pad_t;
  a.ht = (int32_t)ht; a.wt = (int32_t)wt; a.fill = fill; a.m11 = m11;
  size_t lds = 0;
  bool found = false;
  for (const auto& tile : kTiles) {
    a.tw = tile[0]; a.th = tile[1];
    a.capw = cap_of(a.tw, w, ow, ksx);
    a.caph = cap_of(a.th, h, oh, ksy);
    lds = resample_lds_bytes(a.tw, a.th, ksx, ksy, a.capw, a.caph, &a.qp);
    if (lds <= 65536) { found = true; break; }
  }
  if (!found) return DD_ERR_UNSUPPORTED;
  const int64_t gx = (wt + a.tw - 1) / a.tw, gy = (ht + a.th - 1) / a.th;
  if (gy > 65535) return DD_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)gx, (unsigned)gy, (unsigned)m);
  dd_clear_error();
  return dd_dispatch32(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(dd_image_resample_kernel<T>, grid, dim3(kThreads), lds, dd_stream(stream), a);
    return dd_check_launch();
  });
}

extern "C" int dd_image_load_u8(const uint8_t* in, void* out, int32_t m, int32_t h, int32_t w, int32_t oh, int32_t ow,
                                const int32_t* kx, const int32_t* bx, int32_t ksx, const int32_t* ky, const int32_t* by,
                                int32_t ksy, const float* lut, int32_t dtype, int32_t layout, dd_stream_t stream) {
  if (!in || !out || !kx || !bx || !ky || !by || !lut) return DD_ERR_BAD_ARG;
  if (m <= 0 || h <= 0 || w <= 0 || oh <= 0 || ow <= 0 || ksx <= 0 || ksy <= 0) return DD_ERR_BAD_ARG;
  if (dtype != DD_F16 && dtype != DD_BF16 && dtype != DD_F32) return DD_ERR_BAD_ARG;
  if (layout != 0 && layout != 1) return DD_ERR_BAD_ARG;
  if (layout == 1 && !dd_aligned16(out)) return DD_ERR_BAD_ARG;
  if (ksx > DD_IMAGE_MAX_KSIZE || ksy > DD_IMAGE_MAX_KSIZE || m > 65535) return DD_ERR_UNSUPPORTED;
  if (oh >= (1 << 24) || ow >= (1 << 24) || h >= (1 << 24) || w >= (1 << 24)) return DD_ERR_UNSUPPORTED;
  LoadArgs a;
  a.in = in; a.out = out; a.kx = kx; a.bx = bx; a.ky = ky; a.by = by; a.lut = lut;
  a.h = h; a.w = w; a.oh = oh; a.ow = ow; a.ksx = ksx; a.ksy = ksy;
  size_t lds = 0;
  bool found = false;
  for (const auto& tile : kTiles) {
    a.tw = tile[0]; a.th = tile[1];
    a.capw = load_cap_of(a.tw, ksx);
    a.caph = load_cap_of(a.th, ksy);
    lds = load_lds_bytes(a.tw, a.th, ksx, ksy, a.capw, a.caph, &a.qp);
    if (lds <= 65536) { found = true; break; }
  }
  if (!found) return DD_ERR_UNSUPPORTED;
  const int64_t gx = ((int64_t)ow + a.tw - 1) / a.tw, gy = ((int64_t)oh + a.th - 1) / a.th;
  if (gy > 65535) return DD_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)gx, (unsigned)gy, (unsigned)m);
  dd_clear_error();
  return dd_dispatch32(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    auto go = [&](auto kern) { hipLaunchKernelGGL(kern, grid, dim3(kThreads), lds, dd_stream(stream), a); };
    if (layout == 0) go(dd_image_load_kernel<T, 0>);
    else go(dd_image_load_kernel<T, 1>);
    return dd_check_launch();
  });
}
