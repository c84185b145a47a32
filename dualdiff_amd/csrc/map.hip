// Map output: the BEV map picture of the reference's demo path (runner/map_visualizer.py:106-211).
//
//  * dd_map_render_u8: the layers of a map (bytes, 0 / 1) -> the coloured map as an fp32 NCHW image holding colour / 255,
//    and per sample the word of the classes in use.  render_static (:106-118): among the set static layers of a pixel the
//    one of the greatest priority rank; render_dynamic (:121-132): the first set dynamic layer, over the static colour;
//    nothing set: the "nothing" colour.  The image goes into dd_image_resample_u8, whose quantiser returns the colour
//    byte for colour / 255 (the colour tables hold the quotient, built on the host), so PIL's resize runs on the bytes the
//    reference renders.
//  * dd_map_compose_u8: the quarter turn of Image.rotate(90) on a square image, np.pad's zeros and the legend pasted to
//    the right or below (:197-209), for the samples of a batch that share a legend.
//
// dd_map_render_u8: one lane per pixel, lanes along the row of every layer plane (a wave reads 64 consecutive bytes of a
// plane, stores 64 consecutive floats of each colour plane).  The layer loop is uniform, so the tables are read through
// the scalar cache.  The class bits of a lane are OR-ed over its wave by shuffles, over the workgroup through LDS, and
// one vector atomic OR per workgroup folds them into used[sample], which the launcher clears on the stream beforehand.
// dd_map_compose_u8: one lane per output pixel, lanes along the output row.  The turn reads a column of the source per
// output row; at 400 x 400 x 3 bytes the source stays in L2, and the path is launch-bound.
#include "dd_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / DD_WAVE;

__global__ __launch_bounds__(kThreads)
void dd_map_render_kernel(const uint8_t* __restrict__ maps, const float* __restrict__ stab,
                          const float* __restrict__ dtab, float* __restrict__ img, int32_t* __restrict__ used,
                          int32_t c, int32_t ss, int32_t ns, int32_t nd) {
  __shared__ uint32_t wave_bits[kWaves];
  const int tid = threadIdx.x;
  const int64_t smp = blockIdx.y;
  const int p = blockIdx.x * kThreads + tid;
  const bool valid = p < ss;
  uint32_t bits = 0;
  if (valid) {
    const uint8_t* m = maps + smp * c * ss + p;
    int best = ns;                                   // row ns of stab: the "nothing" colour, rank -1
    float best_rank = -1.0f;
    for (int k = 0; k < ns; ++k) {
      const uint32_t v = m[(int64_t)k * ss];
      if (v > 1u) bits |= 0x80000000u;
      const float rank = stab[4 * k + 3];
      if (v != 0u) {
        bits |= 1u << k;
        if (rank > best_rank) { best_rank = rank; best = k; }
      }
    }
    int first = -1;
    for (int j = 0; j < nd; ++j) {
      const uint32_t v = m[(int64_t)(ns + j) * ss];
      if (v > 1u) bits |= 0x80000000u;
      if (v != 0u && first < 0) first = j;
    }
    if (nd > 0) bits |= 1u << (ns + max(first, 0));  // argmax is 0 where nothing is set (:127-128)
    const float* col = first >= 0 ? dtab + 4 * first : stab + 4 * best;
    float* o = img + smp * 3 * ss + p;
    o[0] = col[0];
    o[ss] = col[1];
    o[2 * (int64_t)ss] = col[2];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) bits |= (uint32_t)__shfl_xor((int)bits, o, 64);
  if ((tid & (DD_WAVE - 1)) == 0) wave_bits[tid / DD_WAVE] = bits;
  __syncthreads();
  if (tid == 0) {
    uint32_t all = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) all |= wave_bits[w];
    if (all) atomicOr(reinterpret_cast<unsigned int*>(used) + smp, all);
  }
}

__global__ __launch_bounds__(kThreads)
void dd_map_compose_kernel(const uint8_t* __restrict__ src, const int32_t* __restrict__ index,
                           const uint8_t* __restrict__ legend, uint8_t* __restrict__ out, int32_t m, int32_t t,
                           int32_t lh, int32_t lw, int32_t ly, int32_t lx, int32_t oh, int32_t ow) {
  const int64_t g = blockIdx.y;
  const int64_t px = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (px >= (int64_t)oh * ow) return;
  const int r = (int)(px / ow), c = (int)(px % ow);
  uint32_t b0 = 0, b1 = 0, b2 = 0;
  if (r < t && c < t) {
    int s = index ? index[g] : (int)g;
    s = min(max(s, 0), m - 1);
    const uint8_t* q = src + ((s * (int64_t)t + c) * t + (t - 1 - r)) * 3;      // np.rot90(x, 1)[r, c] = x[c, t - 1 - r]
    b0 = q[0]; b1 = q[1]; b2 = q[2];
  } else if (legend && r >= ly && r < ly + lh && c >= lx && c < lx + lw) {
    const uint8_t* q = legend + ((int64_t)(r - ly) * lw + (c - lx)) * 3;
    b0 = q[0]; b1 = q[1]; b2 = q[2];
  }
  uint8_t* o = out + (g * oh * ow + px) * 3;
  o[0] = (uint8_t)b0;
  o[1] = (uint8_t)b1;
  o[2] = (uint8_t)b2;
}

}  // namespace

extern "C" int dd_map_render_u8(const uint8_t* maps, const float* stab, const float* dtab, float* img, int32_t* used,
                                int32_t b, int32_t c, int32_t s, int32_t ns, int32_t nd, dd_stream_t stream) {
  if (!maps || !stab || !img || !used) return DD_ERR_BAD_ARG;
  if (b <= 0 || c <= 0 || s <= 0 || ns < 0 || nd < 0 || (ns == 0 && nd == 0)) return DD_ERR_BAD_ARG;
  if (nd > 0 && !dtab) return DD_ERR_BAD_ARG;
  if ((int64_t)ns + nd > c) return DD_ERR_BAD_ARG;                              // 64-bit sum
  if ((int64_t)ns + nd > DD_MAP_MAX_LAYERS) return DD_ERR_UNSUPPORTED;
  auto mis = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) != 0; };
  if (mis(stab) || mis(dtab) || mis(img) || mis(used)) return DD_ERR_BAD_ARG;
  if (s >= (1 << 14) || b > 65535) return DD_ERR_UNSUPPORTED;                  // s * s < 2^28: 32-bit pixel indices
  const int32_t ss = s * s;
  const dim3 grid((unsigned)((ss + kThreads - 1) / kThreads), (unsigned)b);
  dd_clear_error();
  if (hipMemsetAsync(used, 0, sizeof(int32_t) * (size_t)b, dd_stream(stream)) != hipSuccess) return DD_ERR_LAUNCH;
  hipLaunchKernelGGL(dd_map_render_kernel, grid, dim3(kThreads), 0, dd_stream(stream), maps, stab, dtab, img, used, c,
                     ss, ns, nd);
  return dd_check_launch();
}

extern "C" int dd_map_compose_u8(const uint8_t* src, const int32_t* index, const uint8_t* legend, uint8_t* out,
                                 int32_t m, int32_t g, int32_t t, int32_t lh, int32_t lw, int32_t side,
                                 dd_stream_t stream) {
  if (!src || !out) return DD_ERR_BAD_ARG;
  if (m <= 0 || g <= 0 || t <= 0 || lh < 0 || lw < 0) return DD_ERR_BAD_ARG;
  if (side != 0 && side != 1) return DD_ERR_BAD_ARG;
  if ((legend != nullptr) != (lh > 0 && lw > 0) || (lh > 0) != (lw > 0)) return DD_ERR_BAD_ARG;
  if (!index && g != m) return DD_ERR_BAD_ARG;
  if ((reinterpret_cast<uintptr_t>(index) & 3u) != 0) return DD_ERR_BAD_ARG;
  if (side == 0 ? lh > t : lw > t) return DD_ERR_BAD_ARG;                      // the legend lies beside or below the map
  if (t >= (1 << 14) || lh >= (1 << 14) || lw >= (1 << 14) || m > 65535 || g > 65535) return DD_ERR_UNSUPPORTED;
  const int32_t oh = side == 0 ? t : t + lh, ow = side == 0 ? t + lw : t;     // < 2^15 each
  const int32_t ly = side == 0 ? 0 : t, lx = side == 0 ? t : 0;
  const int64_t pixels = (int64_t)oh * ow;
  const dim3 grid((unsigned)((pixels + kThreads - 1) / kThreads), (unsigned)g);
  dd_clear_error();
  hipLaunchKernelGGL(dd_map_compose_kernel, grid, dim3(kThreads), 0, dd_stream(stream), src, index, legend, out, m, t,
                     lh, lw, ly, lx, oh, ow);
  return dd_check_launch();
}
