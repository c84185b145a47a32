// The image-mode ORS condition: occupancy volume -> panorama of the first occupied class along each ray, painted with the
// Occ3D palette, the views side by side (networks/occ3d_proj.py:156-198), and the blend of that panorama over the camera
// pictures (:196-203).  The label of a sample is dd_ors_label's (ors_sample.h), the very function dd_ors_project uses.
#include "dd_common.h"
#include "ors_sample.h"

namespace {

struct OrsPalette { uint8_t c[18 * 3]; };

constexpr int ORS_VOXELS = DD_ORS_NX * DD_ORS_NY * DD_ORS_NZ;
constexpr int ORS_UNROLL = 4;

// ONE LANE PER RAY, not a wave per ray with a ballot.  What bounds this kernel is the chain "index -> one byte out of the
// 640 KB volume in L2" per sample, so the work is the number of samples visited.  A wave per ray visits 64 samples per step
// whatever the hit depth: with the median first hit at sample ~39 that is 64 lookups where 40 are needed, it needs 537 600
// waves of a few steps each for 6 x 224 x 400 rays, and its 64 lookups of one step walk ALONG the ray, through up to 32
// different voxel rows.  A lane per ray visits its own depth rounded up to ORS_UNROLL; the 64 lanes of a wave are 64
// neighbouring pixels of one image row, which hit or leave at similar depths (the wave runs as long as its deepest lane)
// and whose lookups of one step fall ACROSS the rays into neighbouring voxels, that is into few cache lines.  The latency
// of the dependent lookup is covered by ORS_UNROLL independent samples in flight per lane and by 8400 waves for 1024 SIMDs.
//
// Both ways of doing less are exact.  (1) Stop at the first label that is not 17 after the mode filter.  (2) Stop once the
// ray has left the volume for good: every voxel index is a monotone function of s (each rounding of the fp32 chain is
// monotone), non-decreasing where the direction's component is >= 0 and non-increasing where it is <= 0, so an index that
// is out of range on the side the ray moves toward stays out of range, and every later label is 17.  An index out of range
// on the OTHER side means that the ray has not entered yet: it goes on.  exits bit 0 / bit 1 switch the two rules (for the
// measurement of what each saves and the test that neither changes a byte).
__global__ __launch_bounds__(256)
void dd_ors_first_hit_kernel(const uint8_t* __restrict__ occ, const float* __restrict__ origin,
                             const float* __restrict__ dir, const int32_t* __restrict__ rig_of_sample,
                             uint8_t* __restrict__ cls, uint8_t* __restrict__ frames, int32_t* __restrict__ visited,
                             int b, int rigs, int n, int h, int w, int samples, float step, int mode, int exits,
                             OrsPalette pal) {
  const int hw = h * w;
  const int64_t total = (int64_t)b * n * hw;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int pix = (int)(i % hw);
    const int64_t r = i / hw;
    const int cam = (int)(r % n);
    const int sm = (int)(r / n);
    const int rig = rig_of_sample[sm];
    int hit = DD_ORS_FREE, seen = 0;
    if (rig >= 0 && rig < rigs) {                               // the wrapper checks the range; never read past a table
      const uint8_t* vol = occ + (int64_t)sm * ORS_VOXELS;
      const float* op = origin + ((int64_t)rig * n + cam) * 3;
      const float* dp = dir + (((int64_t)rig * n + cam) * hw + pix) * 3;
      const float o[3] = {op[0], op[1], op[2]};
      const float d[3] = {dp[0], dp[1], dp[2]};
      bool gone = false;
      for (int s0 = 0; s0 < samples; s0 += ORS_UNROLL) {
        int lab[ORS_UNROLL];
#pragma unroll
        for (int u = 0; u < ORS_UNROLL; ++u) {
          lab[u] = DD_ORS_FREE;
          if (s0 + u < samples) {
            int ix, iy, iz;
            dd_ors_voxel(o, d, s0 + u, step, ix, iy, iz);
            lab[u] = dd_ors_class_at(vol, ix, iy, iz);
            gone |= (d[0] >= 0.f && ix >= DD_ORS_NX) || (d[0] <= 0.f && ix < 0) ||
                    (d[1] >= 0.f && iy >= DD_ORS_NY) || (d[1] <= 0.f && iy < 0) ||
                    (d[2] >= 0.f && iz >= DD_ORS_NZ) || (d[2] <= 0.f && iz < 0);
          }
        }
        seen += min(ORS_UNROLL, samples - s0);
#pragma unroll
        for (int u = 0; u < ORS_UNROLL; ++u) {
          int c = lab[u];
          if (mode == 1 && c <= 10) c = DD_ORS_FREE;            // bg: foregrounds filtered out (:157)
          if (mode == 2 && c >= 11) c = DD_ORS_FREE;            // fg: backgrounds filtered out (:160)
          if (hit == DD_ORS_FREE) hit = c;
        }
        if (((exits & 1) && hit != DD_ORS_FREE) || ((exits & 2) && gone)) break;
      }
    }
    if (cls) cls[i] = (uint8_t)hit;
    if (frames) {
      const int y = pix / w, x = pix - y * w;
      uint8_t* f = frames + ((((int64_t)sm * h + y) * n + cam) * w + x) * 3;
      const int k = min(hit, DD_ORS_FREE) * 3;                  // a byte above 17 in the volume is no class: no colour
      f[0] = pal.c[k + 0];
      f[1] = pal.c[k + 1];
      f[2] = pal.c[k + 2];
    }
    if (visited) visited[i] = seen;
  }
}

// ---- overlay (:196-203) ----------------------------------------------------------------------------------------------
// x = u8 / 255 * 2 - 1 is monotone in the byte, so the minimum and maximum of x over a sample are x(min byte), x(max byte):
// the reduction runs on bytes.  ORS_PARTS workgroups per sample write one (min, max) pair each; the blend kernel's
// workgroups each reduce their sample's ORS_PARTS pairs again (one wave, one load per lane): two launches, no atomics, no
// buffer to clear.
constexpr int ORS_PARTS = 64;

__device__ __forceinline__ void ors_minmax_word(uint32_t v, int& mn, int& mx) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int by = (int)((v >> (8 * k)) & 0xffu);
    mn = min(mn, by);
    mx = max(mx, by);
  }
}

__global__ __launch_bounds__(256)
void dd_ors_minmax_kernel(const uint8_t* __restrict__ cam, int32_t* __restrict__ parts, int32_t* __restrict__ flags,
                          int64_t per) {
  __shared__ int smn[4], smx[4];
  const int part = blockIdx.x, sm = blockIdx.y;
  if (part == 0 && sm == 0 && threadIdx.x == 0) *flags = 0;     // the blend kernel, next in the stream, ORs into it
  const int64_t chunk = (per + ORS_PARTS - 1) / ORS_PARTS;
  const int64_t lo = min(per, (int64_t)part * chunk), hi = min(per, lo + chunk);
  const uint8_t* p = cam + (int64_t)sm * per;
  int mn = 255, mx = 0;
  // bytes up to the first 16-byte boundary, 16-byte vectors, the rest
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(p + lo);
  const int64_t head = min(hi - lo, (int64_t)((16 - (a0 & 15)) & 15));
  const int64_t nvec = (hi - lo - head) / 16;
  for (int64_t j = threadIdx.x; j < head; j += blockDim.x) { const int by = p[lo + j]; mn = min(mn, by); mx = max(mx, by); }
  const uint4* pv = reinterpret_cast<const uint4*>(p + lo + head);
  for (int64_t j = threadIdx.x; j < nvec; j += blockDim.x) {
    const uint4 v = pv[j];
    ors_minmax_word(v.x, mn, mx); ors_minmax_word(v.y, mn, mx); ors_minmax_word(v.z, mn, mx); ors_minmax_word(v.w, mn, mx);
  }
  for (int64_t j = lo + head + nvec * 16 + threadIdx.x; j < hi; j += blockDim.x) {
    const int by = p[j]; mn = min(mn, by); mx = max(mx, by);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { mn = min(mn, __shfl_xor(mn, o, 64)); mx = max(mx, __shfl_xor(mx, o, 64)); }
  if ((threadIdx.x & 63) == 0) { smn[threadIdx.x >> 6] = mn; smx[threadIdx.x >> 6] = mx; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < 4; ++k) { mn = min(mn, smn[k]); mx = max(mx, smx[k]); }
    parts[((int64_t)sm * ORS_PARTS + part) * 2 + 0] = mn;       // an empty part leaves (255, 0), neutral for both
    parts[((int64_t)sm * ORS_PARTS + part) * 2 + 1] = mx;
  }
}

// float32, operation by operation, as numpy and torch apply :196-203 on the CPU
__device__ __forceinline__ float ors_unit(int by) {             // get_img, :127-129: u8 / 255 * 2 - 1
  return __fsub_rn(__fmul_rn(__fdiv_rn((float)by, 255.0f), 2.0f), 1.0f);
}
__device__ __forceinline__ uint32_t ors_blend(uint32_t c, uint32_t u, float xmin, float den) {
  const float d = __fmul_rn(__fdiv_rn(__fsub_rn(ors_unit((int)u), xmin), den), 255.0f);                    // :196
  const float r = c != 0 ? __fadd_rn(__fmul_rn((float)c, 0.7f), __fmul_rn(d, 0.3f)) : d;                   // :199-203
  return (uint32_t)(int)r & 0xffu;                              // astype(uint8) of a value in [0, 256): truncation
}

__global__ __launch_bounds__(256)
void dd_ors_overlay_kernel(const uint8_t* __restrict__ colour, const uint8_t* __restrict__ cam,
                           const int32_t* __restrict__ parts, uint8_t* __restrict__ out, int32_t* __restrict__ flags,
                           int64_t per, int vec4) {
  __shared__ int s_mn, s_mx;
  const int sm = blockIdx.y;
  if (threadIdx.x < 64) {
    static_assert(ORS_PARTS == 64, "one pair per lane of the first wave");
    int mn = parts[((int64_t)sm * ORS_PARTS + threadIdx.x) * 2 + 0];
    int mx = parts[((int64_t)sm * ORS_PARTS + threadIdx.x) * 2 + 1];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { mn = min(mn, __shfl_xor(mn, o, 64)); mx = max(mx, __shfl_xor(mx, o, 64)); }
    if (threadIdx.x == 0) { s_mn = mn; s_mx = mx; }
  }
  __syncthreads();
  const int mn = s_mn, mx = s_mx;
  if (mx <= mn) {                                               // a constant picture: 0 / 0 in the reference
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(flags, 1);
  }
  const float xmin = ors_unit(mn);
  const float den = __fsub_rn(ors_unit(mx), xmin);
  const int64_t base = (int64_t)sm * per;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (vec4) {                                                   // per % 4 == 0 and 4-byte aligned pointers
    const uint32_t* c4 = reinterpret_cast<const uint32_t*>(colour + base);
    const uint32_t* u4 = reinterpret_cast<const uint32_t*>(cam + base);
    uint32_t* o4 = reinterpret_cast<uint32_t*>(out + base);
    for (int64_t j = t0; j < per / 4; j += stride) {
      const uint32_t c = c4[j], u = u4[j];
      uint32_t r = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        r |= (mx <= mn ? 0u : ors_blend((c >> (8 * k)) & 0xffu, (u >> (8 * k)) & 0xffu, xmin, den)) << (8 * k);
      o4[j] = r;
    }
  } else {
    for (int64_t j = t0; j < per; j += stride)
      out[base + j] = mx <= mn ? (uint8_t)0 : (uint8_t)ors_blend(colour[base + j], cam[base + j], xmin, den);
  }
}

unsigned ors_grid(int64_t threads, int64_t cap) {
  const int64_t g = (threads + 255) / 256;
  return (unsigned)(g < 1 ? 1 : g > cap ? cap : g);
}

}  // namespace

extern "C" int dd_ors_first_hit(const uint8_t* occ, const float* origin, const float* dir, const int32_t* rig_of_sample,
                                uint8_t* cls, uint8_t* frames, int32_t* visited, const uint8_t* palette, int32_t b,
                                int32_t rigs, int32_t n, int32_t h, int32_t w, int32_t samples, float step, int32_t mode,
                                int32_t exits, dd_stream_t stream) {
  if (!occ || !origin || !dir || !rig_of_sample || !palette || (!cls && !frames)) return DD_ERR_BAD_ARG;
  if (b <= 0 || rigs <= 0 || n <= 0 || h <= 0 || w <= 0 || samples <= 0) return DD_ERR_BAD_ARG;
  if (mode < 0 || mode > 2 || exits < 0 || exits > 3) return DD_ERR_BAD_ARG;
  if (!(step > 0.f)) return DD_ERR_BAD_ARG;                     // the leave-the-volume rule needs t = s * step to rise with s
  if ((int64_t)h * w > (1 << 30)) return DD_ERR_BAD_ARG;
  dd_clear_error();
  OrsPalette pal;
  for (int k = 0; k < 18 * 3; ++k) pal.c[k] = palette[k];
  const int64_t total = (int64_t)b * n * h * w;
  hipLaunchKernelGGL(dd_ors_first_hit_kernel, dim3(ors_grid(total, 1 << 22)), dim3(256), 0, dd_stream(stream), occ, origin,
                     dir, rig_of_sample, cls, frames, visited, b, rigs, n, h, w, samples, step, mode, exits, pal);
  return dd_check_launch();
}

extern "C" int dd_ors_overlay_u8(const uint8_t* colour, const uint8_t* camera, uint8_t* out, int32_t* parts, int32_t* flags,
                                 int32_t b, int32_t h, int32_t w, dd_stream_t stream) {
  if (!colour || !camera || !out || !parts || !flags || b <= 0 || h <= 0 || w <= 0) return DD_ERR_BAD_ARG;
  if (b > 65535) return DD_ERR_BAD_ARG;                         // a sample is blockIdx.y
  dd_clear_error();
  const int64_t per = (int64_t)h * w * 3;
  hipLaunchKernelGGL(dd_ors_minmax_kernel, dim3(ORS_PARTS, b), dim3(256), 0, dd_stream(stream), camera, parts, flags, per);
  if (dd_check_launch() != DD_OK) return DD_ERR_LAUNCH;
  const uintptr_t bits = reinterpret_cast<uintptr_t>(colour) | reinterpret_cast<uintptr_t>(camera) |
                         reinterpret_cast<uintptr_t>(out);
  const int vec4 = (per % 4 == 0 && (bits & 3) == 0) ? 1 : 0;
  hipLaunchKernelGGL(dd_ors_overlay_kernel, dim3(ors_grid(vec4 ? per / 4 : per, 1024), b), dim3(256), 0, dd_stream(stream),
                     colour, camera, parts, out, flags, per, vec4);
  return dd_check_launch();
}
