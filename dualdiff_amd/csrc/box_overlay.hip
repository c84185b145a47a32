// Box output: the 3D-box overlays of the reference's demo path (misc/test_utils.py:48-65 draw_box_on_imgs, runner/
// box_visualizer.py:89-114 show_box_on_views) in two launches.  The geometry is the reference's; the line is PIL's thin
// line (ImageDraw.line, width 1), not cv2's anti-aliased one: csrc/box_overlay_core.h has both, as functions that also
// run on the host.
//
//  * dd_box_edges: every scene's box corners -> per (scene, view) the integer end points of the boxes that are drawn, in
//    draw order (farthest first), their palette indices, the number drawn and a word of flags.  One 256-thread workgroup
//    owns one (scene, view).  Pass 1: one box per lane and turn, the least z of its eight corners (or "not drawn") into
//    LDS as the sort key.  Pass 2: the rank of a box is the number of boxes drawn before it, counted over the keys in LDS
//    (every lane reads the same key: a broadcast) — O(k^2) compares, 4096 LDS reads per lane at the 1024 boxes a scene may
//    hold; the box is projected and its 64-byte row stored at its rank as four 16-byte vectors.  With more than `cap`
//    boxes drawn the nearest `cap` are kept (the last ones in draw order), and counts[] still holds the true number.
//  * dd_box_draw_u8: pixel-major.  A workgroup owns a tile of 16 x 16 pixels, one pixel per lane, lanes along the row (of
//    64 x 4, 32 x 8 and 16 x 16 the square one rejects the most boxes per tile and measured best: profiles/
//    box_output.txt).  The view's boxes go through LDS 256 at a time from the last slot down: one lane per box tests the
//    box's integer bounding box against the tile, a ballot compacts the survivors in slot order, and every pixel walks
//    them from the last one down and stops at the first box with an edge that covers it — the colour of the last edge in
//    draw order, with no atomics, no scratch buffer and no clipping; a line's cost does not depend on its length.  The
//    loop ends early once every pixel of the tile has its colour.  RGBA pixels are stored as one dword per lane; the RGB segment of a tile row
//    (48 bytes) is laid into LDS at its global address mod 4 and goes out as aligned dwords, the up to three bytes at
//    either end as bytes (image.hip's store), so that no lane writes outside its own segment.
#include "dd_common.h"
#include "box_overlay_core.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / DD_WAVE;
#ifndef DD_BO_TILE_W                           // -DDD_BO_TILE_W=64 / 32: the other shapes tools/box_output_timing.py measured
#define DD_BO_TILE_W 16
#endif
constexpr int kTileW = DD_BO_TILE_W;           // pixels of a tile row; one pixel per lane, lanes along the row
constexpr int kTileH = kThreads / kTileW;
static_assert(kTileW >= 4 && kTileW <= kThreads && (kTileW & (kTileW - 1)) == 0, "a tile row is a power of two of lanes");
constexpr int kChunk = kThreads;               // boxes staged per turn: one per lane
constexpr int kBoxInts = 17;                   // 16 coordinates and the class; an odd stride, so the staging writes spread over the banks

typedef int32_t i32x4 __attribute__((ext_vector_type(4)));

struct EdgeArgs {
  const float* corners;
  const int64_t* labels;
  const int32_t* offsets;
  const float* transforms;
  int32_t* pts;
  int32_t* cls;
  int32_t* counts;
  int32_t* flags;
  int32_t total, views, cap, n_classes;
};

__device__ __forceinline__ void dd_bo_load_box(const float* __restrict__ p, bool vec, float (&r)[24]) {
  if (vec) {
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(p + 4 * k);
      r[4 * k] = v[0]; r[4 * k + 1] = v[1]; r[4 * k + 2] = v[2]; r[4 * k + 3] = v[3];
    }
  } else {
#pragma unroll
    for (int k = 0; k < 24; ++k) r[k] = p[k];
  }
}

__global__ __launch_bounds__(kThreads)
void dd_box_edges_kernel(const EdgeArgs a) {
  __shared__ double key[DD_BO_MAX_BOXES];      // the least z of a drawn box (> 0), -1 of any other
  __shared__ int32_t wave_kept[kWaves];
  const int tid = threadIdx.x, lane = tid & (DD_WAVE - 1), wave = tid / DD_WAVE;
  const int64_t blk = blockIdx.x;              // scene * views + view
  const int scene = (int)(blk / a.views);
  const int n0 = min(max(a.offsets[scene], 0), a.total);
  const int n1 = min(max(a.offsets[scene + 1], n0), a.total);
  const int n = min(n1 - n0, DD_BO_MAX_BOXES), cap = a.cap;
  uint32_t fl = n1 - n0 > DD_BO_MAX_BOXES ? DD_BO_FLAG_CAP : 0;

  double m[12];                                // rows x, y, z of the view's matrix
  const float* t = a.transforms + blk * 16;
#pragma unroll
  for (int k = 0; k < 12; ++k) m[k] = (double)t[k];
  const bool vec = (reinterpret_cast<uintptr_t>(a.corners) & 15u) == 0;

  int mine = 0;
  for (int i = tid; i < n; i += kThreads) {
    float row[24];
    dd_bo_load_box(a.corners + (int64_t)(n0 + i) * 24, vec, row);
    const int32_t c = dd_bo_class(a.labels[n0 + i], a.n_classes);
    if (c < 0) fl |= DD_BO_FLAG_LABEL;
    const double mz = dd_bo_min_z(row, m);
    const bool keep = c >= 0 && dd_bo_drawn(mz);
    key[i] = keep ? mz : -1.0;
    mine += keep ? 1 : 0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
  if (lane == 0) wave_kept[wave] = mine;
  __syncthreads();                             // the keys and the wave totals
  int kept = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) kept += wave_kept[w];
  const int drop = max(kept - cap, 0);         // the farthest `drop` boxes have no slot
  int32_t* prow = a.pts + blk * cap * 16;
  int32_t* crow = a.cls + blk * cap;

  for (int i = tid; i < n; i += kThreads) {
    const double ki = key[i];
    if (!dd_bo_drawn(ki)) continue;
    int rank = 0;
    for (int j = 0; j < n; ++j) rank += dd_bo_before(key[j], j, ki, i) ? 1 : 0;       // a -1 is never before a key > 0
    const int slot = rank - drop;
    if (slot < 0) continue;                    // slot < min(kept, cap) <= cap: rank < kept
    float row[24];
    dd_bo_load_box(a.corners + (int64_t)(n0 + i) * 24, vec, row);
    int32_t p[16];
    if (dd_bo_points(row, m, p)) fl |= DD_BO_FLAG_SATURATED;
    i32x4* o = reinterpret_cast<i32x4*>(prow + (int64_t)slot * 16);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const i32x4 v = {p[4 * k], p[4 * k + 1], p[4 * k + 2], p[4 * k + 3]};
      o[k] = v;
    }
    crow[slot] = dd_bo_class(a.labels[n0 + i], a.n_classes);
  }

  const i32x4 z = {0, 0, 0, 0};
  for (int s = min(kept, cap) + tid; s < cap; s += kThreads) {
    i32x4* o = reinterpret_cast<i32x4*>(prow + (int64_t)s * 16);
    o[0] = z; o[1] = z; o[2] = z; o[3] = z;
    crow[s] = 0;
  }
  if (tid == 0) {
    a.counts[blk] = kept;
    if (kept > cap) fl |= DD_BO_FLAG_CAP;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) fl |= (uint32_t)__shfl_xor((int)fl, o, 64);
  if (lane == 0 && fl) atomicOr(reinterpret_cast<unsigned int*>(a.flags), fl);        // at most one vector atomic per wave
}

struct DrawArgs {
  const uint8_t* frames;
  const int32_t* pts;
  const int32_t* cls;
  const int32_t* counts;
  const uint8_t* palette;
  uint8_t* out;
  int32_t cap, h, w, n_palette;
};

__device__ __forceinline__ int32_t dd_bo_clamp_pt(int32_t v) { return min(max(v, -DD_BO_SAT), DD_BO_SAT); }

template <bool kTransparent>
__global__ __launch_bounds__(kThreads)
void dd_box_draw_kernel(const DrawArgs a) {
  __shared__ int32_t boxes[kChunk * kBoxInts];
  __shared__ int32_t wave_n[kWaves];
  __shared__ uint32_t orow[kTileH][kTileW * 3 / 4 + 1];       // a tile row's RGB segment at its global address mod 4
  const int tid = threadIdx.x, lane = tid & (DD_WAVE - 1), wave = tid / DD_WAVE;
  const int64_t v = blockIdx.z;                // scene * views + view
  const int tx0 = blockIdx.x * kTileW, ty0 = blockIdx.y * kTileH;
  const int tx1 = min(tx0 + kTileW, a.w) - 1, ty1 = min(ty0 + kTileH, a.h) - 1;        // the tile, both ends included
  const int lx = tid % kTileW, ly = tid / kTileW;
  const int px = tx0 + lx, py = ty0 + ly;
  const bool inside = px < a.w && py < a.h;
  const int count = min(max(a.counts[v], 0), a.cap);
  const int32_t* prow = a.pts + v * a.cap * 16;
  const int32_t* crow = a.cls + v * a.cap;

  bool done = !inside;
  int colour = -1;                             // the palette index of the box that covers the pixel
  for (int hi = count; hi > 0; hi -= kChunk) {
    const int s = max(hi - kChunk, 0) + tid;   // this lane's slot: the chunk is [max(hi - 256, 0), hi)
    int32_t p[16];
    bool keep = false;
    if (s < hi) {
      const i32x4* q = reinterpret_cast<const i32x4*>(prow + (int64_t)s * 16);
      int32_t lox = DD_BO_SAT, hix = -DD_BO_SAT, loy = DD_BO_SAT, hiy = -DD_BO_SAT;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const i32x4 u = q[k];
        p[4 * k] = dd_bo_clamp_pt(u[0]); p[4 * k + 1] = dd_bo_clamp_pt(u[1]);
        p[4 * k + 2] = dd_bo_clamp_pt(u[2]); p[4 * k + 3] = dd_bo_clamp_pt(u[3]);
        lox = min(lox, min(p[4 * k], p[4 * k + 2])); hix = max(hix, max(p[4 * k], p[4 * k + 2]));
        loy = min(loy, min(p[4 * k + 1], p[4 * k + 3])); hiy = max(hiy, max(p[4 * k + 1], p[4 * k + 3]));
      }
      keep = hix >= tx0 && lox <= tx1 && hiy >= ty0 && loy <= ty1;
    }
    const uint64_t ballot = __ballot(keep);
    if (lane == 0) wave_n[wave] = __popcll(ballot);
    __syncthreads();
    int before = 0, nsurv = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      const int c = wave_n[w];
      before += w < wave ? c : 0;
      nsurv += c;
    }
    if (keep) {
      int32_t* d = boxes + (before + __popcll(ballot & (((uint64_t)1 << lane) - 1))) * kBoxInts;
#pragma unroll
      for (int k = 0; k < 16; ++k) d[k] = p[k];
      d[16] = min(max(crow[s], 0), a.n_palette - 1);
    }
    __syncthreads();
    if (!done) {
      for (int k = nsurv - 1; k >= 0; --k) {
        const int32_t* b = boxes + k * kBoxInts;
        if (dd_bo_on_box(px, py, b)) {
          colour = b[16];
          done = true;
          break;
        }
      }
    }
    if (__syncthreads_and(done)) break;        // also: every read of `boxes` and wave_n is over before the next turn writes them
  }

  uint32_t r = 0, g = 0, b = 0;
  if (colour >= 0) {
    const uint8_t* c = a.palette + 3 * colour;
    r = c[0]; g = c[1]; b = c[2];
  }
  if (kTransparent) {
    if (inside)
      reinterpret_cast<uint32_t*>(a.out)[(v * a.h + py) * a.w + px] = r | g << 8 | b << 16 | dd_bo_alpha(r, g, b) << 24;
    return;
  }
  const int64_t seg = ((v * a.h + py) * a.w + tx0) * 3;                 // the first byte of this lane's row segment
  uint8_t* gseg = a.out + seg;
  const int mis = (int)(reinterpret_cast<uintptr_t>(gseg) & 3u);
  uint8_t* lrow = reinterpret_cast<uint8_t*>(orow[ly]);
  if (inside) {
    if (colour < 0) {
      const uint8_t* f = a.frames + seg + 3 * lx;
      r = f[0]; g = f[1]; b = f[2];
    }
    uint8_t* d = lrow + mis + 3 * lx;
    d[0] = (uint8_t)r; d[1] = (uint8_t)g; d[2] = (uint8_t)b;
  }
  __syncthreads();
  if (py < a.h) {
    const int nb = (tx1 - tx0 + 1) * 3;        // bytes of the segment, <= 3 kTileW; LDS bytes [mis, mis + nb)
    const int off = 4 * lx;                    // this lane's dword: LDS bytes [off, off + 4), global gseg - mis + off
                                               // (the lanes of a row suffice: 4 kTileW >= 3 kTileW + 3)
    if (off < mis + nb) {
      if (off >= mis && off + 4 <= mis + nb) {
        *reinterpret_cast<uint32_t*>(gseg - mis + off) = orow[ly][lx];
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (off + k >= mis && off + k < mis + nb) gseg[off + k - mis] = lrow[off + k];
      }
    }
  }
}

}  // namespace

extern "C" int dd_box_edges(const float* corners, const int64_t* labels, const int32_t* offsets, const float* transforms,
                            int32_t total, int32_t scenes, int32_t views, int32_t cap, int32_t n_classes, int32_t* pts,
                            int32_t* cls, int32_t* counts, int32_t* flags, dd_stream_t stream) {
  if (!offsets || !transforms || !pts || !cls || !counts || !flags) return DD_ERR_BAD_ARG;
  if (total < 0 || scenes <= 0 || views <= 0 || cap <= 0 || n_classes <= 0) return DD_ERR_BAD_ARG;
  if (total > 0 && (!corners || !labels)) return DD_ERR_BAD_ARG;
  auto mis = [](const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; };
  if (mis(corners, 4) || mis(transforms, 4) || mis(offsets, 4) || mis(cls, 4) || mis(counts, 4) || mis(flags, 4) ||
      mis(labels, 8) || mis(pts, 16))
    return DD_ERR_BAD_ARG;
  if (cap > DD_BOX_EDGES_MAX) return DD_ERR_UNSUPPORTED;
  const int64_t blocks = (int64_t)scenes * views;
  if (blocks >= ((int64_t)1 << 31)) return DD_ERR_UNSUPPORTED;         // blocks * cap * 16 < 2^45: 64-bit element indices
  EdgeArgs a;
  a.corners = corners; a.labels = labels; a.offsets = offsets; a.transforms = transforms;
  a.pts = pts; a.cls = cls; a.counts = counts; a.flags = flags;
  a.total = total; a.views = views; a.cap = cap; a.n_classes = n_classes;
  dd_clear_error();
  if (hipMemsetAsync(flags, 0, sizeof(int32_t), dd_stream(stream)) != hipSuccess) return DD_ERR_LAUNCH;
  hipLaunchKernelGGL(dd_box_edges_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, dd_stream(stream), a);
  return dd_check_launch();
}

extern "C" int dd_box_draw_u8(const uint8_t* frames, const int32_t* pts, const int32_t* cls, const int32_t* counts,
                              const uint8_t* palette, uint8_t* out, int32_t m, int32_t cap, int32_t h, int32_t w,
                              int32_t n_palette, int32_t transparent, dd_stream_t stream) {
  if (!pts || !cls || !counts || !palette || !out) return DD_ERR_BAD_ARG;
  if (transparent != 0 && transparent != 1) return DD_ERR_BAD_ARG;
  if (!transparent && !frames) return DD_ERR_BAD_ARG;
  if (m <= 0 || cap <= 0 || h <= 0 || w <= 0 || n_palette <= 0) return DD_ERR_BAD_ARG;
  auto mis = [](const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; };
  if (mis(pts, 16) || mis(cls, 4) || mis(counts, 4) || (transparent && mis(out, 4))) return DD_ERR_BAD_ARG;
  if (h >= (1 << 15) || w >= (1 << 15) || m > 65535) return DD_ERR_UNSUPPORTED;          // m * h * w * 4 < 2^48
  if ((int64_t)m * cap >= ((int64_t)1 << 40)) return DD_ERR_UNSUPPORTED;                // 64-bit element indices
  DrawArgs a;
  a.frames = frames; a.pts = pts; a.cls = cls; a.counts = counts; a.palette = palette; a.out = out;
  a.cap = cap; a.h = h; a.w = w; a.n_palette = n_palette;
  const dim3 grid((unsigned)((w + kTileW - 1) / kTileW), (unsigned)((h + kTileH - 1) / kTileH), (unsigned)m);
  dd_clear_error();
  if (transparent)
    hipLaunchKernelGGL(dd_box_draw_kernel<true>, grid, dim3(kThreads), 0, dd_stream(stream), a);
  else
    hipLaunchKernelGGL(dd_box_draw_kernel<false>, grid, dim3(kThreads), 0, dd_stream(stream), a);
  return dd_check_launch();
}
