// Box input: every scene's 3D box corners -> the per-view `bboxes_3d_data` that dd_box_tokens reads, i.e. the reference's
// _preprocess_bbox (dataset/utils.py:128-262) with its visibility test (runner/box_visualizer.py:49-86, dataset/utils.py:
// 60-82) in one launch: per (scene, view) the kept boxes in their original order at the front of a row of `cap` slots,
// the tail as the reference pads it (zero points, class -1, mask 0), the number kept, and the largest number kept.
//
// One 256-thread workgroup owns one (scene, view) and takes the scene's boxes 256 at a time, one box per lane:
//   * the visibility test is the reference's float64 arithmetic: the homogeneous corner (x, y, z, 1.0) times the fp32
//     matrix promoted to double, IEEE division (this file is built without fast-math flags);
//   * the slot of a kept box is (boxes kept in earlier chunks) + (kept in the earlier waves of this chunk, wave totals in
//     LDS) + (kept in the lower lanes of its wave: ballot + popcount), so the order is the input's;
//   * a kept box whose slot is < cap has its payload row (96 or 48 bytes) stored with the widest stores the alignment of
//     the output allows: 16, 8 or 4 bytes (rows are multiples of 48 bytes apart, so one test of the base decides);
//   * the workgroup zeroes the tail of its own row, counts[] gets the true number kept (also when it exceeds cap), and one
//     vector atomic max per workgroup folds it into max_len, which the launcher clears on the stream beforehand.
// Nothing is written at or past slot `cap` of a row.
#include "dd_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / DD_WAVE;

struct BoxArgs {
  const float* corners;
  const float* filter_corners;               // never NULL here: the launcher substitutes corners
  const int64_t* labels;
  const int32_t* offsets;
  const float* transforms;
  float* bboxes;
  int64_t* classes;
  uint8_t* masks;
  int32_t* counts;
  int32_t* max_len;
  int32_t total, views, cap, filter_mode;
  double canvas_h, canvas_w;
};

// np.clip: a NaN stays a NaN (fmin / fmax would drop it)
__device__ __forceinline__ double dd_clip_f64(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

// 24 floats of one box; 16-byte loads where the array's base allows them (a row is 96 bytes)
__device__ __forceinline__ void dd_load_box(const float* __restrict__ p, bool vec, float (&r)[24]) {
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

// N floats (a multiple of 4) to a row whose address is a multiple of `align` bytes: 16, 8 or 4
template <int N>
__device__ __forceinline__ void dd_store_row(float* __restrict__ o, int align, const float (&r)[N]) {
  if (align == 16) {
#pragma unroll
    for (int k = 0; k < N / 4; ++k) {
      f32x4 v = {r[4 * k], r[4 * k + 1], r[4 * k + 2], r[4 * k + 3]};
      *reinterpret_cast<f32x4*>(o + 4 * k) = v;
    }
  } else if (align == 8) {
#pragma unroll
    for (int k = 0; k < N / 2; ++k) {
      float2 v = {r[2 * k], r[2 * k + 1]};
      *reinterpret_cast<float2*>(o + 2 * k) = v;
    }
  } else {
#pragma unroll
    for (int k = 0; k < N; ++k) o[k] = r[k];
  }
}

// zero floats [p, p + n) with the whole workgroup: single floats up to the first 16-byte boundary and after the last
__device__ __forceinline__ void dd_zero_f32(float* __restrict__ p, int64_t n, int tid) {
  if (n <= 0) return;
  int64_t lead = (int64_t)(((16u - (uint32_t)(reinterpret_cast<uintptr_t>(p) & 15u)) & 15u) >> 2);
  if (lead > n) lead = n;
  const int64_t n4 = (n - lead) >> 2;
  const int64_t done = lead + 4 * n4;
  if (tid < lead) p[tid] = 0.0f;
  const f32x4 z = {0.0f, 0.0f, 0.0f, 0.0f};
  f32x4* q = reinterpret_cast<f32x4*>(p + lead);
  for (int64_t i = tid; i < n4; i += kThreads) q[i] = z;
  if (tid < n - done) p[done + tid] = 0.0f;
}

template <int P>                               // points per box: 8 (all-xyz) or 4 (cxyz: corners 6, 5, 7, 2)
__global__ __launch_bounds__(kThreads)
void dd_box_views_kernel(const BoxArgs a) {
  __shared__ int32_t wave_kept[2][kWaves];     // double-buffered by chunk parity: one barrier per chunk
  const int tid = threadIdx.x, lane = tid & (DD_WAVE - 1), wave = tid / DD_WAVE;
  const int64_t blk = blockIdx.x;              // scene * views + view
  const int scene = (int)(blk / a.views);
  const int n0 = min(max(a.offsets[scene], 0), a.total);
  const int n1 = min(max(a.offsets[scene + 1], n0), a.total);
  const int n = n1 - n0, cap = a.cap;

  double m[3][4];                              // rows x, y, z of the view's matrix; row 3 is never used
  if (a.filter_mode != 0) {
    const float* t = a.transforms + blk * 16;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) m[r][c] = (double)t[4 * r + c];
  }
  const bool same = a.filter_corners == a.corners;
  const bool vec_f = (reinterpret_cast<uintptr_t>(a.filter_corners) & 15u) == 0;
  const bool vec_c = (reinterpret_cast<uintptr_t>(a.corners) & 15u) == 0;
  float* orow = a.bboxes + blk * cap * (P * 3);
  const uintptr_t oaddr = reinterpret_cast<uintptr_t>(orow);
  const int oalign = (oaddr & 15u) == 0 ? 16 : (oaddr & 7u) == 0 ? 8 : 4;
  int64_t* crow = a.classes + blk * cap;
  uint8_t* mrow = a.masks + blk * cap;

  int kept = 0;                                // boxes kept in earlier chunks (uniform over the workgroup)
  int par = 0;
  for (int base = 0; base < n; base += kThreads, par ^= 1) {
    const int i = base + tid;
    const bool valid = i < n;
    bool keep = valid;
    float row[24];
    if (a.filter_mode != 0 && valid) {
      dd_load_box(a.filter_corners + (int64_t)(n0 + i) * 24, vec_f, row);
      bool any_z = false, any_x = false, any_y = false;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const double x = (double)row[3 * k], y = (double)row[3 * k + 1], z = (double)row[3 * k + 2];
        const double cz = fma(z, m[2][2], fma(y, m[2][1], fma(x, m[2][0], m[2][3])));
        if (a.filter_mode == 1) {
          any_z |= cz > 0.0;
        } else {
          const double cx = fma(z, m[0][2], fma(y, m[0][1], fma(x, m[0][0], m[0][3])));
          const double cy = fma(z, m[1][2], fma(y, m[1][1], fma(x, m[1][0], m[1][3])));
          const double zc = dd_clip_f64(cz, 1e-5, 1e5);
          const double px = cx / zc, py = cy / zc;
          any_z |= (cz / fabs(cz)) > 0.0;      // the reference tests z / |z|: false for 0, an infinity and a NaN
          any_x |= px > 0.0 && px < a.canvas_w;
          any_y |= py > 0.0 && py < a.canvas_h;
        }
      }
      keep = a.filter_mode == 1 ? any_z : (any_z && any_x && any_y);
    }
    const uint64_t ballot = __ballot(keep);
    if (lane == 0) wave_kept[par][wave] = __popcll(ballot);
    __syncthreads();
    int before = 0, chunk = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      const int c = wave_kept[par][w];
      before += w < wave ? c : 0;
      chunk += c;
    }
    const int slot = kept + before + __popcll(ballot & (((uint64_t)1 << lane) - 1));
    if (keep && slot < cap) {
      if (!same || a.filter_mode == 0) dd_load_box(a.corners + (int64_t)(n0 + i) * 24, vec_c, row);
      float* o = orow + (int64_t)slot * (P * 3);
      if (P == 8) {
        dd_store_row<24>(o, oalign, row);
      } else {
        const float pick[12] = {row[18], row[19], row[20], row[15], row[16], row[17],
                                row[21], row[22], row[23], row[6], row[7], row[8]};
        dd_store_row<12>(o, oalign, pick);
      }
      crow[slot] = a.labels[n0 + i];
      mrow[slot] = 1;
    }
    kept += chunk;
  }

  // the tail of the row, as the reference pads it
  const int first = min(kept, cap);
  dd_zero_f32(orow + (int64_t)first * (P * 3), (int64_t)(cap - first) * (P * 3), tid);
  for (int s = first + tid; s < cap; s += kThreads) {
    crow[s] = -1;
    mrow[s] = 0;
  }
  if (tid == 0) {
    a.counts[blk] = kept;
    atomicMax(a.max_len, kept);
  }
}

}  // namespace

extern "C" int dd_box_views(const float* corners, const float* filter_corners, const int64_t* labels,
                            const int32_t* offsets, const float* transforms, int32_t total, int32_t scenes,
                            int32_t views, int32_t cap, int32_t points_mode, int32_t filter_mode, int32_t canvas_h,
                            int32_t canvas_w, float* bboxes, int64_t* classes, uint8_t* masks, int32_t* counts,
                            int32_t* max_len, dd_stream_t stream) {
  if (!offsets || !bboxes || !classes || !masks || !counts || !max_len) return DD_ERR_BAD_ARG;
  if (total < 0 || scenes <= 0 || views <= 0 || cap <= 0) return DD_ERR_BAD_ARG;
  if (total > 0 && (!corners || !labels)) return DD_ERR_BAD_ARG;
  if (points_mode != 0 && points_mode != 1) return DD_ERR_BAD_ARG;
  if (filter_mode < 0 || filter_mode > 2) return DD_ERR_BAD_ARG;
  if (filter_mode == 0 && views != 1) return DD_ERR_BAD_ARG;
  if (filter_mode != 0 && !transforms) return DD_ERR_BAD_ARG;
  if (filter_mode == 2 && (canvas_h <= 0 || canvas_w <= 0)) return DD_ERR_BAD_ARG;
  auto mis = [](const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; };
  if (mis(corners, 4) || mis(filter_corners, 4) || mis(transforms, 4) || mis(offsets, 4) || mis(bboxes, 4) ||
      mis(counts, 4) || mis(max_len, 4) || mis(labels, 8) || mis(classes, 8))
    return DD_ERR_BAD_ARG;
  const int64_t blocks = (int64_t)scenes * views;
  if (blocks >= ((int64_t)1 << 31) || blocks * cap >= ((int64_t)1 << 40)) return DD_ERR_UNSUPPORTED;   // 64-bit element indices
  BoxArgs a;
  a.corners = corners; a.filter_corners = filter_corners ? filter_corners : corners; a.labels = labels;
  a.offsets = offsets; a.transforms = transforms;
  a.bboxes = bboxes; a.classes = classes; a.masks = masks; a.counts = counts; a.max_len = max_len;
  a.total = total; a.views = views; a.cap = cap; a.filter_mode = filter_mode;
  a.canvas_h = (double)canvas_h; a.canvas_w = (double)canvas_w;
  dd_clear_error();
  if (hipMemsetAsync(max_len, 0, sizeof(int32_t), dd_stream(stream)) != hipSuccess) return DD_ERR_LAUNCH;
  if (points_mode == 0)
    hipLaunchKernelGGL(dd_box_views_kernel<8>, dim3((unsigned)blocks), dim3(kThreads), 0, dd_stream(stream), a);
  else
    hipLaunchKernelGGL(dd_box_views_kernel<4>, dim3((unsigned)blocks), dim3(kThreads), 0, dd_stream(stream), a);
  return dd_check_launch();
}
