// FGM loss mask and the masked loss: `heatmap_gt` of the reference's collate_fn (magicdrive/dataset/utils.py:530-559:
// create_heatmap_gt of networks/utils.py:26-39, 100-163, and hd_crop :348-353) from the per-view 3D box corners, and the two
// loss lines of runner/multiview_runner.py:501-507 that consume it.  The mask's arithmetic — the float64 projection, the
// truncation, the hull, matplotlib's crossing rule — is csrc/fgm_mask_core.h, which also compiles for the host.
//
//  * dd_fgm_box_records: one wave per (scene, view, box).  Lane p projects corner p (float64, single operations) and
//    leaves the truncated pixel in LDS; lane 0 builds the ring (at most eight points: an insertion sort and the monotone
//    chain in LDS words, no scratch memory); then the 64 lanes count the pixels the ring paints over its bounding box on
//    the grid, a wave reduction gives the area, and lanes 0..23 store the 96-byte record with the weight.
//  * dd_fgm_mask: pixel-major over the CROPPED output, one pixel per lane, a workgroup per 256 consecutive pixels of a
//    view.  Every pixel walks the view's records — the address is uniform, the record is read through the scalar cache —
//    rejects by bounding box and keeps the greatest weight among the boxes that paint it.  Each output element is written
//    exactly once; the flagged boxes are summed from the records by workgroup (0, 0).  No atomics.
//  * dd_fgm_loss: sum((p - t)^2 (1 + heat)) / N in fp32 and, optionally, its gradient in the same pass: per-workgroup
//    partials in a fixed order, then one workgroup over the partials.  The grid is a function of N alone, so the same
//    inputs give the same bits.  The tensors are a few hundred kilobytes: the loads are scalar, not vectorised.
#include "dd_common.h"
#include "fgm_mask_core.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / DD_WAVE;
typedef int32_t i32x4 __attribute__((ext_vector_type(4)));
static_assert(DD_FG_REC <= DD_WAVE && DD_FG_MAX_POINTS <= DD_WAVE, "a lane per record word and per corner");
static_assert((DD_FG_REC * 4) % 16 == 0 && (DD_FG_BBOX * 4) % 16 == 0, "the bounding box is read as one 16-byte word");

struct RecordArgs {
  const float* corners;
  const uint8_t* masks;
  const float* l2i;
  int32_t* rec;
  double sx, sy;
  int32_t total, m, np, width, height;
};

struct MaskArgs {
  const int32_t* rec;
  float* out;
  int32_t* flags;
  int32_t total, m, width, height, wo, ho;
};

__device__ __forceinline__ int32_t wave_sum(int32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(kThreads)
void dd_fgm_box_records_kernel(RecordArgs a) {
  __shared__ int32_t s_pts[kWaves][2 * DD_FG_MAX_POINTS];
  __shared__ int32_t s_status[kWaves][DD_FG_MAX_POINTS];
  __shared__ int32_t s_work[kWaves][DD_FG_WORK];
  __shared__ int32_t s_rec[kWaves][DD_FG_REC];
  const int tid = threadIdx.x, lane = tid & (DD_WAVE - 1), wave = tid / DD_WAVE;
  const int64_t box = (int64_t)blockIdx.x * kWaves + wave;
  const bool live = box < a.total;
  if (live && lane < a.np) {
    const int64_t view = box / a.m;
    int32_t px = 0, py = 0;
    s_status[wave][lane] = dd_fg_point(a.corners + (box * a.np + lane) * 3, a.l2i + view * 16, a.sx, a.sy, &px, &py);
    s_pts[wave][2 * lane] = px;
    s_pts[wave][2 * lane + 1] = py;
  }
  __syncthreads();
  if (live && lane == 0) dd_fg_record(s_pts[wave], s_status[wave], a.np, a.masks[box] != 0, s_work[wave], s_rec[wave]);
  __syncthreads();
  int32_t cnt = 0;
  if (live) {
    int32_t clip[4];
    dd_fg_clip(s_rec[wave], a.width, a.height, clip);
    if (clip[0] <= clip[1]) {
      const int32_t bw = clip[1] - clip[0] + 1, npx = bw * (clip[3] - clip[2] + 1);          // at most W * H <= 2^20
      for (int32_t i = lane; i < npx; i += DD_WAVE) cnt += dd_fg_inside(s_rec[wave], clip[0] + i % bw, clip[2] + i / bw) ? 1 : 0;
    }
  }
  cnt = wave_sum(cnt);
  if (live && lane < DD_FG_REC) {
    int32_t v = s_rec[wave][lane];
    if (lane == DD_FG_AREA) v = cnt;
    if (lane == DD_FG_WEIGHT) v = dd_bm_f_bits(dd_fg_weight(cnt, a.width, a.height));
    a.rec[box * DD_FG_REC + lane] = v;
  }
}

__global__ __launch_bounds__(kThreads)
void dd_fgm_mask_kernel(MaskArgs a) {
  __shared__ int32_t wave_cnt[kWaves];
  const int tid = threadIdx.x, lane = tid & (DD_WAVE - 1), wave = tid / DD_WAVE;
  const int64_t view = blockIdx.y;
  const int32_t npix = a.wo * a.ho, pix = (int32_t)blockIdx.x * kThreads + tid;
  if (pix < npix) {
    const int32_t tx = pix % a.wo + (a.width - a.wo) / 2, ty = pix / a.wo + (a.height - a.ho);          // hd_crop
    float best = 0.0f;
    const int32_t* r = a.rec + view * a.m * DD_FG_REC;
    for (int32_t k = 0; k < a.m; ++k, r += DD_FG_REC) {
      const i32x4 bb = *reinterpret_cast<const i32x4*>(r + DD_FG_BBOX);
      if (tx >= bb[0] && tx <= bb[1] && ty >= bb[2] && ty <= bb[3] && dd_fg_inside(r, tx, ty))
        best = fmaxf(best, dd_bm_bits_f(r[DD_FG_WEIGHT]));
    }
    a.out[view * npix + pix] = best;
  }
  if (blockIdx.x == 0 && blockIdx.y == 0) {
    int32_t n = 0;
    for (int32_t k = tid; k < a.total; k += kThreads) n += a.rec[(int64_t)k * DD_FG_REC + DD_FG_FLAGGED];
    n = wave_sum(n);
    if (lane == 0) wave_cnt[wave] = n;
    __syncthreads();
    if (tid == 0) {
      int32_t all = 0;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) all += wave_cnt[w];
      a.flags[0] = all;
    }
  }
}

// ---- the loss ---------------------------------------------------------------------------------------------------------

template <typename T>
struct LossArgs {
  const T* pred;
  const T* target;
  const float* heat;
  T* grad;
  float* partials;
  int64_t count;
  int32_t chw, hw;
  float scale;
};

// the workgroup's sum in a fixed order: the lane's serial sum, the butterfly of its wave, waves 0..3 one after the other
__device__ __forceinline__ float group_sum(float acc, float* s_w) {
  const int tid = threadIdx.x;
  acc = wave_sum(acc);
  if ((tid & (DD_WAVE - 1)) == 0) s_w[tid / DD_WAVE] = acc;
  __syncthreads();
  float all = s_w[0];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) all += s_w[w];
  return all;
}

template <typename T>
__global__ __launch_bounds__(kThreads)
void dd_fgm_loss_partials_kernel(LossArgs<T> a) {
  __shared__ float s_w[kWaves];
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  float acc = 0.0f;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < a.count; i += stride) {
    float w = 1.0f;
    if (a.heat) {
      const int64_t v = i / a.chw;
      w = 1.0f + a.heat[v * a.hw + (int32_t)(i - v * a.chw) % a.hw];
    }
    const float d = (float)a.pred[i] - (float)a.target[i];
    acc += d * d * w;
    if (a.grad) a.grad[i] = (T)(d * (w * a.scale));
  }
  const float all = group_sum(acc, s_w);
  if (threadIdx.x == 0) a.partials[blockIdx.x] = all;
}

__global__ __launch_bounds__(kThreads)
void dd_fgm_loss_final_kernel(const float* partials, int32_t groups, float count, float* loss) {
  __shared__ float s_w[kWaves];
  float acc = 0.0f;
  for (int32_t i = threadIdx.x; i < groups; i += kThreads) acc += partials[i];
  const float all = group_sum(acc, s_w);
  if (threadIdx.x == 0) loss[0] = all / count;
}

int32_t loss_groups(int64_t count) {
  const int64_t g = (count + DD_FGM_LOSS_PER_GROUP - 1) / DD_FGM_LOSS_PER_GROUP;
  return (int32_t)(g < 1 ? 1 : (g > DD_FGM_LOSS_MAX_GROUPS ? DD_FGM_LOSS_MAX_GROUPS : g));
}

bool misaligned(const void* p, uintptr_t al) { return (reinterpret_cast<uintptr_t>(p) & (al - 1)) != 0; }

}  // namespace

extern "C" int64_t dd_fgm_workspace_bytes(int32_t total) {
  if (total < 0 || total > DD_FGM_MAX_BOXES) return -1;
  return (int64_t)(total > 0 ? total : 1) * DD_FG_REC * (int64_t)sizeof(int32_t);
}

extern "C" int dd_fgm_mask(const float* corners, const uint8_t* masks, const float* lidar2image, int32_t views, int32_t m,
                           int32_t points, int32_t width, int32_t height, int32_t width_out, int32_t height_out, double sx,
                           double sy, void* workspace, int64_t workspace_bytes, float* out, int32_t* flags,
                           dd_stream_t stream) {
  if (!workspace || !out || !flags) return DD_ERR_BAD_ARG;
  if (views <= 0 || m < 0) return DD_ERR_BAD_ARG;
  if (m > 0 && (!corners || !masks || !lidar2image)) return DD_ERR_BAD_ARG;
  if (points < 1 || points > DD_FG_MAX_POINTS) return DD_ERR_BAD_ARG;
  if (width < 1 || height < 1 || (int64_t)width * height > DD_FGM_MAX_PIXELS) return DD_ERR_BAD_ARG;
  if (width_out < 1 || height_out < 1 || width_out > width || height_out > height) return DD_ERR_BAD_ARG;
  if ((width - width_out) & 1) return DD_ERR_BAD_ARG;                  // hd_crop takes the same number of columns off each side
  if (!(isfinite(sx) && isfinite(sy))) return DD_ERR_BAD_ARG;
  if (misaligned(corners, 4) || misaligned(lidar2image, 4) || misaligned(workspace, 16) || misaligned(out, 4) ||
      misaligned(flags, 4))
    return DD_ERR_BAD_ARG;
  if (views > 65535 || (int64_t)views * m > DD_FGM_MAX_BOXES) return DD_ERR_UNSUPPORTED;
  const int32_t total = views * m;
  const int64_t need = dd_fgm_workspace_bytes(total);
  if (need < 0 || workspace_bytes < need) return DD_ERR_BAD_ARG;
  RecordArgs r;
  r.corners = corners; r.masks = masks; r.l2i = lidar2image; r.rec = static_cast<int32_t*>(workspace);
  r.sx = sx; r.sy = sy;
  r.total = total; r.m = m; r.np = points; r.width = width; r.height = height;
  MaskArgs a;
  a.rec = r.rec; a.out = out; a.flags = flags;
  a.total = total; a.m = m; a.width = width; a.height = height; a.wo = width_out; a.ho = height_out;
  dd_clear_error();
  if (total > 0)
    hipLaunchKernelGGL(dd_fgm_box_records_kernel, dim3((unsigned)((total + kWaves - 1) / kWaves)), dim3(kThreads), 0,
                       dd_stream(stream), r);
  const unsigned tiles = (unsigned)((width_out * height_out + kThreads - 1) / kThreads);
  hipLaunchKernelGGL(dd_fgm_mask_kernel, dim3(tiles, (unsigned)views), dim3(kThreads), 0, dd_stream(stream), a);
  return dd_check_launch();
}

extern "C" int64_t dd_fgm_loss_workspace_bytes(int64_t count) {
  if (count < 1 || count > DD_FGM_LOSS_MAX_COUNT) return -1;
  return (int64_t)loss_groups(count) * (int64_t)sizeof(float);
}

extern "C" int dd_fgm_loss(const void* pred, const void* target, const float* heat, void* grad, float* loss, void* workspace,
                           int64_t workspace_bytes, int64_t views, int32_t channels, int32_t pixels, int32_t pred_dtype,
                           dd_stream_t stream) {
  if (!pred || !target || !loss || !workspace) return DD_ERR_BAD_ARG;
  if (views < 1 || channels < 1 || pixels < 1) return DD_ERR_BAD_ARG;
  if (pred_dtype != DD_F16 && pred_dtype != DD_BF16 && pred_dtype != DD_F32) return DD_ERR_BAD_ARG;
  const uintptr_t al = pred_dtype == DD_F32 ? 4 : 2;
  if (misaligned(pred, al) || misaligned(target, al) || misaligned(grad, al) || misaligned(heat, 4) || misaligned(loss, 4) ||
      misaligned(workspace, 4))
    return DD_ERR_BAD_ARG;
  if (views > DD_FGM_LOSS_MAX_COUNT || (int64_t)channels * pixels > DD_FGM_LOSS_MAX_COUNT ||
      views * ((int64_t)channels * pixels) > DD_FGM_LOSS_MAX_COUNT)
    return DD_ERR_UNSUPPORTED;
  const int64_t count = views * ((int64_t)channels * pixels);
  const int64_t need = dd_fgm_loss_workspace_bytes(count);
  if (need < 0 || workspace_bytes < need) return DD_ERR_BAD_ARG;
  const int32_t groups = loss_groups(count);
  float* partials = static_cast<float*>(workspace);
  dd_clear_error();
  const int rc = dd_dispatch32(pred_dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    LossArgs<T> a;
    a.pred = static_cast<const T*>(pred); a.target = static_cast<const T*>(target); a.heat = heat;
    a.grad = static_cast<T*>(grad); a.partials = partials;
    a.count = count; a.chw = channels * pixels; a.hw = pixels;
    a.scale = (float)(2.0 / (double)count);
    hipLaunchKernelGGL(dd_fgm_loss_partials_kernel<T>, dim3((unsigned)groups), dim3(kThreads), 0, dd_stream(stream), a);
    return DD_OK;
  });
  if (rc != DD_OK) return rc;
  hipLaunchKernelGGL(dd_fgm_loss_final_kernel, dim3(1), dim3(kThreads), 0, dd_stream(stream), partials, groups, (float)count,
                     loss);
  return dd_check_launch();
}
