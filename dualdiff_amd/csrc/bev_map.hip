// Map input: the BEV object layers and aux channels of the reference's LoadBEVSegmentationM (magicdrive/dataset/
// pipeline.py: _project_dynamic_bbox :176-200, _get_dynamic_aux_bbox :88-152, the transposes of :215 and :173) and
// one_hot_decode (dataset/pipeline_utils.py:34-49), from the 3D boxes and the static layers, in two launches.  The
// arithmetic — the float64 projection, np.round, PIL's polygon fill, the aux values — is csrc/bev_map_core.h, which also
// compiles for the host.
//
//  * dd_bev_box_records: one lane per box.  It projects and rounds the bottom rectangle, builds PIL's edge list (the
//    table edges with their float32 slopes, the horizontal spans, the clipped scan range), the vertices' bounding box,
//    the object layer of the label and the eight aux values, and stores the box's 208-byte record in the workspace.
//    Everything that does not depend on the pixel is computed here, once per box, the float64 work included.
//  * dd_bev_map_layers: pixel-major.  A workgroup owns a tile of 16 x 16 pixels of one sample, one pixel per lane, lanes
//    along the LAST index of the transposed outputs (the row while drawing), so that a tile row is 16 consecutive bytes
//    of a mask plane and 64 consecutive bytes of an aux plane.  The scene's boxes go 256 at a time: one lane per box tests
//    the box's bounding box against the tile, a ballot compacts the survivors in input order into LDS, and every pixel
//    evaluates PIL's scan line of its own row for each survivor (at most four edges, a list of at most eight crossings in
//    registers) — the record is read through the scalar cache, its address being uniform.  A pixel ORs the layers of the
//    boxes that cover it and remembers the LAST covering box in input order, whose aux values it writes.  Per-row span
//    lists in a workspace (S x 8 words per box) would save the scan-line arithmetic and cost 6.4 KB written and read back
//    per box at S = 200; with the tile rejection a pixel sees a handful of boxes, and the registers win on both counts.
//    No atomics: the number of boxes of the family that is not drawn is summed by workgroup (0, 0, 0) from the records.
#include "dd_common.h"
#include "bev_map_core.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / DD_WAVE;
constexpr int kTile = 16;
static_assert(kTile * kTile == kThreads, "one pixel per lane");
typedef int32_t i32x4 __attribute__((ext_vector_type(4)));

struct RecordArgs {
  const float* corners;
  const float* bottom_center;
  const float* height;
  const float* visibility;
  const int64_t* labels;
  int32_t* rec;
  double sx, ox, sy, oy;
  int32_t total, size, nd;
};

struct LayerArgs {
  const uint8_t* stat_u8;
  const int32_t* stat_bits;
  const int32_t* rec;
  const int32_t* offsets;
  uint8_t* masks;
  float* aux;
  int32_t* flags;
  int32_t total, size, ns, nd, aux_sel, aux_ch;
};

__global__ __launch_bounds__(kThreads)
void dd_bev_box_records_kernel(RecordArgs a) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= a.total) return;
  float c[24], bc[3];
#pragma unroll
  for (int k = 0; k < 24; ++k) c[k] = a.corners[i * 24 + k];
#pragma unroll
  for (int k = 0; k < 3; ++k) bc[k] = a.bottom_center[i * 3 + k];
  int32_t rec[DD_BM_REC];
#pragma unroll
  for (int k = 0; k < DD_BM_REC; ++k) rec[k] = 0;
  dd_bm_box(c, bc, a.height[i], a.visibility[i], a.labels[i], a.nd, a.sx, a.ox, a.sy, a.oy, a.size, rec);
  i32x4* out = reinterpret_cast<i32x4*>(a.rec + i * DD_BM_REC);
#pragma unroll
  for (int k = 0; k < DD_BM_REC / 4; ++k) {
    i32x4 v;
    v[0] = rec[4 * k]; v[1] = rec[4 * k + 1]; v[2] = rec[4 * k + 2]; v[3] = rec[4 * k + 3];
    out[k] = v;
  }
}

__global__ __launch_bounds__(kThreads)
void dd_bev_map_layers_kernel(LayerArgs a) {
  __shared__ int32_t list[kThreads];
  __shared__ int32_t wave_cnt[kWaves];
  const int tid = threadIdx.x, lane = tid & (DD_WAVE - 1), wave = tid / DD_WAVE;
  const int32_t s = a.size;
  const int32_t j0 = blockIdx.x * kTile, i0 = blockIdx.y * kTile;
  const int32_t j = j0 + (tid & (kTile - 1));          // the last index of the outputs: the row while drawing
  const int32_t i = i0 + tid / kTile;                  // the index before it: the column while drawing
  const int64_t smp = blockIdx.z;
  const bool valid = i < s && j < s;
  int32_t lo = a.offsets[smp], hi = a.offsets[smp + 1];
  lo = min(max(lo, 0), a.total);
  hi = min(max(hi, lo), a.total);
  uint32_t dyn = 0;
  int32_t last = -1;
  for (int32_t base = lo; base < hi; base += kThreads) {
    const int32_t idx = base + tid;
    bool keep = false;
    if (idx < hi) {
      const int32_t* r = a.rec + (int64_t)idx * DD_BM_REC + DD_BM_BBOX;
      const i32x4 bb = *reinterpret_cast<const i32x4*>(r);
      keep = bb[0] <= bb[1] && bb[1] >= i0 && bb[0] <= i0 + kTile - 1 && bb[3] >= j0 && bb[2] <= j0 + kTile - 1;
    }
    const uint64_t m = __ballot(keep);
    if (lane == 0) wave_cnt[wave] = __popcll(m);
    __syncthreads();
    int32_t before = 0, kept = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      const int32_t n = wave_cnt[w];
      if (w < wave) before += n;
      kept += n;
    }
    if (keep) list[before + __popcll(m & ((1ull << lane) - 1ull))] = idx;
    __syncthreads();
    for (int32_t k = 0; k < kept; ++k) {
      const int32_t bi = __builtin_amdgcn_readfirstlane(list[k]);
      const int32_t* r = a.rec + (int64_t)bi * DD_BM_REC;
      if (valid && dd_bm_covers(r, i, j)) {
        last = bi;                                     // survivors are in input order
        const int32_t lab = r[DD_BM_LABEL];
        if (lab >= 0) dyn |= 1u << lab;
      }
    }
    __syncthreads();
  }
  if (valid) {
    const int64_t plane = (int64_t)s * s, pix = (int64_t)i * s + j;
    uint8_t* mo = a.masks + smp * (a.ns + a.nd) * plane + pix;
    if (a.stat_bits) {                                 // one_hot_decode: layer c = bit c
      const uint32_t v = (uint32_t)a.stat_bits[smp * plane + pix];
      for (int c = 0; c < a.ns; ++c) mo[c * plane] = (uint8_t)((v >> c) & 1u);
    } else {
      const uint8_t* si = a.stat_u8 + smp * a.ns * plane + pix;
      for (int c = 0; c < a.ns; ++c) mo[c * plane] = si[c * plane];
    }
    for (int c = 0; c < a.nd; ++c) mo[(a.ns + c) * plane] = (uint8_t)((dyn >> c) & 1u);
    if (a.aux) {
      float v[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = 0.0f;
      if (last >= 0) {
        const int32_t* r = a.rec + (int64_t)last * DD_BM_REC;
        double cx, cy;
        memcpy(&cx, r + DD_BM_CENTRE, 8);
        memcpy(&cy, r + DD_BM_CENTRE + 2, 8);
        v[0] = dd_bm_bits_f(r[DD_BM_AUX]);
        v[1] = (float)dd_bm_dadd((double)i, -cx);      // coords (float32 x, y) - centre in float64 (:132)
        v[2] = (float)dd_bm_dadd((double)j, -cy);
#pragma unroll
        for (int k = 0; k < 5; ++k) v[3 + k] = dd_bm_bits_f(r[DD_BM_AUX + 1 + k]);
      }
      float* ao = a.aux + smp * a.aux_ch * plane + pix;
      int ch = 0;
      if (a.aux_sel & 1) ao[(ch++) * plane] = v[0];
      if (a.aux_sel & 2) { ao[ch * plane] = v[1]; ao[(ch + 1) * plane] = v[2]; ch += 2; }
      if (a.aux_sel & 4) {
#pragma unroll
        for (int k = 0; k < 4; ++k) ao[(ch + k) * plane] = v[3 + k];
        ch += 4;
      }
      if (a.aux_sel & 8) ao[ch * plane] = v[7];
    }
  }
  if (blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0) {
    int32_t n = 0;
    for (int32_t k = tid; k < a.total; k += kThreads) n += a.rec[(int64_t)k * DD_BM_REC + DD_BM_FLAGGED];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    __syncthreads();
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

}  // namespace

extern "C" int64_t dd_bev_map_workspace_bytes(int32_t total) {
  if (total < 0 || total > DD_BEV_MAP_MAX_BOXES) return -1;
  return (int64_t)(total > 0 ? total : 1) * DD_BM_REC * (int64_t)sizeof(int32_t);
}

extern "C" int dd_bev_map_layers(const void* stat, int32_t static_bits, const float* corners, const float* bottom_center,
                                 const float* height, const float* visibility, const int64_t* labels,
                                 const int32_t* offsets, int32_t total, int32_t b, int32_t size, int32_t ns, int32_t nd,
                                 int32_t aux_sel, double sx, double ox, double sy, double oy, void* workspace,
                                 int64_t workspace_bytes, uint8_t* masks, float* aux, int32_t* flags, dd_stream_t stream) {
  if (!offsets || !workspace || !masks || !flags) return DD_ERR_BAD_ARG;
  if (static_bits != 0 && static_bits != 1) return DD_ERR_BAD_ARG;
  if (total < 0 || b <= 0 || size <= 0 || ns < 0 || nd < 0 || ns + nd <= 0) return DD_ERR_BAD_ARG;
  if (ns + nd > DD_BEV_MAP_MAX_LAYERS || aux_sel < 0 || aux_sel > 15) return DD_ERR_BAD_ARG;
  if (ns > 0 && !stat) return DD_ERR_BAD_ARG;
  if ((aux_sel != 0) != (aux != nullptr)) return DD_ERR_BAD_ARG;
  if (total > 0 && (!corners || !bottom_center || !height || !visibility || !labels)) return DD_ERR_BAD_ARG;
  if (!(isfinite(sx) && isfinite(ox) && isfinite(sy) && isfinite(oy))) return DD_ERR_BAD_ARG;
  auto mis = [](const void* p, uintptr_t al) { return (reinterpret_cast<uintptr_t>(p) & (al - 1)) != 0; };
  if (mis(corners, 4) || mis(bottom_center, 4) || mis(height, 4) || mis(visibility, 4) || mis(labels, 8) ||
      mis(offsets, 4) || mis(workspace, 16) || mis(aux, 4) || mis(flags, 4) || (static_bits && mis(stat, 4)))
    return DD_ERR_BAD_ARG;
  if (total > DD_BEV_MAP_MAX_BOXES || size > DD_BEV_MAP_MAX_SIZE || b > 65535) return DD_ERR_UNSUPPORTED;
  const int64_t need = dd_bev_map_workspace_bytes(total);
  if (need < 0 || workspace_bytes < need) return DD_ERR_BAD_ARG;
  int ch = 0;
  if (aux_sel & 1) ch += 1;
  if (aux_sel & 2) ch += 2;
  if (aux_sel & 4) ch += 4;
  if (aux_sel & 8) ch += 1;
  RecordArgs r;
  r.corners = corners; r.bottom_center = bottom_center; r.height = height; r.visibility = visibility; r.labels = labels;
  r.rec = static_cast<int32_t*>(workspace);
  r.sx = sx; r.ox = ox; r.sy = sy; r.oy = oy;
  r.total = total; r.size = size; r.nd = nd;
  LayerArgs a;
  a.stat_u8 = static_bits ? nullptr : static_cast<const uint8_t*>(stat);
  a.stat_bits = static_bits ? static_cast<const int32_t*>(stat) : nullptr;
  a.rec = r.rec; a.offsets = offsets; a.masks = masks; a.aux = aux; a.flags = flags;
  a.total = total; a.size = size; a.ns = ns; a.nd = nd; a.aux_sel = aux_sel; a.aux_ch = ch;
  if (ns == 0) a.stat_bits = nullptr;                 // nothing is read from stat
  dd_clear_error();
  if (total > 0)
    hipLaunchKernelGGL(dd_bev_box_records_kernel, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                       dd_stream(stream), r);
  const unsigned tiles = (unsigned)((size + kTile - 1) / kTile);
  hipLaunchKernelGGL(dd_bev_map_layers_kernel, dim3(tiles, tiles, (unsigned)b), dim3(kThreads), 0, dd_stream(stream), a);
  return dd_check_launch();
}
