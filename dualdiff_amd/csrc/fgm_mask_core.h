// FGM loss mask, the arithmetic core: what csrc/fgm_mask.hip computes per box corner (the float64 projection, the clip, the
// scale, the truncation), per box (the polygon: the strict convex hull, or the surviving points in corner order) and per
// pixel (matplotlib's crossing rule in int64), as plain functions that compile for the device and for the host.  The
// stand-alone host program tools/fgm_mask_hostcheck.cpp runs them in the kernels' sequence, and tests/test_fgm_mask_cpu.py
// compares its maps with the numpy restatement (tests/fgm_reference.py) without a GPU.
//
// What is restated is `process_one_instance_test` of the reference (magicdrive/networks/utils.py:107-163):
//   coords = [x, y, z, 1] @ T.T in float64 (corners fp32, T the float32 lidar2image), every product and sum one IEEE
//   operation, summed k = 0..3; points with z <= 0 dropped; z clipped to [1e-5, 1e5]; x / z * (W / 1600), y / z * (H / 900);
//   truncated toward zero; scipy's ConvexHull(coords).vertices where it succeeds — the strict hull, counter-clockwise in
//   (x, y) — and the points as they are where it raises (fewer than three hull vertices); matplotlib's
//   Polygon(coords, closed=True).contains_point((tx, ty), radius=0) per pixel: the even-odd rule over the edges v0 -> v1 of
//   the closed ring with f = (vy >= ty): where f0 != f1 the edge toggles iff
//   ((v1y - ty) * (v0x - v1x) >= (v1x - tx) * (v0y - v1y)) == f1.
//
// Integer ranges: a truncated coordinate is at most 2^25 in magnitude (DD_FG_BOUND; a box beyond is not painted but
// counted), a pixel coordinate is in [0, 2^20), so every difference is below 2^27, every product below 2^54 and every
// difference of two products below 2^55: exact in int64 — and, below 2^53, equal to the reference's float64 products.
#pragma once
#include "bev_map_core.h"                       // DD_BM_HD, the single-operation float64 helpers (DD_BM_NO_CONTRACT)

#define DD_FG_BOUND (1 << 25)                   // the greatest magnitude of a truncated coordinate
#define DD_FG_MAX_POINTS 8
#define DD_FG_REC 24                            // int32 words of one box record (96 bytes, a multiple of 16)
// word offsets in a record
#define DD_FG_RING 0                            // 8 vertices x (x, y)
#define DD_FG_NV 16                             // vertices of the ring, 0..8
#define DD_FG_FLAGGED 17                        // 1: an unsupported box (not painted)
#define DD_FG_WEIGHT 18                         // float32(1.0 - area / (W * H)) as bits
#define DD_FG_AREA 19                           // pixels of the uncropped grid the ring paints
#define DD_FG_BBOX 20                           // x0, x1, y0, y1 of the ring (x0 > x1: the box paints nothing)

// point status
#define DD_FG_DROPPED 0                         // z <= 0
#define DD_FG_KEPT 1
#define DD_FG_BAD 2                             // not finite, or beyond DD_FG_BOUND: the box is unsupported

// One corner c = (x, y, z) through T (16 floats, row-major) -> status, and the truncated pixel where kept.
DD_BM_HD int dd_fg_point(const float* c, const float* t, double sx, double sy, int32_t* px, int32_t* py) {
  const double v0 = (double)c[0], v1 = (double)c[1], v2 = (double)c[2];
  double r[3];
  for (int row = 0; row < 3; ++row) {
    double acc = dd_bm_dmul(v0, (double)t[4 * row]);
    acc = dd_bm_dadd(acc, dd_bm_dmul(v1, (double)t[4 * row + 1]));
    acc = dd_bm_dadd(acc, dd_bm_dmul(v2, (double)t[4 * row + 2]));
    acc = dd_bm_dadd(acc, dd_bm_dmul(1.0, (double)t[4 * row + 3]));
    r[row] = acc;
  }
  if (!(isfinite(r[0]) && isfinite(r[1]) && isfinite(r[2]))) return DD_FG_BAD;
  if (!(r[2] > 0.0)) return DD_FG_DROPPED;
  double z = r[2];
  z = z < 1e-5 ? 1e-5 : z;
  z = z > 1e5 ? 1e5 : z;
  const double x = dd_bm_dmul(dd_bm_ddiv(r[0], z), sx), y = dd_bm_dmul(dd_bm_ddiv(r[1], z), sy);
  if (!(isfinite(x) && isfinite(y))) return DD_FG_BAD;
  const double tx = trunc(x), ty = trunc(y);
  if (fabs(tx) > (double)DD_FG_BOUND || fabs(ty) > (double)DD_FG_BOUND) return DD_FG_BAD;
  *px = (int32_t)tx;
  *py = (int32_t)ty;
  return DD_FG_KEPT;
}

DD_BM_HD int64_t dd_fg_cross(const int32_t* o, const int32_t* a, const int32_t* b) {
  return ((int64_t)a[0] - o[0]) * ((int64_t)b[1] - o[1]) - ((int64_t)a[1] - o[1]) * ((int64_t)b[0] - o[0]);
}

// The box's record from its points' pixels (pts: P x (x, y)) and statuses: ring, vertex count, bounding box, flagged.
// masked = 0: an empty record.  Weight and area are the caller's (they need the pixel count).  work: DD_FG_WORK words of
// the caller's (LDS on the device, so that the indexed arrays of the sort and the chain do not become scratch memory).
#define DD_FG_WORK (8 * DD_FG_MAX_POINTS)
DD_BM_HD void dd_fg_record(const int32_t* pts, const int32_t* status, int32_t n_points, int32_t masked, int32_t* work,
                           int32_t* rec) {
  for (int i = 0; i < DD_FG_REC; ++i) rec[i] = 0;
  rec[DD_FG_BBOX] = 1;                                                   // x0 > x1
  if (!masked) return;
  int32_t (*p)[2] = reinterpret_cast<int32_t (*)[2]>(work);                          // the kept points, corner order
  int32_t (*s)[2] = reinterpret_cast<int32_t (*)[2]>(work + 2 * DD_FG_MAX_POINTS);    // sorted
  int32_t (*h)[2] = reinterpret_cast<int32_t (*)[2]>(work + 4 * DD_FG_MAX_POINTS);    // the chain, at most 2 n entries
  int n = 0;
  for (int i = 0; i < n_points; ++i) {
    if (status[i] == DD_FG_BAD) { rec[DD_FG_FLAGGED] = 1; return; }
    if (status[i] == DD_FG_KEPT) { p[n][0] = pts[2 * i]; p[n][1] = pts[2 * i + 1]; ++n; }
  }
  if (n == 0) return;
  for (int i = 0; i < n; ++i) {                                          // insertion sort by (x, y)
    int j = i;
    for (; j > 0 && (s[j - 1][0] > p[i][0] || (s[j - 1][0] == p[i][0] && s[j - 1][1] > p[i][1])); --j) {
      s[j][0] = s[j - 1][0]; s[j][1] = s[j - 1][1];
    }
    s[j][0] = p[i][0]; s[j][1] = p[i][1];
  }
  int k = 0;                                                             // monotone chain, strict: <= 0 pops
  if (n >= 2) {
    for (int i = 0; i < n; ++i) {
      while (k >= 2 && dd_fg_cross(h[k - 2], h[k - 1], s[i]) <= 0) --k;
      h[k][0] = s[i][0]; h[k][1] = s[i][1]; ++k;
    }
    const int t = k + 1;
    for (int i = n - 2; i >= 0; --i) {
      while (k >= t && dd_fg_cross(h[k - 2], h[k - 1], s[i]) <= 0) --k;
      h[k][0] = s[i][0]; h[k][1] = s[i][1]; ++k;
    }
    --k;
  }
  int nv;
  if (k >= 3) {
    nv = k;
    for (int i = 0; i < nv; ++i) { rec[DD_FG_RING + 2 * i] = h[i][0]; rec[DD_FG_RING + 2 * i + 1] = h[i][1]; }
  } else {                                                               // ConvexHull raised: the points in corner order
    nv = n;
    for (int i = 0; i < nv; ++i) { rec[DD_FG_RING + 2 * i] = p[i][0]; rec[DD_FG_RING + 2 * i + 1] = p[i][1]; }
  }
  rec[DD_FG_NV] = nv;
  int32_t x0 = rec[DD_FG_RING], x1 = x0, y0 = rec[DD_FG_RING + 1], y1 = y0;
  for (int i = 1; i < nv; ++i) {
    x0 = dd_bm_min(x0, rec[DD_FG_RING + 2 * i]); x1 = dd_bm_max(x1, rec[DD_FG_RING + 2 * i]);
    y0 = dd_bm_min(y0, rec[DD_FG_RING + 2 * i + 1]); y1 = dd_bm_max(y1, rec[DD_FG_RING + 2 * i + 1]);
  }
  rec[DD_FG_BBOX] = x0; rec[DD_FG_BBOX + 1] = x1; rec[DD_FG_BBOX + 2] = y0; rec[DD_FG_BBOX + 3] = y1;
}

// Does the ring of the record paint pixel (tx, ty)?  A pixel outside the ring's bounding box is never painted: an edge
// toggles only where ty lies in its y range, and left of every vertex all crossing edges of a closed ring toggle (an even
// number), right of every vertex none does.
DD_BM_HD bool dd_fg_inside(const int32_t* rec, int32_t tx, int32_t ty) {
  const int32_t nv = rec[DD_FG_NV];
  bool in = false;
  for (int i = 0; i < DD_FG_MAX_POINTS; ++i) {
    if (i >= nv) break;
    const int j = i + 1 < nv ? i + 1 : 0;
    const int64_t x0 = rec[DD_FG_RING + 2 * i], y0 = rec[DD_FG_RING + 2 * i + 1];
    const int64_t x1 = rec[DD_FG_RING + 2 * j], y1 = rec[DD_FG_RING + 2 * j + 1];
    const bool f0 = y0 >= ty, f1 = y1 >= ty;
    if (f0 != f1 && (((y1 - ty) * (x0 - x1) >= (x1 - tx) * (y0 - y1)) == f1)) in = !in;
  }
  return in;
}

// float32(1.0 - area / (W * H)), the division and the subtraction in float64 (utils.py:161)
DD_BM_HD float dd_fg_weight(int32_t area, int32_t width, int32_t height) {
  return (float)dd_bm_dadd(1.0, -dd_bm_ddiv((double)area, (double)((int64_t)width * height)));
}

// The part of the ring's bounding box on the W x H grid: x0, x1, y0, y1 (x0 > x1: none).
DD_BM_HD void dd_fg_clip(const int32_t* rec, int32_t width, int32_t height, int32_t* c) {
  c[0] = dd_bm_max(rec[DD_FG_BBOX], 0); c[1] = dd_bm_min(rec[DD_FG_BBOX + 1], width - 1);
  c[2] = dd_bm_max(rec[DD_FG_BBOX + 2], 0); c[3] = dd_bm_min(rec[DD_FG_BBOX + 3], height - 1);
  if (rec[DD_FG_BBOX] > rec[DD_FG_BBOX + 1] || c[2] > c[3]) { c[0] = 1; c[1] = 0; }
}
