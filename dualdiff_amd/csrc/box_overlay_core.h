// Box output, the arithmetic core: what csrc/box_overlay.hip computes per box and per pixel — the projection of one box
// into one view (its eight integer points, or "not drawn") and the membership of a pixel in one thin line — as plain
// functions that compile for the device and for the host.  The stand-alone host program tools/box_overlay_hostcheck.cpp
// runs the same functions in the kernels' sequence under the address and undefined-behaviour sanitizers, so that the
// integer ranges stated below are checked without a GPU.
//
// Geometry (include/dualdiff_hip.h: dd_box_edges has the whole rule):
//   (x, y, z) = rows 0..2 of the view's matrix, promoted to double, times (corner promoted to double, 1.0), summed by
//   fused multiply-adds from the translation column on, as dd_box_views does; a box is drawn iff all eight z > 0;
//   zc = clip(z, 1e-5, 1e5), u = x / zc, v = y / zc in IEEE double; the integer point is u, v truncated toward zero, a
//   value beyond +-2^29 (or a NaN) saturated there.
// The line, from (x0, y0) to (x1, y1), is PIL's thin line (ImageDraw.line, width 1) in closed form: with dx = |x1 - x0|,
// dy = |y1 - y0|, xs, ys = +-1 (+1 when the end is >= the start), step i in [0, max(dx, dy)]:
//   dx >= dy:  (x0 + xs i, y0 + ys floor((2 dy i + dx) / (2 dx)))      (dx == 0: the single pixel (x0, y0))
//   else:      (x0 + xs floor((2 dx i + dy) / (2 dy)), y0 + ys i)
// It is not symmetric in its end points.  The membership test has no division: floor(a / b) == k  <=>  b k <= a < b (k +
// 1) for b > 0.  With every end point within +-2^29 and the pixel in [0, 2^15), dx, dy, i, k <= 2^30 + 2^15, so every
// product below is under 2^62.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define DD_BO_HD __host__ __device__ __forceinline__
#else
#define DD_BO_HD inline
#endif

#define DD_BO_SAT (1 << 29)                    // the greatest magnitude of an integer point
#define DD_BO_MAX_BOXES 1024                   // boxes of one scene (include/dualdiff_hip.h: DD_BOX_EDGES_MAX)

// flag bits (include/dualdiff_hip.h: DD_BOX_FLAG_*)
#define DD_BO_FLAG_LABEL 1                     // a label outside [-n_classes, n_classes)
#define DD_BO_FLAG_SATURATED 2                 // a coordinate beyond +-2^29
#define DD_BO_FLAG_CAP 4                       // a view kept more than cap boxes

// the twelve edges of a box in draw order, each from its first corner to its second
#define DD_BO_EDGES 12
#define DD_BO_EDGE_A(e) ((0x652443311000ull >> (4 * (e))) & 15)      // 0 0 0 1 1 3 3 4 4 2 5 6, edge 0 in the low nibble
#define DD_BO_EDGE_B(e) ((0x766757252431ull >> (4 * (e))) & 15)      // 1 3 4 2 5 2 7 5 7 6 6 7

// np.clip: a NaN stays a NaN
DD_BO_HD double dd_bo_clip(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

// one row of the matrix times (x, y, z, 1)
DD_BO_HD double dd_bo_row(const double* m, double x, double y, double z) {
  return fma(z, m[2], fma(y, m[1], fma(x, m[0], m[3])));
}

// The palette index of a label, as Python indexes: [-n, n) -> [0, n); -1 for any other label.
DD_BO_HD int32_t dd_bo_class(int64_t label, int32_t n) {
  if (label >= 0 && label < n) return (int32_t)label;
  if (label < 0 && label >= -(int64_t)n) return (int32_t)(label + n);
  return -1;
}

// G2: the least z of the eight corners when all of them are > 0, else a value <= 0 or a NaN ("not drawn": test with
// dd_bo_drawn).  c: 24 floats, m: rows 0..2 of the matrix (12 doubles, row-major with a row length of 4).
DD_BO_HD double dd_bo_min_z(const float* c, const double* m) {
  double lo = 0.0;
  bool all = true;
  for (int k = 0; k < 8; ++k) {
    const double z = dd_bo_row(m + 8, (double)c[3 * k], (double)c[3 * k + 1], (double)c[3 * k + 2]);
    all = all && z > 0.0;
    lo = (k == 0 || z < lo) ? z : lo;
  }
  return all ? lo : -1.0;
}
DD_BO_HD bool dd_bo_drawn(double min_z) { return min_z > 0.0; }

// G4: truncation toward zero, saturated; *sat is set when the value lay beyond +-2^29 (or was a NaN: then -2^29)
DD_BO_HD int32_t dd_bo_trunc(double u, bool* sat) {
  if (!(u >= -(double)DD_BO_SAT)) { *sat = true; return -DD_BO_SAT; }
  if (u > (double)DD_BO_SAT) { *sat = true; return DD_BO_SAT; }
  return (int32_t)u;
}

// The eight integer points of a drawn box: pts[2 k] = x, pts[2 k + 1] = y of corner k.  -> whether any saturated.
DD_BO_HD bool dd_bo_points(const float* c, const double* m, int32_t* pts) {
  bool sat = false;
  for (int k = 0; k < 8; ++k) {
    const double x = (double)c[3 * k], y = (double)c[3 * k + 1], z = (double)c[3 * k + 2];
    const double zc = dd_bo_clip(dd_bo_row(m + 8, x, y, z), 1e-5, 1e5);
    pts[2 * k] = dd_bo_trunc(dd_bo_row(m, x, y, z) / zc, &sat);
    pts[2 * k + 1] = dd_bo_trunc(dd_bo_row(m + 4, x, y, z) / zc, &sat);
  }
  return sat;
}

// G3: whether box j (key kj) is drawn before box i (key ki): the greater least z first, ties to the lower index
DD_BO_HD bool dd_bo_before(double kj, int j, double ki, int i) { return kj > ki || (kj == ki && j < i); }

// Whether pixel (px, py) lies on the line from (x0, y0) to (x1, y1); every argument within the ranges stated above.
DD_BO_HD bool dd_bo_on_line(int32_t px, int32_t py, int32_t x0, int32_t y0, int32_t x1, int32_t y1) {
  const int32_t dx = x1 >= x0 ? x1 - x0 : x0 - x1;                         // differences fit 32 bits: <= 2^30 + 2^15
  const int32_t dy = y1 >= y0 ? y1 - y0 : y0 - y1;
  const int32_t ix = x1 >= x0 ? px - x0 : x0 - px;                         // steps along x from the start
  const int32_t iy = y1 >= y0 ? py - y0 : y0 - py;
  if (ix < 0 || ix > dx || iy < 0 || iy > dy) return false;                // outside the line's own bounding box
  if (dx >= dy) {
    if (dx == 0) return true;                                              // ix == iy == 0 here
    const int64_t a = 2 * (int64_t)dy * ix + dx, b = 2 * (int64_t)dx;
    return b * iy <= a && a < b * (iy + 1);
  }
  const int64_t a = 2 * (int64_t)dx * iy + dy, b = 2 * (int64_t)dy;
  return b * ix <= a && a < b * (ix + 1);
}

// Whether pixel (px, py) lies on any of the twelve edges of the box with points pts[16].
DD_BO_HD bool dd_bo_on_box(int32_t px, int32_t py, const int32_t* pts) {
  bool hit = false;
  for (int e = 0; e < DD_BO_EDGES; ++e) {
    const int a = (int)DD_BO_EDGE_A(e), b = (int)DD_BO_EDGE_B(e);
    hit = hit || dd_bo_on_line(px, py, pts[2 * a], pts[2 * a + 1], pts[2 * b], pts[2 * b + 1]);
  }
  return hit;
}

// G8: the alpha of a drawn colour
DD_BO_HD uint32_t dd_bo_alpha(uint32_t r, uint32_t g, uint32_t b) { return (r | g | b) ? 255u : 0u; }
