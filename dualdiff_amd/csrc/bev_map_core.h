// Map input, the arithmetic core: what csrc/bev_map.hip computes per box (the rounded bottom rectangle, the edge table of
// PIL's polygon fill, the eight aux values) and per pixel (whether PIL's `ImageDraw.polygon(xy, fill=1)` paints it), as
// plain functions that compile for the device and for the host.  The stand-alone host program tools/bev_map_hostcheck.cpp
// runs them in the kernels' sequence, and tests/test_map_input_cpu.py compares its pixels with Pillow's and with the numpy
// restatement (tests/map_input_reference.py) without a GPU.
//
// The fill is Pillow's ImagingDrawPolygon + polygon_generic (Draw.c) for an 8-bit image, no outline, as established
// pixel for pixel against Pillow 12.2 (INTEGRATION.md §4t has the rule in words):
//   edges i -> i + 1 around the ring; a horizontal edge that continues the previous horizontal edge in the same
//   direction widens that one; the closing edge only where the last point is not the first; a horizontal edge (a
//   repeated point is one) is painted as the span xmin..xmax of its row and stays out of the edge table;
//   per row y in [max(ymin, 0), min(ymax, S)], per table edge in order with ymin <= y <= ymax: x = (y - y0) * dx + x0 in
//   float32 (two roundings); doubled where y == edge.ymax and y < the clipped global ymax; otherwise, where dx != 0 and x
//   is an integer, the "connect discontiguous corners" step over the earlier table edges k of the same strict slope sign
//   that start with this edge on this row, or end with it, at the same x: slot k of the list becomes the pixel next to
//   the one the adjacent row (y + 1; y - 1 on the last row) rounds to, half away from zero, never short of x itself;
//   the list is sorted and taken in pairs, start = ROUND_UP (half away from zero), end = ROUND_DOWN (half toward zero),
//   with a running x_pos that starts at (int)xx[0].
// All float32 operations are single IEEE operations: no contraction into fused multiply-adds, on either side.
//
// Integer ranges: a rounded vertex is saturated at +-2^20 (DD_BM_SAT; the reference's cast of such a value is undefined),
// so y - y0 and every x below stay under 2^22 in magnitude and exact in float32 where they are integers.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#if defined(__HIPCC__)
#define DD_BM_HD __host__ __device__ __forceinline__
#else
#define DD_BM_HD inline
#endif

#define DD_BM_SAT (1 << 20)                    // the greatest magnitude of a rounded vertex coordinate
#define DD_BM_REC 52                           // int32 words of one box record (208 bytes, a multiple of 16)
// word offsets in a record
#define DD_BM_TABLE 0                          // 4 table edges x (x0, y0, ymin, ymax, dx bits)
#define DD_BM_HLINE 20                         // 4 horizontal spans x (y, xmin, xmax)
#define DD_BM_NT 32                            // table edges
#define DD_BM_NH 33                            // horizontal spans
#define DD_BM_GYMIN 34                         // first and last row of the scan, clipped to [0, S]
#define DD_BM_GYMAX 35
#define DD_BM_BBOX 36                          // x0, x1, y0, y1 of the vertices (x0 > x1: the box paints nothing)
#define DD_BM_LABEL 40                         // the object layer, -1 for none
#define DD_BM_FLAGGED 41                       // 1: a quad of the family that is not drawn (see dd_bm_unsupported)
#define DD_BM_CENTRE 42                        // canvas centre x, y as two doubles (8-byte aligned)
#define DD_BM_AUX 46                           // visibility, half-extents h and w, heading v0 and v1, height: six floats

// One IEEE operation each.  The device compiler contracts a * b + c into a fused multiply-add by default (and HIP's
// __fmul_rn / __fadd_rn are plain operators, so they do not prevent it): the pragma takes the `contract` flag off the
// operation itself, which survives inlining.  The host side is also built with -ffp-contract=off (the build line is in
// tools/bev_map_hostcheck.cpp) and keeps the results in volatiles for compilers without the pragma.
#if defined(__clang__)
#define DD_BM_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define DD_BM_NO_CONTRACT
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define DD_BM_RESULT
#else
#define DD_BM_RESULT volatile
#endif
DD_BM_HD float dd_bm_mul(float a, float b) { DD_BM_NO_CONTRACT DD_BM_RESULT float r = a * b; return r; }
DD_BM_HD float dd_bm_add(float a, float b) { DD_BM_NO_CONTRACT DD_BM_RESULT float r = a + b; return r; }
DD_BM_HD double dd_bm_dmul(double a, double b) { DD_BM_NO_CONTRACT DD_BM_RESULT double r = a * b; return r; }
DD_BM_HD double dd_bm_dadd(double a, double b) { DD_BM_NO_CONTRACT DD_BM_RESULT double r = a + b; return r; }
DD_BM_HD double dd_bm_ddiv(double a, double b) { DD_BM_NO_CONTRACT DD_BM_RESULT double r = a / b; return r; }
DD_BM_HD double dd_bm_dsqrt(double a) { return sqrt(a); }

DD_BM_HD int32_t dd_bm_min(int32_t a, int32_t b) { return a < b ? a : b; }
DD_BM_HD int32_t dd_bm_max(int32_t a, int32_t b) { return a > b ? a : b; }
DD_BM_HD float dd_bm_bits_f(int32_t v) { float f; memcpy(&f, &v, 4); return f; }
DD_BM_HD int32_t dd_bm_f_bits(float f) { int32_t v; memcpy(&v, &f, 4); return v; }

// x * scale + offset in float64, then np.round (half to even) and the cast to int32, saturated
DD_BM_HD double dd_bm_canvas(float v, double scale, double offset) { return dd_bm_dadd(dd_bm_dmul((double)v, scale), offset); }
DD_BM_HD int32_t dd_bm_vertex(double c) {
  const double r = rint(c);
  if (!(r > -(double)DD_BM_SAT)) return -DD_BM_SAT;        // a NaN too
  if (r > (double)DD_BM_SAT) return DD_BM_SAT;
  return (int32_t)r;
}

// The family that is NOT drawn: two opposite vertices equal, the other two distinct from them and from each other, and
// one of those two more than one pixel (Chebyshev) from the repeated vertex.  No rectangle rounds to such a quad.
DD_BM_HD bool dd_bm_unsupported_at(const int32_t* q, int a, int b, int c) {
  const int32_t ax = q[2 * a], ay = q[2 * a + 1], bx = q[2 * b], by = q[2 * b + 1], cx = q[2 * c], cy = q[2 * c + 1];
  if ((bx == ax && by == ay) || (cx == ax && cy == ay) || (bx == cx && by == cy)) return false;
  const int32_t db = dd_bm_max(abs(bx - ax), abs(by - ay)), dc = dd_bm_max(abs(cx - ax), abs(cy - ay));
  return db > 1 || dc > 1;
}
DD_BM_HD bool dd_bm_unsupported(const int32_t* q) {
  if (q[0] == q[4] && q[1] == q[5] && dd_bm_unsupported_at(q, 0, 1, 3)) return true;
  if (q[2] == q[6] && q[3] == q[7] && dd_bm_unsupported_at(q, 1, 0, 2)) return true;
  return false;
}

// The edge table and the horizontal spans of the ring q (x0, y0, ..., x3, y3) into words [0, 40) of a record.
DD_BM_HD void dd_bm_edges(const int32_t* q, int32_t size, int32_t* rec) {
  int32_t ex0[4], ey0[4], ex1[4], ey1[4], exmin[4], exmax[4];
  int n = 0;
  for (int i = 0; i < 3; ++i) {
    const int32_t x0 = q[2 * i], y0 = q[2 * i + 1], x1 = q[2 * i + 2], y1 = q[2 * i + 3];
    if (y0 == y1 && i != 0 && y0 == q[2 * i - 1]) {
      const int32_t xp = q[2 * i - 2];
      if (x1 > x0 && x0 > xp) { exmax[n - 1] = x1; continue; }
      if (x1 < x0 && x0 < xp) { exmin[n - 1] = x1; continue; }
    }
    ex0[n] = x0; ey0[n] = y0; ex1[n] = x1; ey1[n] = y1;
    exmin[n] = dd_bm_min(x0, x1); exmax[n] = dd_bm_max(x0, x1);
    ++n;
  }
  if (q[6] != q[0] || q[7] != q[1]) {
    ex0[n] = q[6]; ey0[n] = q[7]; ex1[n] = q[0]; ey1[n] = q[1];
    exmin[n] = dd_bm_min(q[6], q[0]); exmax[n] = dd_bm_max(q[6], q[0]);
    ++n;
  }
  int32_t gmin = size - 1, gmax = 0, nt = 0, nh = 0;
  for (int i = 0; i < 40; ++i) rec[i] = 0;
  for (int i = 0; i < n; ++i) {
    const int32_t lo = dd_bm_min(ey0[i], ey1[i]), hi = dd_bm_max(ey0[i], ey1[i]);
    gmin = dd_bm_min(gmin, lo); gmax = dd_bm_max(gmax, hi);
    if (lo == hi) {
      rec[DD_BM_HLINE + 3 * nh] = lo; rec[DD_BM_HLINE + 3 * nh + 1] = exmin[i]; rec[DD_BM_HLINE + 3 * nh + 2] = exmax[i];
      ++nh;
    } else {
      int32_t* t = rec + DD_BM_TABLE + 5 * nt;
      t[0] = ex0[i]; t[1] = ey0[i]; t[2] = lo; t[3] = hi;
      t[4] = dd_bm_f_bits((float)(ex1[i] - ex0[i]) / (float)(ey1[i] - ey0[i]));      // one IEEE division
      ++nt;
    }
  }
  rec[DD_BM_NT] = nt; rec[DD_BM_NH] = nh;
  rec[DD_BM_GYMIN] = dd_bm_max(gmin, 0); rec[DD_BM_GYMAX] = dd_bm_min(gmax, size);
  rec[DD_BM_BBOX] = dd_bm_min(dd_bm_min(q[0], q[2]), dd_bm_min(q[4], q[6]));
  rec[DD_BM_BBOX + 1] = dd_bm_max(dd_bm_max(q[0], q[2]), dd_bm_max(q[4], q[6]));
  rec[DD_BM_BBOX + 2] = dd_bm_min(dd_bm_min(q[1], q[3]), dd_bm_min(q[5], q[7]));
  rec[DD_BM_BBOX + 3] = dd_bm_max(dd_bm_max(q[1], q[3]), dd_bm_max(q[5], q[7]));
}

// One box: corners (24 floats), bottom centre (3 floats), height, visibility, label -> its record.
// sx, ox / sy, oy: lidar2canvas (pipeline.py:70-74): canvas x = x * sx + ox.
DD_BM_HD void dd_bm_box(const float* c, const float* bc, float height, float visibility, int64_t label, int32_t n_object,
                        double sx, double ox, double sy, double oy, int32_t size, int32_t* rec) {
  const int ring[4] = {0, 3, 7, 4};                                   // pipeline.py:100, :187
  int32_t q[8];
  for (int j = 0; j < 4; ++j) {
    q[2 * j] = dd_bm_vertex(dd_bm_canvas(c[3 * ring[j]], sx, ox));
    q[2 * j + 1] = dd_bm_vertex(dd_bm_canvas(c[3 * ring[j] + 1], sy, oy));
  }
  dd_bm_edges(q, size, rec);
  const bool bad = dd_bm_unsupported(q);
  if (bad) { rec[DD_BM_BBOX] = 1; rec[DD_BM_BBOX + 1] = 0; }
  rec[DD_BM_LABEL] = (label >= 0 && label < n_object) ? (int32_t)label : -1;
  rec[DD_BM_FLAGGED] = bad ? 1 : 0;
  // :101-103: centre, front = mean of corners 4, 7, left = mean of corners 0, 4 — the means in float32
  const float fx = dd_bm_mul(dd_bm_add(c[12], c[21]), 0.5f), fy = dd_bm_mul(dd_bm_add(c[13], c[22]), 0.5f);
  const float lx = dd_bm_mul(dd_bm_add(c[0], c[12]), 0.5f), ly = dd_bm_mul(dd_bm_add(c[1], c[13]), 0.5f);
  const double cx = dd_bm_canvas(bc[0], sx, ox), cy = dd_bm_canvas(bc[1], sy, oy);
  const double d0 = dd_bm_dadd(dd_bm_canvas(fx, sx, ox), -cx), d1 = dd_bm_dadd(dd_bm_canvas(fy, sy, oy), -cy);
  const double e0 = dd_bm_dadd(dd_bm_canvas(lx, sx, ox), -cx), e1 = dd_bm_dadd(dd_bm_canvas(ly, sy, oy), -cy);
  const double hh = dd_bm_dsqrt(dd_bm_dadd(dd_bm_dmul(d0, d0), dd_bm_dmul(d1, d1)));          // :137
  const double ww = dd_bm_dsqrt(dd_bm_dadd(dd_bm_dmul(e0, e0), dd_bm_dmul(e1, e1)));          // :138
  const double den = dd_bm_dadd(hh, 1e-6);                                                     // :140-141
  memcpy(rec + DD_BM_CENTRE, &cx, 8);
  memcpy(rec + DD_BM_CENTRE + 2, &cy, 8);
  rec[DD_BM_AUX] = dd_bm_f_bits(visibility);
  rec[DD_BM_AUX + 1] = dd_bm_f_bits((float)hh);
  rec[DD_BM_AUX + 2] = dd_bm_f_bits((float)ww);
  rec[DD_BM_AUX + 3] = dd_bm_f_bits((float)dd_bm_ddiv(d0, den));
  rec[DD_BM_AUX + 4] = dd_bm_f_bits((float)dd_bm_ddiv(d1, den));
  rec[DD_BM_AUX + 5] = dd_bm_f_bits(height);
}

DD_BM_HD float dd_bm_at(const int32_t* t, int32_t y) {
  return dd_bm_add(dd_bm_mul((float)(y - t[1]), dd_bm_bits_f(t[4])), (float)t[0]);
}
// C's lroundf on the double value of f, as a float: half away from zero
DD_BM_HD float dd_bm_lround(float f) {
  const double d = (double)f;
  return (float)(d >= 0.0 ? floor(d + 0.5) : -floor(-d + 0.5));
}
DD_BM_HD int32_t dd_bm_round_up(float f) { return (int32_t)(f >= 0.0f ? floorf(dd_bm_add(f, 0.5f)) : -floorf(dd_bm_add(fabsf(f), 0.5f))); }
DD_BM_HD int32_t dd_bm_round_down(float f) { return (int32_t)(f >= 0.0f ? ceilf(dd_bm_add(f, -0.5f)) : -ceilf(dd_bm_add(fabsf(f), -0.5f))); }

// Does the fill of the record's quad paint pixel (px, py) (px the column while drawing, py the row)?  rec: words [0, 36).
// The caller has px, py on the canvas, so hline8's clipping never applies.
DD_BM_HD bool dd_bm_covers(const int32_t* rec, int32_t px, int32_t py) {
  bool in = false;
  const int32_t nh = rec[DD_BM_NH], nt = rec[DD_BM_NT];
  for (int i = 0; i < 4; ++i) {
    const int32_t* h = rec + DD_BM_HLINE + 3 * i;
    if (i < nh && py == h[0] && px >= h[1] && px <= h[2]) in = true;
  }
  const int32_t gmax = rec[DD_BM_GYMAX];
  if (py < rec[DD_BM_GYMIN] || py > gmax) return in;
  float xx[8];
  for (int s = 0; s < 8; ++s) xx[s] = INFINITY;
  int j = 0;
  for (int i = 0; i < 4; ++i) {
    const int32_t* cur = rec + DD_BM_TABLE + 5 * i;
    if (i >= nt || py < cur[2] || py > cur[3]) continue;
    const float x = dd_bm_at(cur, py), dx = dd_bm_bits_f(cur[4]);
    for (int s = 0; s < 8; ++s) if (s == j) xx[s] = x;
    ++j;
    if (py == cur[3] && py < gmax) {
      for (int s = 0; s < 8; ++s) if (s == j) xx[s] = x;
      ++j;
    } else if (dx != 0.0f && rintf(x) == x) {
      bool done = false;
      for (int k = 0; k < 3; ++k) {
        const int32_t* oth = rec + DD_BM_TABLE + 5 * k;
        if (k >= i || done) continue;
        const float odx = dd_bm_bits_f(oth[4]);
        if ((dx > 0.0f && odx <= 0.0f) || (dx < 0.0f && odx >= 0.0f)) continue;
        if (!((py == cur[2] && py == oth[2]) || (py == cur[3] && py == oth[3]))) continue;
        if (x != dd_bm_at(oth, py)) continue;
        const int32_t adj = py == gmax ? py - 1 : py + 1;
        const float a = dd_bm_at(cur, adj), b = dd_bm_at(oth, adj);
        float v;
        if (py == cur[3]) v = dx > 0.0f ? fminf(dd_bm_lround(fmaxf(a, b)) + 1.0f, x) : fmaxf(dd_bm_lround(fminf(a, b)) - 1.0f, x);
        else v = dx > 0.0f ? fmaxf(dd_bm_lround(fminf(a, b)) - 1.0f, x) : fminf(dd_bm_lround(fmaxf(a, b)) + 1.0f, x);
        if (k < j)
          for (int s = 0; s < 3; ++s) if (s == k) xx[s] = v;
        done = true;
      }
    }
  }
  if (j == 0) return in;
  for (int p = 0; p < 7; ++p)                                           // the unused slots hold +inf and stay behind
    for (int s = 0; s < 7 - p; ++s) {
      const float lo = fminf(xx[s], xx[s + 1]), hi = fmaxf(xx[s], xx[s + 1]);
      xx[s] = lo; xx[s + 1] = hi;
    }
  int32_t x_pos = (int32_t)xx[0];
  for (int i = 1; i < 8; i += 2) {
    if (i >= j) break;
    const int32_t x_end = dd_bm_round_down(xx[i]);
    if (x_end < x_pos) continue;
    int32_t x_start = dd_bm_round_up(xx[i - 1]);
    if (x_pos > x_start) {
      x_start = x_pos;
      if (x_end < x_start) continue;
    }
    if (px >= x_start && px <= x_end) in = true;
    x_pos = x_end + 1;
  }
  return in;
}
