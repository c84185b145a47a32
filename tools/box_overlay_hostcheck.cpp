// Stand-alone host program for the arithmetic of box output (csrc/box_overlay_core.h): it runs the sequence of the two
// kernels of csrc/box_overlay.hip — keys, ranks, projection into the rows, then per pixel the walk over the boxes from
// the last slot down — with the header's own functions on the CPU, in heap blocks of exactly the sizes the kernels'
// buffers have, so that the host sanitizers see every index and every integer product:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include \
//       tools/box_overlay_hostcheck.cpp -o box_overlay_hostcheck && ./box_overlay_hostcheck case.bin out.bin
//
// case.bin (little endian): int32 scenes, views, total, cap, n_classes, h, w, transparent, n_palette; int32 offsets[scenes
// + 1]; float corners[total][8][3]; int64 labels[total]; float transforms[scenes][views][4][4]; uint8 palette[n_palette]
// [3]; uint8 frames[scenes * views][h][w][3] unless transparent.
// out.bin: int32 pts[scenes][views][cap][8][2], cls[scenes][views][cap], counts[scenes][views], flags[1]; uint8
// out[scenes * views][h][w][3 or 4].  tests/test_box_output_cpu.py compares them with the oracle byte for byte.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../dualdiff_amd/csrc/box_overlay_core.h"

namespace {

template <typename T>
T* block(size_t n) {                           // exactly n elements on the heap: one past the end is a sanitizer report
  return static_cast<T*>(n ? malloc(n * sizeof(T)) : malloc(1));
}

template <typename T>
bool read_n(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s case.bin out.bin\n", argv[0]);
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  int32_t hd[9];
  if (!f || !read_n(f, hd, 9)) return 3;
  const int32_t scenes = hd[0], views = hd[1], total = hd[2], cap = hd[3], n_classes = hd[4], h = hd[5], w = hd[6],
                transparent = hd[7], n_palette = hd[8];
  if (scenes <= 0 || views <= 0 || total < 0 || cap <= 0 || cap > DD_BO_MAX_BOXES || n_classes <= 0 || h <= 0 || w <= 0 ||
      h >= (1 << 15) || w >= (1 << 15) || n_palette <= 0)
    return 4;
  const size_t m = (size_t)scenes * views, ch = transparent ? 4 : 3;
  int32_t* offsets = block<int32_t>(scenes + 1);
  float* corners = block<float>((size_t)total * 24);
  int64_t* labels = block<int64_t>(total);
  float* transforms = block<float>(m * 16);
  uint8_t* palette = block<uint8_t>((size_t)n_palette * 3);
  uint8_t* frames = transparent ? nullptr : block<uint8_t>(m * h * w * 3);
  if (!read_n(f, offsets, scenes + 1) || !read_n(f, corners, (size_t)total * 24) || !read_n(f, labels, total) ||
      !read_n(f, transforms, m * 16) || !read_n(f, palette, (size_t)n_palette * 3) ||
      (frames && !read_n(f, frames, m * h * w * 3)))
    return 5;
  fclose(f);
  int32_t* pts = block<int32_t>(m * cap * 16);
  int32_t* cls = block<int32_t>(m * cap);
  int32_t* counts = block<int32_t>(m);
  uint8_t* out = block<uint8_t>(m * h * w * ch);
  int32_t flags = 0;

  // dd_box_edges: one (scene, view) at a time, as a workgroup does it
  std::vector<double> key(DD_BO_MAX_BOXES);
  for (size_t blk = 0; blk < m; ++blk) {
    const int scene = (int)(blk / views);
    int n0 = offsets[scene] < 0 ? 0 : offsets[scene];
    if (n0 > total) n0 = total;
    int n1 = offsets[scene + 1] < n0 ? n0 : offsets[scene + 1];
    if (n1 > total) n1 = total;
    int n = n1 - n0;
    if (n > DD_BO_MAX_BOXES) { n = DD_BO_MAX_BOXES; flags |= DD_BO_FLAG_CAP; }
    double mat[12];
    for (int k = 0; k < 12; ++k) mat[k] = (double)transforms[blk * 16 + k];
    int kept = 0;
    for (int i = 0; i < n; ++i) {
      const int32_t c = dd_bo_class(labels[n0 + i], n_classes);
      if (c < 0) flags |= DD_BO_FLAG_LABEL;
      const double mz = dd_bo_min_z(corners + (size_t)(n0 + i) * 24, mat);
      const bool keep = c >= 0 && dd_bo_drawn(mz);
      key[i] = keep ? mz : -1.0;
      kept += keep;
    }
    const int drop = kept > cap ? kept - cap : 0;
    int32_t* prow = pts + blk * cap * 16;
    int32_t* crow = cls + blk * cap;
    for (int i = 0; i < n; ++i) {
      if (!dd_bo_drawn(key[i])) continue;
      int rank = 0;
      for (int j = 0; j < n; ++j) rank += dd_bo_before(key[j], j, key[i], i) ? 1 : 0;
      const int slot = rank - drop;
      if (slot < 0) continue;
      if (dd_bo_points(corners + (size_t)(n0 + i) * 24, mat, prow + (size_t)slot * 16)) flags |= DD_BO_FLAG_SATURATED;
      crow[slot] = dd_bo_class(labels[n0 + i], n_classes);
    }
    for (int s = kept < cap ? kept : cap; s < cap; ++s) {
      memset(prow + (size_t)s * 16, 0, 16 * sizeof(int32_t));
      crow[s] = 0;
    }
    counts[blk] = kept;
    if (kept > cap) flags |= DD_BO_FLAG_CAP;
  }

  // dd_box_draw_u8: every pixel walks its view's boxes from the last slot down
  for (size_t v = 0; v < m; ++v) {
    const int count = counts[v] < 0 ? 0 : (counts[v] > cap ? cap : counts[v]);
    for (int py = 0; py < h; ++py) {
      for (int px = 0; px < w; ++px) {
        int colour = -1;
        for (int k = count - 1; k >= 0 && colour < 0; --k)
          if (dd_bo_on_box(px, py, pts + (v * cap + k) * 16)) colour = cls[v * cap + k];
        uint32_t r = 0, g = 0, b = 0;
        if (colour >= 0) {
          const uint8_t* c = palette + 3 * (colour < n_palette ? colour : n_palette - 1);
          r = c[0]; g = c[1]; b = c[2];
        } else if (!transparent) {
          const uint8_t* c = frames + ((v * h + py) * w + px) * 3;
          r = c[0]; g = c[1]; b = c[2];
        }
        uint8_t* o = out + ((v * h + py) * w + px) * ch;
        o[0] = (uint8_t)r; o[1] = (uint8_t)g; o[2] = (uint8_t)b;
        if (transparent) o[3] = (uint8_t)dd_bo_alpha(r, g, b);
      }
    }
  }

  f = fopen(argv[2], "wb");
  if (!f) return 6;
  fwrite(pts, sizeof(int32_t), m * cap * 16, f);
  fwrite(cls, sizeof(int32_t), m * cap, f);
  fwrite(counts, sizeof(int32_t), m, f);
  fwrite(&flags, sizeof(int32_t), 1, f);
  fwrite(out, 1, m * h * w * ch, f);
  fclose(f);
  free(offsets); free(corners); free(labels); free(transforms); free(palette); free(frames);
  free(pts); free(cls); free(counts); free(out);
  printf("ok: %zu views, %d x %d, flags %d\n", m, h, w, flags);
  return 0;
}
