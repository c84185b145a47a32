// Stand-alone host program: the FGM loss mask as csrc/fgm_mask_core.h states it — the functions the kernels of
// csrc/fgm_mask.hip call, in the kernels' sequence — run on the CPU over the boxes given on standard input, so that
// tests/test_fgm_mask_cpu.py can compare the maps, the areas and the flagged count with the numpy restatement without a
// GPU.
//
//   c++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I dualdiff_amd/csrc tools/fgm_mask_hostcheck.cpp -o fgm_mask_hostcheck
//
// Input, all integers: "W H W_out H_out views m P sx sy" (sx, sy: the bits of the two float64 scale factors), then per
// view the bits of the 16 float32 of its matrix, then per box of the view its mask (0 / 1) and the bits of its P * 3 float32
// corner coordinates.  Output: per view a line "areas" with the m areas and a line of H_out * W_out hexadecimal words, the
// bits of the float32 map row by row; a last line "flags N".
#include <stdio.h>

#include <vector>

#include "fgm_mask_core.h"

static bool read_f32(float* f) {
  unsigned long long u;
  if (scanf("%llu", &u) != 1) return false;
  const uint32_t v = (uint32_t)u;
  memcpy(f, &v, 4);
  return true;
}

int main() {
  int w, h, wo, ho, views, m, np;
  unsigned long long sxb, syb;
  if (scanf("%d %d %d %d %d %d %d %llu %llu", &w, &h, &wo, &ho, &views, &m, &np, &sxb, &syb) != 9) return 2;
  if (w < 1 || h < 1 || (long long)w * h > (1 << 20) || wo < 1 || ho < 1 || wo > w || ho > h || ((w - wo) & 1) || views < 0 ||
      m < 0 || np < 1 || np > DD_FG_MAX_POINTS)
    return 2;
  double sx, sy;
  memcpy(&sx, &sxb, 8);
  memcpy(&sy, &syb, 8);
  int flags = 0;
  for (int v = 0; v < views; ++v) {
    std::vector<float> t(16);
    for (int i = 0; i < 16; ++i)
      if (!read_f32(&t[i])) return 2;
    std::vector<std::vector<int32_t>> recs;
    for (int k = 0; k < m; ++k) {
      int masked;
      if (scanf("%d", &masked) != 1) return 2;
      std::vector<float> c((size_t)np * 3);
      for (float& f : c)
        if (!read_f32(&f)) return 2;
      // launch 1: a lane per point, then one lane for the record, then the wave counts the area
      std::vector<int32_t> pts((size_t)np * 2), status((size_t)np), work(DD_FG_WORK), rec(DD_FG_REC);
      for (int i = 0; i < np; ++i) status[i] = dd_fg_point(&c[3 * i], t.data(), sx, sy, &pts[2 * i], &pts[2 * i + 1]);
      dd_fg_record(pts.data(), status.data(), np, masked, work.data(), rec.data());
      int32_t clip[4], area = 0;
      dd_fg_clip(rec.data(), w, h, clip);
      for (int y = clip[2]; clip[0] <= clip[1] && y <= clip[3]; ++y)
        for (int x = clip[0]; x <= clip[1]; ++x) area += dd_fg_inside(rec.data(), x, y) ? 1 : 0;
      rec[DD_FG_AREA] = area;
      rec[DD_FG_WEIGHT] = dd_bm_f_bits(dd_fg_weight(area, w, h));
      flags += rec[DD_FG_FLAGGED];
      recs.push_back(rec);
    }
    printf("areas");
    for (int k = 0; k < m; ++k) printf(" %d", recs[k][DD_FG_AREA]);
    printf("\n");
    // launch 2: pixel-major
    for (int oy = 0; oy < ho; ++oy)
      for (int ox = 0; ox < wo; ++ox) {
        const int32_t tx = ox + (w - wo) / 2, ty = oy + (h - ho);
        float best = 0.0f;
        for (int k = 0; k < m; ++k) {
          const int32_t* r = recs[k].data();
          if (tx < r[DD_FG_BBOX] || tx > r[DD_FG_BBOX + 1] || ty < r[DD_FG_BBOX + 2] || ty > r[DD_FG_BBOX + 3]) continue;
          if (dd_fg_inside(r, tx, ty)) best = fmaxf(best, dd_bm_bits_f(r[DD_FG_WEIGHT]));
        }
        printf("%08x ", (unsigned)dd_bm_f_bits(best));
      }
    printf("\n");
  }
  printf("flags %d\n", flags);
  return 0;
}
