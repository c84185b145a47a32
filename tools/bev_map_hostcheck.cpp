// Stand-alone host program: PIL's polygon fill as csrc/bev_map_core.h states it — the functions the kernels of
// csrc/bev_map.hip call — run on the CPU over the quads given on standard input, so that tests/test_map_input_cpu.py can
// compare their pixels with the numpy restatement and with Pillow without a GPU.
//
//   c++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I dualdiff_amd/csrc tools/bev_map_hostcheck.cpp -o bev_map_hostcheck
//
// Input: one quad per line, "S x0 y0 x1 y1 x2 y2 x3 y3" (S the canvas side, integers).  Output: one line per quad, "F" for
// a quad of the family that is not drawn, else S * S characters '0' / '1', row by row (row = y, column = x).
#include <stdio.h>

#include <string>
#include <vector>

#include "bev_map_core.h"

int main() {
  int s, q[8];
  while (scanf("%d %d %d %d %d %d %d %d %d", &s, q, q + 1, q + 2, q + 3, q + 4, q + 5, q + 6, q + 7) == 9) {
    if (s <= 0 || s > 4096) return 2;
    std::vector<int32_t> rec(DD_BM_REC);                  // a heap block of exactly the record's size
    int32_t ring[8];
    for (int i = 0; i < 8; ++i) ring[i] = q[i] < -DD_BM_SAT ? -DD_BM_SAT : (q[i] > DD_BM_SAT ? DD_BM_SAT : q[i]);
    if (dd_bm_unsupported(ring)) {
      puts("F");
      continue;
    }
    dd_bm_edges(ring, s, rec.data());
    std::string line((size_t)s * s, '0');
    for (int y = 0; y < s; ++y)
      for (int x = 0; x < s; ++x)
        if (dd_bm_covers(rec.data(), x, y)) line[(size_t)y * s + x] = '1';
    puts(line.c_str());
  }
  return 0;
}
