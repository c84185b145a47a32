// Stand-alone host program for the validation paths of dd_map_render_u8 and dd_map_compose_u8 (csrc/map.hip): every call
// below must be rejected with DD_ERR_BAD_ARG or DD_ERR_UNSUPPORTED before the first HIP runtime call, so it runs on a
// machine without a GPU.  It is meant to be built with the host sanitizers, which check the launchers' own host code (not
// the kernels):
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//       dualdiff_amd/csrc/map.hip tools/map_render_hostcheck.cpp -o map_render_hostcheck && ./map_render_hostcheck
//
// Exit status 0 and "ok" when every call answers as expected; otherwise the number of the first call that did not.
#include <stdio.h>

#include "../include/dualdiff_hip.h"

namespace {

struct Render {
  const uint8_t* maps; const float* stab; const float* dtab; float* img; int32_t* used;
  int32_t b, c, s, ns, nd;
};

struct Compose {
  const uint8_t* src; const int32_t* index; const uint8_t* legend; uint8_t* out;
  int32_t m, g, t, lh, lw, side;
};

int run(const Render& r) {
  return dd_map_render_u8(r.maps, r.stab, r.dtab, r.img, r.used, r.b, r.c, r.s, r.ns, r.nd, nullptr);
}

int run(const Compose& c) {
  return dd_map_compose_u8(c.src, c.index, c.legend, c.out, c.m, c.g, c.t, c.lh, c.lw, c.side, nullptr);
}

}  // namespace

int main() {
  // real host buffers, so that the pointers are valid and aligned; nothing reads them, because every call is rejected
  static uint8_t maps[2 * 18 * 12 * 12], src[4 * 40 * 40 * 3], legend[4 * 40 * 3], out[2 * 44 * 40 * 3];
  static float stab[9 * 4 + 1], dtab[10 * 4 + 1], img[2 * 3 * 12 * 12 + 1];
  static int32_t used[2 + 1], index[2 + 1];
  const Render good = {maps, stab, dtab, img, used, 2, 18, 12, 8, 10};
  const Compose fine = {src, index, legend, out, 4, 2, 40, 4, 40, 1};
  int n = 0, failed = 0;
  auto expect = [&](auto c, int want) {
    ++n;
    const int got = run(c);
    if (got != want && !failed) {
      failed = n;
      fprintf(stderr, "call %d: got %d, expected %d\n", n, got, want);
    }
  };
  Render r;
  r = good; r.maps = nullptr; expect(r, DD_ERR_BAD_ARG);
  r = good; r.stab = nullptr; expect(r, DD_ERR_BAD_ARG);
  r = good; r.dtab = nullptr; expect(r, DD_ERR_BAD_ARG);                                 // ten dynamic layers, no table
  r = good; r.img = nullptr; expect(r, DD_ERR_BAD_ARG);
  r = good; r.used = nullptr; expect(r, DD_ERR_BAD_ARG);
  r = good; r.b = 0; expect(r, DD_ERR_BAD_ARG);
  r = good; r.c = 0; expect(r, DD_ERR_BAD_ARG);
  r = good; r.s = 0; expect(r, DD_ERR_BAD_ARG);
  r = good; r.s = -12; expect(r, DD_ERR_BAD_ARG);
  r = good; r.ns = -1; expect(r, DD_ERR_BAD_ARG);
  r = good; r.nd = -1; expect(r, DD_ERR_BAD_ARG);
  r = good; r.ns = 0; r.nd = 0; expect(r, DD_ERR_BAD_ARG);                               // nothing to draw
  r = good; r.c = 17; expect(r, DD_ERR_BAD_ARG);                                         // more layers than the map has
  r = good; r.ns = 0x7fffffff; r.nd = 0x7fffffff; expect(r, DD_ERR_BAD_ARG);             // 64-bit sum, no overflow
  r = good; r.stab = (const float*)((const char*)stab + 2); expect(r, DD_ERR_BAD_ARG);   // not element-aligned
  r = good; r.dtab = (const float*)((const char*)dtab + 1); expect(r, DD_ERR_BAD_ARG);
  r = good; r.img = (float*)((char*)img + 2); expect(r, DD_ERR_BAD_ARG);
  r = good; r.used = (int32_t*)((char*)used + 1); expect(r, DD_ERR_BAD_ARG);
  r = good; r.c = 40; r.ns = 16; r.nd = 16; expect(r, DD_ERR_UNSUPPORTED);               // 32 layers: bit 31 is taken
  r = good; r.c = 0x7fffffff; r.ns = 0; r.nd = 32; expect(r, DD_ERR_UNSUPPORTED);
  r = good; r.s = 1 << 14; expect(r, DD_ERR_UNSUPPORTED);
  r = good; r.s = 0x7fffffff; expect(r, DD_ERR_UNSUPPORTED);
  r = good; r.b = 65536; expect(r, DD_ERR_UNSUPPORTED);
  Compose c;
  c = fine; c.src = nullptr; expect(c, DD_ERR_BAD_ARG);
  c = fine; c.out = nullptr; expect(c, DD_ERR_BAD_ARG);
  c = fine; c.m = 0; expect(c, DD_ERR_BAD_ARG);
  c = fine; c.g = 0; expect(c, DD_ERR_BAD_ARG);
  c = fine; c.t = 0; expect(c, DD_ERR_BAD_ARG);
  c = fine; c.t = -40; expect(c, DD_ERR_BAD_ARG);
  c = fine; c.lh = -1; expect(c, DD_ERR_BAD_ARG);
  c = fine; c.lw = -1; expect(c, DD_ERR_BAD_ARG);
  c = fine; c.side = 2; expect(c, DD_ERR_BAD_ARG);
  c = fine; c.side = -1; expect(c, DD_ERR_BAD_ARG);
  c = fine; c.legend = nullptr; expect(c, DD_ERR_BAD_ARG);                               // a size without a legend
  c = fine; c.lh = 0; expect(c, DD_ERR_BAD_ARG);                                         // a legend without a size
  c = fine; c.lw = 0; expect(c, DD_ERR_BAD_ARG);
  c = fine; c.lh = 0; c.lw = 0; expect(c, DD_ERR_BAD_ARG);
  c = fine; c.legend = nullptr; c.lh = 0; expect(c, DD_ERR_BAD_ARG);
  c = fine; c.index = nullptr; expect(c, DD_ERR_BAD_ARG);                                // g != m needs an index
  c = fine; c.index = (const int32_t*)((const char*)index + 2); expect(c, DD_ERR_BAD_ARG);
  c = fine; c.lw = 41; expect(c, DD_ERR_BAD_ARG);                                        // wider than the picture it lies below
  c = fine; c.side = 0; c.lh = 41; c.lw = 4; expect(c, DD_ERR_BAD_ARG);                  // taller than the picture beside it
  c = fine; c.t = 1 << 14; expect(c, DD_ERR_UNSUPPORTED);
  c = fine; c.t = 0x7fffffff; c.lh = 0x7fffffff; c.lw = 0x7fffffff; expect(c, DD_ERR_UNSUPPORTED);
  c = fine; c.side = 0; c.lh = 40; c.lw = 1 << 14; expect(c, DD_ERR_UNSUPPORTED);
  c = fine; c.m = 65536; expect(c, DD_ERR_UNSUPPORTED);
  c = fine; c.g = 65536; expect(c, DD_ERR_UNSUPPORTED);
  if (failed) return failed;
  printf("ok: %d calls rejected before any launch\n", n);
  return 0;
}
