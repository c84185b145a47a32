// Stand-alone host program for the validation paths of dd_box_views (csrc/boxes.hip): every call below must be rejected
// with DD_ERR_BAD_ARG or DD_ERR_UNSUPPORTED before the first HIP runtime call, so it runs on a machine without a GPU.  It is
// meant to be built with the host sanitizers, which check the launcher's own host code (not the kernel):
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//       dualdiff_amd/csrc/boxes.hip tools/box_views_hostcheck.cpp -o box_views_hostcheck && ./box_views_hostcheck
//
// Exit status 0 and "ok" when every call answers as expected; otherwise the number of the first call that did not.
#include <stdio.h>

#include "../include/dualdiff_hip.h"

namespace {

struct Call {
  const float* corners; const float* filter_corners; const int64_t* labels; const int32_t* offsets; const float* transforms;
  int32_t total, scenes, views, cap, points_mode, filter_mode, canvas_h, canvas_w;
  float* bboxes; int64_t* classes; uint8_t* masks; int32_t* counts; int32_t* max_len;
};

int run(const Call& c) {
  return dd_box_views(c.corners, c.filter_corners, c.labels, c.offsets, c.transforms, c.total, c.scenes, c.views, c.cap,
                      c.points_mode, c.filter_mode, c.canvas_h, c.canvas_w, c.bboxes, c.classes, c.masks, c.counts, c.max_len,
                      nullptr);
}

}  // namespace

int main() {
  // real host buffers, so that the pointers are valid and aligned; nothing reads them, because every call is rejected
  static float corners[4 * 24 + 1], transforms[16 * 6], bboxes[6 * 32 * 24 + 1];
  static int64_t labels[4 + 1], classes[6 * 32 + 1];
  static int32_t offsets[2] = {0, 4}, counts[6], max_len[1];
  static uint8_t masks[6 * 32];
  const Call good = {corners, nullptr, labels, offsets, transforms, 4, 1, 6, 32, 0, 1, 224, 400,
                     bboxes, classes, masks, counts, max_len};
  int n = 0, failed = 0;
  auto expect = [&](Call c, int want) {
    ++n;
    const int got = run(c);
    if (got != want && !failed) {
      failed = n;
      fprintf(stderr, "call %d: got %d, expected %d\n", n, got, want);
    }
  };
  Call c;
  c = good; c.corners = nullptr; expect(c, DD_ERR_BAD_ARG);
  c = good; c.labels = nullptr; expect(c, DD_ERR_BAD_ARG);
  c = good; c.offsets = nullptr; expect(c, DD_ERR_BAD_ARG);
  c = good; c.bboxes = nullptr; expect(c, DD_ERR_BAD_ARG);
  c = good; c.classes = nullptr; expect(c, DD_ERR_BAD_ARG);
  c = good; c.masks = nullptr; expect(c, DD_ERR_BAD_ARG);
  c = good; c.counts = nullptr; expect(c, DD_ERR_BAD_ARG);
  c = good; c.max_len = nullptr; expect(c, DD_ERR_BAD_ARG);
  c = good; c.total = -1; expect(c, DD_ERR_BAD_ARG);
  c = good; c.scenes = 0; expect(c, DD_ERR_BAD_ARG);
  c = good; c.views = 0; expect(c, DD_ERR_BAD_ARG);
  c = good; c.views = -6; expect(c, DD_ERR_BAD_ARG);
  c = good; c.cap = 0; expect(c, DD_ERR_BAD_ARG);
  c = good; c.points_mode = 2; expect(c, DD_ERR_BAD_ARG);
  c = good; c.points_mode = -1; expect(c, DD_ERR_BAD_ARG);
  c = good; c.filter_mode = 3; expect(c, DD_ERR_BAD_ARG);
  c = good; c.filter_mode = -1; expect(c, DD_ERR_BAD_ARG);
  c = good; c.filter_mode = 0; expect(c, DD_ERR_BAD_ARG);                               // keep-all with six views
  c = good; c.transforms = nullptr; expect(c, DD_ERR_BAD_ARG);
  c = good; c.filter_mode = 2; c.transforms = nullptr; expect(c, DD_ERR_BAD_ARG);
  c = good; c.filter_mode = 2; c.canvas_h = 0; expect(c, DD_ERR_BAD_ARG);
  c = good; c.filter_mode = 2; c.canvas_w = -400; expect(c, DD_ERR_BAD_ARG);
  c = good; c.corners = (const float*)((const char*)corners + 2); expect(c, DD_ERR_BAD_ARG);      // not element-aligned
  c = good; c.filter_corners = (const float*)((const char*)corners + 1); expect(c, DD_ERR_BAD_ARG);
  c = good; c.labels = (const int64_t*)((const char*)labels + 4); expect(c, DD_ERR_BAD_ARG);
  c = good; c.classes = (int64_t*)((char*)classes + 4); expect(c, DD_ERR_BAD_ARG);
  c = good; c.bboxes = (float*)((char*)bboxes + 2); expect(c, DD_ERR_BAD_ARG);
  c = good; c.scenes = 0x7fffffff; c.views = 0x7fffffff; expect(c, DD_ERR_UNSUPPORTED);           // 64-bit product, no overflow
  c = good; c.scenes = 1 << 20; c.views = 1 << 10; c.cap = 0x7fffffff; expect(c, DD_ERR_UNSUPPORTED);
  if (failed) return failed;
  printf("ok: %d calls rejected before any launch\n", n);
  return 0;
}
