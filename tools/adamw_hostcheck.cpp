// Stand-alone host program: one fused optimizer step as csrc/adamw_core.h states it — the functions the kernels of
// csrc/adamw.hip call, in the kernels' chunk and lane order — run on the CPU over the table given on standard input, so that
// tests/test_adamw_cpu.py can compare every bit of the result with the numpy restatement without a GPU.
//
//   c++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I dualdiff_amd/csrc tools/adamw_hostcheck.cpp -o adamw_hostcheck
//
// Input, all unsigned integers (floating-point values as their bits): "chunk n_rows shadow_bf16 lr_len has_scale
// found_inf_in", then the float64 beta1 beta2 eps weight_decay max_norm beta1_pow beta2_pow, then "step skipped", the lr_len
// fp32 table entries, the fp32 grad_scale; then per row "numel has_g" and per element "p g m v" (g is there only with
// has_g).  Output: a line "state step skipped found_inf" followed by the bits of beta1_pow, beta2_pow (16 hex digits) and
// grad_norm, clip_coef, decay, w1, b2, w2, step_size, bc2_sqrt, eps (8 hex digits); then per row four lines "p", "m", "v", "s"
// (the shadow, 4 hex digits each).
#include <stdio.h>

#include <vector>

#include "adamw_core.h"

static const int kThreads = 256, kWave = 64;

static bool rd(unsigned long long* u) { return scanf("%llu", u) == 1; }
static bool rd_f32(float* f) {
  unsigned long long u;
  if (!rd(&u)) return false;
  const uint32_t v = (uint32_t)u;
  memcpy(f, &v, 4);
  return true;
}
static bool rd_f64(double* d) {
  unsigned long long u;
  if (!rd(&u)) return false;
  memcpy(d, &u, 8);
  return true;
}
static unsigned long long bits64(double d) { unsigned long long u; memcpy(&u, &d, 8); return u; }

// the workgroup's sum: the butterfly of each wave (every lane ends with the same bits: a + b == b + a), waves in order
static double group_sum(std::vector<double> lanes) {
  for (int o = kWave / 2; o > 0; o >>= 1) {
    std::vector<double> next(lanes.size());
    for (int l = 0; l < kThreads; ++l) next[l] = dd_aw_dadd(lanes[l], lanes[(l & ~(kWave - 1)) | ((l & (kWave - 1)) ^ o)]);
    lanes = next;
  }
  double all = lanes[0];
  for (int w = 1; w < kThreads / kWave; ++w) all = dd_aw_dadd(all, lanes[w * kWave]);
  return all;
}

struct Row {
  std::vector<float> p, g, m, v;
  bool has_g;
};

int main() {
  unsigned long long chunk, n_rows, bf16, lr_len, has_scale, handed, step, skipped;
  if (!rd(&chunk) || !rd(&n_rows) || !rd(&bf16) || !rd(&lr_len) || !rd(&has_scale) || !rd(&handed)) return 2;
  if (chunk != DD_ADAMW_CHUNK || lr_len < 1 || lr_len > 1024 || n_rows > 4096) return 2;
  double beta1, beta2, eps, wd, max_norm;
  dd_adamw_state st;
  memset(&st, 0, sizeof st);
  if (!rd_f64(&beta1) || !rd_f64(&beta2) || !rd_f64(&eps) || !rd_f64(&wd) || !rd_f64(&max_norm) || !rd_f64(&st.beta1_pow) ||
      !rd_f64(&st.beta2_pow) || !rd(&step) || !rd(&skipped))
    return 2;
  st.step = (int64_t)step;
  st.skipped = (int64_t)skipped;
  std::vector<float> lr(lr_len);
  for (float& f : lr)
    if (!rd_f32(&f)) return 2;
  float scale;
  if (!rd_f32(&scale)) return 2;
  std::vector<Row> rows(n_rows);
  for (Row& r : rows) {
    unsigned long long n, has_g;
    if (!rd(&n) || !rd(&has_g) || n > (1u << 24)) return 2;
    r.has_g = has_g != 0;
    r.p.resize(n); r.g.resize(n); r.m.resize(n); r.v.resize(n);
    for (size_t i = 0; i < n; ++i) {
      if (!rd_f32(&r.p[i])) return 2;
      if (r.has_g && !rd_f32(&r.g[i])) return 2;
      if (!rd_f32(&r.m[i]) || !rd_f32(&r.v[i])) return 2;
    }
  }
  const float inv = has_scale ? dd_aw_inv_scale(scale) : 1.0f;
  // launch 1: a workgroup per chunk; lane l takes elements 4 (256 i + l) + c in rising i, c
  std::vector<double> partials;
  bool bad = false;
  for (const Row& r : rows)
    for (size_t at = 0; at < r.p.size(); at += DD_ADAMW_CHUNK) {
      std::vector<double> lanes(kThreads, 0.0);
      const size_t n = r.p.size() - at < DD_ADAMW_CHUNK ? r.p.size() - at : DD_ADAMW_CHUNK;
      if (r.has_g)
        for (int l = 0; l < kThreads; ++l)
          for (size_t i = 0; i < DD_ADAMW_CHUNK / (4 * kThreads); ++i)
            for (size_t c = 0; c < 4; ++c) {
              const size_t e = 4 * (i * kThreads + l) + c;
              if (e >= n) continue;
              const float gu = dd_aw_unscale(r.g[at + e], inv);
              bad = bad || dd_aw_nonfinite(gu);
              lanes[l] = dd_aw_dadd(lanes[l], dd_aw_square(gu));
            }
      partials.push_back(group_sum(lanes));
    }
  // launch 2: lane l sums partials l + 256 i
  std::vector<double> lanes(kThreads, 0.0);
  for (size_t i = 0; i < partials.size(); ++i) lanes[i % kThreads] = dd_aw_dadd(lanes[i % kThreads], partials[i]);
  dd_aw_scalars(&st, group_sum(lanes), bad || handed != 0, inv, lr.data(), (int32_t)lr_len, beta1, beta2, eps, wd, max_norm);
  // launch 3
  if (!st.found_inf) {
    const dd_aw_coef c = dd_aw_coef_of(&st);
    for (Row& r : rows)
      for (size_t i = 0; r.has_g && i < r.p.size(); ++i) dd_aw_update(r.g[i], &r.p[i], &r.m[i], &r.v[i], c);
  }
  printf("state %lld %lld %d %016llx %016llx", (long long)st.step, (long long)st.skipped, (int)st.found_inf,
         bits64(st.beta1_pow), bits64(st.beta2_pow));
  const float out[9] = {st.grad_norm, st.clip_coef, st.decay, st.w1, st.b2, st.w2, st.step_size, st.bc2_sqrt, st.eps};
  for (float f : out) printf(" %08x", (unsigned)dd_aw_bits(f));
  printf("\n");
  for (const Row& r : rows) {
    const std::vector<float>* what[3] = {&r.p, &r.m, &r.v};
    const char* name[3] = {"p", "m", "v"};
    for (int k = 0; k < 3; ++k) {
      printf("%s", name[k]);
      for (float f : *what[k]) printf(" %08x", (unsigned)dd_aw_bits(f));
      printf("\n");
    }
    printf("s");
    for (float f : r.p) printf(" %04x", (unsigned)(bf16 ? dd_aw_bf16_bits(f) : dd_aw_f16_bits(f)));
    printf("\n");
  }
  return 0;
}
