// Fused optimizer step, the arithmetic core: what csrc/adamw.hip computes per gradient element (the unscale, the square
// for the norm), once per step (the scalars: norm, clip coefficient, skip decision, step count, bias corrections) and per
// parameter element (torch.optim.AdamW's single-tensor update with the unscale and the clip folded in), as plain functions
// that compile for the device and for the host.  The stand-alone host program tools/adamw_hostcheck.cpp runs them in the
// kernels' chunk order, and tests/test_adamw_cpu.py compares its output bit for bit with the numpy restatement
// (tests/adamw_reference.py) without a GPU.
//
// The update, every line one IEEE fp32 operation (no contraction, division and square root correctly rounded):
//   gu = fl(g * inv_scale)                          inv_scale = fp32(1 / float64(grad_scale))
//   gc = fl(gu * clip_coef)
//   p  = fl(p * decay)                              decay     = fp32(1 - lr * wd)
//   m  = fl(m + fl(w1 * fl(gc - m)))                w1        = fp32(1 - beta1)
//   v  = fl(fl(v * b2) + fl(fl(w2 * gc) * gc))      w2        = fp32(1 - beta2), b2 = fp32(beta2)
//   den = fl(fl(sqrt(v) / bc2_sqrt) + eps)          bc2_sqrt  = fp32(sqrt(1 - beta2^step))
//   p  = fl(p - fl(step_size * fl(m / den)))        step_size = fp32(lr / (1 - beta1^step))
//   shadow = p rounded to nearest even in fp16 or bf16
// — torch/optim/adamw.py's _single_tensor_adamw (amsgrad=False, maximize=False) after GradScaler's unscale and
// torch.nn.utils.clip_grad_norm_.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/dualdiff_hip.h"

#if defined(__HIPCC__)
#define DD_AW_HD __host__ __device__ __forceinline__
#else
#define DD_AW_HD inline
#endif

// One IEEE operation each: the pragma takes the `contract` flag off the operation itself, which survives inlining (as in
// csrc/bev_map_core.h); adamw.hip is also compiled with -ffp-contract=off, and so is the host program, which keeps the
// results in volatiles for compilers without the pragma.
#if defined(__clang__)
#define DD_AW_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define DD_AW_NO_CONTRACT
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define DD_AW_RESULT
#else
#define DD_AW_RESULT volatile
#endif
DD_AW_HD float dd_aw_mul(float a, float b) { DD_AW_NO_CONTRACT DD_AW_RESULT float r = a * b; return r; }
DD_AW_HD float dd_aw_add(float a, float b) { DD_AW_NO_CONTRACT DD_AW_RESULT float r = a + b; return r; }
DD_AW_HD float dd_aw_sub(float a, float b) { DD_AW_NO_CONTRACT DD_AW_RESULT float r = a - b; return r; }
DD_AW_HD float dd_aw_div(float a, float b) { DD_AW_NO_CONTRACT DD_AW_RESULT float r = a / b; return r; }
DD_AW_HD float dd_aw_sqrt(float a) { DD_AW_RESULT float r = sqrtf(a); return r; }
DD_AW_HD double dd_aw_dmul(double a, double b) { DD_AW_NO_CONTRACT DD_AW_RESULT double r = a * b; return r; }
DD_AW_HD double dd_aw_dadd(double a, double b) { DD_AW_NO_CONTRACT DD_AW_RESULT double r = a + b; return r; }
DD_AW_HD double dd_aw_dsub(double a, double b) { DD_AW_NO_CONTRACT DD_AW_RESULT double r = a - b; return r; }
DD_AW_HD double dd_aw_ddiv(double a, double b) { DD_AW_NO_CONTRACT DD_AW_RESULT double r = a / b; return r; }

DD_AW_HD uint32_t dd_aw_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
DD_AW_HD bool dd_aw_nonfinite(float f) { return (dd_aw_bits(f) & 0x7f800000u) == 0x7f800000u; }

// ---- per gradient element: launch 1 ----------------------------------------------------------------------------------
// GradScaler._unscale_grads_: inv_scale = scale.double().reciprocal().float()
DD_AW_HD float dd_aw_inv_scale(float scale) { return (float)dd_aw_ddiv(1.0, (double)scale); }
DD_AW_HD float dd_aw_unscale(float g, float inv_scale) { return dd_aw_mul(g, inv_scale); }
// fp32 x fp32 is exact in float64 (48 bits of product)
DD_AW_HD double dd_aw_square(float gu) { return dd_aw_dmul((double)gu, (double)gu); }

// ---- once per step: launch 2 -------------------------------------------------------------------------------------------
// sum: the float64 sum of the squares; bad: a gradient element was not finite after the unscale, or the scaler handed a
// non-zero found_inf in.  grad_norm and clip_coef are written on every step, taken or not; a skipped step changes
// nothing else but found_inf and skipped.
DD_AW_HD void dd_aw_scalars(dd_adamw_state* s, double sum, bool bad, float inv_scale, const float* lr_table, int32_t lr_len,
                            double beta1, double beta2, double eps, double weight_decay, double max_norm) {
  const double norm = sqrt(sum);
  double coef = 1.0;
  if (max_norm >= 0.0) {
    coef = dd_aw_ddiv(max_norm, dd_aw_dadd(norm, 1e-6));
    if (!(coef < 1.0)) coef = 1.0;                                    // clamp(max=1); a NaN norm belongs to a skipped step
  }
  s->grad_norm = (float)norm;
  s->clip_coef = (float)coef;
  s->inv_scale = inv_scale;
  s->found_inf = bad ? 1 : 0;
  if (bad) {
    s->skipped += 1;
    return;
  }
  s->step += 1;
  s->beta1_pow = dd_aw_dmul(s->beta1_pow, beta1);
  s->beta2_pow = dd_aw_dmul(s->beta2_pow, beta2);
  const int64_t at = s->step - 1 < (int64_t)lr_len - 1 ? s->step - 1 : (int64_t)lr_len - 1;
  const float lr = lr_table[at];
  s->lr = lr;
  s->decay = (float)dd_aw_dsub(1.0, dd_aw_dmul((double)lr, weight_decay));
  s->w1 = (float)dd_aw_dsub(1.0, beta1);
  s->b2 = (float)beta2;
  s->w2 = (float)dd_aw_dsub(1.0, beta2);
  s->step_size = (float)dd_aw_ddiv((double)lr, dd_aw_dsub(1.0, s->beta1_pow));
  s->bc2_sqrt = (float)sqrt(dd_aw_dsub(1.0, s->beta2_pow));
  s->eps = (float)eps;
}

// ---- per parameter element: launch 3 -----------------------------------------------------------------------------------
struct dd_aw_coef {
  float inv_scale, clip_coef, decay, w1, b2, w2, step_size, bc2_sqrt, eps;
};
DD_AW_HD dd_aw_coef dd_aw_coef_of(const dd_adamw_state* s) {
  dd_aw_coef c;
  c.inv_scale = s->inv_scale; c.clip_coef = s->clip_coef; c.decay = s->decay; c.w1 = s->w1; c.b2 = s->b2; c.w2 = s->w2;
  c.step_size = s->step_size; c.bc2_sqrt = s->bc2_sqrt; c.eps = s->eps;
  return c;
}
DD_AW_HD void dd_aw_update(float g, float* p, float* m, float* v, const dd_aw_coef& c) {
  const float gc = dd_aw_mul(dd_aw_unscale(g, c.inv_scale), c.clip_coef);
  const float pd = dd_aw_mul(*p, c.decay);
  const float mn = dd_aw_add(*m, dd_aw_mul(c.w1, dd_aw_sub(gc, *m)));
  const float vn = dd_aw_add(dd_aw_mul(*v, c.b2), dd_aw_mul(dd_aw_mul(c.w2, gc), gc));
  const float den = dd_aw_add(dd_aw_div(dd_aw_sqrt(vn), c.bc2_sqrt), c.eps);
  *p = dd_aw_sub(pd, dd_aw_mul(c.step_size, dd_aw_div(mn, den)));
  *m = mn;
  *v = vn;
}

// fp32 -> the bits of the nearest bf16 / fp16, ties to even (what torch's .to(dtype) stores)
DD_AW_HD uint16_t dd_aw_bf16_bits(float f) {
  const uint32_t u = dd_aw_bits(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0;
  return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
DD_AW_HD uint16_t dd_aw_f16_bits(float f) {
#if defined(__HIP_DEVICE_COMPILE__)
  const _Float16 h = (_Float16)f;                                     // v_cvt_f16_f32: nearest even, overflow to infinity
  uint16_t r;
  memcpy(&r, &h, 2);
  return r;
#else
  uint32_t x = dd_aw_bits(f);
  const uint32_t sign = (x >> 16) & 0x8000u;
  x &= 0x7fffffffu;
  if (x >= 0x7f800000u) return (uint16_t)(sign | (x > 0x7f800000u ? 0x7e00u : 0x7c00u));
  if (x >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);            // 65520 and above round to infinity
  if (x <= 0x33000000u) return (uint16_t)sign;                        // 2^-25 and below round to zero
  if (x < 0x38800000u) {                                              // a subnormal half: units of 2^-24
    const int shift = 126 - (int)(x >> 23);                           // 14..24
    const uint32_t mant = (x & 0x7fffffu) | 0x800000u, half = 1u << (shift - 1);
    uint32_t r = mant >> shift;
    const uint32_t rem = mant & ((1u << shift) - 1u);
    if (rem > half || (rem == half && (r & 1u))) ++r;
    return (uint16_t)(sign | r);
  }
  uint32_t r = (x - 0x38000000u) >> 13;
  const uint32_t rem = x & 0x1fffu;
  if (rem > 0x1000u || (rem == 0x1000u && (r & 1u))) ++r;
  return (uint16_t)(sign | r);
#endif
}
