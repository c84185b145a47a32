// Cross-attention PROBABILITIES for gfx950 (head_dim 40 / 80 / 160, at most DD_ATTN_PROBS_MAX_LK keys):
//        w[b,h,i,j] = softmax_{j < n}( scale * Q[b,i,h,:] . K[b,j,h,:] )
// written as float32, per head or as the mean over the heads — what the reference keeps for its attention heat maps
// (tools/unet_modify.py:31,47; pipeline/explore_pipeline_bev_controlnet.py:437-453).  dd_attention and dd_xattn320 never
// form these numbers in memory; this kernel OBSERVES a layer (same q, same k) and leaves its hidden states alone.
//
// One wave owns (batch entry, 16 query rows) across ALL heads: no atomics, the head mean is a sum in head order, and
// the result does not change from run to run.  Products as in attention.hip ("swapped", the softmax row on a lane):
//        S^T[key][q] = K . Q^T     (MFMA A = K rows, B = Q rows, both read from global memory as 16-byte fragments)
// so lane (g, c) of the result of key tile t holds keys 16 t + 4 g + {0..3} of query row c.  A row of at most 256 scores
// is 16 such tiles = 64 registers: the softmax is a plain two-pass over registers — the exact maximum, then
// p = exp2(fma(s, c, -m)) and the fp32 sum of the unrounded p, one normalisation.  Nothing is rounded to the storage type.
// Keys past n are never read (their fragments are zeros) and never take part in the maximum or the sum.
#include "dd_common.h"

namespace {

constexpr int AP_NT = DD_ATTN_PROBS_MAX_LK / 16;   // key tiles of a row

struct ProbsParams {
  const void* q; const void* k; float* p;
  int64_t ldq, ldk, qbs, kbs, qhs, khs;
  int64_t ldp, pbs, phs;
  int heads, lq, lk, nqb;
  float c;             // scale * log2(e), or 1 for a prescaled q
  float mul;           // weight (per_head) or weight / heads (mean)
  int per_head, accumulate;
  int vec;             // every row of P starts 16-byte aligned: whole float4 groups go out as one store
  const int32_t* lk_dev;
};

template <typename T, int D>
__global__ __launch_bounds__(64)
void dd_attn_probs_kernel(const ProbsParams p) {
  using V8 = typename dd_vec<T>::v8;
  constexpr int KSTEPS = (D + 31) / 32;

  const int lane = threadIdx.x;
  const int g = lane >> 4;
  const int c = lane & 15;
  // keys per batch entry: a kernel argument, or one word of device memory (as dd_attn_desc.lk_dev); p.lk is the capacity
  const int n = p.lk_dev ? min(max(__builtin_amdgcn_readfirstlane(*p.lk_dev), 1), p.lk) : p.lk;
  const int ntiles = (n + 15) >> 4;

  const int b = blockIdx.x / p.nqb;
  const int qrow = (blockIdx.x - b * p.nqb) * 16 + c;
  const bool qok = qrow < p.lq;

  const T* qb = reinterpret_cast<const T*>(p.q) + (int64_t)b * p.qbs + (int64_t)qrow * p.ldq;
  const T* kb = reinterpret_cast<const T*>(p.k) + (int64_t)b * p.kbs;
  float* prow = p.p + (int64_t)b * p.pbs + (int64_t)qrow * p.ldp;

  // v[t][r] * mul -> columns 16 t + 4 g + r of this lane's row.  Store: columns n .. lk-1 are written as zeros;
  // accumulate: they are not touched.  Nothing is written at or past column lk.
  auto emit = [&](float* row, const f32x4 (&v)[AP_NT]) {
    if (!qok) return;
    const int lim = p.accumulate ? n : p.lk;
#pragma unroll
    for (int t = 0; t < AP_NT; ++t) {
      if (t * 16 >= lim) break;                          // uniform
      const int col0 = t * 16 + g * 4;
      float o[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] = (col0 + r < n) ? p.mul * v[t][r] : 0.0f;
      if (p.vec && col0 + 3 < lim) {
        f32x4* dst = reinterpret_cast<f32x4*>(row + col0);
        f32x4 ov = {o[0], o[1], o[2], o[3]};
        if (p.accumulate) {
          const f32x4 old = *dst;
          ov[0] += old[0]; ov[1] += old[1]; ov[2] += old[2]; ov[3] += old[3];
        }
        *dst = ov;
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (col0 + r < lim) row[col0 + r] = p.accumulate ? row[col0 + r] + o[r] : o[r];
      }
    }
  };

  f32x4 macc[AP_NT];
#pragma unroll
  for (int t = 0; t < AP_NT; ++t) macc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int h = 0; h < p.heads; ++h) {
    V8 qf[KSTEPS];
#pragma unroll
    for (int ks = 0; ks < KSTEPS; ++ks) {
      const int d0 = ks * 32 + g * 8;
      u32x4 u = {0u, 0u, 0u, 0u};
      if (qok && d0 < D) u = dd_ld16(qb + (int64_t)h * p.qhs + d0);
      qf[ks] = dd_as_v8<T>(u);
    }
    const T* kh = kb + (int64_t)h * p.khs;

    f32x4 s[AP_NT];
#pragma unroll
    for (int t = 0; t < AP_NT; ++t) {
      s[t] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (t < ntiles) {                                  // uniform
        const int krow = t * 16 + c;
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks) {
          const int d0 = ks * 32 + g * 8;
          u32x4 u = {0u, 0u, 0u, 0u};
          if (krow < n && d0 < D) u = dd_ld16(kh + (int64_t)krow * p.ldk + d0);
          s[t] = dd_mfma16(dd_as_v8<T>(u), qf[ks], s[t]);
        }
      }
    }

    // exact row maximum over the n keys: this lane's keys, then the three other lane groups of the same query row
    float mx = -INFINITY;
#pragma unroll
    for (int t = 0; t < AP_NT; ++t)
      if (t < ntiles) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (t * 16 + g * 4 + r < n) mx = fmaxf(mx, s[t][r]);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float m = mx * p.c;

    float l = 0.f;
#pragma unroll
    for (int t = 0; t < AP_NT; ++t)
      if (t < ntiles) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float pe = (t * 16 + g * 4 + r < n) ? __builtin_amdgcn_exp2f(fmaf(s[t][r], p.c, -m)) : 0.0f;
          s[t][r] = pe;
          l += pe;
        }
      }
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    const float inv = 1.0f / l;                          // l >= the maximum's own p, which is 1 up to rounding

#pragma unroll
    for (int t = 0; t < AP_NT; ++t)
      if (t < ntiles) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float w = __fmul_rn(s[t][r], inv);
          if (p.per_head) s[t][r] = w;
          else macc[t][r] = __fadd_rn(macc[t][r], w);    // head order, fp32
        }
      }
    if (p.per_head) emit(prow + (int64_t)h * p.phs, s);
  }
  if (!p.per_head) emit(prow, macc);
}

template <typename T>
int launch_probs(const ProbsParams& p, int head_dim, int batch, hipStream_t s) {
  const dim3 grid((unsigned)(batch * p.nqb));
  switch (head_dim) {
    case 40: hipLaunchKernelGGL((dd_attn_probs_kernel<T, 40>), grid, dim3(64), 0, s, p); break;
    case 80: hipLaunchKernelGGL((dd_attn_probs_kernel<T, 80>), grid, dim3(64), 0, s, p); break;
    case 160: hipLaunchKernelGGL((dd_attn_probs_kernel<T, 160>), grid, dim3(64), 0, s, p); break;
    default: return DD_ERR_UNSUPPORTED;
  }
  return dd_check_launch();
}

}  // namespace

extern "C" int dd_attn_probs(const void* q, const void* k, float* p, int64_t ldq, int64_t ldk, int64_t q_batch_stride,
                             int64_t k_batch_stride, int64_t q_head_stride, int64_t k_head_stride, int64_t ldp,
                             int64_t p_batch_stride, int64_t p_head_stride, int32_t batch, int32_t lq, int32_t lk,
                             int32_t heads, int32_t head_dim, float scale, int32_t q_prescaled, int32_t per_head,
                             int32_t accumulate, float weight, const int32_t* lk_dev, int32_t qk_dtype,
                             dd_stream_t stream) {
  if (!q || !k || !p) return DD_ERR_BAD_ARG;
  if (batch <= 0 || lq <= 0 || lk <= 0 || heads <= 0 || head_dim <= 0) return DD_ERR_BAD_ARG;
  if (qk_dtype != DD_F16 && qk_dtype != DD_BF16) return DD_ERR_BAD_ARG;
  if (ldq <= 0 || ldk <= 0 || (ldq & 7) || (ldk & 7)) return DD_ERR_BAD_ARG;
  if (q_batch_stride < 0 || k_batch_stride < 0 || (q_batch_stride & 7) || (k_batch_stride & 7)) return DD_ERR_BAD_ARG;
  if (q_head_stride < 0 || k_head_stride < 0 || (q_head_stride & 7) || (k_head_stride & 7)) return DD_ERR_BAD_ARG;
  if (!dd_aligned16(q) || !dd_aligned16(k)) return DD_ERR_BAD_ARG;
  if (reinterpret_cast<uintptr_t>(p) & 3u) return DD_ERR_BAD_ARG;
  if (lk_dev && (reinterpret_cast<uintptr_t>(lk_dev) & 3u)) return DD_ERR_BAD_ARG;
  if (ldp < lk || p_batch_stride < 0 || p_head_stride < 0) return DD_ERR_BAD_ARG;
  if (!q_prescaled && !(scale > 0.0f)) return DD_ERR_BAD_ARG;
  if (head_dim != 40 && head_dim != 80 && head_dim != 160) return DD_ERR_UNSUPPORTED;
  if (lk > DD_ATTN_PROBS_MAX_LK) return DD_ERR_UNSUPPORTED;
  const int nqb = (lq + 15) / 16;
  if ((int64_t)batch * nqb >= ((int64_t)1 << 31)) return DD_ERR_UNSUPPORTED;
  ProbsParams pp;
  pp.q = q; pp.k = k; pp.p = p;
  pp.ldq = ldq; pp.ldk = ldk; pp.qbs = q_batch_stride; pp.kbs = k_batch_stride;
  pp.qhs = q_head_stride ? q_head_stride : head_dim;
  pp.khs = k_head_stride ? k_head_stride : head_dim;
  pp.ldp = ldp; pp.pbs = p_batch_stride; pp.phs = p_head_stride;
  pp.heads = heads; pp.lq = lq; pp.lk = lk; pp.nqb = nqb;
  pp.c = q_prescaled ? 1.0f : scale * 1.44269504088896340736f;
  pp.per_head = per_head ? 1 : 0;
  pp.accumulate = accumulate ? 1 : 0;
  pp.mul = per_head ? weight : weight / (float)heads;
  pp.vec = ((reinterpret_cast<uintptr_t>(p) & 15u) == 0 && !(ldp & 3) && !(p_batch_stride & 3) && !(p_head_stride & 3)) ? 1 : 0;
  pp.lk_dev = lk_dev;
  dd_clear_error();
  return dd_dispatch16(qk_dtype, [&](auto t) {
    return launch_probs<typename decltype(t)::type>(pp, head_dim, batch, dd_stream(stream));
  });
}
