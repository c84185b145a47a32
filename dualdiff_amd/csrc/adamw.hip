// Fused optimizer step: GradScaler's unscale, torch.nn.utils.clip_grad_norm_ and torch.optim.AdamW's update
// (runner/multiview_runner.py:512-521 of the reference) in three launches over a table of parameter tensors, with the step
// count, the learning rate and the skip decision in device memory.  The arithmetic is csrc/adamw_core.h, which also
// compiles for the host.
//
//  * dd_adamw_norm_kernel: a workgroup per chunk of DD_ADAMW_CHUNK gradient elements.  Lane l takes elements
//    4 (256 i + l) .. + 3 of the chunk in rising i — one 16-byte load where the gradient is 16-byte aligned, four dword
//    loads otherwise, the same elements either way, so the order of the sum does not depend on where the tensor lies —
//    and adds fl32(g * inv_scale)^2 in float64; the wave's butterfly, the four waves in order: one partial and one
//    "saw a non-finite value" mark per chunk.  Nothing is cleared beforehand, nothing is added atomically.
//  * dd_adamw_scalars_kernel: one workgroup sums the partials the same way and lane 0 runs dd_aw_scalars on the state block.
//  * dd_adamw_update_kernel: a workgroup per chunk; reads found_inf and returns when it is set.  The update is
//    elementwise, so the access shape is free: 16-byte loads and stores from the first element at which p, g, m and v are
//    all 16-byte aligned (rows carved from one flat buffer share the offset), a scalar head before it and a scalar tail
//    after the last full vector; where the four pointers disagree, coalesced dword accesses.  34 bytes per element with a
//    shadow: memory-bound, 8 vectors per lane, no LDS.
#include "dd_common.h"
#include "adamw_core.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / DD_WAVE;
constexpr int kVecs = DD_ADAMW_CHUNK / (4 * kThreads);
static_assert(DD_ADAMW_CHUNK % (4 * kThreads) == 0, "a chunk is a whole number of 16-byte vectors per lane");
static_assert(sizeof(dd_adamw_row) == 48 && sizeof(dd_adamw_state) == 96, "the layouts the header promises");

// The table's pointers are read from memory, so the compiler cannot know that they are global addresses: say it, or
// every access is a flat one.
typedef __attribute__((address_space(1))) float gfloat;
typedef __attribute__((address_space(1))) const float gcfloat;
typedef __attribute__((address_space(1))) uint16_t ghalf;
typedef __attribute__((address_space(1))) f32x4 gf32x4;
typedef __attribute__((address_space(1))) const f32x4 gcf32x4;
typedef __attribute__((address_space(1))) u32x2 gu32x2;
template <typename G>
__device__ __forceinline__ G* as_global(const void* p) { return (G*)reinterpret_cast<uintptr_t>(p); }

// DD_ADAMW_NT: bit 0 = non-temporal stores, bit 1 = non-temporal loads in launch 3's 16-byte body.  Both: 12 GB stream
// through once per step and nothing is read again before it has left every cache.  Same-machine A/B on one branch, three
// alternating rounds (profiles/adamw.txt): launch 3 1886 - 1911 us plain, 1851 - 1859 us with both (-2.5 %), either one
// alone within 1 % of plain; the whole step 2345 - 2372 against 2251 - 2265 us.  -DDD_ADAMW_NT=0 builds the plain form.
#ifndef DD_ADAMW_NT
#define DD_ADAMW_NT 3
#endif
__device__ __forceinline__ f32x4 ld4(gcfloat* q) {
#if DD_ADAMW_NT & 2
  return __builtin_nontemporal_load((gcf32x4*)q);
#else
  return *(gcf32x4*)q;
#endif
}
__device__ __forceinline__ void st4(gfloat* q, f32x4 x) {
#if DD_ADAMW_NT & 1
  __builtin_nontemporal_store(x, (gf32x4*)q);
#else
  *(gf32x4*)q = x;
#endif
}
__device__ __forceinline__ void st2(ghalf* q, u32x2 x) {
#if DD_ADAMW_NT & 1
  __builtin_nontemporal_store(x, (gu32x2*)q);
#else
  *(gu32x2*)q = x;
#endif
}

struct StepArgs {
  const dd_adamw_row* rows;
  const int32_t* chunks;
  dd_adamw_state* state;
  double* partials;
  int32_t* marks;
  const float* lr_table;
  const float* grad_scale;
  const float* found_inf_in;
  double beta1, beta2, eps, weight_decay, max_norm;
  int64_t n_chunks;
  int32_t n_rows, lr_len, shadow_bf16;
};

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = dd_aw_dadd(v, __shfl_xor(v, o, 64));
  return v;
}

// the workgroup's sum in a fixed order: the wave's butterfly, waves 0..3 one after the other
__device__ __forceinline__ double group_sum(double acc, double* s_w) {
  const int tid = threadIdx.x;
  acc = wave_sum(acc);
  if ((tid & (DD_WAVE - 1)) == 0) s_w[tid / DD_WAVE] = acc;
  __syncthreads();
  double all = s_w[0];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) all = dd_aw_dadd(all, s_w[w]);
  return all;
}

__device__ __forceinline__ float inv_scale_of(const float* grad_scale) {
  return grad_scale ? dd_aw_inv_scale(grad_scale[0]) : 1.0f;
}

// The chunk's row and extent; false: the pair names nothing (or a row without a gradient).
__device__ __forceinline__ bool chunk_of(const StepArgs& a, dd_adamw_row* r, int64_t* off, int32_t* n) {
  const int64_t c = blockIdx.x;
  const int32_t row = a.chunks[2 * c], ci = a.chunks[2 * c + 1];
  if (row < 0 || row >= a.n_rows || ci < 0) return false;
  *r = a.rows[row];
  *off = (int64_t)ci * DD_ADAMW_CHUNK;
  if (!r->g || *off >= r->numel) return false;
  const int64_t left = r->numel - *off;
  *n = (int32_t)(left < DD_ADAMW_CHUNK ? left : DD_ADAMW_CHUNK);
  return true;
}

__global__ __launch_bounds__(kThreads)
void dd_adamw_norm_kernel(StepArgs a) {
  __shared__ double s_w[kWaves];
  const int tid = threadIdx.x;
  dd_adamw_row r;
  int64_t off = 0;
  int32_t n = 0;
  double acc = 0.0;
  int bad = 0;
  if (chunk_of(a, &r, &off, &n)) {                                   // uniform over the workgroup
    const float inv = inv_scale_of(a.grad_scale);
    gcfloat* g = as_global<gcfloat>(r.g) + off;
    const bool vec = (reinterpret_cast<uintptr_t>(g) & 15u) == 0;
#pragma unroll
    for (int i = 0; i < kVecs; ++i) {
      const int32_t e = 4 * (i * kThreads + tid);
      if (e >= n) break;
      float x[4] = {0.0f, 0.0f, 0.0f, 0.0f};                         // past the end: +0, which leaves the sum's bits alone
      if (vec && e + 4 <= n) {
        const f32x4 q = *(gcf32x4*)(g + e);
        x[0] = q[0]; x[1] = q[1]; x[2] = q[2]; x[3] = q[3];
      } else {
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (e + c < n) x[c] = g[e + c];
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float gu = dd_aw_unscale(x[c], inv);
        bad |= dd_aw_nonfinite(gu) ? 1 : 0;
        acc = dd_aw_dadd(acc, dd_aw_square(gu));
      }
    }
  }
  const double all = group_sum(acc, s_w);
  const int any = __syncthreads_or(bad);
  if (tid == 0) {
    a.partials[blockIdx.x] = all;
    a.marks[blockIdx.x] = any ? 1 : 0;
  }
}

__global__ __launch_bounds__(kThreads)
void dd_adamw_scalars_kernel(StepArgs a) {
  __shared__ double s_w[kWaves];
  const int tid = threadIdx.x;
  double acc = 0.0;
  int bad = 0;
  for (int64_t i = tid; i < a.n_chunks; i += kThreads) {
    acc = dd_aw_dadd(acc, a.partials[i]);
    bad |= a.marks[i];
  }
  const double all = group_sum(acc, s_w);
  const int any = __syncthreads_or(bad);
  if (tid == 0) {
    const bool handed = a.found_inf_in && a.found_inf_in[0] != 0.0f;
    dd_aw_scalars(a.state, all, any != 0 || handed, inv_scale_of(a.grad_scale), a.lr_table, a.lr_len, a.beta1, a.beta2,
                  a.eps, a.weight_decay, a.max_norm);
  }
}

__device__ __forceinline__ uint16_t shadow_bits(float p, int bf16) { return bf16 ? dd_aw_bf16_bits(p) : dd_aw_f16_bits(p); }

__device__ __forceinline__ void update_one(gfloat* p, gcfloat* g, gfloat* m, gfloat* v, ghalf* sh, int32_t e, int bf16,
                                           const dd_aw_coef& c) {
  float pe = p[e], me = m[e], ve = v[e];
  dd_aw_update(g[e], &pe, &me, &ve, c);
  p[e] = pe; m[e] = me; v[e] = ve;
  if (sh) sh[e] = shadow_bits(pe, bf16);
}

__global__ __launch_bounds__(kThreads)
void dd_adamw_update_kernel(StepArgs a) {
  if (a.state->found_inf) return;
  const int tid = threadIdx.x;
  dd_adamw_row r;
  int64_t off = 0;
  int32_t n = 0;
  if (!chunk_of(a, &r, &off, &n)) return;
  const dd_aw_coef c = dd_aw_coef_of(a.state);
  gfloat* p = as_global<gfloat>(r.p) + off;
  gcfloat* g = as_global<gcfloat>(r.g) + off;
  gfloat* m = as_global<gfloat>(r.m) + off;
  gfloat* v = as_global<gfloat>(r.v) + off;
  ghalf* sh = r.shadow ? as_global<ghalf>(r.shadow) + off : nullptr;
  const int bf16 = a.shadow_bf16;
  // head: the elements before the first 16-byte line, when the four pointers share their place in it; nvec: full vectors
  const uintptr_t place = reinterpret_cast<uintptr_t>(p) & 15u;
  const bool together = (reinterpret_cast<uintptr_t>(g) & 15u) == place && (reinterpret_cast<uintptr_t>(m) & 15u) == place &&
                        (reinterpret_cast<uintptr_t>(v) & 15u) == place;
  int32_t head = (int32_t)(((16u - place) & 15u) >> 2);
  if (head > n) head = n;
  const int32_t nvec = together ? (n - head) >> 2 : 0;
  if (!together) head = 0;
  const int32_t tail = head + 4 * nvec;
  if (tid < head) update_one(p, g, m, v, sh, tid, bf16, c);
  const bool sh8 = sh && ((reinterpret_cast<uintptr_t>(sh + head) & 7u) == 0);
  for (int32_t k = tid; k < nvec; k += kThreads) {
    const int32_t e = head + 4 * k;
    f32x4 pq = ld4(p + e);
    const f32x4 gq = ld4(g + e);
    f32x4 mq = ld4(m + e);
    f32x4 vq = ld4(v + e);
    uint16_t h[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float pe = pq[j], me = mq[j], ve = vq[j];
      dd_aw_update(gq[j], &pe, &me, &ve, c);
      pq[j] = pe; mq[j] = me; vq[j] = ve;
      h[j] = shadow_bits(pe, bf16);
    }
    st4(p + e, pq);
    st4(m + e, mq);
    st4(v + e, vq);
    if (sh8) {
      u32x2 w;
      w[0] = (uint32_t)h[0] | ((uint32_t)h[1] << 16);
      w[1] = (uint32_t)h[2] | ((uint32_t)h[3] << 16);
      st2(sh + e, w);
    } else if (sh) {
#pragma unroll
      for (int j = 0; j < 4; ++j) sh[e + j] = h[j];
    }
  }
  for (int32_t e = tail + tid; e < n; e += kThreads) update_one(p, g, m, v, sh, e, bf16, c);
}

bool misaligned(const void* p, uintptr_t al) { return (reinterpret_cast<uintptr_t>(p) & (al - 1)) != 0; }

}  // namespace

extern "C" int64_t dd_adamw_workspace_bytes(int64_t n_chunks) {
  if (n_chunks < 0 || n_chunks > 2147483647) return -1;
  const int64_t n = n_chunks > 0 ? n_chunks : 1;
  return n * (int64_t)(sizeof(double) + sizeof(int32_t));
}

extern "C" int dd_adamw_step(const dd_adamw_row* rows, int32_t n_rows, const int32_t* chunks, int64_t n_chunks,
                             dd_adamw_state* state, const float* lr_table, int32_t lr_len, const float* grad_scale,
                             const float* found_inf_in, double beta1, double beta2, double eps, double weight_decay,
                             double max_norm, int32_t shadow_dtype, void* workspace, int64_t workspace_bytes,
                             int32_t launches, dd_stream_t stream) {
  if (!state || !lr_table || !workspace) return DD_ERR_BAD_ARG;
  if (n_rows < 0 || n_chunks < 0 || n_chunks > 2147483647 || lr_len < 1) return DD_ERR_BAD_ARG;
  if ((n_rows > 0 && !rows) || (n_chunks > 0 && !chunks)) return DD_ERR_BAD_ARG;
  if (!(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0)) return DD_ERR_BAD_ARG;
  if (!(eps >= 0.0 && isfinite(eps) && weight_decay >= 0.0 && isfinite(weight_decay)) || max_norm != max_norm)
    return DD_ERR_BAD_ARG;
  if (shadow_dtype != DD_F16 && shadow_dtype != DD_BF16) return DD_ERR_BAD_ARG;
  if (launches < 1 || launches > DD_ADAMW_ALL) return DD_ERR_BAD_ARG;
  if (misaligned(rows, 8) || misaligned(chunks, 4) || misaligned(state, 8) || misaligned(lr_table, 4) ||
      misaligned(grad_scale, 4) || misaligned(found_inf_in, 4) || misaligned(workspace, 8))
    return DD_ERR_BAD_ARG;
  const int64_t need = dd_adamw_workspace_bytes(n_chunks);
  if (need < 0 || workspace_bytes < need) return DD_ERR_BAD_ARG;
  StepArgs a;
  a.rows = rows; a.chunks = chunks; a.state = state;
  a.partials = static_cast<double*>(workspace);
  a.marks = reinterpret_cast<int32_t*>(a.partials + (n_chunks > 0 ? n_chunks : 1));
  a.lr_table = lr_table; a.grad_scale = grad_scale; a.found_inf_in = found_inf_in;
  a.beta1 = beta1; a.beta2 = beta2; a.eps = eps; a.weight_decay = weight_decay; a.max_norm = max_norm;
  a.n_chunks = n_chunks; a.n_rows = n_rows; a.lr_len = lr_len; a.shadow_bf16 = shadow_dtype == DD_BF16 ? 1 : 0;
  dd_clear_error();
  if ((launches & 1) && n_chunks > 0)
    hipLaunchKernelGGL(dd_adamw_norm_kernel, dim3((unsigned)n_chunks), dim3(kThreads), 0, dd_stream(stream), a);
  if (launches & 2) hipLaunchKernelGGL(dd_adamw_scalars_kernel, dim3(1), dim3(kThreads), 0, dd_stream(stream), a);
  if ((launches & 4) && n_chunks > 0)
    hipLaunchKernelGGL(dd_adamw_update_kernel, dim3((unsigned)n_chunks), dim3(kThreads), 0, dd_stream(stream), a);
  return dd_check_launch();
}
