// CLIP text encoder (SD-v1.5 `text_encoder`, transformers.CLIPTextModel): the two pieces the C-ABI lacked.
//
//  * dd_clip_embed: token + position embedding gather (CLIPTextEmbeddings) and the pooling index of every sequence
//    (CLIPTextTransformer: pooler_output = last_hidden_state[b, ids[b].argmax()], or the first eos_token_id) in one launch.
//  * dd_causal_attention: softmax_{j <= i}(scale * q_i . k_j) v_j at head_dim 64 for sequences of at most
//    DD_CAUSAL_ATTN_MAX_L tokens (CLIPAttention with the causal mask only: SD-v1.5 passes no attention_mask).
//
// Causal attention, one wave per (sequence, head, 16-query tile) — a 77-token prompt at b = 2 is 2 x 12 x 5 = 120 waves
// on 120 CUs instead of 24 (sequence, head) pairs.  Products as in attention.hip ("swapped", the softmax row on a lane):
//        S^T[key][q] = K . Q^T     (MFMA A = K rows, B = Q rows, both read from global memory as 16-byte fragments)
//        O^T[d][q]   = V^T . P^T   (MFMA A = V^T via ds_read_b64_tr_b16 from the LDS copy of V, B = P^T in registers)
// A query tile meets at most MAX_L / 16 key tiles, so its whole score strip stays in registers: the softmax is a plain
// two-pass (max, then exp2 and sum), no running max and no rescale.  Key tiles above the diagonal are never multiplied;
// the diagonal tile gets the per-element mask, and a masked score gives p = 0 exactly (a select, not exp2 of -inf).
// Numerics as attention.hip: fp32 scores and softmax with scale * log2(e) folded into exp2, P rounded to the storage type
// before P.V, the row sum taken over the unrounded fp32 p, fp32 accumulation, one rounding at the store.
#include "dd_common.h"

namespace {

constexpr int CA_D = 64;                          // head_dim
constexpr int CA_MAXT = DD_CAUSAL_ATTN_MAX_L / 16; // key tiles a query tile can meet
constexpr int CA_VSTR = CA_D + 8;                 // LDS row pitch of V (elements): 144 B, keeps 16-byte rows off one bank group

struct CausalParams {
  const void* q; const void* k; const void* v; void* o;
  int64_t ldq, ldk, ldv, ldo;
  int64_t qbs, kbs, vbs, obs;
  int l, heads, nqt;
  float scale_log2;
};

template <typename T>
__global__ __launch_bounds__(64)
void dd_causal_attn_kernel(const CausalParams p) {
  using V8 = typename dd_vec<T>::v8;
  using V4 = typename dd_vec<T>::v4;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];   // 32 * ceil(nqt / 2) rows of V: 13.5 KB at l = 77
  T* vs = reinterpret_cast<T*>(smem);

  const int lane = threadIdx.x;
  const int g = lane >> 4;
  const int c = lane & 15;
  const int item = blockIdx.x;
  const int bh = item / p.nqt;
  const int qt = p.nqt - 1 - (item - bh * p.nqt);          // the longest tiles of a (sequence, head) first
  const int b = bh / p.heads;
  const int h = bh - b * p.heads;
  const int l = p.l;

  const T* qbase = reinterpret_cast<const T*>(p.q) + (int64_t)b * p.qbs + h * CA_D;
  const T* kbase = reinterpret_cast<const T*>(p.k) + (int64_t)b * p.kbs + h * CA_D;
  const T* vbase = reinterpret_cast<const T*>(p.v) + (int64_t)b * p.vbs + h * CA_D;

  const int ntile = qt + 1;                                  // key tiles 0 .. qt
  const int nchunk = (ntile + 1) >> 1;                       // 32-key chunks of the P.V product
  // Every global load of the wave is issued before the first result is used (the kernel is one dependent chain: loads issued
  // tile by tile behind uniform branches cost one memory latency per tile).
  // ---- Q fragments: query row q0 + c (clamped: rows past the sequence are computed on row l - 1 and not stored) ----
  const int qrow = qt * 16 + c;
  const int qrd = min(qrow, l - 1);
  V8 qf[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) qf[ks] = dd_as_v8<T>(dd_ld16(qbase + (int64_t)qrd * p.ldq + ks * 32 + g * 8));
  // ---- K fragments of key tiles 0 .. qt (rows clamped likewise: such keys are above the diagonal of every stored row) ----
  u32x4 kreg[CA_MAXT][2];
#pragma unroll
  for (int t = 0; t < CA_MAXT; ++t) {
    kreg[t][0] = kreg[t][1] = u32x4{0u, 0u, 0u, 0u};
    if (t < ntile) {                                          // uniform
      const T* krow = kbase + (int64_t)min(t * 16 + c, l - 1) * p.ldk + g * 8;
      kreg[t][0] = dd_ld16(krow);
      kreg[t][1] = dd_ld16(krow + 32);
    }
  }
  // ---- V rows 0 .. 32 * nchunk - 1 (8 rows per pass of the wave); rows past the sequence are zeros: their p is 0, and
  //      0 * x must stay 0 ----
  u32x4 vreg[CA_MAXT * 2];
  const int vrow = lane >> 3, vch = lane & 7;
#pragma unroll
  for (int it = 0; it < CA_MAXT * 2; ++it) {
    vreg[it] = u32x4{0u, 0u, 0u, 0u};
    if (it < nchunk * 4 && it * 8 + vrow < l) vreg[it] = dd_ld16(vbase + (int64_t)(it * 8 + vrow) * p.ldv + vch * 8);
  }

  // ---- scores: lane (c, g) holds keys t * 16 + g * 4 + r of query c ----
  f32x4 s[CA_MAXT];
#pragma unroll
  for (int t = 0; t < CA_MAXT; ++t) {
    s[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (t < ntile) {                                          // uniform
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) acc = dd_mfma16(dd_as_v8<T>(kreg[t][ks]), qf[ks], acc);
      s[t] = acc;
    }
  }

  // ---- two-pass softmax over the strip (log2 units) ----
  float mx = -INFINITY;
#pragma unroll
  for (int t = 0; t < CA_MAXT; ++t) {
    if (t < ntile) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s[t][r] *= p.scale_log2;
        const bool keep = t < qt || (g * 4 + r) <= c;        // the diagonal tile: key <= query
        if (keep) mx = fmaxf(mx, s[t][r]);
      }
    }
  }
  mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));                    // key 0 is never masked: finite for finite inputs
  float sum = 0.f;
#pragma unroll
  for (int t = 0; t < CA_MAXT; ++t) {
    if (t < ntile) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool keep = t < qt || (g * 4 + r) <= c;
        const float pe = keep ? __builtin_amdgcn_exp2f(s[t][r] - mx) : 0.f;
        s[t][r] = pe;
        sum += pe;
      }
    }
  }
  sum += __shfl_xor(sum, 16, 64);
  sum += __shfl_xor(sum, 32, 64);

#pragma unroll
  for (int it = 0; it < CA_MAXT * 2; ++it)
    if (it < nchunk * 4) dd_st16(vs + (it * 8 + vrow) * CA_VSTR + vch * 8, vreg[it]);   // uniform
  __syncthreads();                                            // V tile visible

  // ---- O^T = V^T . P^T over 32-key chunks ----
  f32x4 oacc[CA_D / 16];
#pragma unroll
  for (int dt = 0; dt < CA_D / 16; ++dt) oacc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int cc = 0; cc < CA_MAXT / 2; ++cc) {
    if (cc < nchunk) {                                        // uniform
      V8 pf;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        pf[r] = (T)s[2 * cc][r];
        pf[4 + r] = (T)s[2 * cc + 1][r];                      // a tile above the diagonal: zeros
      }
#pragma unroll
      for (int dt = 0; dt < CA_D / 16; ++dt) {
        V8 vf;
        const T* a0 = vs + (cc * 32 + g * 4 + (c >> 2)) * CA_VSTR + dt * 16 + (c & 3) * 4;
        const T* a1 = a0 + 16 * CA_VSTR;
        s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3)))*)(a0));
        s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3)))*)(a1));
        __builtin_memcpy(&vf, &lo, 8);
        __builtin_memcpy(reinterpret_cast<char*>(&vf) + 8, &hi, 8);
        oacc[dt] = dd_mfma16(vf, pf, oacc[dt]);
      }
    }
  }

  if (qrow >= l) return;
  const float inv = 1.0f / sum;
  T* orow = reinterpret_cast<T*>(p.o) + (int64_t)b * p.obs + (int64_t)qrow * p.ldo + h * CA_D;
#pragma unroll
  for (int dt = 0; dt < CA_D / 16; ++dt) {
    V4 ov;
#pragma unroll
    for (int e = 0; e < 4; ++e) ov[e] = (T)(oacc[dt][e] * inv);
    *reinterpret_cast<V4*>(orow + dt * 16 + g * 4) = ov;
  }
}

// ---- embedding gather + pooling index ---------------------------------------------------------------------------------
// Blocks 0 .. nb_rows - 1 walk the (row, 16-byte chunk) pairs of the output; the blocks after them find the pooling
// position, one wave per sequence.
template <typename T>
__global__ __launch_bounds__(256)
void dd_clip_embed_kernel(const int64_t* __restrict__ ids, const T* __restrict__ tok, const T* __restrict__ pos,
                          T* __restrict__ out, int32_t* __restrict__ pool, int batch, int l, int c, int vocab, int eos,
                          int nb_rows) {
  if ((int)blockIdx.x < nb_rows) {
    const int cpr = c >> 3;
    const int64_t total = (int64_t)batch * l * cpr;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int64_t row = idx / cpr;
    const int ch = (int)(idx - row * cpr);
    const int t = (int)(row % l);
    int64_t id = ids[row];
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);        // no id can read outside the table
    float a[8], b[8];
    dd_unpack8<T>(dd_ld16(tok + id * c + ch * 8), a);
    dd_unpack8<T>(dd_ld16(pos + (int64_t)t * c + ch * 8), b);
#pragma unroll
    for (int e = 0; e < 8; ++e) a[e] += b[e];
    dd_st16(out + row * c + ch * 8, dd_pack8<T>(a));
    return;
  }
  const int seq = ((int)blockIdx.x - nb_rows) * 4 + (threadIdx.x >> 6);
  if (seq >= batch) return;
  const int lane = threadIdx.x & 63;
  const int64_t* row = ids + (int64_t)seq * l;
  // eos == 2 (SD-v1.5's config): first position of the largest id; else: first position holding eos, 0 when absent
  int64_t best = INT64_MIN;
  int at = INT32_MAX;
  for (int j = lane; j < l; j += 64) {
    const int64_t id = row[j];
    if (eos == 2) {
      if (id > best) { best = id; at = j; }
    } else if (id == eos && j < at) {
      at = j;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int64_t ob = __shfl_xor(best, o, 64);
    const int oa = __shfl_xor(at, o, 64);
    if (ob > best || (ob == best && oa < at)) { best = ob; at = oa; }
  }
  if (lane == 0) pool[seq] = at == INT32_MAX ? 0 : at;
}

}  // namespace

extern "C" int dd_clip_embed(const int64_t* ids, const void* tok, const void* pos, void* out, int32_t* pool_index,
                             int32_t batch, int32_t l, int32_t c, int32_t vocab, int32_t eos_token_id, int32_t dtype,
                             dd_stream_t stream) {
  if (!ids || !tok || !pos || !out || !pool_index) return DD_ERR_BAD_ARG;
  if (batch <= 0 || l <= 0 || c <= 0 || vocab <= 0) return DD_ERR_BAD_ARG;
  if (dtype != DD_F16 && dtype != DD_BF16) return DD_ERR_BAD_ARG;
  if (c & 7) return DD_ERR_BAD_ARG;
  if (!dd_aligned16(tok) || !dd_aligned16(pos) || !dd_aligned16(out)) return DD_ERR_BAD_ARG;
  if ((reinterpret_cast<uintptr_t>(ids) & 7u) || (reinterpret_cast<uintptr_t>(pool_index) & 3u)) return DD_ERR_BAD_ARG;
  const int64_t chunks = (int64_t)batch * l * (c >> 3);
  const int64_t nb_rows = (chunks + 255) / 256;
  const int64_t nb = nb_rows + (batch + 3) / 4;
  if (nb >= ((int64_t)1 << 31)) return DD_ERR_UNSUPPORTED;
  dd_clear_error();
  return dd_dispatch16(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(dd_clip_embed_kernel<T>, dim3((unsigned)nb), dim3(256), 0, dd_stream(stream), ids, (const T*)tok,
                       (const T*)pos, (T*)out, pool_index, batch, l, c, vocab, eos_token_id, (int)nb_rows);
    return dd_check_launch();
  });
}

extern "C" int dd_causal_attention(const void* q, const void* k, const void* v, void* o, int64_t ldq, int64_t ldk,
                                   int64_t ldv, int64_t ldo, int64_t q_batch_stride, int64_t k_batch_stride,
                                   int64_t v_batch_stride, int64_t o_batch_stride, int32_t batch, int32_t l,
                                   int32_t heads, int32_t head_dim, float scale, int32_t dtype, dd_stream_t stream) {
  if (!q || !k || !v || !o) return DD_ERR_BAD_ARG;
  if (batch <= 0 || l <= 0 || heads <= 0 || head_dim <= 0) return DD_ERR_BAD_ARG;
  if (dtype != DD_F16 && dtype != DD_BF16) return DD_ERR_BAD_ARG;
  if (ldq <= 0 || ldk <= 0 || ldv <= 0 || ldo <= 0) return DD_ERR_BAD_ARG;
  if ((ldq & 7) || (ldk & 7) || (ldv & 7) || (ldo & 7)) return DD_ERR_BAD_ARG;
  if ((q_batch_stride & 7) || (k_batch_stride & 7) || (v_batch_stride & 7) || (o_batch_stride & 7)) return DD_ERR_BAD_ARG;
  if (!dd_aligned16(q) || !dd_aligned16(k) || !dd_aligned16(v) || !dd_aligned16(o)) return DD_ERR_BAD_ARG;
  if (head_dim != CA_D || l > DD_CAUSAL_ATTN_MAX_L) return DD_ERR_UNSUPPORTED;
  const int nqt = (l + 15) / 16;
  if ((int64_t)batch * heads * nqt >= ((int64_t)1 << 31)) return DD_ERR_UNSUPPORTED;
  CausalParams p;
  p.q = q; p.k = k; p.v = v; p.o = o;
  p.ldq = ldq; p.ldk = ldk; p.ldv = ldv; p.ldo = ldo;
  p.qbs = q_batch_stride; p.kbs = k_batch_stride; p.vbs = v_batch_stride; p.obs = o_batch_stride;
  p.l = l; p.heads = heads; p.nqt = nqt;
  p.scale_log2 = scale * 1.44269504088896340736f;
  const dim3 grid((unsigned)(batch * heads * nqt));
  dd_clear_error();
  const size_t smem = (size_t)((nqt + 1) / 2) * 32 * CA_VSTR * 2;   // <= 18 KB
  return dd_dispatch16(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(dd_causal_attn_kernel<T>, grid, dim3(64), smem, dd_stream(stream), p);
    return dd_check_launch();
  });
}
