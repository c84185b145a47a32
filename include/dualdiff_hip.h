/*
 * dualdiff_hip.h — C-ABI of the MI355X (gfx950) denoising hot path.
 *
 * Every entry point is a plain `extern "C"` launcher: device pointers + sizes + a
 * hipStream_t (passed as void*).  Launchers never allocate, never synchronise and
 * never throw: they validate arguments, enqueue kernels on `stream` and return 0
 * or a negative DD_ERR_* code.  All scratch memory is caller-owned (`ws`).
 * Launchers are graph-capture safe (hipGraph / torch.cuda.graph).
 *
 * The reference (yangzhaojason/DualDiff, MD_txt_con_fusion/) has no FFI: its hot
 * path reaches cuDNN/cuBLAS/xformers through torch.nn modules built by
 * diffusers-0.17.1.  Each launcher below names the reference call site whose
 * arithmetic it replaces (file:line relative to MD_txt_con_fusion/).
 *
 * Layout convention: activations are token-major / NHWC, i.e. a feature map
 * (M, C, H, W) is stored as rows = M*H*W, cols = C, row stride `ld*` in elements.
 * dtype: DD_F16 (reference eval dtype, misc/test_utils.py:98) or DD_BF16.
 * Accumulation, normalisation statistics and softmax are fp32.
 */
#ifndef DUALDIFF_HIP_H
#define DUALDIFF_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2 (round 4): dd_gemm_desc gained splitk_inkernel / prefetch / prefetch_bytes and dd_attn_desc kv_batch_map2 in round 3
 * without a bump; the GroupNorm workspace's first 256 B are barrier state.
 * 3 (round 5): what was measured and never dispatched is gone — dd_gemm_desc lost ln_gamma / ln_beta / w_scale (row-panel
 * family), splitk_inkernel, prefetch / prefetch_bytes; dd_attn_desc.variant takes 0 only; the cooperative GroupNorm
 * entry points (dd_groupnorm_is_coop / _set_coop) are removed and its workspace carries no barrier state.
 * 4 (round 6): dd_attn_desc / dd_xattn_desc gained lk_dev — the key count of a cross-attention read from DEVICE memory,
 * so that one recorded HIP graph serves every context length (78 + N_box tokens: the reference's collate function pads
 * the boxes to the batch's maximum, dataset/utils.py:165-244, so the length changes from sample to sample) up to the
 * capacity it was recorded at.
 * A binding must check BOTH the version and the descriptor sizes (dd_desc_size) before the first launch: a stale
 * pair would read past the caller's struct. */
#define DD_ABI_VERSION 4

enum { DD_F16 = 0, DD_BF16 = 1 };

enum {
  DD_OK = 0,
  DD_ERR_BAD_ARG = -1,     /* null pointer / non-positive size / misaligned */
  DD_ERR_UNSUPPORTED = -2, /* shape or option not implemented by the kernels */
  DD_ERR_LAUNCH = -3,      /* hipGetLastError() != hipSuccess after launch */
  DD_ERR_WORKSPACE = -4    /* caller workspace too small */
};

typedef void* dd_stream_t; /* hipStream_t */

int dd_abi_version(void);
/* sizeof() of descriptor `which` as THIS library was compiled: 0 dd_gemm_desc, 1 dd_attn_desc, 2 dd_xattn_desc,
 * 3 dd_gemm8_desc, 4 dd_box_tokens_desc; -1 for an unknown index.  The binding compares with its own struct sizes at load time. */
int64_t dd_desc_size(int which);
const char* dd_error_string(int code);
/* Reports the compile-time gfx target string ("gfx950"). */
const char* dd_target_arch(void);

/* ------------------------------------------------------------------------- *
 * GEMM / implicit-GEMM convolution with fused epilogue.
 *
 *   out[r, n] (op)= alpha * ( sum_k A[r, k] * W[n, k] + bias[n]
 *                             + rowvec[r / rows_per_inst, n] ) + res[r, n]
 *
 * Replaces: every nn.Linear / 1x1 nn.Conv2d / 3x3 nn.Conv2d on the path —
 *   attention to_q/to_k/to_v/to_out        networks/box_adapter.py:102-110,163
 *   SFA projections                        networks/txt_con_fusion.py:110-116,169
 *   attn4 + connector                      networks/blocks.py:203-220
 *   ResnetBlock2D conv1/conv2/shortcut, Down/Upsample2D conv, proj_in/proj_out,
 *   FeedForward (GEGLU)                    diffusers-0.17.1 (instantiated at
 *                                          networks/unet_addon_rawbox.py:240-295,
 *                                          networks/unet_2d_condition_multiview.py:181-216)
 *   zero convs + conditioning_scale + branch sum
 *                                          networks/unet_addon_rawbox.py:1029-1055,
 *                                          pipeline/pipeline_bev_controlnet.py:421-429
 *   ControlNetConditioningEmbedding convs  networks/map_embedder.py:114-138
 *
 * W is [N][K] row-major (torch Linear layout; conv weights pre-packed to
 * [Cout][ky][kx][Cin]).  K % 8 == 0, N % 8 == 0, all pointers 16-byte aligned,
 * lda/ldc/ldres multiples of 8.
 * ------------------------------------------------------------------------- */
enum { DD_EPI_NONE = 0, DD_EPI_GEGLU = 1, DD_EPI_SILU = 2 };

typedef struct dd_gemm_desc {
  /* A operand (dense mode): rows x K, row stride lda.  Optional second source
   * concatenated along K (K = k1 + k2): columns [0,k1) from a, [k1,K) from a2. */
  const void* a;
  const void* a2;    /* may be NULL */
  int64_t lda, lda2;
  int32_t k1;        /* == K when a2 == NULL */
  /* Problem size */
  int32_t rows, n, k;
  /* Weights / epilogue operands */
  const void* w;       /* [n_w][k]; n_w = n (or 2n for DD_EPI_GEGLU) */
  const void* bias;    /* [n_w] or NULL */
  const void* rowvec;  /* [rows/rows_per_inst][ld_rowvec] or NULL (time-emb add) */
  int32_t rows_per_inst, ld_rowvec;
  const void* res;     /* [rows][ldres] or NULL */
  int64_t ldres;
  void* out;           /* [rows][ldc] */
  int64_t ldc;
  float alpha;         /* see formula */
  int32_t accumulate;  /* 1: out += value (read-modify-write), 0: out = value */
  int32_t epilogue;    /* DD_EPI_*; GEGLU: out[r,n] = h * gelu_erf(g) with h = col n,
                          g = col n + N of the 2N-wide product (FeedForward/GEGLU) */
  /* conv mode (conv != 0): A is an NHWC image batch and K = 9*cin (3x3, pad 1).
   * Optional nearest-neighbour upsample of the input to (hv, wv) before the conv
   * (Upsample2D with explicit output size,
   *  networks/unet_2d_condition_multiview.py:369-374,500-501). */
  int32_t conv;        /* 0 dense, 1 conv3x3 */
  int32_t hin, win, cin;   /* stored input image */
  int32_t hv, wv;          /* virtual (post-upsample) input size; == hin,win if none */
  int32_t hout, wout, stride;
  /* dtype / tuning */
  int32_t dtype;       /* DD_F16 / DD_BF16 */
  int32_t tile;        /* 0 = auto, else tile-config id (see dd_gemm_num_tiles) */
  int32_t split_k;     /* 0 = auto, 1 = off, >1 = number of K slices */
  void* ws;            /* split-K workspace (>= dd_gemm_workspace_bytes): 64 KiB reserved, then the fp32
                          partial slabs; one buffer serves all launches of a stream. */
  int64_t ws_bytes;
  /* LayerNorm fold (dense mode, K in {320, 640, 1280}, no a2, no split-K): `a` holds the
   * UN-normalised rows x; the kernel computes each row's mean / rstd over its K columns in its
   * prologue and evaluates  LN(x) W^T + b  as
   *     rstd_r * (x W'^T - mean_r * ln_colsum) + ln_bias,
   * with W' = W * gamma (passed as `w`), ln_colsum[n] = sum_k W'[n,k], ln_bias[n] = W beta + b
   * (both fp32, n_w entries).  Replaces LayerNorm + Linear of norm1->to_q/k/v, norm2->to_q,
   * norm4->attn4 q/k/v, norm3->GEGLU proj (blocks.py:150-236).  `bias` must be NULL.  */
  const void* ln_colsum;   /* NULL = no fold */
  const void* ln_bias;
  float ln_eps;
  int32_t out_f32;     /* 1: `out` is fp32 [rows][ldc] (attention logits of the VAE mid block, which must not be
                          rounded to the storage type before the softmax); no GEGLU / accumulate */
  /* LayerNorm statistics carried from the producer to the consumer (both optional, fp32):
   * ln_stats_out: this GEMM's epilogue also writes, per output row and per 32-column group, the sum and the
   *   sum of squares of the values it stores, taken in fp32 before their rounding to the storage type (so a
   *   consumer normalises with the statistics of the unrounded result): [rows][n / 32][2] (n % 32 == 0, no split-K, no GEGLU).  Every
   *   transformer-block GEMM whose output feeds a LayerNorm (proj_in, to_out + residual; blocks.py:150-236)
   *   holds those values in registers anyway.
   * ln_stats_in: with the LayerNorm fold above, the row mean / rstd come from such a table of the `a`
   *   tensor ([rows][k / 32][2]) instead of a pass over the rows in every column tile's prologue. */
  void* ln_stats_out;
  const void* ln_stats_in;
  /* Head-major output (dense mode, plain epilogue, no split-K): with out_headmajor_d = D > 0 (D % 8 == 0,
   * n % D == 0) output column c of row r is stored at  out[((c / D) * rows + r) * D + c % D]  — one
   * contiguous [rows][D] plane per head of a fused Q|K|V projection, so that the attention kernel streams
   * a head's K/V rows as one linear range instead of D-element pieces of every fused row
   * (attn1 / attn4 of blocks.py:150-236).  The first `hm_scaled_planes` planes (the Q heads) are
   * multiplied by `hm_scale` in fp32 before the store rounding (softmax scale * log2 e, see
   * dd_attn_desc.q_prescaled).  ldc is ignored. */
  int32_t out_headmajor_d;
  int32_t hm_scaled_planes;
  float hm_scale;
  /* A split-K GEMM is two launches (partial slabs, then reduce + epilogue).  phase = 0 enqueues both (normal use);
   * 1 = the partial-slab launch only, 2 = the reduce launch only — so that a profiler-less caller (bench.py's
   * HIP-event brackets) can time the two kernels separately.  Ignored when split-K is off. */
  int32_t phase;
  /* LayerNorm EMITTED BY THE EPILOGUE (dense mode, n == 320, tile 40 = 80 whole rows x 320 columns per workgroup):
   * besides out = alpha * (A W^T + bias) + res, the kernel writes ln_out = LayerNorm(out) * lno_gamma + lno_beta
   * (two-pass fp32 statistics over the values as ROUNDED to the storage type, eps = ln_eps) — the producer of the
   * transformer's residual stream hands the next sub-layer its normalised input, so norm1 / norm2 / norm3 / norm4
   * of the 28x50 level (networks/blocks.py:150-236) need no launch of their own.  ln_out: T [rows][ld_ln_out]. */
  void* ln_out;            /* NULL = off */
  int64_t ld_ln_out;
  const void* lno_gamma;
  const void* lno_beta;
  /* Folded nearest upsample (conv mode, stride 1, hv > hin, wv > win, both <= 64, cin % 64 == 0): under a nearest map the
   * three taps of an axis read at most two distinct source pixels, so the tap slices of the weight that read the same pixel
   * are summed ahead of time and every output pixel becomes a 2 x 2-tap conv with k = 4 * cin.  Per axis an output
   * coordinate o with s = src(o) is of class 0 (taps read s-1 | s s: slot weights W-1 | W0+W1), 1 (s s | s+1: W-1+W0 | W1)
   * or 2 (the last coordinate of an odd size, tap +1 outside the output: W-1 | W0); a pixel's class is 3 * (row class)
   * + (column class).  `w` holds one [n][sy][sx][cin] matrix per NON-EMPTY class, in class order; k = 4 * cin.  A map
   * with a coordinate that fits no class (three distinct sources, a downscale) is DD_ERR_UNSUPPORTED: the caller keeps
   * the 9-tap form (upfold = 0).  Only LDS-DMA ring tiles carry the kernel (dd_gemm2u_kernel). */
  int32_t upfold;
} dd_gemm_desc;

int dd_gemm(const dd_gemm_desc* d, dd_stream_t stream);
/* Workspace bytes dd_gemm needs for this descriptor (0 when split-K is off). */
int64_t dd_gemm_workspace_bytes(const dd_gemm_desc* d);
int dd_gemm_num_tiles(void);
/* id of the index-th tile configuration (for tuners); -1 when out of range. */
int dd_gemm_tile_id(int index);
/* Name of the kernel symbol dd_gemm would launch for `d` (for profile matching). */
const char* dd_gemm_kernel_name(const dd_gemm_desc* d);

/* conv3x3 with a chosen top / left zero padding pad_lo: output pixel o reads input rows and columns
 * o*stride - pad_lo + 0..2; reads past the bottom / right edge of the stored image are zero, as in every conv.
 *   pad_lo = 1: exactly dd_gemm / dd_gemm_workspace_bytes / dd_gemm_kernel_name (same plan, kernel and bits).
 *   pad_lo = 0: diffusers' Downsample2D(padding=0) of the VAE encoder's down blocks,
 *               F.pad(x, (0, 1, 0, 1)) followed by nn.Conv2d(c, c, 3, stride=2, padding=0)
 *               (AutoencoderKL.encode, runner/base_runner.py:469-475).  conv = 1, stride = 2, hv == hin, wv == win,
 *               hin, win >= 2, hout = (hin - 2) / 2 + 1, wout = (win - 2) / 2 + 1, no GEGLU; else DD_ERR_UNSUPPORTED or
 *               DD_ERR_BAD_ARG.  Only the register-staged tiles (ids 1-5, dd_gemm_pad0_kernel) have the kernel; any
 *               other tile is DD_ERR_UNSUPPORTED ("unsupported" from the name query), so the LDS-DMA, direct small-image
 *               and pipelined families and the thin conv never take it. */
int dd_gemm_conv_pad(const dd_gemm_desc* d, int32_t pad_lo, dd_stream_t stream);
int64_t dd_gemm_conv_pad_workspace_bytes(const dd_gemm_desc* d, int32_t pad_lo);
const char* dd_gemm_conv_pad_kernel_name(const dd_gemm_desc* d, int32_t pad_lo);

/* ------------------------------------------------------------------------- *
 * GroupNorm (+ optional SiLU), NHWC, optional channel-concat of two sources.
 *   y[m, p, c] = act( (x[m,p,c] - mean[m,g]) * rstd[m,g] * gamma[c] + beta[c] )
 * Replaces torch.nn.GroupNorm + SiLU inside ResnetBlock2D (eps 1e-5), the
 * Transformer2DModel input norm (eps 1e-6, no SiLU) and conv_norm_out
 * (networks/unet_2d_condition_multiview.py:519-522).
 * ws: fp32 scratch, >= dd_groupnorm_workspace_bytes(M, G), private to the stream (first 256 bytes reserved).
 * C1 + C2 = C, C % G == 0, C1 % 8 == 0, C2 % 8 == 0, C <= 4096, G <= 64.
 * A 16-byte vector (8 channels from a multiple of 8) must touch at most two groups: C / G = 4 or >= 6; 1, 2, 3 and 5
 * channels per group are DD_ERR_UNSUPPORTED (also from dd_groupnorm_splitk; dd_groupnorm_is_fused reports 0).
 * ------------------------------------------------------------------------- */
int dd_groupnorm_nhwc(const void* x1, int32_t c1, const void* x2, int32_t c2,
                      const void* gamma, const void* beta, void* y,
                      int32_t m, int32_t hw, int32_t groups, float eps,
                      int32_t apply_silu, int32_t dtype, void* ws, int64_t ws_bytes,
                      dd_stream_t stream);
int64_t dd_groupnorm_workspace_bytes(int32_t m, int32_t groups);
/* Which kernels dd_groupnorm_nhwc launches for an image of hw pixels x c channels: 256 / 1024 = ONE launch of
 * dd_gn_fused_kernel with that many threads (slab in registers), 0 = dd_gn_stats_kernel + dd_gn_apply_kernel
 * (for profile matching, like dd_gemm_kernel_name). */
int dd_groupnorm_is_fused(int32_t hw, int32_t c, int32_t groups);
/* GroupNorm(+SiLU) that CONSUMES the partial slabs of a split-K dd_gemm launched with phase = 1 (in place of that GEMM's
 * reduce launch): x[r, c] = T( sum_z partial[z][r][c] + bias[c] + rowvec[r / hw][c] + res[r][c] ) — exactly what the
 * reduce launch would have stored (alpha = 1, no activation, no accumulate) — then y = GroupNorm(x) as above; x itself
 * is written only when x_out != NULL.  ResnetBlock2D: conv1 -> norm2 (x is not needed) and conv2 -> the Transformer2D
 * input norm (x is the residual stream).  partial = (char*)ws + 65536 of the dd_gemm call, nsplit = its slice count
 * (dd_gemm_kernel_name reports it).  Single-launch images only (dd_groupnorm_is_fused != 0), else DD_ERR_UNSUPPORTED. */
int dd_groupnorm_splitk(const float* partial, int32_t nsplit, const void* bias, const void* rowvec, int32_t ld_rowvec,
                        const void* res, int64_t ldres, void* x_out, const void* gamma, const void* beta, void* y,
                        int32_t m, int32_t hw, int32_t c, int32_t groups, float eps, int32_t apply_silu, int32_t dtype,
                        dd_stream_t stream);

/* LayerNorm over the last dim (eps 1e-5, affine) — BasicTransformerBlock
 * norm1/2/3 (diffusers) and norm4 (networks/blocks.py:67-71,191-194). */
int dd_layernorm(const void* x, const void* gamma, const void* beta, void* y,
                 int64_t rows, int32_t c, float eps, int32_t dtype, dd_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Scaled-dot-product attention, flash-style (online softmax, fp32 state).
 *   O[b, i, h, :] (op)= softmax_j( scale * Q[b,i,h,:].K[kb,j,h,:] ) V[kb,j,h,:]
 * with kb = kv_batch_map ? kv_batch_map[b] : b.
 * Replaces xformers.ops.memory_efficient_attention at
 *   networks/box_adapter.py:150-156 (attn1/attn2 processor),
 *   networks/txt_con_fusion.py:156-162 (SFA), :313-318 (SFA+),
 *   networks/blocks.py:203-217 (attn4: one call per neighbour with
 *   accumulate=1 realises the sum over neighbours).
 * No mask (attention_mask is None on the inference path, blocks.py:166-187).
 * Q/K/V/O are (batch, len, heads*head_dim) views with row strides ld* (elements),
 * so they may alias slices of a fused QKV projection.  head_dim in {40,80,160}.
 * ------------------------------------------------------------------------- */
typedef struct dd_attn_desc {
  const void* q; const void* k; const void* v; void* o;
  int64_t ldq, ldk, ldv, ldo;         /* row strides in elements */
  int64_t q_batch_stride, k_batch_stride, v_batch_stride, o_batch_stride;
  int32_t batch, heads, head_dim, lq, lk;
  float scale;
  const int32_t* kv_batch_map;        /* device ptr [batch] or NULL */
  int32_t accumulate;                 /* 1: O += result */
  int32_t dtype;
  int32_t variant;                    /* 0 (the tuning variants of rounds 1-3 are gone: anything else is DD_ERR_UNSUPPORTED) */
  /* head h of q / k / v starts at element h * {q,k,v}_head_stride of its batch (0 = head_dim: the heads
   * are column blocks of one row, the reference's layout).  A head-major projection (dd_gemm_desc.
   * out_headmajor_d) passes ld = head_dim, batch stride = l * head_dim, head stride = rows * head_dim. */
  int64_t q_head_stride, k_head_stride, v_head_stride;
  int32_t q_prescaled;                /* 1: q already carries scale * log2(e); `scale` is ignored */
  /* Neighbour PAIR in one launch (networks/blocks.py:203-217, attn4 with neighboring_attn_type="add"):
   *   O[b] (op)= Attn(Q[b], K/V[kv_batch_map[b]]) + Attn(Q[b], K/V[kv_batch_map2[b]])
   * — two softmaxes with their own normalisation, summed in fp32 and rounded once.  Needs kv_batch_map and the default
   * variant (0); NULL = single attention. */
  const int32_t* kv_batch_map2;
  /* NULL, or a 4-byte-aligned DEVICE pointer to the number of keys every batch entry really has: the kernel reads it at
   * its start (clamped to [1, lk]) and `lk` is then only the CAPACITY — it sizes the strides the caller built and selects
   * the instantiation; keys lk_dev[0] .. lk-1 are never read.  Same arithmetic as a launch with lk = lk_dev[0] and the
   * same strides: bit-identical results. */
  const int32_t* lk_dev;
} dd_attn_desc;

int dd_attention(const dd_attn_desc* d, dd_stream_t stream);
/* Name of the kernel instantiation dd_attention would launch for `d` and its grid (query rows per wave, key tile and
 * waves per SIMD follow from the shape): for profile matching and for testing the dispatch without a GPU, like
 * dd_gemm_kernel_name.  "invalid" / "unsupported" mirror DD_ERR_BAD_ARG / DD_ERR_UNSUPPORTED; nothing is launched. */
const char* dd_attention_kernel_name(const dd_attn_desc* d);

/* ------------------------------------------------------------------------- *
 * Cross-attention probabilities (csrc/attn_probs.hip): the numbers dd_attention and dd_xattn320 never write.
 *   w[b,h,i,j] = softmax_{j < n}( scale * Q[b,i,h,:] . K[b,j,h,:] )       n = lk_dev ? clamp(lk_dev[0], 1, lk) : lk
 *   per_head = 1:  P[b,h,i,j] (op)= weight * w[b,h,i,j]
 *   per_head = 0:  P[b,i,j]   (op)= weight * (1 / heads) * sum_h w[b,h,i,j]     (fp32 sum in ascending h)
 * Replaces the probabilities the reference's visualisation processor keeps, tools/unet_modify.py:31,47
 * (attn.get_attention_scores of every attn2 layer), which pipeline/explore_pipeline_bev_controlnet.py:352-354,437-453,
 * 494-500,576 collects as cross_attn_map and tools/explore_attn.py:97-151 averages over heads, steps and layers.
 * Q / K are addressed as in dd_attn_desc (ldq / ldk, batch strides, head strides with 0 = head_dim; q_prescaled = 1: q
 * carries scale * log2 e and `scale` is ignored), elements of `qk_dtype` (DD_F16 / DD_BF16).  P is FLOAT32: element
 * (b, [h,] i, j) at  b * p_batch_stride [+ h * p_head_stride] + i * ldp + j  (elements; p_head_stride is ignored for
 * per_head = 0).  accumulate = 0 stores, and columns n .. lk-1 are then written as exact zeros; accumulate = 1 adds to
 * what is there and does not touch columns n .. lk-1.  Nothing is written outside columns 0 .. lk-1 of a row.
 * Arithmetic: fp32 MFMA scores of the 16-bit operands; the EXACT row maximum m over the n keys (a row of at most
 * DD_ATTN_PROBS_MAX_LK scores stays in registers: no online rescale); p = exp2(fma(s, c, -m c)), c = scale * log2 e;
 * the fp32 sum of the unrounded p; one normalisation; nothing is rounded to the storage type.  One wave owns a
 * (batch entry, 16 query rows) across all heads: no atomics, identical bits from run to run, and a launch with lk_dev
 * gives the bits of a launch with lk = lk_dev[0] and the same strides.
 * head_dim in {40, 80, 160} and lk <= DD_ATTN_PROBS_MAX_LK, else DD_ERR_UNSUPPORTED.  DD_ERR_BAD_ARG: a NULL q / k / p,
 * q / k not 16-byte aligned, p or lk_dev not 4-byte aligned, a non-positive batch / lq / lk / heads / head_dim, ld or
 * strides of q / k that are negative or no multiples of 8, ldp < lk, a negative stride of p, scale <= 0 without
 * q_prescaled, an unknown qk_dtype.  Both are decided before anything is launched.  (P rows go out as 16-byte stores
 * where p is 16-byte aligned and ldp and its strides are multiples of 4, as single floats otherwise.) */
#define DD_ATTN_PROBS_MAX_LK 256
int dd_attn_probs(const void* q, const void* k, float* p, int64_t ldq, int64_t ldk, int64_t q_batch_stride,
                  int64_t k_batch_stride, int64_t q_head_stride, int64_t k_head_stride, int64_t ldp,
                  int64_t p_batch_stride, int64_t p_head_stride, int32_t batch, int32_t lq, int32_t lk, int32_t heads,
                  int32_t head_dim, float scale, int32_t q_prescaled, int32_t per_head, int32_t accumulate,
                  float weight, const int32_t* lk_dev, int32_t qk_dtype, dd_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Attention-map pictures (csrc/attn_heat.hip): the per-token heat-map sheets the reference's analysis script makes of
 * the averaged map, `view_images_{view}.png` and `view_images_{view}box.png` (tools/explore_attn.py:114-151, with
 * text_under_image :13-23 and view_images :25-53).  Between the two entry points lies dd_image_resample_u8 (PIL's
 * bicubic resize of :129 / :149, its bottom pad the white strip of :15-16): three launches, no host synchronisation.
 *
 * dd_attn_heat: normalise and colour the selected context columns (:118-128, :138-148), one launch.
 *   maps   float [views][q][ldm] (device), q = h * w: element (v, r, j) at v * view_stride + r * ldm + j (elements),
 *          ldm >= n.  Only 4-byte alignment is asked, so a buffer with a padded pitch and a contiguous one both do.
 *   cols   int32 [t] (device): the columns to draw, each in [0, n) (clamped to it: nothing else is ever read).
 *   table  float [257][4] (device): per colour-map index {r / 255, g / 255, b / 255, unused}; row 256 is the NaN colour
 *          (matplotlib's "bad" colour, black).
 *   img    float [views * t][3][h][w]: tile v * t + i is column cols[i] of view v, as colour / 255.  The quotients are
 *          the caller's, so that dd_image_resample_u8 quantises them back to the colour bytes.
 *   Arithmetic, per (view, column): the exact minimum and maximum of the column over the q rows; per pixel
 *          X = (double(x) - double(min)) / (double(max) - double(min)) in IEEE fp64 (:120-122, with np.float64 for the
 *          removed np.float), k = min(int(X * 256.0), 255), and k = 256 where X is NaN (a constant column: 0 / 0) —
 *          matplotlib's Colormap.__call__ on a float in [0, 1] (:123-127).  float32 subnormals and signed zeros convert
 *          to double exactly (the double is built from the bits; the extrema are found by integer compares).  A
 *          non-finite input gives an unspecified colour; the index is clamped to the table.
 *   No atomics, identical bits from run to run.
 * DD_ERR_BAD_ARG, before any runtime call: a NULL maps / cols / table / img, views / h / w / n / t <= 0, ldm < n, a
 * negative view_stride, a pointer that is not 4-byte aligned.  views * t > 65535 or h * w >= 2^31: DD_ERR_UNSUPPORTED.
 *
 * dd_attn_sheet_u8: view_images' canvas (:25-53) for `sheets` sheets of rows x cols cells, one launch.
 *   tiles  uint8 [m][th][tw][3] (device): the resized tiles (dd_image_resample_u8's output, strip included);
 *   index  int32 [sheets][rows * cols] (device): the tile of each cell, row-major (:46-49); -1 (anything outside
 *          [0, m)) is an all-255 cell, the reference's "empty" image;
 *   labels uint8 [m][lh][tw][3] (device): pasted over the bottom lh rows of the tile of the same number
 *          (text_under_image's strip, :13-23), or NULL with lh == 0;
 *   gap    the gutter between cells, int(tile height * offset_ratio) of :39;
 *   out    uint8 [sheets][rows * th + gap * (rows - 1)][cols * tw + gap * (cols - 1)][3], 255 in the gutters (:44-45).
 *          Every byte is written exactly once, no alignment is asked of it.
 * DD_ERR_BAD_ARG, before any runtime call: a NULL tiles / index / out, m / sheets / rows / cols / th / tw <= 0, lh or
 * gap < 0, labels without lh or lh without labels, lh > th, a misaligned index.  sheets > 65535, or a sheet of 2^31
 * pixels or more (th + gap and tw + gap included): DD_ERR_UNSUPPORTED.
 * ------------------------------------------------------------------------- */
int dd_attn_heat(const float* maps, const int32_t* cols, const float* table, float* img, int32_t views, int32_t h,
                 int32_t w, int32_t n, int32_t t, int64_t ldm, int64_t view_stride, dd_stream_t stream);
int dd_attn_sheet_u8(const uint8_t* tiles, const int32_t* index, const uint8_t* labels, uint8_t* out, int32_t m,
                     int32_t sheets, int32_t rows, int32_t cols, int32_t th, int32_t tw, int32_t lh, int32_t gap,
                     dd_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Fused cross-attention of the 320-channel level (8 heads x 40, <= 128 context keys per view-instance), ONE launch:
 *   out[r, :] = ( softmax_j( scale * (x[r] Wq^T)_h . K[i, j]_h ) V[i, j]_h )_h Wo^T + bo + res[r, :]
 * for query row r of view-instance i = r / rows_per_inst; optionally also ln_out = LayerNorm(out) (two-pass fp32
 * statistics over the rounded values, eps ln_eps).  Replaces to_q -> memory_efficient_attention -> to_out (+ residual)
 * of Semantic Fusion Attention (networks/txt_con_fusion.py:108-181: x = res = the ORS condition map, K / V = to_k /
 * to_v of the 77 text tokens) and of the text / box cross-attention attn2 of the 28x50 transformer blocks
 * (networks/box_adapter.py:102-163 inside blocks.py:166-187: x = LayerNorm2(h), res = h).  q and the attention output
 * never reach HBM.  x / res / out: [instances * rows_per_inst][320] with row pitches ld* (elements).  K / V: element
 * (instance i, key j, head h, d) at  k + i * k_inst_stride + j * ldk + h * k_head_stride + d  (elements; all strides
 * multiples of 8) — row-major column slices of a wider projection (ldk = its width, head stride 40, instance stride
 * lk * ldk) and head-major planes written by dd_gemm's out_headmajor_d = 40 (ldk = 40, head stride = total rows * 40,
 * instance stride lk * 40: a head's keys are one contiguous block, which is what the kernel streams fastest).
 * wq / wo: the [320][320] torch Linear weights PACKED by dd_xattn_pack_weight (K-step-major, pre-swizzled, so that the
 * kernel's LDS-DMA copies them linearly); bo [320] (required: pass zeros for a bias-free projection).
 * ------------------------------------------------------------------------- */
typedef struct dd_xattn_desc {
  const void* x; int64_t ldx;
  const void* res; int64_t ldres;          /* NULL = no residual */
  const void* wq; const void* wo; const void* bo;
  const void* k; const void* v; int64_t ldk, ldv;
  int64_t k_inst_stride, k_head_stride, v_inst_stride, v_head_stride;
  void* out; int64_t ldo;
  int32_t instances, rows_per_inst, lk;
  int32_t channels, heads;                 /* 320, 8: anything else is DD_ERR_UNSUPPORTED */
  float scale;
  int32_t dtype;
  void* ln_out; int64_t ld_ln_out;         /* NULL = off */
  const void* ln_gamma; const void* ln_beta; float ln_eps;
  const int32_t* lk_dev;                   /* as dd_attn_desc.lk_dev: keys per instance from device memory, lk = capacity */
} dd_xattn_desc;

int dd_xattn320(const dd_xattn_desc* d, dd_stream_t stream);
/* w: [320][320] row-major (torch Linear: out x in) -> packed: 102,400 elements in the streaming order of dd_xattn320. */
int dd_xattn_pack_weight(const void* w, void* packed, int32_t dtype, dd_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Small HBM-bound helpers.
 * ------------------------------------------------------------------------- */
/* y = a + b (+ c)   — ControlNet residual add into UNet skips
 * (networks/unet_2d_condition_multiview.py:464-473,487-488). c may be NULL. */
int dd_add(const void* a, const void* b, const void* c, void* y, int64_t n,
           int32_t dtype, dd_stream_t stream);
/* y = x * s (in place allowed) */
int dd_scale(const void* x, void* y, float s, int64_t n, int32_t dtype, dd_stream_t stream);
/* SiLU elementwise (time embedding act). */
int dd_silu(const void* x, void* y, int64_t n, int32_t dtype, dd_stream_t stream);

/* NCHW <-> NHWC (only at the 4-channel latent / drop-in boundary). */
int dd_nchw_to_nhwc(const void* x, void* y, int32_t m, int32_t c, int32_t hw,
                    int32_t c_pad, int32_t dtype, dd_stream_t stream);
int dd_nhwc_to_nchw(const void* x, void* y, int32_t m, int32_t c, int32_t hw,
                    int32_t ldx, int32_t dtype, dd_stream_t stream);

/* Sinusoidal timestep embedding, diffusers `Timesteps(dim, flip_sin_to_cos=True,
 * downscale_freq_shift=0)` (networks/unet_addon_rawbox.py:142-144,921-927;
 * unet_2d_condition_multiview.py:404-409): out[i, :] = [cos(t_i f), sin(t_i f)],
 * f_j = exp(-ln(10000) j / (dim/2)).  t: fp32 device array [n]. */
int dd_timestep_embedding(const float* t, void* out, int32_t n, int32_t dim,
                          int32_t flip_sin_to_cos, float freq_shift,
                          int32_t dtype, dd_stream_t stream);

/* NeRF-style Fourier features (networks/embedder.py:18-67, used by the camera and 3-D box token
 * embedders, unet_addon_rawbox.py:308-325, bbox_embedder.py:187): for every row of `dims` inputs
 *   out[r] = [x (if include_input), sin(f_0 x), cos(f_0 x), ..., sin(f_{F-1} x), cos(f_{F-1} x)],
 * each block `dims` wide.  x: fp32 / fp16 / bf16 per `in_dtype` (DD_F16, DD_BF16 or DD_F32); the
 * arithmetic is fp32; out in `out_dtype`.  freqs: HOST array of num_freqs (<= 16) frequencies. */
#define DD_F32 2
int dd_fourier_embed(const void* x, void* out, int64_t rows, int32_t dims, const float* freqs,
                     int32_t num_freqs, int32_t include_input, int32_t in_dtype, int32_t out_dtype,
                     dd_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Token / condition preparation of a ControlNet branch (csrc/tokens.hip, round 4): what the reference does with ~40
 * tiny torch ops per step (unet_addon_rawbox.py:308-361,832-896,1007; bbox_embedder.py:164-203;
 * map_embedder.py:116-125) as four launches.
 * ------------------------------------------------------------------------- */
/* NCHW (m, c, h, views * w) -> NHWC rows of m * views instances (h, w, c_pad), channels zero-padded; views = 1 is the
 * plain layout change (LDS-tiled: both sides coalesced), views = 6 the panorama split of map_embedder.py:116-125.
 * c_pad % 8 == 0, y 16-byte aligned. */
int dd_nchw_to_nhwc_views(const void* x, void* y, int32_t m, int32_t c, int32_t h, int32_t w, int32_t views,
                          int32_t c_pad, int32_t dtype, dd_stream_t stream);
/* dd_fourier_embed with a strided source and a padded destination: row r = outer * inner + j reads its `dims` inputs at
 * x[outer * stride_outer + j * stride_inner + d * stride_dim] and writes its features at
 * out[outer * out_ld + j * width ...], width = dims * (include_input + 2 * num_freqs); the out_ld - inner * width
 * (<= dims) trailing columns of every outer row are zeroed (K padding of the Linear that follows).  Camera parameters
 * (b, n, 3, 7) -> (b n, 189 padded to 192): dims 3, inner 7, strides (21, 1, 7) (unet_addon_rawbox.py:308-325). */
int dd_fourier_embed_strided(const void* x, void* out, int64_t rows, int32_t dims, const float* freqs,
                             int32_t num_freqs, int32_t include_input, int32_t in_dtype, int32_t out_dtype,
                             int32_t inner, int64_t stride_outer, int64_t stride_inner, int64_t stride_dim,
                             int64_t out_ld, dd_stream_t stream);
/* Both operands of the box MLP (bbox_embedder.py:164-203).  For every box r: pos[r] = masks[r] ? Fourier features of its
 * points : null_pos  (T [rows][points_per_box * 3 * (include_input + 2 num_freqs)], the input of bbox_proj), and
 * cat[r][cls_offset ...] = masks[r] ? class_tokens[classes[r]] : null_class  (the right half of the concat
 * second_linear reads; bbox_proj writes the left half); cls_out (optional) gets the same class rows (box adapter).
 * points: [rows][points_per_box][3] in `points_dtype` (DD_F16 / DD_BF16 / DD_F32; values pass through that dtype as in
 * the reference); classes int64; masks uint8 (NULL = keep all); normalize: (p - xyz_min) / xyz_range first. */
typedef struct dd_box_tokens_desc {
  const void* points; const int64_t* classes; const uint8_t* masks;
  const void* class_tokens; const void* null_pos; const void* null_class;
  void* pos; void* cat; void* cls_out;
  int32_t rows, points_per_box, num_freqs, include_input, class_token_dim, cls_offset;
  int64_t ld_cat;
  int32_t normalize, points_dtype, dtype;
  int32_t n_classes;   /* rows of class_tokens: a kept box's class index is wrapped like torch indexing (-1 = last row); one still
                          outside [0, n_classes) gets NaN tokens instead of reading out of bounds.  0 = unchecked (ABI 2 callers) */
  float freqs[16]; float xyz_min[3]; float xyz_range[3];
} dd_box_tokens_desc;
int dd_box_tokens(const dd_box_tokens_desc* d, dd_stream_t stream);
/* Context assembly: full[i] = [cam_i | text | box tokens] and (optional) txt[i] = text for instance i = (scene, view)
 * (unet_addon_rawbox.py:337-361, :1007, :977).  cam [m][dim]; text [scenes][lt][dim] (text_per_view: [m][lt][dim]);
 * box [scenes * box_views][nbox][dim], box_views in {n_cam, 1} (NULL when nbox == 0); full [m][1 + lt + nbox][dim];
 * txt [m][lt][dim] or NULL.  dim % 8 == 0, all 16-byte aligned. */
int dd_ctx_assemble(const void* cam, const void* text, const void* box, void* full, void* txt, int32_t m,
                    int32_t n_cam, int32_t lt, int32_t nbox, int32_t dim, int32_t text_per_view, int32_t box_views,
                    int32_t dtype, dd_stream_t stream);

/* ORS projection (networks/occ3d_proj.py:49-113 + dataset/utils.py:412-420): every
 * latent pixel's ray is sampled at `samples` equidistant points (step metres apart) in a
 * 200 x 200 x 16 class volume (uint8, x-major, 0.4 m voxels: x, y in [-40, 40) m, z in [-1, 5.4) m);
 * the nearest voxel's class is taken, 17 outside the volume.
 *   origin [n_cam][3], dir [n_cam][hw][3]: fp32 ray origins / unit directions (ego frame);
 *   labels (may be NULL): uint8 [n_cam][hw][samples];
 *   cond   (may be NULL): [n_cam][samples][hw] in `dtype` = class / 17 after the optional
 *           foreground (class <= 10 -> 17, keep_fg == 0) / background (class >= 11 -> 17, keep_bg == 0)
 *           filtering — the ORS-3D ControlNet condition (unet_addon_rawbox.py:967-990).
 * Integer output: bit-exact against the reference's fp32 arithmetic (separate multiply / add, true
 * divisions, round-half-even). */
int dd_ors_project(const uint8_t* occ, const float* origin, const float* dir, uint8_t* labels, void* cond,
                   int32_t n_cam, int32_t hw, int32_t samples, float step, int32_t keep_fg, int32_t keep_bg,
                   int32_t dtype, dd_stream_t stream);

/* ORS panorama, the image-mode condition (networks/occ3d_proj.py:156-198; read as ./occ_proj/occ_bg/{token}.png by
 * misc/test_utils.py:219-222): the FIRST occupied class along each ray, painted with a palette, the views side by side.
 * The samples and their labels are dd_ors_project's; nothing per sample is written.  One launch for a batch.
 *   occ [b][200][200][16] uint8; origin [rigs][n][3], dir [rigs][n][h * w][3] fp32; rig_of_sample [b] int32 DEVICE memory,
 *   each in [0, rigs): the ray table sample i uses (the caller checks the range; a value outside gives class 17);
 *   mode: 0 all labels count; 1 (bg) labels <= 10 become 17 first (:157); 2 (fg) labels >= 11 become 17 first (:160);
 *   the first sample s in 0 .. samples - 1 whose label is not 17 gives the class (:165-168), 17 when there is none.  Class
 *   0 is a class: it hides what lies behind it in modes 0 and 2.
 *   cls (may be NULL): uint8 [b][n][h][w], the class;
 *   frames (may be NULL): uint8 [b][h][n * w][3], its colour, palette[class] (:192-197); not both NULL;
 *   visited (may be NULL): int32 [b][n][h][w], the number of samples the ray looked up (for measurements);
 *   palette: 18 x 3 bytes in HOST memory, passed on by value (colors_map[:, :3] of :171-191 is the reference's);
 *   exits: bit 0 stop at the first hit, bit 1 stop once the ray has left the volume for good; 3 for use, the results are
 *   the same for every value.  step > 0. */
int dd_ors_first_hit(const uint8_t* occ, const float* origin, const float* dir, const int32_t* rig_of_sample,
                     uint8_t* cls, uint8_t* frames, int32_t* visited, const uint8_t* palette, int32_t b, int32_t rigs,
                     int32_t n, int32_t h, int32_t w, int32_t samples, float step, int32_t mode, int32_t exits,
                     dd_stream_t stream);

/* The blend of an ORS panorama over the camera pictures (networks/occ3d_proj.py:196-203), all uint8 [b][h][w][3], w the
 * width of the whole panorama.  Per sample: x = u8 / 255 * 2 - 1 (:127-129), d = (x - min x) / (max x - min x) * 255
 * (:196); per channel element with colour c: c * 0.7f + d * 0.3f where c != 0, d where c == 0 (:199-203), truncated to
 * uint8; float32 operation by operation, as numpy and torch apply it on the CPU.  Two launches: the reduction and the
 * blend.  parts: int32 [b][64][2] workspace; flags: one int32, written: bit 0 = a sample's camera picture is constant
 * (max == min, NaN in the reference; that sample's output is 0). */
int dd_ors_overlay_u8(const uint8_t* colour, const uint8_t* camera, uint8_t* out, int32_t* parts, int32_t* flags,
                      int32_t b, int32_t h, int32_t w, dd_stream_t stream);

/* Row softmax of fp32 logits into the storage type: p[r][c] = softmax_c(s[r][c]) for c < cols
 * (diffusers AttnProcessor `get_attention_scores` with upcast_softmax — the single 512-wide head of
 * the VAE decoder's mid-block attention, decode_latents pipeline_bev_controlnet.py:101-113).
 * s: fp32 [rows][lds]; p: T [rows][ldp], columns cols..ldp-1 are zero-filled (K padding of the PV GEMM). */
int dd_softmax_rows(const float* s, void* p, int64_t rows, int32_t cols, int64_t lds, int64_t ldp,
                    int32_t dtype, dd_stream_t stream);

/* conv3x3 with tiny Cout (conv_out 320->4): y NCHW fp32/T. x NHWC (rows, cin),
 * w [cout][9*cin]; writes y as NCHW (m, cout, h, w) in dtype T.
 * (networks/unet_2d_condition_multiview.py:522) */
int dd_conv3x3_small_cout(const void* x, const void* w, const void* bias, void* y_nchw,
                          int32_t m, int32_t h, int32_t wd, int32_t cin, int32_t cout,
                          int32_t dtype, dd_stream_t stream);

/* VAE encoder posterior (diffusers AutoencoderKL.encode -> DiagonalGaussianDistribution, scaled as the reference's
 * runner/base_runner.py:469-475 does): per latent pixel, in fp32,
 *   p = wq x + bq                      quant_conv (1x1, 8 -> 8); x = the 8 channels conv_out wrote
 *   mean = p[0:4], logvar = clamp(p[4:8], -30, 20)
 *   z = mean + exp(0.5 logvar) * noise, or z = mean when noise == NULL (mode())
 *   out = scale * z
 * moments: T NHWC rows (m * h * w, 8), 16-byte aligned; wq: fp32 [8][8] (out, in); bq: fp32 [8];
 * noise: T NCHW (m, 4, h, w) or NULL; z: NCHW (m, 4, h, w), fp32 when out_f32 else T. */
int dd_vae_posterior(const void* moments, const float* wq, const float* bq, const void* noise, void* z,
                     int32_t m, int32_t h, int32_t w, float scale, int32_t out_f32, int32_t dtype, dd_stream_t stream);

/* ------------------------------------------------------------------------- *
 * FID feature extractor (csrc/conv2d.hip): the InceptionV3 of the reference's evaluation step, tools/fid_score.py:93-156
 * (get_activations) -> magicdrive/misc/inception.py (pytorch-fid's FID network).  Backward-compatible additions to ABI 4.
 *
 * dd_conv2d_nhwc: every BasicConv2d of that network (inception.py: the torchvision Inception blocks it instantiates at
 * :84-124 and the FID variants at :224-341; each is conv without bias -> BatchNorm2d(eps = 1e-3) in eval -> ReLU):
 *   out[p, c_off + n] = relu( scale[n] * sum_{ky,kx,ci} x[img, oy s - pad_h + ky, ox s - pad_w + kx, ci] w[n, ky, kx, ci]
 *                             + shift[n] )
 * x: T NHWC [m][h][wd][cin], dense, 16-byte aligned, cin % 8 == 0 (the stem's 3 channels are zero-padded to 8 by
 * dd_inception_input and by the weight packing); w: T [cout][kh][kw][cin], 16-byte aligned; cout % 4 == 0;
 * scale / shift: fp32 [cout] (gamma / sqrt(var + eps) and beta - mean * that: BatchNorm stays in fp32, it is NOT folded
 * into the 16-bit weights); accumulation in fp32; relu: 0 / 1.
 * kh, kw in 1..7; stride 1 or 2 (both axes); 0 <= pad_h <= kh / 2, 0 <= pad_w <= kw / 2; taps outside the image read
 * zero; hout = (h + 2 pad_h - kh) / stride + 1 (likewise wout), p = (img * hout + oy) * wout + ox.
 * out: T, row stride ldc >= c_off + cout elements, ldc % 4 == 0, c_off % 4 == 0, 8-byte aligned: a branch writes its
 * slice of the block's concatenated tensor (the torch.cat of inception.py:246, 274, 307, 341); other columns are untouched.
 * tile: 0 = chosen from the shape, 1 = 64 pixels x 64 channels, 2 = 128 x 64 per workgroup.
 * Shapes outside these rules are DD_ERR_UNSUPPORTED, bad pointers / sizes / a slice that does not fit ldc DD_ERR_BAD_ARG.
 * storage_type (here and below): DD_F16 / DD_BF16, the element type T of activations and weights; any other value is
 * DD_ERR_BAD_ARG (tests/test_fid_cpu.py). */
int dd_conv2d_nhwc(const void* x, const void* w, const float* scale, const float* shift, void* out, int64_t ldc,
                   int32_t c_off, int32_t m, int32_t h, int32_t wd, int32_t cin, int32_t cout, int32_t kh, int32_t kw,
                   int32_t stride, int32_t pad_h, int32_t pad_w, int32_t relu, int32_t tile, int32_t storage_type,
                   dd_stream_t stream);
/* Name of the kernel instantiation dd_conv2d_nhwc launches for rows = m * hout * wout output pixels, for profile
 * matching; "" for arguments it would reject. */
const char* dd_conv2d_kernel_name(int64_t rows, int32_t cout, int32_t tile, int32_t storage_type);

/* The 3 x 3 pools of that network, NHWC, c % 8 == 0, x dense [m][h][wd][c], out as dd_conv2d_nhwc's (ldc % 8 == 0,
 * c_off % 8 == 0, 16-byte aligned):
 *   mode 0: max, stride 2, pad 0   (F.max_pool2d(x, kernel_size=3, stride=2): inception.py:89, 98 and the grid
 *                                   reductions Mixed_6a / Mixed_7a)
 *   mode 1: max, stride 1, pad 1   (FIDInceptionE_2, :333-338; only in-image taps take part)
 *   mode 2: average, stride 1, pad 1, divided by the number of in-image taps (count_include_pad=False, the FID patch
 *           at :241-242, 269-270, 302-303) */
int dd_pool3x3_nhwc(const void* x, void* out, int64_t ldc, int32_t c_off, int32_t m, int32_t h, int32_t wd, int32_t c,
                    int32_t mode, int32_t storage_type, dd_stream_t stream);
/* AdaptiveAvgPool2d(1) (inception.py:122) / get_activations' adaptive_avg_pool2d (tools/fid_score.py:147-148):
 * x T [m][hw][c] -> out fp32 [m][c], summed in fp32 in pixel order. */
int dd_global_avgpool_nhwc(const void* x, float* out, int32_t m, int32_t hw, int32_t c, int32_t storage_type,
                           dd_stream_t stream);
/* The head of forward(inp) (inception.py:146-153): x [m][3][h][wd] in [0, 1], in_type DD_F16 / DD_BF16 / 2 (fp32)
 * -> F.interpolate(size=(oh, ow), mode='bilinear', align_corners=False) (no antialiasing; resize = 0 skips it and needs
 * oh == h, ow == wd) -> 2 x - 1 (normalize = 0 skips it) -> out T NHWC [m][oh][ow][c_pad], channels 3 .. c_pad - 1
 * zero, c_pad % 8 == 0. */
int dd_inception_input(const void* x, void* out, int32_t m, int32_t h, int32_t wd, int32_t oh, int32_t ow,
                       int32_t c_pad, int32_t resize, int32_t normalize, int32_t in_type, int32_t storage_type,
                       dd_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Image output (csrc/image.hip): what the reference does to the decoded images before it saves them — the host copy
 * and diffusers' numpy_to_pil, `(images * 255).round().astype("uint8")` (pipeline/pipeline_bev_controlnet.py:112,540,
 * numpy_to_pil_double :72-80), then per view torchvision's Resize(cfg.fid.resize, BICUBIC) and Pad(cfg.fid.padding) on
 * the PIL image (perception/data_prepare/val_set_gen.py:147-159, applied at :44).
 * ------------------------------------------------------------------------- */
/* x: NCHW (m, 3, h, w) in `dtype` (DD_F16, DD_BF16 or DD_F32), contiguous -> out: NHWC (m, h, w, 3) bytes,
 *   v = m11 ? clamp(float(x) / 2 + 0.5, 0, 1) : clamp(float(x), 0, 1)     (m11: a decoder output in [-1, 1], the
 *                                                                           arithmetic of decode_latents, :110-111)
 *   q = (uint8) rint(v * 255)          one fp32 multiply, round to nearest even (numpy's round)
 * out needs no alignment (dword stores where an image's first byte is 4-byte aligned, byte stores otherwise).
 * m <= 65535 and h * w < 2^31, else DD_ERR_UNSUPPORTED. */
int dd_image_quantize_u8(const void* x, uint8_t* out, int32_t m, int32_t h, int32_t w, int32_t m11, int32_t dtype,
                         dd_stream_t stream);

/* PIL's Image.resize(BICUBIC) of the quantised image (ImagingResample on 8-bit pixels: two passes of integer
 * arithmetic over fixed-point coefficient tables) followed by Pad, in one launch and without the uint8 input image:
 *   q                = the bytes dd_image_quantize_u8 would write for x
 *   t[r, X, c]       = clamp8( ((1 << 21) + sum_{j < bx[X].count} q[r, bx[X].xmin + j, c] * kx[X][j]) >> 22 )
 *   out[Y, X, c]     = clamp8( ((1 << 21) + sum_{j < by[Y].count} t[by[Y].xmin + j, X, c] * ky[Y][j]) >> 22 )
 * in int32 with an arithmetic shift, clamp8 = clamp to [0, 255]; t is rounded and clipped to a byte between the
 * passes, as PIL does.  The (oh, ow) result sits at (pad_t, pad_l) of out, (m, pad_t + oh + pad_b, pad_l + ow + pad_r,
 * 3) bytes; every other pixel of out is `fill`.  out needs no alignment.
 * Tables (device memory, int32): kx [ow][ksx], bx [ow][2] = {xmin, count}; ky [oh][ksy], by [oh][2].  They are PIL's
 * precompute_coeffs + normalize_coeffs_8bpc, built by the caller in float64 (dualdiff_amd/pipeline/image_output.py:
 * resample_tables): scale = in / out, fs = max(scale, 1), support = 2 fs, ksize = 2 ceil(support) + 1; for output xx:
 * c = (xx + 0.5) scale, xmin = max(int(c - support + 0.5), 0), count = min(int(c + support + 0.5), in) - xmin,
 * w[x] = bicubic((x + xmin - c + 0.5) / fs) with a = -0.5, normalised by their left-to-right sum, then
 * k = int(w * 2^22 +- 0.5) (towards the sign of w), zero after `count`.  An axis that keeps its size takes the one-tap
 * table {k = 1 << 22, xmin = xx, count = 1} (PIL skips that pass; the bytes are the same).
 * A workgroup owns an output tile and keeps its slice of t in LDS; the slice is sized for PIL's tables, whose T
 * consecutive outputs read at most ceil((T - 1) in / out) + ksize + 1 inputs.  Entries of other tables are clamped to
 * the image and to that slice: the result is then unspecified, nothing outside the buffers is touched.
 * 1 <= ksx, ksy <= DD_IMAGE_MAX_KSIZE (in / out up to 8; a tile that does not fit 64 KB of LDS at the smallest tile
 * size), m <= 65535: else DD_ERR_UNSUPPORTED.  NULL pointers, non-positive sizes, negative pads, fill outside [0, 255]:
 * DD_ERR_BAD_ARG.  Both are decided before anything is launched. */
#define DD_IMAGE_MAX_KSIZE 33
int dd_image_resample_u8(const void* x, uint8_t* out, int32_t m, int32_t h, int32_t w, int32_t oh, int32_t ow,
                         const int32_t* kx, const int32_t* bx, int32_t ksx, const int32_t* ky, const int32_t* by,
                         int32_t ksy, int32_t pad_l, int32_t pad_t, int32_t pad_r, int32_t pad_b, int32_t fill,
                         int32_t m11, int32_t dtype, dd_stream_t stream);

/* Image input, the other direction: uint8 camera frames -> the normalised pixel values the VAE encoder takes, i.e. the
 * reference's dataset transform  pil.resize((newW, newH)).crop(box) -> ToTensor -> Normalize(mean, std)  in one launch:
 *   t[r, X, c]   = clamp8( ((1 << 21) + sum_{j < bx[X].count} in[r, bx[X].xmin + j, c] * kx[X][j]) >> 22 )
 *   p[Y, X, c]   = clamp8( ((1 << 21) + sum_{j < by[Y].count} t[by[Y].xmin + j, X, c] * ky[Y][j]) >> 22 )
 *   out[.., c]   = T( lut[c][p[Y, X, c]] )                                  one rounding, to `dtype`
 * — the formulas of dd_image_resample_u8 (int32, arithmetic shift, the horizontal pass first and rounded to a byte), on
 * bytes that are already there.
 * in: (m, h, w, 3) bytes, contiguous, device memory, any alignment.
 * Tables: as for dd_image_resample_u8 (xmin absolute into `in`), but kx / bx hold `ow` rows and ky / by `oh` rows that
 * START at the first output column / row of the crop: the caller passes the tables of the resized image offset by the
 * crop's left / top, and ow x oh is the crop's size.  Nothing outside the crop is computed.
 * lut: float[3][256], device memory: the normalisation per channel, built by the caller (for torchvision's ToTensor +
 * Normalize: lut[c][b] = (float(b) / 255 - mean[c]) / std[c] in float32).  The kernel does no floating-point arithmetic.
 * out, in `dtype` (DD_F16, DD_BF16 or DD_F32):
 *   layout 0: (m, 3, oh, ow) NCHW;
 *   layout 1: (m * oh * ow, 8) channels-last rows with channels 3..7 written as zero (what conv_in of the VAE encoder
 *             reads); out 16-byte aligned.
 * A workgroup's LDS slice is sized from ksize alone (in / out <= max(ksize - 1, 4) / 4 for PIL's tables); entries of other
 * tables are clamped to the image and to that slice: the result is then unspecified, nothing outside the buffers is
 * touched.  NULL pointers, non-positive sizes, an unknown dtype or layout, a misaligned layout-1 out: DD_ERR_BAD_ARG.
 * ksx, ksy > DD_IMAGE_MAX_KSIZE, m > 65535, a side of 2^24 or more, no tile that fits 64 KB of LDS: DD_ERR_UNSUPPORTED.
 * Both are decided before anything is launched. */
int dd_image_load_u8(const uint8_t* in, void* out, int32_t m, int32_t h, int32_t w, int32_t oh, int32_t ow,
                     const int32_t* kx, const int32_t* bx, int32_t ksx, const int32_t* ky, const int32_t* by,
                     int32_t ksy, const float* lut, int32_t dtype, int32_t layout, dd_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Box input (csrc/boxes.hip): 3D box corners -> the per-view `bboxes_3d_data` of the reference's collate function
 * (dataset/utils.py:128-262: per-view visibility, order-preserving selection, padding), in the layout dd_box_tokens reads.
 *   corners        [total][8][3] fp32: the payload, every scene's boxes concatenated;
 *   filter_corners same shape, or NULL (= corners): the corners that are transformed for the visibility test (the
 *                  reference tests the box re-centred to (0.5, 0.5, 0.5), runner/box_visualizer.py:63);
 *   labels         [total] int64;
 *   offsets        [scenes + 1] int32: scene s owns boxes offsets[s] .. offsets[s + 1] (clamped to [0, total] and to
 *                  non-decreasing by the kernel; an empty scene is legal);
 *   transforms     [scenes][views][4][4] fp32, row-major; NULL only for filter_mode 0.
 * points_mode 0: all 8 corners (`all-xyz`); 1: corners 6, 5, 7, 2 in that order (`cxyz`, dataset/utils.py:224).
 * filter_mode 0: keep every box (`view_shared`; views must be 1);
 *             1: `ensure_positive_z`: keep a box if any corner has z > 0;
 *             2: `ensure_canvas`: zc = clip(z, 1e-5, 1e5), x /= zc, y /= zc; keep if any corner has z / |z| > 0 AND any
 *                corner has 0 < x < canvas_w AND any corner has 0 < y < canvas_h (three independent "any").
 * (x, y, z) = rows 0..2 of  matrix (promoted to double) * (corner promoted to double, 1.0), float64 with IEEE division as
 * in runner/box_visualizer.py:71-85; the order of the four-term sums is the kernel's (fused multiply-adds from the
 * translation column on), so a quantity within rounding of its threshold may decide differently than another summation.
 * Out, for every (scene, view), rows of `cap` slots and P = 8 or 4 points:
 *   bboxes  [scenes][views][cap][P][3] fp32: the kept boxes' payload points in their original order, then zeros;
 *   classes [scenes][views][cap] int64: their labels, then -1;
 *   masks   [scenes][views][cap] bytes: 1 for a kept box, then 0;
 *   counts  [scenes][views] int32: the number kept, also when it exceeds cap (the boxes beyond cap are dropped);
 *   max_len [1] int32: the largest count of this launch, whatever it held before (cleared on the stream, then a vector
 *           atomic max per workgroup).
 * Every slot below cap is written and nothing at or past it.  Pointers need their element's alignment only (4 bytes for
 * the fp32 / int32 arrays, 8 for the int64 ones); rows move as 16-byte vectors where the base allows it.
 * DD_ERR_BAD_ARG, decided before the first runtime call: a NULL required pointer (corners / labels may be NULL when
 * total == 0), total < 0, non-positive scenes / views / cap, an unknown mode, filter_mode 0 with views != 1, filter_mode
 * 1 or 2 without transforms, filter_mode 2 with a non-positive canvas, a misaligned pointer.  scenes * views >= 2^31 or
 * scenes * views * cap >= 2^40: DD_ERR_UNSUPPORTED.
 * ------------------------------------------------------------------------- */
int dd_box_views(const float* corners, const float* filter_corners, const int64_t* labels, const int32_t* offsets,
                 const float* transforms, int32_t total, int32_t scenes, int32_t views, int32_t cap,
                 int32_t points_mode, int32_t filter_mode, int32_t canvas_h, int32_t canvas_w, float* bboxes,
                 int64_t* classes, uint8_t* masks, int32_t* counts, int32_t* max_len, dd_stream_t stream);

/* ------------------------------------------------------------------------- *
 * JPEG output (csrc/jpeg.hip): the uint8 frames dd_image_resample_u8 / dd_image_quantize_u8 write -> the files the
 * reference saves with PIL's `Image.save(<name>.jpg)` and no options (perception/data_prepare/val_set_gen.py:44,
 * tools/downstream_v3_batched.py:244-252), byte for byte: libjpeg's baseline encoder, 4:2:0 chroma, the `islow` integer
 * DCT, quantisation by 8 q rounding half away from zero, libjpeg's dummy blocks at the right and bottom edge.
 *
 * frames: uint8 [m][h][w][3] (device).  header: the file up to and including SOS, header_len bytes in DEVICE memory, built
 * by the caller once per (h, w, quality) (pipeline/image_output.py: jpeg_header).  tables: uint32 [672] (device), from the
 * same place as the header's DQT segments:
 *   [0, 128)    q[2][64]: the luma and chroma quantisation values in zigzag order, as DQT holds them
 *   [128, 160)  dc[2][16]: Huffman entry (code << 8) | length of DC size s, luma then chroma
 *   [160, 672)  ac[2][256]: the entry of AC symbol (run << 4) | size
 * (a q outside 1..65535 and a length above 16 are clamped: no table contents make the kernels leave their buffers).
 * out: uint8 [m][capacity], row i = file i; lengths: int32 [m], the TRUE length of file i also when it exceeds capacity —
 * the row then holds the first `capacity` bytes of the file and nothing is written outside it.
 * workspace: at least dd_jpeg_workspace_bytes(m, h, w) bytes, 16-byte aligned, contents don't care before and after.
 * Six launches on `stream` whatever m and the content are, no host synchronisation: the call can be captured in a graph.
 * DD_ERR_BAD_ARG, before any runtime call: a NULL pointer, m / h / w / header_len <= 0, h or w above 65535, capacity <
 * header_len + 2, a misaligned workspace / tables / lengths, workspace_bytes too small.  m > 65535 or more than 262144
 * MCUs (16 x 16 pixels) per frame: DD_ERR_UNSUPPORTED; dd_jpeg_workspace_bytes returns -1 for either kind.
 * ------------------------------------------------------------------------- */
int64_t dd_jpeg_workspace_bytes(int32_t m, int32_t h, int32_t w);
int dd_jpeg_encode_u8(const uint8_t* frames, int32_t m, int32_t h, int32_t w, const uint8_t* header, int32_t header_len,
                      const uint32_t* tables, void* workspace, int64_t workspace_bytes, uint8_t* out, int64_t capacity,
                      int32_t* lengths, dd_stream_t stream);

/* ------------------------------------------------------------------------- *
 * PNG output (csrc/png.hip): the same uint8 frames -> lossless .png files, as the reference's demo and validation path
 * saves its view grids (tools/test.py:74-97, runner/img_utils.py:5-40).  Not PIL's bytes (zlib's lazy-match parse is one
 * sequential chain): a valid PNG that decodes to exactly the input, in a format fixed so that every step is local to a
 * row, a run of equal bytes or a 16 KiB chunk: 8-bit RGB, colour type 2, no interlace; per row the
 * filter 0..4 with the smallest sum of min(b, 256 - b), ties to the lowest type; the filtered stream in chunks of 16384
 * bytes, each one dynamic-Huffman block over literals and distance-1 matches (zlib Z_RLE's rule) that an empty stored
 * block aligns, or one stored block where that is shorter; one IDAT per chunk.
 *
 * frames: uint8 [m][h][w][3] (device), any alignment.  out: uint8 [m][capacity], row i = file i; lengths: int32 [m], the
 * TRUE length of file i also when it exceeds capacity — the row then holds the first `capacity` bytes of the file and
 * nothing is written outside it.  No file is longer than 51 + 17 * ceil(n / 16384) + n bytes, n = h * (1 + 3 * w).
 * workspace: at least dd_png_workspace_bytes(m, h, w) bytes, 16-byte aligned, contents don't care before and after.
 * Four launches on `stream` whatever m and the content are, no host synchronisation: the call can be captured in a graph.
 * DD_ERR_BAD_ARG, before any runtime call: a NULL pointer, m / h / w <= 0, capacity < 51 (signature, IHDR, IEND, the zlib
 * header and the Adler-32), a misaligned workspace / lengths, workspace_bytes too small.  m > 65535 or a frame whose
 * longest possible file exceeds 2^31 - 1 bytes: DD_ERR_UNSUPPORTED; dd_png_workspace_bytes returns -1 for either kind.
 * ------------------------------------------------------------------------- */
int64_t dd_png_workspace_bytes(int32_t m, int32_t h, int32_t w);
int dd_png_encode_u8(const uint8_t* frames, int32_t m, int32_t h, int32_t w, void* workspace, int64_t workspace_bytes,
                     uint8_t* out, int64_t capacity, int32_t* lengths, dd_stream_t stream);
/* The same for frames of `channels` bytes per pixel, uint8 [m][h][w][channels]: 3 is dd_png_encode_u8 (the same bytes), 4
 * is RGBA — colour type 6, the filters' left neighbour four bytes back, n = h * (1 + 4 * w) in the bound above.  The
 * RGBA box overlays (dd_box_draw_u8, transparent = 1) are saved through it.  Any other `channels`: DD_ERR_BAD_ARG (-1 from
 * dd_png_workspace_bytes_c); everything else as above. */
int64_t dd_png_workspace_bytes_c(int32_t m, int32_t h, int32_t w, int32_t channels);
int dd_png_encode_u8c(const uint8_t* frames, int32_t m, int32_t h, int32_t w, int32_t channels, void* workspace,
                      int64_t workspace_bytes, uint8_t* out, int64_t capacity, int32_t* lengths, dd_stream_t stream);

/* ------------------------------------------------------------------------- *
 * JPEG input (csrc/jpeg_decode.hip, csrc/jpeg_decode_core.h): the entropy-coded segments of m baseline .jpg files of one
 * geometry -> uint8 frames [m][h][w][3] (device), byte for byte what PIL's `Image.open(f).convert("RGB")` returns for
 * the camera files the reference opens (configs/dataset/Nuscenes.yaml:98,183 LoadMultiViewImageFromFiles,
 * networks/occ3d_proj.py:124, tools/fid_score.py:79): libjpeg's Huffman decoder, the `islow` integer inverse DCT, the
 * "fancy" triangle chroma upsampling (plain 2 x 2 replication where the chroma plane is at most two columns wide, i.e. for
 * 4:2:0 frames of width 1..4, as jdsample.c chooses), the 16-bit fixed-point colour conversion.  The host reads the files' headers only
 * (pipeline/jpeg_input.py: parse_jpeg); no pass over the scan bytes runs there.
 *
 * scan: scan_bytes bytes (device) that hold every frame's segment — the bytes between SOS and EOI, still byte-stuffed —
 * frame i at scan + offsets[i], lengths[i] bytes, at any byte alignment; offsets / lengths: int32 [m] (device).  Every
 * read is clamped to [0, scan_bytes) and to max_scan_bytes per frame, whatever offsets and lengths hold.
 * tables: one block of 4016 bytes per frame (device, 4-byte aligned), little-endian, as jpeg_input.table_block builds it:
 *   [0, 384)      uint16 q[3][64]: the quantisation values of component Y, Cb, Cr in natural (row-major) order
 *   [384, 392)    uint8 tdc[3], tac[3]: the DC / AC Huffman table (0 or 1) of each component; 2 bytes of padding
 *   [392, 4008)   four Huffman tables of 904 bytes, DC 0, DC 1, AC 0, AC 1:
 *                   uint16 lut[256]  the next 8 bits -> (code length << 8) | symbol, 0 for a code longer than 8 bits
 *                   int32 lim[17]    lim[l] = (the largest code of length <= l, plus 1) << (16 - l)
 *                   int32 off[17]    symbol of a code of length l = vals[off[l] + (next 16 bits >> (16 - l))]
 *                   uint8 vals[256]
 *   [4008, 4016)  padding
 * (no table contents make the kernels leave their buffers: lengths are clamped, indices masked).
 * sampling: 420 (luma 2 x 2, chroma 1 x 1) or 444 (all 1 x 1).  out: uint8 [m][h][w][3], any alignment; only rows below h
 * and columns below w are stored.  status: int32 [m], per frame 0 or an OR of DD_JPEG_EXHAUSTED (the stream ended before
 * the frame's last block), DD_JPEG_BAD_CODE (a bit pattern in no table, or a symbol baseline does not have),
 * DD_JPEG_BAD_RUN (a zero run past coefficient 63), DD_JPEG_TRAILING (a byte or more of the stream is left behind the
 * last block: libjpeg decodes such a file with a warning, this decoder leaves it to the caller); the frame's pixels are
 * then unspecified, the other frames' are not affected.
 * rounds: how often every subsequence of DD_JPEG_SUB_BITS bits is decoded again from its left neighbour's exit state
 * before the in-order repair pass decodes whatever is still not proven; 0..64, or -1 for DD_JPEG_DECODE_ROUNDS.  The
 * result does not depend on it (0 sends the whole stream through the repair pass); it is there for tests and timing.
 * workspace: at least dd_jpeg_decode_workspace_bytes(m, h, w, sampling, max_scan_bytes) bytes, 16-byte aligned, contents
 * don't care before and after; max_scan_bytes >= every lengths[i].
 * One memset and 9 + rounds launches on `stream` (a round whose subsequences all stand costs about 5 us), whatever m and the content are; no host synchronisation, no waiting
 * between workgroups: the call can be captured in a graph.
 * DD_ERR_BAD_ARG, before any runtime call: a NULL pointer, m / h / w / scan_bytes / max_scan_bytes <= 0, h or w above
 * 65535, a sampling other than 420 / 444, rounds outside -1..64, a misaligned workspace / tables / offsets / lengths /
 * status, workspace_bytes too small.  m > 65535, more than 262144 MCUs per frame or max_scan_bytes above 2^27:
 * DD_ERR_UNSUPPORTED; dd_jpeg_decode_workspace_bytes returns -1 for either kind.
 * ------------------------------------------------------------------------- */
#define DD_JPEG_SUB_BITS 1024
#define DD_JPEG_DECODE_ROUNDS 10
#define DD_JPEG_EXHAUSTED 1
#define DD_JPEG_BAD_CODE 2
#define DD_JPEG_BAD_RUN 4
#define DD_JPEG_TRAILING 8
int64_t dd_jpeg_decode_workspace_bytes(int32_t m, int32_t h, int32_t w, int32_t sampling, int64_t max_scan_bytes);
int dd_jpeg_decode_u8(const uint8_t* scan, int64_t scan_bytes, const int32_t* offsets, const int32_t* lengths,
                      int64_t max_scan_bytes, const void* tables, int32_t m, int32_t h, int32_t w, int32_t sampling,
                      uint8_t* out, int32_t* status, void* workspace, int64_t workspace_bytes, int32_t rounds,
                      dd_stream_t stream);

/* ------------------------------------------------------------------------- *
 * PNG input (csrc/png_decode.hip, csrc/png_decode_core.h): the IDAT payloads of m .png files of one geometry -> uint8
 * frames [m][h][w][3] (device), byte for byte what PIL's `Image.open(f).convert("RGB")` returns: the files of the
 * reference's default ORS condition, one RGBA panorama of six views per sample (magicdrive/dataset/dataset_wrapper.py:62-81
 * OccFolderSetWrapper(mode='image'), misc/test_utils.py:218-222), and the files dd_png_encode_u8 writes
 * (tools/test.py:74-97).  Bit depth 8, no interlace, colour type 0 (grey, replicated), 2 (RGB) or 6 (RGBA, alpha
 * dropped); any zlib stream: stored, fixed and dynamic blocks, distances up to 32768, any number of blocks.  The host walks
 * the chunks and checks their CRCs (pipeline/png_input.py: parse_png); inflate, the Adler-32, the five row filters and
 * the conversion run on the device.
 *
 * streams: streams_bytes bytes (device) that hold every file's concatenated IDAT payloads, chunk framing stripped.
 * files: int32 [m][4] (device): the stream's offset in `streams`, its length, the file's colour type, and the index in
 * `tab` of the file's IDAT boundaries or -1.  Every read is clamped to the stream and to [0, streams_bytes), whatever the
 * tables hold.  tab: int32 [ntab] (device, may be NULL when ntab is 0): for a file that has the shape of
 * dd_png_encode_u8's format — colour type 2, exactly ceil(h (1 + 3 w) / 16384) IDATs — its n + 1 IDAT boundaries relative
 * to the stream's start.  The shape proves nothing, so the device verifies: one workgroup per IDAT inflates it from bit 0
 * into its 16 KiB slot, and the file counts as chunked only if every one consumed exactly its payload, produced exactly
 * its slot, reached with no match before its slot and met BFINAL exactly at the end of the last one — then the result is
 * the sequential decode's, by induction over the chunks.  Any other file is inflated by one workgroup from its first
 * block to its last, in the launch behind, with no host synchronisation between the two.
 * colour_types: int32 [m] in HOST memory, read before the launches: the same colour types, for validation.
 * chunked: 1 to use `tab`, 0 to send every file through the sequential path (the frames do not depend on it).
 * out: uint8 [m][h][w][3].  status: int32 [m], per frame 0 or one of the DD_PNG_* bits below — the first thing found
 * wrong; the frame's pixels are then unspecified, the other frames' are not affected.  paths: int32 [m], 1 where the
 * chunk-parallel result was used.  workspace: at least dd_png_decode_workspace_bytes(m, h, w) bytes, 16-byte aligned.
 * One memset and four launches on `stream` (three with chunked 0 or ntab 0) whatever m and the content are; every loop
 * of the kernels consumes input bits or counts against the frame's size, every read is bounded by the stream and every
 * write by the frame, so a broken file costs its own frame and nothing else.  No host synchronisation: the call can be
 * captured in a graph.
 * DD_ERR_BAD_ARG, before any runtime call: a NULL pointer, m / h / w / streams_bytes <= 0, ntab < 0, chunked not 0 / 1,
 * a colour type other than 0 / 2 / 6, a misaligned workspace / files / tab / status / paths, workspace_bytes too small.
 * m > 65535 or a frame of more than 2^31 - 16385 filtered bytes at four bytes per pixel: DD_ERR_UNSUPPORTED;
 * dd_png_decode_workspace_bytes returns -1 for either kind.
 *
 * dd_png_condition: the collate step of that condition (dataset/utils.py:348-408), one launch: uint8 frames [b][h][w][3],
 * each a panorama of `views` views side by side, -> float32 [b][3][oh][views * ow], the `ToTensor()` value lut[byte] of
 * rows top .. top + oh and, per view, columns left .. left + ow (crop_hd: top 176, left 32, 256 x 704 of 432 x 768).
 * lut: float32 [256] (device): byte / 255, built by the caller.  DD_ERR_BAD_ARG: a NULL pointer, a size <= 0, top or
 * left < 0, w no multiple of views, a crop that leaves the view, a misaligned out / lut.
 *
 * dd_png_condition_resize: the same step for image_size [192, 384], `crop_drivewm` (dataset/utils.py:355-358 pad_top,
 * :374-388, called at :398-403), one launch, no host synchronisation: every view of uint8 frames [b][h][w][3] gets
 * `pad_top` zero rows on top, is resized to rh x rw as torchvision 0.11.3's `transforms.Resize((216, 384))` resizes a float
 * tensor — `F.interpolate(mode="bilinear", align_corners=False)`, no antialias, PER VIEW: the clamp at a view's last column
 * and the rounding of the coordinates are the view's own — and cropped to rows top .. top + oh, columns left .. left + ow
 * (hd_crop: top 24, left 0, 192 x 384 of 216 x 384); out float32 [b][3][oh][views * ow], 16-byte aligned.
 * row_taps / col_taps: int32 [rh][2] / [rw][2] (device), per resized row / column its two source positions (i0, i1) in the
 * PADDED view, [0, h + pad_top) / [0, w / views); clamped to that range whatever they hold.  row_weights / col_weights:
 * float32 [rh][2] / [rw][2], (l0, l1).  The caller builds them in float32 (image_tables.bilinear_tables):
 *   scale = float(in) / float(out);  src = fmaf(scale, float(dst) + 0.5f, -0.5f), src < 0 -> 0;  i0 = (int)src,
 *   i1 = i0 + (i0 < in - 1);  l1 = clamp(src - i0, 0, 1), l0 = 1 - l1.
 * With A, B the values lut[byte] (0.0f in a padded row) at (i0 row, i0 / i1 column) and C, D those of row i1:
 *   t = fmaf(bl0, A, bl1 * B);  u = fmaf(bl0, C, bl1 * D);  out = fmaf(al0, t, al1 * u),
 * every product and every fused multiply-add rounded once to float32 — the form that torch's multi-threaded CPU kernel
 * takes at the reference's geometry; torch's single-threaded one differs from it in the last place.  An identity resize
 * (rh = h + pad_top, rw = w / views) has l1 = 0 everywhere and returns dd_png_condition's bits.
 * DD_ERR_BAD_ARG, before any runtime call: a NULL pointer, a size <= 0, pad_top / top / left < 0, w no multiple of views, a
 * crop that leaves the resized view, an out that is not 16-byte aligned, a misaligned table.  A frame of 2^31 bytes or
 * more, or a batch of more than 2^40: DD_ERR_UNSUPPORTED.
 * ------------------------------------------------------------------------- */
#define DD_PNG_TRUNCATED 1
#define DD_PNG_BAD_BLOCK 2
#define DD_PNG_BAD_STORED 4
#define DD_PNG_BAD_LENGTHS 8
#define DD_PNG_BAD_SYMBOL 16
#define DD_PNG_BAD_DISTANCE 32
#define DD_PNG_TOO_LONG 64
#define DD_PNG_TOO_SHORT 128
#define DD_PNG_BAD_ADLER 256
#define DD_PNG_BAD_ZLIB 512
#define DD_PNG_BAD_FILTER 1024
int64_t dd_png_decode_workspace_bytes(int32_t m, int32_t h, int32_t w);
int dd_png_decode_u8(const uint8_t* streams, int64_t streams_bytes, const int32_t* files, const int32_t* tab, int32_t ntab,
                     const int32_t* colour_types, int32_t m, int32_t h, int32_t w, int32_t chunked, uint8_t* out,
                     int32_t* status, int32_t* paths, void* workspace, int64_t workspace_bytes, dd_stream_t stream);
int dd_png_condition(const uint8_t* frames, float* out, const float* lut, int32_t b, int32_t h, int32_t w, int32_t views,
                     int32_t top, int32_t left, int32_t oh, int32_t ow, dd_stream_t stream);
int dd_png_condition_resize(const uint8_t* frames, float* out, const float* lut, const int32_t* row_taps,
                            const float* row_weights, const int32_t* col_taps, const float* col_weights, int32_t b, int32_t h,
                            int32_t w, int32_t views, int32_t pad_top, int32_t rh, int32_t rw, int32_t top, int32_t left,
                            int32_t oh, int32_t ow, dd_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Map output (csrc/map.hip): the picture the reference's `visualize_map` makes of a sample's BEV map
 * (runner/map_visualizer.py:143-211; misc/test_utils.py:344-348 calls it per sample, tools/test.py:76 saves it).
 *
 * dd_map_render_u8: the colouring (:106-132, :180-190) and the classes in use (:114-115, :127-128), one launch.
 *   maps  uint8 [b][c][s][s] (device), 0 / 1: static layers are planes [0, ns), dynamic layers [ns, ns + nd); planes from
 *         ns + nd on are not read.  ns + nd <= c.
 *   stab  float [ns + 1][4] (device): per static layer {r / 255, g / 255, b / 255, rank}, rank = its index in the
 *         reference's STATIC_PRIORITY (:49-60); row ns is the "nothing" colour (:43), whose rank is not read.
 *   dtab  float [nd][4] (device): per dynamic layer its colour / 255; NULL when nd == 0.
 *   img   float [b][3][s][s]: per pixel the colour / 255 of the first set dynamic layer (argmax, :127-130), else of the set
 *         static layer of the greatest rank (:67-73; the first one among equal ranks), else of "nothing".  The quotients
 *         are the caller's, so that dd_image_resample_u8 quantises them back to the colour bytes.
 *   used  int32 [b]: whatever it held before, bit k < ns: static layer k is set at some pixel; bit ns + j: dynamic layer j
 *         is the argmax at some pixel, which for j = 0 includes every pixel with no dynamic layer set; bit 31: some read
 *         byte is neither 0 nor 1 (the picture is then unspecified).  Cleared on the stream, then one vector atomic OR
 *         per workgroup.
 * DD_ERR_BAD_ARG, before any runtime call: a NULL maps / stab / img / used, NULL dtab with nd > 0, b / c / s <= 0, ns or
 * nd < 0, ns + nd == 0 or > c, a table, img or used that is not 4-byte aligned.  ns + nd > DD_MAP_MAX_LAYERS (bit 31 is
 * taken), s >= 2^14 or b > 65535: DD_ERR_UNSUPPORTED.
 *
 * dd_map_compose_u8: what follows the resize (:197-209) for g samples that share a legend, one launch.
 *   src    uint8 [m][t][t][3] (device): the resized, not yet turned pictures (dd_image_resample_u8's output);
 *   index  int32 [g] (device): the sample of src each output takes, clamped to [0, m); NULL: g == m, in order;
 *   legend uint8 [lh][lw][3] (device), or NULL with lh == lw == 0;
 *   side   0: the legend to the right (the reference's choice for lh > lw), out [g][t][t + lw][3], lh <= t;
 *          1: below, out [g][t + lh][t][3], lw <= t.
 *   out[r][c] = src[c][t - 1 - r] for r, c < t: Image.rotate(90) of a square image, i.e. np.rot90(x, 1); the legend at
 *   (0, t) or (t, 0); zero elsewhere, as np.pad leaves it.
 * DD_ERR_BAD_ARG, before any runtime call: a NULL src / out, m / g / t <= 0, lh or lw < 0, a legend without a size or a
 * size without a legend, side not 0 / 1, NULL index with g != m, a misaligned index, a legend longer than the side it
 * lies along.  t, lh or lw >= 2^14, m or g > 65535: DD_ERR_UNSUPPORTED.
 * ------------------------------------------------------------------------- */
#define DD_MAP_MAX_LAYERS 31
int dd_map_render_u8(const uint8_t* maps, const float* stab, const float* dtab, float* img, int32_t* used, int32_t b,
                     int32_t c, int32_t s, int32_t ns, int32_t nd, dd_stream_t stream);
int dd_map_compose_u8(const uint8_t* src, const int32_t* index, const uint8_t* legend, uint8_t* out, int32_t m, int32_t g,
                      int32_t t, int32_t lh, int32_t lw, int32_t side, dd_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Box output (csrc/box_overlay.hip, csrc/box_overlay_core.h): the 3D-box overlays of the reference's demo path
 * (misc/test_utils.py:48-65 draw_box_on_imgs -> runner/box_visualizer.py:89-114 show_box_on_views; tools/test.py:86-97
 * saves them as `{n}_ori_box.png` / `{n}_gen{t}_box.png`).  The geometry is the reference's.  The line is PIL's thin line
 * (`ImageDraw.line(..., width=1)`), not the anti-aliased `cv2.line(..., LINE_AA)` the reference draws through mmdet3d: the
 * pictures differ from the reference's in the anti-aliasing fringe of the 1-pixel lines, and only there.
 *
 * dd_box_edges: one launch, no host synchronisation.  Inputs as dd_box_views takes them (device):
 *   corners    [total][8][3] fp32: the boxes re-centred to (0.5, 0.5, 0.5) (runner/box_visualizer.py:94);
 *   labels     [total] int64;  offsets [scenes + 1] int32 (clamped as dd_box_views clamps them);
 *   transforms [scenes][views][4][4] fp32, row-major: img_aug_matrix @ lidar2image (:102-104).
 *  G1 (x, y, z) = rows 0..2 of the matrix (promoted to double) * (corner promoted to double, 1.0), summed as dd_box_views
 *     sums (fused multiply-adds from the translation column on): a quantity within rounding of a threshold or of an
 *     integer may come out differently under another summation order.
 *  G2 a box is drawn in a view iff all 8 of its z are > 0 and its label lies in [-n_classes, n_classes).
 *  G3 draw order: descending least z of the box (farthest first), ties to the lower index.
 *  G4 zc = clip(z, 1e-5, 1e5), u = x / zc, v = y / zc (IEEE double); the integer point is u, v truncated toward zero;
 *     a value beyond +-2^29 is stored as +-2^29 (a NaN as -2^29) and sets DD_BOX_FLAG_SATURATED.
 *  G6 the class is the label, a negative one + n_classes (Python's indexing).
 * Out, for every (scene, view), rows of `cap` slots in draw order:
 *   pts    [scenes][views][cap][8][2] int32, 16-byte aligned: (x, y) of corner 0..7; slots past the count are zero;
 *   cls    [scenes][views][cap] int32: the class in [0, n_classes); zero past the count;
 *   counts [scenes][views] int32: the number of boxes drawn, also when it exceeds cap — then the nearest `cap` are in the
 *          row (the last `cap` of the draw order) and DD_BOX_FLAG_CAP is set;
 *   flags  [1] int32: whatever it held before, an OR of DD_BOX_FLAG_* over the launch (cleared on the stream, then at
 *          most one vector atomic OR per wave).  DD_BOX_FLAG_SATURATED is set for boxes that are in a row only.
 * A scene holds at most DD_BOX_EDGES_MAX boxes: of a longer one the first DD_BOX_EDGES_MAX are read and DD_BOX_FLAG_CAP
 * is set.  DD_ERR_BAD_ARG, before any runtime call: a NULL pointer (corners / labels may be NULL when total == 0),
 * total < 0, non-positive scenes / views / cap / n_classes, a pointer that is not aligned to its element (pts: 16
 * bytes).  cap > DD_BOX_EDGES_MAX or scenes * views >= 2^31: DD_ERR_UNSUPPORTED.
 *
 * dd_box_draw_u8: one launch, no host synchronisation, deterministic (no atomics).
 *   frames  uint8 [m][h][w][3] (device), m = scenes * views; NULL is allowed with transparent = 1 (not read then);
 *   pts, cls, counts: as dd_box_edges writes them (a count is clamped to [0, cap], a point to +-2^29, a class to
 *           [0, n_palette));  palette uint8 [n_palette][3] (device): RGB per class;
 *   out     uint8 [m][h][w][3], or [m][h][w][4] with transparent = 1 (then 4-byte aligned).
 *  G5 a box is its 12 edges (0,1) (0,3) (0,4) (1,2) (1,5) (3,2) (3,7) (4,5) (4,7) (2,6) (5,6) (6,7), each PIL's thin
 *     line FROM its first corner TO its second (the line is not symmetric in its end points): with dx = |x1 - x0|,
 *     dy = |y1 - y0|, xs, ys = +-1 (+1 when the end is >= the start) and i = 0 .. max(dx, dy), the pixels
 *     (x0 + xs i, y0 + ys floor((2 dy i + dx) / (2 dx))) for dx >= dy (dx == 0: the one pixel (x0, y0)), else
 *     (x0 + xs floor((2 dx i + dy) / (2 dy)), y0 + ys i).  Nothing is clipped: a pixel asks every line whether it is on it.
 *  G7 a pixel has the colour of the last box in slot order with an edge that covers it; lines are opaque.
 *  G8 transparent = 0: every other pixel is the frame's.  transparent = 1: the boxes on black, A = 255 where any of
 *     R, G, B is > 0, else 0 (misc/test_utils.py:49-64).
 * DD_ERR_BAD_ARG, before any runtime call: a NULL pts / cls / counts / palette / out, NULL frames with transparent = 0,
 * transparent not 0 / 1, non-positive m / cap / h / w / n_palette, a misaligned pts (16), cls, counts (4) or RGBA out
 * (4).  h or w >= 2^15, m > 65535 or m * cap >= 2^40: DD_ERR_UNSUPPORTED.
 * ------------------------------------------------------------------------- */
#define DD_BOX_EDGES_MAX 1024
#define DD_BOX_FLAG_LABEL 1      /* a label outside [-n_classes, n_classes): that box is not drawn */
#define DD_BOX_FLAG_SATURATED 2  /* a coordinate beyond +-2^29 */
#define DD_BOX_FLAG_CAP 4        /* a view drew more than cap boxes, or a scene held more than DD_BOX_EDGES_MAX */
int dd_box_edges(const float* corners, const int64_t* labels, const int32_t* offsets, const float* transforms,
                 int32_t total, int32_t scenes, int32_t views, int32_t cap, int32_t n_classes, int32_t* pts, int32_t* cls,
                 int32_t* counts, int32_t* flags, dd_stream_t stream);
int dd_box_draw_u8(const uint8_t* frames, const int32_t* pts, const int32_t* cls, const int32_t* counts,
                   const uint8_t* palette, uint8_t* out, int32_t m, int32_t cap, int32_t h, int32_t w, int32_t n_palette,
                   int32_t transparent, dd_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Map input (csrc/bev_map.hip, csrc/bev_map_core.h): the BEV object layers and aux channels that the reference's
 * LoadBEVSegmentationM makes from the 3D boxes on the host (magicdrive/dataset/pipeline.py: _project_dynamic_bbox
 * :176-200 and the transpose of :215; _get_dynamic_aux_bbox :88-152 and the transpose of :173), joined to the static
 * layers, which may arrive as the int32 bit fields of the h5 cache (one_hot_decode, dataset/pipeline_utils.py:34-49).
 * Two launches: dd_bev_box_records (one lane per box: its 208-byte record into the workspace) and dd_bev_map_layers
 * (pixel-major, a workgroup per 16 x 16 tile and sample).  No atomics, nothing cleared, nothing allocated.
 *   stat: static_bits = 0: uint8 [b][ns][size][size] holding 0 / 1, copied; static_bits = 1: int32 [b][size][size], layer
 *     c = bit c (4-byte aligned).  May be NULL with ns = 0.
 *   corners fp32 [total][8][3] (the caller's box.corners), bottom_center fp32 [total][3], height, visibility fp32 [total],
 *   labels int64 [total]; offsets int32 [b + 1]: sample i owns boxes offsets[i] .. offsets[i + 1] - 1 in input order
 *   (values are clamped to [0, total]).  All device memory.
 *   sx, ox, sy, oy: lidar2canvas (:70-74): canvas x = x * sx + ox and canvas y = y * sy + oy in float64, two roundings;
 *     the vertex is np.round (half to even) of that, cast to int32, saturated at +-2^20.  Ring: corners 0, 3, 7, 4.
 *   masks: uint8 [b][ns + nd][size][size], any alignment: the static layers, then layer ns + c = the union of PIL's
 *     ImageDraw.polygon(fill=1) of the boxes with label c, at [x][y] (the transposed picture); labels outside [0, nd)
 *     draw no layer.
 *   aux (NULL iff aux_sel = 0): fp32 [b][ch][size][size] at [x][y], the channels of the LAST box in input order whose
 *     polygon covers the pixel, whatever its label, 0 where there is none; aux_sel: bit 0 visibility (1 channel), bit 1
 *     center_offset (2: float32(x) - centre in float64), bit 2 center_ohw (4: |front - centre|, |left - centre|, (front -
 *     centre) / (|front - centre| + 1e-6), float64 with IEEE division and square root, front / left the float32 means of
 *     corners 4, 7 and 0, 4), bit 3 height (1), in this order.
 *   flags: one int32, WRITTEN: the number of boxes whose rounded quad is of the family that is not drawn — two opposite
 *     vertices equal, the other two distinct from them and from each other, one of them more than one pixel (Chebyshev)
 *     from the repeated vertex; no rectangle rounds to such a quad.  Such a box draws nothing in masks and aux.
 *   workspace: at least dd_bev_map_workspace_bytes(total) bytes, 16-byte aligned, contents don't care before and after.
 * DD_ERR_BAD_ARG, before any runtime call: a NULL offsets / workspace / masks / flags, NULL stat with ns > 0, a NULL box
 * array with total > 0, aux NULL with aux_sel != 0 or the reverse, static_bits not 0 / 1, total < 0, non-positive b /
 * size / ns + nd, negative ns / nd, ns + nd > DD_BEV_MAP_MAX_LAYERS (one_hot_encode's limit), aux_sel outside [0, 15], a
 * scale or offset that is not finite, a misaligned array, workspace_bytes too small.  total > DD_BEV_MAP_MAX_BOXES,
 * size > DD_BEV_MAP_MAX_SIZE or b > 65535: DD_ERR_UNSUPPORTED; dd_bev_map_workspace_bytes returns -1 for such a total.
 * ------------------------------------------------------------------------- */
#define DD_BEV_MAP_MAX_LAYERS 30
#define DD_BEV_MAP_MAX_BOXES (1 << 20)
#define DD_BEV_MAP_MAX_SIZE 4096
int64_t dd_bev_map_workspace_bytes(int32_t total);
int dd_bev_map_layers(const void* stat, int32_t static_bits, const float* corners, const float* bottom_center,
                      const float* height, const float* visibility, const int64_t* labels, const int32_t* offsets,
                      int32_t total, int32_t b, int32_t size, int32_t ns, int32_t nd, int32_t aux_sel, double sx,
                      double ox, double sy, double oy, void* workspace, int64_t workspace_bytes, uint8_t* masks,
                      float* aux, int32_t* flags, dd_stream_t stream);

/* ------------------------------------------------------------------------- *
 * FGM loss mask (csrc/fgm_mask.hip, csrc/fgm_mask_core.h): `heatmap_gt` of the reference's collate_fn (magicdrive/dataset/
 * utils.py:530-559), i.e. create_heatmap_gt(for_mask, lidar2image, metas, resolution) (magicdrive/networks/utils.py:26-39
 * and :100-163: process_one_view_test, process_one_instance_test) followed by hd_crop (dataset/utils.py:348-353).
 * Two launches: dd_fgm_box_records (one wave per box: its 96-byte record into the workspace, the area by a wave
 * reduction) and dd_fgm_mask (pixel-major over the cropped output).  No atomics, nothing cleared, nothing allocated, no
 * host synchronisation.
 *   corners fp32 [views][m][points][3] (`for_mask["bboxes"]`, views = b * n), masks uint8 [views][m] (non-zero: the box
 *   counts), lidar2image fp32 [views][4][4] (torch.bmm(camera_intrinsics, lidar2camera)).  All device memory.
 *   Per box with mask set (utils.py:117-161): [x, y, z, 1] @ T.T in float64, every product and sum one IEEE operation,
 *     summed k = 0..3; points with z <= 0 dropped; z clipped to [1e-5, 1e5]; x / z * sx and y / z * sy (sx = W / 1600, sy =
 *     H / 900 as float64 quotients); truncated toward zero.  The polygon is the strict convex hull counter-clockwise in
 *     (x, y) (scipy's ConvexHull(...).vertices) where that has >= 3 vertices, else the surviving points in corner order
 *     (where ConvexHull raises); no point: nothing painted.  A pixel is painted where matplotlib's
 *     Polygon(...).contains_point(p, radius=0) holds: the even-odd rule over the closed ring's edges v0 -> v1 with f = (vy >=
 *     ty), an edge with f0 != f1 toggling iff ((v1y - ty) (v0x - v1x) >= (v1x - tx) (v0y - v1y)) == f1, in int64.  area =
 *     the painted pixels of the UNCROPPED width x height grid; weight = float32(1.0 - area / (width * height)), float64.
 *   out: fp32 [views][height_out][width_out]: per pixel the greatest weight among the boxes that paint it, 0 where none
 *     does (torch.stack(res).max(0)); pixel (ox, oy) is grid pixel (ox + (width - width_out) / 2, oy + height - height_out),
 *     hd_crop's window.  Every element is written.
 *   flags: one int32, WRITTEN: the number of masked boxes that are unsupported — a projected x, y or z of a corner that
 *     is not finite, or a surviving corner whose scaled coordinate is not finite or truncates beyond 2^25 in magnitude
 *     (where the reference's float64 products of the crossing test stop being exact and its integer cast is undefined;
 *     it takes z within ~1e-5 of the camera plane).  Such a box paints nothing.
 *   workspace: at least dd_fgm_workspace_bytes(views * m) bytes, 16-byte aligned, contents don't care before; after the
 *     call it holds the records (csrc/fgm_mask_core.h: ring, vertex count, flagged, weight, area, bounding box).
 * DD_ERR_BAD_ARG, before any runtime call: a NULL workspace / out / flags, a NULL input with m > 0, views <= 0, m < 0,
 * points outside [1, 8], width or height < 1, width * height > DD_FGM_MAX_PIXELS, an output larger than the grid or
 * smaller than 1, width - width_out odd, a scale that is not finite, a misaligned array, workspace_bytes too small.
 * views > 65535 or views * m > DD_FGM_MAX_BOXES: DD_ERR_UNSUPPORTED; dd_fgm_workspace_bytes returns -1 for such a total.
 *
 * dd_fgm_loss: the loss lines of runner/multiview_runner.py:501-507 — F.mse_loss(pred, target, reduction='none'), `loss *
 * heatmap_gt[0].unsqueeze(2)`, the two .mean()s and their sum — as one read of each input:
 *     loss[0] = sum((p - t)^2 * (1 + heat)) / N  in fp32,   N = views * channels * pixels,
 * and, where grad is not NULL, grad = 2 (p - t) (1 + heat) / N in pred's type, in the same pass ((p - t), (1 + heat), its
 * product with float32(2 / N), the product of the two: four fp32 roundings and the output cast).
 *   pred, target, grad: [views][channels][pixels] of pred_dtype (DD_F16 / DD_BF16 / DD_F32); heat fp32 [views][pixels] or NULL
 *   (the plain mean); loss: one fp32.
 *   Reduction, fixed: groups = clamp(ceil(N / DD_FGM_LOSS_PER_GROUP), 1, DD_FGM_LOSS_MAX_GROUPS) workgroups of 256
 *   lanes; lane l of group g sums elements (g * 256 + l) + k * groups * 256 in rising k, the 64 lanes of a wave by a
 *   butterfly, the four waves in order; one workgroup then sums the partials the same way and divides by float32(N).  The
 *   same inputs give the same bits.  workspace: dd_fgm_loss_workspace_bytes(N) bytes (the partials), 4-byte aligned.
 * DD_ERR_BAD_ARG: a NULL pred / target / loss / workspace, a non-positive extent, an unknown pred_dtype, a misaligned array,
 * workspace_bytes too small.  N > DD_FGM_LOSS_MAX_COUNT: DD_ERR_UNSUPPORTED (dd_fgm_loss_workspace_bytes: -1).
 * ------------------------------------------------------------------------- */
#define DD_FGM_MAX_BOXES (1 << 20)
#define DD_FGM_MAX_PIXELS (1 << 20)
#define DD_FGM_LOSS_PER_GROUP 1024
#define DD_FGM_LOSS_MAX_GROUPS 1024
#define DD_FGM_LOSS_MAX_COUNT 2147483647
int64_t dd_fgm_workspace_bytes(int32_t total);
int dd_fgm_mask(const float* corners, const uint8_t* masks, const float* lidar2image, int32_t views, int32_t m,
                int32_t points, int32_t width, int32_t height, int32_t width_out, int32_t height_out, double sx, double sy,
                void* workspace, int64_t workspace_bytes, float* out, int32_t* flags, dd_stream_t stream);
int64_t dd_fgm_loss_workspace_bytes(int64_t count);
int dd_fgm_loss(const void* pred, const void* target, const float* heat, void* grad, float* loss, void* workspace,
                int64_t workspace_bytes, int64_t views, int32_t channels, int32_t pixels, int32_t pred_dtype,
                dd_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Fused optimizer step (csrc/adamw.hip, csrc/adamw_core.h): the last three lines of the reference's training step
 * (runner/multiview_runner.py:512-521) — accelerator.clip_grad_norm_, torch.optim.AdamW.step() under a GradScaler
 * (mixed_precision: fp16) and the scheduler's step — in three launches with nothing read back: the step count, the
 * learning rate and the skip decision live in device memory, so a step can be captured into a graph.
 *   rows: n_rows descriptors in device memory, one per parameter tensor.  p, g, m, v: fp32, 4-byte aligned; g NULL: the
 *     row is left entirely alone (a parameter without a gradient); shadow: NULL, or numel elements of shadow_dtype (DD_F16 /
 *     DD_BF16), 2-byte aligned, rewritten with the new p; numel >= 0.
 *   chunks: n_chunks pairs (row, chunk of the row) of int32 in device memory: chunk c of a row covers its elements
 *     [c * DD_ADAMW_CHUNK, min((c + 1) * DD_ADAMW_CHUNK, numel)).  Every element of every row with numel > 0 is covered
 *     once; a pair that names no row or lies past a row's end is skipped.
 *   state: the block below, device memory, 8-byte aligned.  lr_table: lr_len >= 1 fp32 in device memory, indexed by the
 *     number of steps taken before this one, the last entry for every step past the end.
 *   grad_scale: NULL (1), or one fp32 in device memory; inv_scale = fp32(1 / float64(grad_scale)).  found_inf_in: NULL,
 *     or one fp32 in device memory whose non-zero value skips the step (GradScaler's `optimizer.found_inf`).
 *   max_norm < 0: no clipping (clip_coef = 1).
 * Launch 1 (a workgroup per chunk): gu = fl32(g * inv_scale) per element; the workgroup's float64 sum of gu^2 (an fp32
 *   square is exact in float64) in a fixed order — lane l sums elements 4 (256 i + l) + c of the chunk in rising i, c; the
 *   64 lanes of a wave by a butterfly; waves 0..3 in order — into partials[chunk], and whether a gu was not finite.
 * Launch 2 (one workgroup): the partials summed the same way (lane l: partials l + 256 i), then, in float64, each result
 *   rounded to fp32 once: grad_norm = sqrt(sum), clip_coef = min(max_norm / (grad_norm + 1e-6), 1)
 *   (torch.nn.utils.clip_grad_norm_); found_inf = a non-finite gu or a non-zero found_inf_in.  Skipped step: skipped += 1 and
 *   nothing else.  Taken step: step += 1, beta1_pow *= beta1, beta2_pow *= beta2, lr = lr_table[min(step - 1, lr_len - 1)],
 *   decay = 1 - lr wd, w1 = 1 - beta1, b2 = beta2, w2 = 1 - beta2, step_size = lr / (1 - beta1_pow),
 *   bc2_sqrt = sqrt(1 - beta2_pow), eps.
 * Launch 3 (a workgroup per chunk; returns at once when found_inf is set): csrc/adamw_core.h's update, every operation
 *   one IEEE fp32 operation, then the shadow.  16-byte accesses where p, g, m and v of the row share their offset in a
 *   16-byte line (a scalar head of up to three elements and a scalar tail), dword accesses otherwise.  The gradients
 *   are not rewritten: they keep their scaled, unclipped values.
 * The same inputs give the same bits, wherever the tensors lie.  launches: bit 0 / 1 / 2 = issue launch 1 / 2 / 3
 * (DD_ADAMW_ALL for a step; single launches are for timing).  workspace: dd_adamw_workspace_bytes(n_chunks) bytes,
 * 8-byte aligned: the partials and the non-finite marks.
 * DD_ERR_BAD_ARG, before any runtime call: a NULL rows / chunks with n_rows / n_chunks > 0, a NULL state / lr_table /
 * workspace, negative counts, lr_len < 1, betas outside [0, 1), eps or weight_decay negative or not finite, a NaN max_norm,
 * an unknown shadow_dtype, launches outside [1, 7], a misaligned pointer, workspace_bytes too small.
 * ------------------------------------------------------------------------- */
#ifndef DD_ADAMW_CHUNK                            /* another size only in an A/B build (tools/adamw_timing.py) */
#define DD_ADAMW_CHUNK 8192
#endif
#define DD_ADAMW_ALL 7
typedef struct dd_adamw_row {
  void* p;
  const void* g;
  void* m;
  void* v;
  void* shadow;
  int64_t numel;
} dd_adamw_row;                                   /* 48 bytes */
typedef struct dd_adamw_state {
  int64_t step;                                   /* steps taken */
  double beta1_pow, beta2_pow;                    /* beta^step, advanced by one multiplication per taken step */
  float grad_norm, clip_coef;                     /* of the last call, taken or not */
  int32_t found_inf, reserved0;                   /* 1: the last call was skipped */
  int64_t skipped;                                /* calls skipped */
  float lr, decay, w1, b2, w2, step_size, bc2_sqrt, eps;   /* of the last taken step */
  float inv_scale, reserved1[3];                  /* of the last call */
} dd_adamw_state;                                 /* 96 bytes */
int64_t dd_adamw_workspace_bytes(int64_t n_chunks);
int dd_adamw_step(const dd_adamw_row* rows, int32_t n_rows, const int32_t* chunks, int64_t n_chunks,
                  dd_adamw_state* state, const float* lr_table, int32_t lr_len, const float* grad_scale,
                  const float* found_inf_in, double beta1, double beta2, double eps, double weight_decay, double max_norm,
                  int32_t shadow_dtype, void* workspace, int64_t workspace_bytes, int32_t launches, dd_stream_t stream);

/* ------------------------------------------------------------------------- *
 * CLIP text encoder (csrc/clip.hip): the SD-v1.5 `text_encoder` (transformers.CLIPTextModel) that the reference calls at
 * runner/base_runner.py:119,511-514, runner/multiview_runner.py:145,427-428 (`text_encoder(ids)[0]`), through diffusers'
 * _encode_prompt at pipeline/pipeline_bev_controlnet.py:273 and at networks/bbox_embedder.py:133-145
 * (`text_encoder(ids).pooler_output[0]`).  Its Linear / LayerNorm layers run on dd_gemm / dd_layernorm; these two entry
 * points are the rest.
 * ------------------------------------------------------------------------- */
/* CLIPTextEmbeddings + the pooling position of CLIPTextTransformer, one launch:
 *   out[b * l + t, :] = T( float(tok[clamp(ids[b, t], 0, vocab - 1)]) + float(pos[t]) )      (one rounding)
 *   pool_index[b]     = eos_token_id == 2 ? first position of the largest id of sequence b   (ids[b].argmax())
 *                                         : first position with ids[b, t] == eos_token_id, 0 when there is none
 * — the row of sequence b that pooler_output reads, left in device memory so that pooling needs no host synchronisation.
 * ids: int64 [batch * l] (device); tok [vocab][c], pos [>= l][c], out [batch * l][c] in `dtype`; pool_index int32 [batch].
 * c % 8 == 0, tok / pos / out 16-byte aligned (rows move as 16-byte vectors), else DD_ERR_BAD_ARG.  Ids outside
 * [0, vocab) are clamped for the gather (nothing is read outside the table); the pooling rule sees them as they are. */
int dd_clip_embed(const int64_t* ids, const void* tok, const void* pos, void* out, int32_t* pool_index,
                  int32_t batch, int32_t l, int32_t c, int32_t vocab, int32_t eos_token_id, int32_t dtype,
                  dd_stream_t stream);

/* Causal self-attention (CLIPAttention with the causal mask only — SD-v1.5's config has no use_attention_mask, padding
 * tokens attend like any other position):
 *   O[b, i, h, :] = softmax_{j <= i}( scale * Q[b,i,h,:].K[b,j,h,:] ) V[b,j,h,:]
 * Q / K / V / O: element (b, i, h, d) at  base + b * batch_stride + i * ld + h * head_dim + d  (elements), so Q, K, V may
 * be column slices of one fused [batch * l][3 * heads * head_dim] projection.  head_dim == 64 and
 * 1 <= l <= DD_CAUSAL_ATTN_MAX_L, else DD_ERR_UNSUPPORTED; NULL / misaligned (16 bytes; ld and batch strides multiples of
 * 8) / non-positive arguments are DD_ERR_BAD_ARG; both are decided before anything is launched.  Numerics as dd_attention:
 * fp32 scores and softmax (exp2 with scale * log2 e), probabilities rounded to `dtype` before P.V, fp32 accumulation, one
 * rounding at the store; a masked key's probability is exactly 0. */
#define DD_CAUSAL_ATTN_MAX_L 128
int dd_causal_attention(const void* q, const void* k, const void* v, void* o, int64_t ldq, int64_t ldk, int64_t ldv,
                        int64_t ldo, int64_t q_batch_stride, int64_t k_batch_stride, int64_t v_batch_stride,
                        int64_t o_batch_stride, int32_t batch, int32_t l, int32_t heads, int32_t head_dim, float scale,
                        int32_t dtype, dd_stream_t stream);

/* conv3x3 / pad 1 / stride 1 or 2 for THIN channel counts on large NHWC images — the first layers of
 * ControlNetConditioningEmbedding (networks/map_embedder.py:79-113: 3 -> 16 -> 16 -> 32 -> 32 channels on 224x400 ..
 * 112x200).  x (m, hin, win, cin), w [cout][9*cin] (k = tap * cin + channel), bias [cout] or NULL,
 * y (m, hout, wout, cout) with hout = (hin - 1) / stride + 1; optional SiLU.  cin in {8, 16, 32} (3 input channels are
 * zero-padded to 8 by the caller), cout in {16, 32}; other combinations: DD_ERR_UNSUPPORTED. */
int dd_conv3x3_thin(const void* x, const void* w, const void* bias, void* y, int32_t m, int32_t hin, int32_t win,
                    int32_t cin, int32_t cout, int32_t stride, int32_t silu, int32_t dtype, dd_stream_t stream);

/* Classifier-free guidance + DDIM (eta = 0) update, fused:
 *   eps = eps_u + g (eps_c - eps_u);  x0 = (x - sqrt(1-a_t) eps)/sqrt(a_t);
 *   x' = sqrt(a_prev) x0 + sqrt(1-a_prev) eps
 * (pipeline/pipeline_bev_controlnet.py:487-499 with diffusers DDIMScheduler.step).
 * eps: [2][n] (uncond first, :489), x / x_out: [n] in dtype T; coef: device fp32[4] =
 * {sqrt(a_t), sqrt(1-a_t), sqrt(a_prev), sqrt(1-a_prev)} read at kernel time so the
 * launch can be replayed from a graph. x_dup: optional second copy of x' (the CFG
 * duplicate `torch.cat([latents]*2)`, :384-386) or NULL. */
int dd_cfg_ddim_step(const void* eps, const void* x, void* x_out, void* x_dup,
                     const float* coef, float guidance, int64_t n,
                     int32_t dtype, dd_stream_t stream);

/* Classifier-free guidance + UniPC (bh2, order <= 2, x0-prediction) step, fused — the scheduler the
 * reference's test pipeline installs (misc/test_utils.py:161-162) and steps at
 * pipeline/pipeline_bev_controlnet.py:487-499:
 *   eps = eps_u + g (eps_c - eps_u);  x0 = a_x x + a_e eps
 *   x_c = use_c ? c_l last + c_1 m1 + c_2 m2 + c_0 x0 : x        (corrector)
 *   x'  = p_x x_c + p_0 x0 + p_1 m1                              (predictor)
 *   last <- x_c;  m2 <- m1;  m1 <- x0
 * eps: [2][n] (uncond first), x / x_out / x_dup: [n] in dtype T; last, m1, m2: [n] fp32 history owned by
 * the caller (any values on the first step: use_c = 0, p_1 = 0 there); coef: device fp32[10] =
 * {a_x, a_e, use_c, c_l, c_1, c_2, c_0, p_x, p_0, p_1} read at kernel time (graph replay). */
int dd_cfg_unipc_step(const void* eps, const void* x, void* x_out, void* x_dup, float* last, float* m1,
                      float* m2, const float* coef, float guidance, int64_t n, int32_t dtype,
                      dd_stream_t stream);

/* Given-view sampling (pipeline/pipeline_bev_controlnet_given_view.py: some views are held to clean latents c
 * the caller supplies, the sampler generates the others).  add_noise(c, n0, t) = sqrt(acp[t]) c + sqrt(1-acp[t]) n0
 * (scheduler.add_noise) is evaluated in fp32 on fp32 c and rounded once to the storage type T.
 * The views are the n / view_elems consecutive blocks of view_elems elements (the view-instances of x);
 * given: device bytes, one per view-instance, non-zero for a given view; clean: fp32 [n] (c of the given views, any
 * values elsewhere); noise0: [n] in T, the latents at loop entry (original_noise, :264).
 *
 * dd_cfg_ddim_step_given / dd_cfg_unipc_step_given: dd_cfg_ddim_step / dd_cfg_unipc_step (same arguments, same
 * arithmetic, bit-identical results on views whose byte is 0) plus, on the given views:
 *   mode 1 (conditional_latents_change_every_input = True, :283-295): the step stores add_noise(c, n0, t_next) in
 *     x_out and x_dup instead of the update — the overwrite at the top of the NEXT step, fused into this step's
 *     store.  gcoef: device fp32[3] = {sqrt(acp[t_next]), sqrt(1-acp[t_next]), renoise} read at kernel time (graph
 *     replay); renoise = 0 on the last step, which stores the update (nothing is overwritten after the loop).  The
 *     UniPC history is advanced from the step's input x as on every other view.
 *   mode 2 (change_every_input = False, :380-389): the guided noise is replaced by n0 before the update (gcoef unused,
 *     but must be a valid pointer).
 * Grid: one blockIdx.y per view-instance (n / view_elems <= 65535, view_elems < 2^31, else DD_ERR_UNSUPPORTED).
 * DD_ERR_BAD_ARG: a NULL pointer (x_dup may be NULL), view_elems <= 0 or not dividing n, mode not 1 or 2, dtype. */
int dd_cfg_ddim_step_given(const void* eps, const void* x, void* x_out, void* x_dup, const float* coef,
                           float guidance, const uint8_t* given, const float* clean, const void* noise0,
                           const float* gcoef, int32_t mode, int64_t n, int64_t view_elems, int32_t dtype,
                           dd_stream_t stream);
int dd_cfg_unipc_step_given(const void* eps, const void* x, void* x_out, void* x_dup, float* last, float* m1,
                            float* m2, const float* coef, float guidance, const uint8_t* given, const float* clean,
                            const void* noise0, const float* gcoef, int32_t mode, int64_t n, int64_t view_elems,
                            int32_t dtype, dd_stream_t stream);

/* The pre-loop noising of the given views (:265-276 in mode 2; the first step's overwrite :283-295 in mode 1):
 * x[v] = x_dup[v] = add_noise(c, n0, timesteps[0]) on the given views, other views untouched; sqrt_acp / sqrt_1m_acp
 * are sqrt(acp[timesteps[0]]) and sqrt(1 - acp[timesteps[0]]).  x_dup may be NULL.  Once per sample, before step 0. */
int dd_given_views_noise(void* x, void* x_dup, const uint8_t* given, const float* clean, const void* noise0,
                         float sqrt_acp, float sqrt_1m_acp, int64_t n, int64_t view_elems, int32_t dtype,
                         dd_stream_t stream);

/* ------------------------------------------------------------------------- *
 * EXTENSION (BASELINE configs[4]: "fp8 weights (CDNA4 fp8 MFMA)"; no reference semantics — README.md:47-49 is prose):
 * W8A8 projection on the fp8 matrix path.
 *   dd_rowquant_fp8: y = gamma ? LayerNorm(x) (dd_layernorm's arithmetic, rounded to the storage type) : x;
 *       scale[r] = max(max_c |y[r, c]| / 448, 2^-126) (1 for a zero row; the floor keeps 1 / scale finite for every finite
 *       nonzero row and changes none above 448 * 2^-126);  q[r, c] = e4m3fn(clamp(y[r, c] * (1 / scale[r]), +-448)) in IEEE
 *       fp32, round to nearest even;  q rows have pitch ldq bytes (multiple of 128, ldq - c < 512, bytes c .. ldq - 1
 *       zero) — the LayerNorm launch of norm1 / norm2 / norm4 (networks/blocks.py:150-222) doubles as the activation
 *       quantiser.  A row of y that holds a NaN or an Inf gets scale[r] = NaN (its bytes are finite codes): dd_gemm8
 *       returns such a row as NaN in every column, as LayerNorm followed by the 16-bit GEMM would.
 *   dd_gemm8: out[r, n] = a_scale[r] * w_scale[n] * sum_k A8[r, k] W8[n, k] + bias[n] + res[r, n], fp32 accumulation in
 *       v_mfma_scale_f32_16x16x128_f8f6f4 (unit block scales), A8 [rows][lda] / W8 [n][ldw] OCP e4m3fn bytes whose rows are
 *       zero padded to k_padded (multiple of 128); output in `dtype`, row-major or head-major planes as dd_gemm's
 *       out_headmajor_d (the fused Q|K|V projection of attn1 / attn4, to_q of attn2), or with the GEGLU gate.
 * ------------------------------------------------------------------------- */
int dd_rowquant_fp8(const void* x, const void* gamma, const void* beta, void* q, float* scale, int64_t rows, int32_t c,
                    int64_t ldq, float eps, int32_t dtype, dd_stream_t stream);

typedef struct dd_gemm8_desc {
  const void* a; const float* a_scale; int64_t lda;
  const void* w; const float* w_scale; int64_t ldw;
  const void* bias; const void* res; int64_t ldres;
  void* out; int64_t ldc;
  int32_t rows, n, k_padded;
  int32_t dtype;                          /* of bias / res / out */
  int32_t out_headmajor_d, hm_scaled_planes; float hm_scale;
  int32_t geglu;                          /* 1: W8 / w_scale / bias have 2n rows (h | g); out[r, c] = h * gelu_erf(g) — the
                                             GEGLU projection of FeedForward behind norm3 (diffusers FeedForward / GEGLU) */
} dd_gemm8_desc;

int dd_gemm8(const dd_gemm8_desc* d, dd_stream_t stream);

/* Measurement aid (not on the data path): one wave busy-waits `ticks_100mhz` ticks of the constant-rate 100 MHz
 * s_memrealtime counter and stores its first and last counter reading in stamps[0], stamps[1] (device memory).
 * bench.py brackets it with HIP events to learn what an event pair adds to a kernel of KNOWN device-side duration. */
int dd_probe_spin(uint64_t* stamps, uint32_t ticks_100mhz, dd_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DUALDIFF_HIP_H */
