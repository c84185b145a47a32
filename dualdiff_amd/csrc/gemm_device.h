// MFMA GEMM / implicit-GEMM 3x3 convolution with fused epilogue for gfx950.
//
//   out[r, n] (op)= alpha * (sum_k A[r,k] W[n,k] + bias[n] + rowvec[r/rpi, n]) + res[r, n]
//
// Design (MI355X-first, not a CUDA tiling):
//  * wave64, v_mfma_f32_16x16x32_{f16,bf16}; fp32 accumulate.
//  * The MFMA "A" operand is the WEIGHT tile and the "B" operand the ACTIVATION tile, so
//    the accumulator of a lane is a run of consecutive output channels of one row.  The
//    weight rows of a wave are permuted on the global->LDS load so that each lane ends up
//    with 4*TN *consecutive* channels -> 16-byte NHWC stores, 128 B contiguous per row.
//  * Both operands are K-contiguous ([rows][K] activations, [N][K] weights), staged as
//    [row][64] tiles in LDS with a 16-byte-chunk XOR swizzle (conflict-free ds_read_b128).
//  * Register-staged software pipeline: global loads of K-tile t+1 are issued before the
//    MFMAs of tile t and written to the other LDS buffer afterwards (one barrier / K-step).
//  * conv mode gathers the im2col row on the fly (NHWC: one tap = one contiguous Cin run);
//    padding, stride 2 and the nearest-neighbour upsample are folded into the gather.
//  * XCD-aware tile order: consecutive tiles that share an activation panel are mapped to
//    the same XCD (private L2).
//  * split-K for the deep, weight-bound levels (336..1092 rows x K up to 23040).
//
// This header: the device helpers every kernel family shares (epilogues, LDS-DMA primitives).  The families live in
// gemm1.hip, gemm2_kernel.h (+ gemm23 / gemm2_geglu / gemm2_conv / gemm2_upfold.hip), gemm3_kernel.h, gemm4.hip and conv3s.hip; the tile
// table and the dispatch in gemm_tiles.h; the planner, the split-K reduce and the C entry points in gemm.hip.
#pragma once
#include "dd_common.h"
#include "dd_debug.h"
#include "gemm_tiles.h"
#include <type_traits>

using namespace ddg;

namespace {

// n / d for 0 <= n < 2^22 (host-checked: rows) and the host-side inv = 1.0f / d: (n + 0.5) * inv is never within
// float rounding of an integer boundary there (error <= 2^-23 * (n + 0.5) / d < 0.5 / d), so truncation gives the exact quotient — 3 VALU
// instructions instead of the ~35 of a 32-bit integer division (the table-building prologues divide by the
// image size and width once per tile row: a third of the direct conv kernel's VALU instructions).
__device__ __forceinline__ int dd_fdiv(int n, float inv) { return (int)(((float)n + 0.5f) * inv); }


template <typename T>
__device__ __forceinline__ void store8(const GemmParams& p, int64_t row, int col, float (&v)[8]) {
  if (p.hm_d) {                            // one [rows][D] plane per head; the Q planes carry the softmax scale
    const int plane = col / p.hm_d;
    if (plane < p.hm_planes) {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] *= p.hm_scale;
    }
    dd_st16(reinterpret_cast<T*>(p.out) + ((int64_t)plane * p.rows + row) * p.hm_d + (col - plane * p.hm_d),
            dd_pack8<T>(v));
    return;
  }
  if (p.out_f32) {
    float* o = reinterpret_cast<float*>(p.out) + row * p.ldc + col;
    *reinterpret_cast<f32x4*>(o) = f32x4{v[0], v[1], v[2], v[3]};
    *reinterpret_cast<f32x4*>(o + 4) = f32x4{v[4], v[5], v[6], v[7]};
  } else {
    dd_st16(reinterpret_cast<T*>(p.out) + row * p.ldc + col, dd_pack8<T>(v));
  }
}

// --- epilogue on 8 consecutive output channels of one row --------------------------------
template <typename T>
__device__ __forceinline__ void epilogue_store8(const GemmParams& p, int row, int col, float (&v)[8]) {
  if (p.bias) {
    float b[8];
    dd_unpack8<T>(dd_ld16(reinterpret_cast<const T*>(p.bias) + col), b);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] += b[i];
  }
  if (p.rowvec) {
    const int inst = dd_fdiv(row, p.inv_rpi);
    float b[8];
    dd_unpack8<T>(dd_ld16(reinterpret_cast<const T*>(p.rowvec) + (int64_t)inst * p.ld_rowvec + col), b);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] += b[i];
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] *= p.alpha;
  if (p.res) {
    float b[8];
    dd_unpack8<T>(dd_ld16(reinterpret_cast<const T*>(p.res) + (int64_t)row * p.ldres + col), b);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] += b[i];
  }
  if (p.act == DD_EPI_SILU) {
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = dd_silu_f(v[i]);
  }
  if (p.accumulate) {
    float b[8];
    dd_unpack8<T>(dd_ld16(reinterpret_cast<T*>(p.out) + (int64_t)row * p.ldc + col), b);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] += b[i];
  }
  store8<T>(p, row, col, v);
}

// XCD-aware bijective remap of a 1-D block id (guide T1): blocks b, b+8, ... share an XCD;
// give each XCD a contiguous range of tiles.
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
  const int xcd = bid & 7;
  const int q = nwg >> 3, r = nwg & 7;
  const int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  return base + (bid >> 3);
}

// ---- accumulator tile -> global (shared by both kernel families) ---------------------------
// acc[tn][tm][reg]: output row = tile row tm*16 + (lane & 15),
//                   output col = q*(4*TN) + tn*4 + reg  (q = lane >> 4)   [non-GEGLU]
// Every global read of the epilogue (bias, time-embedding vector, residual, accumulate target) is
// issued before the stores of its row batch: `out` may alias `res`, so a load placed after a store could
// not be hoisted by the compiler and the tile would pay one memory round trip per 8-column group.
// MAPPED (the folded-upsample conv): tile row tm*16 + (lane & 15) of the wave goes to output row rowmap[tm]; a row that is
// not stored has rowmap[tm] >= row_end.
template <typename T, int TM, int TN, bool GEGLU, bool MAPPED = false>
__device__ __forceinline__ void store_tile(const GemmParams& p, f32x4 (&acc)[TN][TM], int block_m0,
                                           int block_n0, int wave_m, int wave_n, int lane, int row_end,
                                           const float* ln_mean = nullptr, const float* ln_rstd = nullptr,
                                           const int* rowmap = nullptr) {
  static_assert(!(MAPPED && GEGLU), "no mapped GEGLU epilogue");
  const int q = lane >> 4;
  const int c = lane & 15;
  const int row0 = block_m0 + wave_m * (TM * 16) + c;
  if constexpr (GEGLU) {
    constexpr int TH = TN / 2;
    constexpr int NG = TH / 2;
    const int col0 = block_n0 + wave_n * (TH * 16) + q * (4 * TH);
    u32x4 bh[NG], bg[NG];
    f32x4 lsh[NG][2], lsg[NG][2], lbh[NG][2], lbg[NG][2];     // LayerNorm fold: column sums / folded bias
    if (ln_mean) {
#pragma unroll
      for (int g8 = 0; g8 < NG; ++g8) {
        const int col = min(col0 + g8 * 8, p.n - 8);
#pragma unroll
        for (int h2 = 0; h2 < 2; ++h2) {
          lsh[g8][h2] = *reinterpret_cast<const f32x4*>(p.ln_colsum + col + 4 * h2);
          lsg[g8][h2] = *reinterpret_cast<const f32x4*>(p.ln_colsum + p.n + col + 4 * h2);
          lbh[g8][h2] = *reinterpret_cast<const f32x4*>(p.ln_bias + col + 4 * h2);
          lbg[g8][h2] = *reinterpret_cast<const f32x4*>(p.ln_bias + p.n + col + 4 * h2);
        }
      }
    }
    if (p.bias) {
#pragma unroll
      for (int g8 = 0; g8 < NG; ++g8) {
        const int col = min(col0 + g8 * 8, p.n - 8);
        bh[g8] = dd_ld16(reinterpret_cast<const T*>(p.bias) + col);
        bg[g8] = dd_ld16(reinterpret_cast<const T*>(p.bias) + p.n + col);
      }
    }
#pragma unroll
    for (int tm = 0; tm < TM; ++tm) {
      const int row = row0 + tm * 16;
      if (row >= row_end) continue;
#pragma unroll
      for (int g8 = 0; g8 < NG; ++g8) {
        const int col = col0 + g8 * 8;
        if (col >= p.n) continue;
        float h[8], g[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          h[e] = acc[g8 * 2 + (e >> 2)][tm][e & 3];
          g[e] = acc[TH + g8 * 2 + (e >> 2)][tm][e & 3];
        }
        if (ln_mean) {
          const int lr = wave_m * (TM * 16) + tm * 16 + c;
          const float mu = ln_mean[lr], rs = ln_rstd[lr];
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            h[e] = rs * (h[e] - mu * lsh[g8][e >> 2][e & 3]) + lbh[g8][e >> 2][e & 3];
            g[e] = rs * (g[e] - mu * lsg[g8][e >> 2][e & 3]) + lbg[g8][e >> 2][e & 3];
          }
        }
        if (p.bias) {
          float b[8];
          dd_unpack8<T>(bh[g8], b);
#pragma unroll
          for (int e = 0; e < 8; ++e) h[e] += b[e];
          dd_unpack8<T>(bg[g8], b);
#pragma unroll
          for (int e = 0; e < 8; ++e) g[e] += b[e];
        }
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = dd_geglu_f(h[e], g[e]);
        dd_st16(reinterpret_cast<T*>(p.out) + (int64_t)row * p.ldc + col, dd_pack8<T>(v));
      }
    }
  } else {
    constexpr int NG = TN / 2;
    const int col0 = block_n0 + wave_n * (TN * 16) + q * (4 * TN);
    if (p.partial) {                       // split-K slab: fp32 stores; dd_splitk_reduce_kernel (a second launch) adds the
      // slabs and runs the epilogue.  (An IN-LAUNCH ordered reduction by the last-arriving K-slice — write-through slabs,
      // agent-scope ticket, sc1 loads — was built in round 3, bit-identical, 3-80 % slower on the step's 23 split-K
      // shapes, and removed in round 5: profiles/r03_splitk_inkernel_ab.txt.)
#pragma unroll
      for (int tm = 0; tm < TM; ++tm) {
        const int row = MAPPED ? rowmap[tm] : row0 + tm * 16;
        if (row >= row_end) continue;
#pragma unroll
        for (int g8 = 0; g8 < NG; ++g8) {
          const int col = col0 + g8 * 8;
          if (col >= p.n) continue;
          float* dst = p.partial + ((int64_t)blockIdx.z * p.rows + row) * p.n + col;
          *reinterpret_cast<f32x4*>(dst) = acc[g8 * 2][tm];
          *reinterpret_cast<f32x4*>(dst + 4) = acc[g8 * 2 + 1][tm];
        }
      }
      return;
    }
    // Rows are handled in (at most) two batches: per batch, phase 1 issues ALL its loads (clamped
    // addresses, nothing predicated), phase 2 does the arithmetic and the stores.  One batch would
    // keep TM*TN/2*3 16-B vectors live next to the accumulators (128x128 tile: > 256 VGPRs).
    constexpr int TMB = (TM >= 4 && TM % 2 == 0) ? TM / 2 : TM;      // batches must tile TM exactly
    u32x4 rb[NG];
    int colc[NG];
#pragma unroll
    for (int g8 = 0; g8 < NG; ++g8) colc[g8] = min(col0 + g8 * 8, p.n - 8);
    if (p.bias) {
#pragma unroll
      for (int g8 = 0; g8 < NG; ++g8) rb[g8] = dd_ld16(reinterpret_cast<const T*>(p.bias) + colc[g8]);
    }
    f32x4 lcs[NG][2], lcb[NG][2];                        // LayerNorm fold: column sums / folded bias
    if (ln_mean) {
#pragma unroll
      for (int g8 = 0; g8 < NG; ++g8)
#pragma unroll
        for (int h2 = 0; h2 < 2; ++h2) {
          lcs[g8][h2] = *reinterpret_cast<const f32x4*>(p.ln_colsum + colc[g8] + 4 * h2);
          lcb[g8][h2] = *reinterpret_cast<const f32x4*>(p.ln_bias + colc[g8] + 4 * h2);
        }
    }
#pragma unroll
    for (int tb = 0; tb < TM; tb += TMB) {
      u32x4 rv[TMB][NG], rr[TMB][NG], ra[TMB][NG];
#pragma unroll
      for (int t2 = 0; t2 < TMB; ++t2) {
        const int rowc = min(MAPPED ? rowmap[tb + t2] : row0 + (tb + t2) * 16, p.rows - 1);
        if (p.rowvec) {
          const int inst = dd_fdiv(rowc, p.inv_rpi);
#pragma unroll
          for (int g8 = 0; g8 < NG; ++g8)
            rv[t2][g8] = dd_ld16(reinterpret_cast<const T*>(p.rowvec) + (int64_t)inst * p.ld_rowvec + colc[g8]);
        }
        if (p.res) {
#pragma unroll
          for (int g8 = 0; g8 < NG; ++g8)
            rr[t2][g8] = dd_ld16(reinterpret_cast<const T*>(p.res) + (int64_t)rowc * p.ldres + colc[g8]);
        }
        if (p.accumulate) {
#pragma unroll
          for (int g8 = 0; g8 < NG; ++g8)
            ra[t2][g8] = dd_ld16(reinterpret_cast<const T*>(p.out) + (int64_t)rowc * p.ldc + colc[g8]);
        }
      }
      // arithmetic in the reference's order (bias, time vector, alpha, residual, act, accumulate) + stores
#pragma unroll
      for (int t2 = 0; t2 < TMB; ++t2) {
        const int tm = tb + t2;
        const int row = MAPPED ? rowmap[tm] : row0 + tm * 16;
        float st_s = 0.f, st_q = 0.f;                      // row statistics of this lane's columns
        if (row < row_end) {
#pragma unroll
        for (int g8 = 0; g8 < NG; ++g8) {
          const int col = col0 + g8 * 8;
          if (col >= p.n) continue;
          float v[8], b[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = acc[g8 * 2 + (e >> 2)][tm][e & 3];
          if (ln_mean) {
            const int lr = wave_m * (TM * 16) + tm * 16 + c;
            const float mu = ln_mean[lr], rs = ln_rstd[lr];
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = rs * (v[e] - mu * lcs[g8][e >> 2][e & 3]) + lcb[g8][e >> 2][e & 3];
          }
          if (p.bias) {
            dd_unpack8<T>(rb[g8], b);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] += b[e];
          }
          if (p.rowvec) {
            dd_unpack8<T>(rv[t2][g8], b);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] += b[e];
          }
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] *= p.alpha;
          if (p.res) {
            dd_unpack8<T>(rr[t2][g8], b);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] += b[e];
          }
          if (p.act == DD_EPI_SILU) {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = dd_silu_f(v[e]);
          }
          if (p.accumulate) {
            dd_unpack8<T>(ra[t2][g8], b);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] += b[e];
          }
          store8<T>(p, row, col, v);
          if (p.stat_out) {
#pragma unroll
            for (int e = 0; e < 8; ++e) { st_s += v[e]; st_q += v[e] * v[e]; }
          }
        }
        }
        if constexpr (TN == 2 || TN == 4) {
          if (p.stat_out) {              // uniform: every lane of the wave takes part in the shuffles
            // a lane holds 4*TN columns of its row; 32-column groups are 4 (TN = 2) or 2 (TN = 4) lanes q
            st_s += __shfl_xor(st_s, 16, 64);  st_q += __shfl_xor(st_q, 16, 64);
            if (TN == 2) { st_s += __shfl_xor(st_s, 32, 64);  st_q += __shfl_xor(st_q, 32, 64); }
            const int gcol = block_n0 + wave_n * (TN * 16) + (TN == 2 ? 0 : (q >> 1) * 32);
            const bool writer = TN == 2 ? q == 0 : (q & 1) == 0;
            if (writer && row < row_end && gcol < p.n) {
              float* dst = p.stat_out + ((int64_t)row * (p.n >> 5) + (gcol >> 5)) * 2;
              dst[0] = st_s;
              dst[1] = st_q;
            }
          }
        }
      }
    }
  }
}

// ---- epilogue of the 80 x 320 tile that ALSO emits LayerNorm(out) ---------------------------------------------
// A workgroup of 10 waves (1 x 10, TM = 5, TN = 2) owns 80 WHOLE rows of a 320-wide output: after bias / alpha /
// residual it rounds the row to T (what the next layer reads), stores it, and normalises it right there — two-pass
// fp32 statistics over the rounded values (the arithmetic of dd_layernorm), partial sums of the 10 waves combined
// through LDS in a fixed order (bit-reproducible) — writing LayerNorm(out) as a second tensor.  The producer of
// the residual stream thereby hands the next sub-layer its normalised input: no LayerNorm launch, no re-read of
// the stream (norm1 / norm2 / norm3 / norm4 of the 28x50 level, blocks.py:150-236).
template <typename T>
__device__ __forceinline__ void store_tile_ln(const GemmParams& p, f32x4 (&acc)[2][5], int block_m0, int wave_n,
                                              int lane, float* scratch) {
  constexpr int TM = 5, NWV = 10, BM = 80, NCOL = 320;
  const int q = lane >> 4, c = lane & 15;
  const int col = wave_n * 32 + q * 8;
  float bias[8], ga[8], be[8];
  if (p.bias) dd_unpack8<T>(dd_ld16(reinterpret_cast<const T*>(p.bias) + col), bias);
  dd_unpack8<T>(dd_ld16(reinterpret_cast<const T*>(p.lno_gamma) + col), ga);
  dd_unpack8<T>(dd_ld16(reinterpret_cast<const T*>(p.lno_beta) + col), be);
  u32x4 rr[TM];
  if (p.res) {
#pragma unroll
    for (int tm = 0; tm < TM; ++tm) {
      const int64_t rowc = min(block_m0 + tm * 16 + c, p.rows - 1);
      rr[tm] = dd_ld16(reinterpret_cast<const T*>(p.res) + rowc * p.ldres + col);
    }
  }
  float v[TM][8], part[TM];
#pragma unroll
  for (int tm = 0; tm < TM; ++tm) {
    const int row = block_m0 + tm * 16 + c;
    float r[8];
    if (p.res) dd_unpack8<T>(rr[tm], r);
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float x = acc[e >> 2][tm][e & 3];
      if (p.bias) x += bias[e];
      x *= p.alpha;
      if (p.res) x += r[e];
      v[tm][e] = (float)(T)x;                            // the stored (rounded) value is what gets normalised
      s += v[tm][e];
    }
    if (row < p.rows) dd_st16(reinterpret_cast<T*>(p.out) + (int64_t)row * p.ldc + col, dd_pack8<T>(v[tm]));
    s += __shfl_xor(s, 16, 64);
    s += __shfl_xor(s, 32, 64);
    part[tm] = s;
  }
  __syncthreads();                                       // every wave is done with the operand ring: LDS is scratch now
  if (q == 0) {
#pragma unroll
    for (int tm = 0; tm < TM; ++tm) scratch[wave_n * BM + tm * 16 + c] = part[tm];
  }
  __syncthreads();
  float mean[TM];
#pragma unroll
  for (int tm = 0; tm < TM; ++tm) {
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < NWV; ++w) s += scratch[w * BM + tm * 16 + c];
    mean[tm] = s * (1.0f / (float)NCOL);
    float ss = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) { const float d = v[tm][e] - mean[tm]; ss += d * d; }
    ss += __shfl_xor(ss, 16, 64);
    ss += __shfl_xor(ss, 32, 64);
    part[tm] = ss;
  }
  __syncthreads();
  if (q == 0) {
#pragma unroll
    for (int tm = 0; tm < TM; ++tm) scratch[wave_n * BM + tm * 16 + c] = part[tm];
  }
  __syncthreads();
#pragma unroll
  for (int tm = 0; tm < TM; ++tm) {
    const int row = block_m0 + tm * 16 + c;
    float ss = 0.f;
#pragma unroll
    for (int w = 0; w < NWV; ++w) ss += scratch[w * BM + tm * 16 + c];
    const float rstd = rsqrtf(ss * (1.0f / (float)NCOL) + p.ln_eps);
    float o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (v[tm][e] - mean[tm]) * rstd * ga[e] + be[e];
    if (row < p.rows) dd_st16(reinterpret_cast<T*>(p.ln_out) + (int64_t)row * p.ld_ln_out + col, dd_pack8<T>(o));
  }
}

template <int N>
__device__ __forceinline__ void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// buffer_load_dwordx4 ... offen lds: SGPR descriptor + a 32-bit byte offset per lane + a scalar
// offset.  An offset outside the descriptor's range reads zeros (hardware range check), which is how
// padding taps and tile tails are produced — no 64-bit pointer arithmetic, no select against a zero page.
__device__ __forceinline__ void bdma16(__amdgpu_buffer_rsrc_t rsrc, uint32_t voff, uint32_t soff, void* lds_wave_base) {
  if constexpr (!dd_dbg::NODMA)
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void*)lds_wave_base, 16,
                                             (int)voff, (int)soff, 0, 0);
}
// every buffer is < 2^31 bytes (checked on the host), so this lane offset is out of range whatever
// scalar offset is added to it
constexpr uint32_t DD_OOB = 0x80000000u;

// DD_STAMP*, C3_SEG*, dd_dbg::*: hooks of the diagnostic builds, all empty / false in the product (dd_debug.h).

// (dd_gemm3_kernel and dd_gemm4_kernel)
template <int WM, int WN>
constexpr int gemm3_min_waves() {
  // Four-wave workgroups are compiled for TWO waves per SIMD (<= 256 registers) even where only one ring fits the LDS:
  // with the 512-register budget of one wave per SIMD hipcc moves the accumulators to AGPRs and rotates them through
  // v_accvgpr_read / _write / _mov in every K-step of this loop (measured on the 5-slot 96x64 ring: 11.6 us against 9.5).
  return WM * WN == 4 ? 2 : 1;
}

}  // namespace
