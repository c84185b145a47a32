// =============================================================================================
// Kernel family 2: LDS-DMA (buffer_load_dwordx4 ... lds, 16 B / lane) multi-stage ring.
//  * no staging registers and no ds_write: tiles land in LDS asynchronously, NSTAGE-1 K-steps ahead;
//  * the XOR swizzle is applied on the per-lane SOURCE offset (the DMA destination is lane-linear);
//  * padding taps / tile tails use an out-of-range lane offset: the descriptor's range check makes
//    the DMA deliver zeros, so nothing is predicated;
//  * counted s_waitcnt vmcnt(N) + raw s_barrier: one barrier per K-step, loads stay in flight
//    across it.
// =============================================================================================
// Compiled by four translation units, one per form (gemm23.hip for the dense one, gemm2_geglu.hip, gemm2_conv.hip, gemm2_upfold.hip): this kernel is
// more than half of the library's device code, and one unit of it would be the whole build's critical path.
#pragma once
#include "gemm_device.h"

namespace {

// Occupancy target (round 3): the DENSE four-wave instantiations had grown to 240-272 registers (LayerNorm fold, row
// statistics, head-major planes, persistent walk ... all live in one body), i.e. ONE wave per SIMD and one workgroup per CU
// although their 48-72 KB rings would let two in — the situation in which a latency-bound K loop has nothing to hide
// behind.  Where two rings fit the LDS the compiler is told to fit two workgroups (<= 256 registers per wave).
template <int NW, int TM, int TN, int NSTAGE, bool CONV>
constexpr int gemm2_min_blocks() {
  return (!CONV && NW == 4 && TM * TN <= 8 && NSTAGE <= 3) ? 2 : 1;
}

// The body of dd_gemm2_kernel and of dd_gemm2u_kernel (UPF: the folded-upsample conv, `u` its class table — CONV with
// 2 x 2 summed taps per output pixel, K = 4 * cin, and the rows of a tile taken from one class of output pixels).
template <typename T, int WAVES_M, int WAVES_N, int TM, int TN, int NSTAGE, bool CONV, bool GEGLU, bool UPF>
__device__ __forceinline__ void dd_gemm2_body(const GemmParams& p, const UpfoldTab* u) {
  static_assert(!UPF || (CONV && !GEGLU), "the folded upsample is a conv form");
  using V8 = typename dd_vec<T>::v8;
  constexpr int NW = WAVES_M * WAVES_N;
  constexpr int BM = WAVES_M * TM * 16;
  constexpr int BN = WAVES_N * TN * 16;
  constexpr int BN_OUT = GEGLU ? BN / 2 : BN;
  constexpr int XI = BM / 8 / NW;                 // DMA wave-instructions (8 rows x 128 B) per wave
  constexpr int WI = BN / 8 / NW;
  constexpr int LPS = XI + WI;                    // DMA instructions per thread per stage
  constexpr int STAGE = (BM + BN) * BK;           // elements per ring slot
  static_assert(BM % (8 * NW) == 0 && BN % (8 * NW) == 0, "tile/waves mismatch");
  static_assert(NW % 2 == 0, "swizzle must not depend on the instruction index");
  static_assert(TN % 2 == 0 && (!GEGLU || TN % 4 == 0), "TN");
  static_assert(NSTAGE >= 2 && NSTAGE <= 8, "NSTAGE");
  static_assert((NSTAGE - 2) * LPS <= 63, "vmcnt is a 6-bit counter");

  DD_STAMP_DECL();
  DD_STAMP(0);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  T* ring = reinterpret_cast<T*>(smem);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);    // provably wave-uniform -> SALU address math
  const int wave_m = wave / WAVES_N;
  const int wave_n = wave % WAVES_N;

  // PERSISTENT mode (p.persist: dense, no split-K, more tiles than resident workgroups): a workgroup walks the tiles
  // lin, lin + gridDim.x, ... and the DMA ring runs AHEAD across the tile boundary — the first NSTAGE-1 stages of
  // the next tile are issued during the last K-steps of the current one, so only the very first tile of a workgroup
  // pays the pipeline fill (measured: 25 % of a 5-step tile's life at K = 320, tools/gemm2_stamps.py) and the
  // epilogue's stores overlap the next tile's loads.
  const int ntiles = p.tiles_m * p.tiles_n;
  int lin = blockIdx.x;                              // the tile being multiplied (consumer side)
  int tile = xcd_remap(lin, ntiles);
  int block_m0 = (tile / p.tiles_n) * BM;
  int block_n0 = (tile % p.tiles_n) * BN_OUT;
  // UPF: the class of this row tile (all scalar); block_m0 counts the rows of that class
  int u_rc = 0, u_cc = 0, u_widx = 0, u_ny = 1, u_nx = 1, u_y0 = 0, u_x0 = 0, u_rows = 0;
  float u_inv_plane = 1.f, u_inv_nx = 1.f;
  if constexpr (UPF) {
    const int tmi = tile / p.tiles_n;
    int cls = 0;
#pragma unroll
    for (int c = 1; c < 9; ++c) if (tmi >= (int)u->tile0[c]) cls = c;
    int t0 = 0;
#pragma unroll
    for (int c = 0; c < 9; ++c)
      if (c == cls) { t0 = u->tile0[c]; u_widx = u->widx[c]; u_inv_plane = u->inv_plane[c]; }
    u_rc = (cls * 11) >> 5;                          // cls / 3
    u_cc = cls - u_rc * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (c == u_rc) { u_ny = u->ny[c]; u_y0 = u->y0[c]; }
      if (c == u_cc) { u_nx = u->nx[c]; u_x0 = u->x0[c]; u_inv_nx = u->inv_nx[c]; }
    }
    u_rows = u->m * u_ny * u_nx;
    block_m0 = (tmi - t0) * BM;
  }
  // UPF: tile row r of the class -> instance, output y, output x (false: a padding row past the class's end)
  auto u_pixel = [&](const int r, int& inst, int& oy, int& ox) __attribute__((always_inline)) {
    const bool rv = r < u_rows;
    const int rr = rv ? r : 0;
    inst = dd_fdiv(rr, u_inv_plane);
    const int rem = rr - inst * (u_ny * u_nx);
    const int iy = dd_fdiv(rem, u_inv_nx);
    oy = u->y[u_y0 + iy];
    ox = u->x[u_x0 + rem - iy * u_nx];
    return rv;
  };

  const int kbeg = blockIdx.z * p.k_per_split;
  const int kend = min(p.k, kbeg + p.k_per_split);
  const int nk = (kend - kbeg + BK - 1) / BK;

  // DMA mapping: instruction j of this wave fills tile rows (j*NW + wave)*8 .. +7; lane l writes
  // row (l >> 3), chunk position (l & 7).  Logical chunk = position ^ ((row >> 1) & 7), which for an
  // even number of waves does not depend on j.
  const int lrow = lane >> 3;
  const int lc = (lane & 7) ^ ((((wave & 1) << 2) + (lane >> 4)) & 7);
  const uint32_t lcb = (uint32_t)lc * 16u;          // this lane's 16-B chunk inside the 128-B K segment

  // All address state lives in per-lane byte-offset tables that change at most once per conv tap
  // (or at the a/a2 seam); a K-step only moves SCALAR offsets.  K, cin and k1 are multiples of 64
  // here (the host routes other shapes to the register-staged family), so a K-step never straddles
  // a tap or the seam.  Exactly ONE DMA instruction per (operand, j) and stage: the counted vmcnt
  // waits below rely on it.
  uint32_t wv[WI];                                  // weight rows: n * K * 2 + chunk, or out of range
  auto make_wv = [&](const int bn0) __attribute__((always_inline)) {
#pragma unroll
  for (int j = 0; j < WI; ++j) {
    const int R = (j * NW + wave) * 8 + lrow;
    const int wvi = R / (TN * 16);
    const int rho = R % (TN * 16);
    const int tn = rho >> 4, r = rho & 15;
    int n_glob;
    if (GEGLU) {
      constexpr int TH = TN / 2;
      const int t = tn % TH;
      const int loc = wvi * (TH * 16) + (r >> 2) * (4 * TH) + t * 4 + (r & 3);
      const int col = bn0 + loc;
      n_glob = (col < p.n) ? col + (tn >= TH ? p.n : 0) : -1;
    } else {
      const int loc = wvi * (TN * 16) + (r >> 2) * (4 * TN) + tn * 4 + (r & 3);
      const int col = bn0 + loc;
      n_glob = (col < p.n) ? col : -1;
    }
    wv[j] = n_glob >= 0 ? (uint32_t)(UPF ? u_widx * p.n + n_glob : n_glob) * (uint32_t)p.k * 2u + lcb : DD_OOB;
  }
  };
  make_wv(block_n0);

  uint32_t xe[XI];                                  // activation rows: offsets for the current tap / source a
  uint32_t xe2[CONV ? 1 : XI];                      // dense: offsets into a2
  uint32_t syo[CONV ? XI : 1][3], sxo[CONV ? XI : 1][3], xbits[CONV ? XI : 1];   // conv: per-tap source offsets
#pragma unroll
  for (int j = 0; j < XI; ++j) {
    const int r = block_m0 + (j * NW + wave) * 8 + lrow;
    [[maybe_unused]] const bool rv = r < p.rows;        // (UPF: a row is valid by its class, u_pixel)
    if constexpr (UPF) {
      // slot 0 / 1 of an axis reads source s - 1 / s (classes 0, 2) or s / s + 1 (class 1), s = src(o); a slot outside the
      // image gets the out-of-range offset like any padding tap
      int inst, oy, ox;
      const bool uv = u_pixel(r, inst, oy, ox);
      const int sy0 = min((int)floorf(oy * p.scale_h), p.hin - 1) - (u_rc != 1);
      const int sx0 = min((int)floorf(ox * p.scale_w), p.win - 1) - (u_cc != 1);
      uint32_t bits = 0;
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int iy = sy0 + t, ix = sx0 + t;
        const bool vy = iy >= 0 && iy < p.hin, vx = ix >= 0 && ix < p.win;
        const int sy = min(max(iy, 0), p.hin - 1), sx = min(max(ix, 0), p.win - 1);
        syo[j][t] = (uint32_t)((inst * p.hin + sy) * p.win) * (uint32_t)p.cin * 2u + lcb;
        sxo[j][t] = (uint32_t)(sx * p.cin) * 2u;
        if (vy) bits |= 1u << t;
        if (vx) bits |= 4u << t;
      }
      syo[j][2] = sxo[j][2] = 0;
      uint32_t m4 = 0;                                // bit (sy*2+sx): slot reads a real pixel
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (uv && ((bits >> (t >> 1)) & 1u) && ((bits >> (2 + (t & 1))) & 1u)) m4 |= 1u << t;
      xbits[j] = m4;
      xe[j] = DD_OOB;
    } else if (CONV) {
      const int hw = p.hout * p.wout;
      const int rr = rv ? r : 0;
      const int inst = dd_fdiv(rr, p.inv_hw);
      const int rem = rr - inst * hw;
      const int oy = dd_fdiv(rem, p.inv_wout);
      const int ox = rem - oy * p.wout;
      const int iy0 = oy * p.stride - 1, ix0 = ox * p.stride - 1;
      uint32_t bits = 0;
#pragma unroll
      for (int t = 0; t < 3; ++t) {
        const int iy = iy0 + t, ix = ix0 + t;
        const bool vy = iy >= 0 && iy < p.hv, vx = ix >= 0 && ix < p.wv;
        int sy = min(max(iy, 0), p.hv - 1), sx = min(max(ix, 0), p.wv - 1);
        if (p.upsample) {                             // torch nearest: min(floor(dst * in/out), in - 1)
          sy = min((int)floorf(sy * p.scale_h), p.hin - 1);
          sx = min((int)floorf(sx * p.scale_w), p.win - 1);
        }
        syo[j][t] = (uint32_t)((inst * p.hin + sy) * p.win) * (uint32_t)p.cin * 2u + lcb;
        sxo[j][t] = (uint32_t)(sx * p.cin) * 2u;
        if (vy) bits |= 1u << t;
        if (vx) bits |= 8u << t;
      }
      uint32_t m9 = 0;                                // bit (ky*3+kx): tap reads a real pixel
#pragma unroll
      for (int t = 0; t < 9; ++t)
        if (rv && ((bits >> (t / 3)) & 1u) && ((bits >> (3 + t % 3)) & 1u)) m9 |= 1u << t;
      xbits[j] = m9;
      xe[j] = DD_OOB;
    } else {
      xe[j] = rv ? (uint32_t)r * (uint32_t)p.lda * 2u + lcb : DD_OOB;
      xe2[j] = rv ? (uint32_t)r * (uint32_t)p.lda2 * 2u + lcb : DD_OOB;
    }
  }
  auto make_xe = [&](const int bm0) __attribute__((always_inline)) {       // dense: tables of another row tile
#pragma unroll
    for (int j = 0; j < XI; ++j) {
      const int r = bm0 + (j * NW + wave) * 8 + lrow;
      const bool rv = r < p.rows;
      xe[j] = rv ? (uint32_t)r * (uint32_t)p.lda * 2u + lcb : DD_OOB;
      xe2[j] = rv ? (uint32_t)r * (uint32_t)p.lda2 * 2u + lcb : DD_OOB;
    }
  };
  // conv: point xe[] at tap `tap` (table select by mask arithmetic: a select of array elements
  // would force the tables to scratch)
  auto set_tap = [&](int tap) __attribute__((always_inline)) {
    if (CONV) {
      const int ky = UPF ? tap >> 1 : (tap * 11) >> 5;         // tap / 3 for tap in [0, 9]; UPF: slot / 2 for slot in [0, 4]
      const int kx = UPF ? tap & 1 : tap - ky * 3;
      const uint32_t y0 = 0u - (uint32_t)(ky == 0), y1 = 0u - (uint32_t)(ky == 1), y2 = 0u - (uint32_t)(ky == 2);
      const uint32_t x0 = 0u - (uint32_t)(kx == 0), x1 = 0u - (uint32_t)(kx == 1), x2 = 0u - (uint32_t)(kx == 2);
#pragma unroll
      for (int j = 0; j < XI; ++j) {
        const uint32_t oy = (syo[j][0] & y0) | (syo[j][1] & y1) | (syo[j][2] & y2);
        const uint32_t ox = (sxo[j][0] & x0) | (sxo[j][1] & x1) | (sxo[j][2] & x2);
        const uint32_t m = 0u - ((xbits[j] >> tap) & 1u);
        xe[j] = ((oy + ox) & m) | (DD_OOB & ~m);
      }
    }
  };
  const __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.w), 0, p.w_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_a = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.a), 0, p.a_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_a2 = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<void*>(p.a2 ? p.a2 : p.a), 0, p.a2 ? p.a2_bytes : p.a_bytes, 0x00020000);

  // issue cursor (all scalar): next K offset, and for conv its tap / channel split
  int ik0 = kbeg;
  int itap = CONV ? kbeg / p.cin : 0;
  int ici0 = CONV ? kbeg - itap * p.cin : 0;
  set_tap(itap);
  auto issue_next = [&](int slot) __attribute__((always_inline)) {
    T* xs = ring + slot * STAGE;
    T* ws = xs + BM * BK;
    const uint32_t ksoff = dd_dbg::SAMEK ? 0u : (uint32_t)ik0 * 2u;
#pragma unroll
    for (int j = 0; j < WI; ++j) bdma16(rs_w, wv[j], ksoff, ws + (j * NW + wave) * 8 * BK);
    if (CONV) {
      const uint32_t csoff = (uint32_t)ici0 * 2u;
#pragma unroll
      for (int j = 0; j < XI; ++j) bdma16(rs_a, xe[j], csoff, xs + (j * NW + wave) * 8 * BK);
      ici0 += BK;
      if (ici0 >= p.cin) {                            // scalar branch, no DMA inside
        ici0 = 0;
        ++itap;
        set_tap(itap);
      }
    } else if (ik0 >= p.k1) {                         // scalar; both arms issue XI DMAs
      const uint32_t k2 = (uint32_t)(ik0 - p.k1) * 2u;
#pragma unroll
      for (int j = 0; j < XI; ++j) bdma16(rs_a2, xe2[j], k2, xs + (j * NW + wave) * 8 * BK);
    } else {
#pragma unroll
      for (int j = 0; j < XI; ++j) bdma16(rs_a, xe[j], ksoff, xs + (j * NW + wave) * 8 * BK);
    }
    ik0 += BK;
  };

  f32x4 acc[TN][TM];
#pragma unroll
  for (int i = 0; i < TN; ++i)
#pragma unroll
    for (int j = 0; j < TM; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int frow = lane & 15;
  const int fswz = (lane >> 1) & 7;
  const int fchunk = lane >> 4;

  DD_STAMP(1);
#pragma unroll
  for (int s0 = 0; s0 < NSTAGE - 1; ++s0)
    if (s0 < nk) issue_next(s0);
  DD_STAMP(2);

  // LayerNorm fold: row statistics of the block's A rows (K = 40 * lpr columns: lpr lanes share a
  // row, five 16-B vectors per lane), computed while the first stages are in flight.
  __shared__ float s_ln_mean[BM], s_ln_rstd[BM];
  if (!CONV && p.ln_colsum && p.stat_in) {
    // the producer of `a` left per-row partial sums (one pair per 32 columns): a few loads per row
    const int parts = p.k >> 5;
    const float inv_k = 1.0f / (float)p.k;
    for (int r = tid; r < BM; r += NW * 64) {
      const float* src = p.stat_in + (int64_t)min(block_m0 + r, p.rows - 1) * parts * 2;
      float sum = 0.f, sq = 0.f;
      for (int i = 0; i < parts; i += 2) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(src + i * 2);
        sum += v[0] + v[2];
        sq += v[1] + v[3];
      }
      const float mean = sum * inv_k;
      s_ln_mean[r] = mean;
      s_ln_rstd[r] = rsqrtf(fmaxf(sq * inv_k - mean * mean, 0.f) + p.ln_eps);
    }
    __syncthreads();
  } else if (!CONV && p.ln_colsum) {
    const int lpr = p.k / 40;                           // 8 / 16 / 32 (host-checked)
    const int rpw = 64 / lpr;
    const int sub = lane & (lpr - 1);
    const float inv_k = 1.0f / (float)p.k;
    for (int r0 = wave * rpw; r0 < BM; r0 += NW * rpw) {
      const int r = r0 + lane / lpr;
      const int64_t grow = min(block_m0 + r, p.rows - 1);
      float sum = 0.f, sq = 0.f;
      u32x4 raw[5];
#pragma unroll
      for (int i = 0; i < 5; ++i)
        raw[i] = dd_ld16(reinterpret_cast<const T*>(p.a) + grow * p.lda + (sub + i * lpr) * 8);
#pragma unroll
      for (int i = 0; i < 5; ++i) {
        float f[8];
        dd_unpack8<T>(raw[i], f);
#pragma unroll
        for (int e = 0; e < 8; ++e) { sum += f[e]; sq += f[e] * f[e]; }
      }
      for (int o = lpr >> 1; o > 0; o >>= 1) { sum += __shfl_xor(sum, o, 64); sq += __shfl_xor(sq, o, 64); }
      if (sub == 0) {
        const float mean = sum * inv_k;
        s_ln_mean[r] = mean;
        s_ln_rstd[r] = rsqrtf(fmaxf(sq * inv_k - mean * mean, 0.f) + p.ln_eps);
      }
    }
    __syncthreads();
  }

  // (A staggered schedule — the second half of the waves half a K-step out of phase, as in the direct conv kernel — was
  //  measured on tiles 16 / 20 / 26 in round 3: 2-9 % SLOWER here (L0 conv 41.4 -> 45.0 us, GEGLU 53.0 -> 55.0 us); its
  //  code was removed in round 5.)
  V8 wf[2][TN], xf[2][TM];
  auto mfma_step = [&]() __attribute__((always_inline)) {
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
      for (int i = 0; i < TN; ++i)
#pragma unroll
        for (int j = 0; j < TM; ++j) acc[i][j] = dd_mfma16(wf[ks][i], xf[ks][j], acc[i][j]);
    }
    __builtin_amdgcn_s_setprio(0);
  };
  int sbase = 0;                       // ring slot of this tile's stage 0 (persistent: tiles follow each other in the ring)
  bool have_next = false;              // persistent: another tile follows, its first stages are issued from this one
  auto kstep = [&](const int kt) __attribute__((always_inline)) {
    // stage kt must have landed; up to NSTAGE-2 younger stages may stay in flight
    if (NSTAGE == 2) {
      wait_vmcnt<0>();
    } else {
      const int ahead = have_next ? NSTAGE - 2 : min(nk - 1 - kt, NSTAGE - 2);     // scalar; stages allowed to stay in flight
      if (ahead <= 0) wait_vmcnt<0>();
      else if (ahead == 1 || NSTAGE <= 3) wait_vmcnt<(NSTAGE > 2 ? 1 : 0) * LPS>();
      else if (ahead == 2 || NSTAGE <= 4) wait_vmcnt<(NSTAGE > 3 ? 2 : 0) * LPS>();
      else if (ahead == 3 || NSTAGE <= 5) wait_vmcnt<(NSTAGE > 4 ? 3 : 0) * LPS>();
      else if (ahead == 4 || NSTAGE <= 6) wait_vmcnt<(NSTAGE > 5 ? 4 : 0) * LPS>();
      else if (ahead == 5 || NSTAGE <= 7) wait_vmcnt<(NSTAGE > 6 ? 5 : 0) * LPS>();
      else wait_vmcnt<(NSTAGE > 7 ? 6 : 0) * LPS>();
    }
    __builtin_amdgcn_s_barrier();          // everyone's share of stage kt landed; slot (kt-1) is free
    // (issuing the DMAs after the fragment reads, or between the two MFMA halves, measured the same)
    {
      const int a = kt + NSTAGE - 1;                 // the stage to issue now, counted from this tile's stage 0
      const int islot = (sbase + a) % NSTAGE;
      if (a < nk) {
        issue_next(islot);
      } else if (have_next) {                        // into the next tile (nk >= NSTAGE - 1: host-checked)
        if constexpr (!CONV) {
          if (a == nk) {                             // the issue side crosses the tile boundary: new address tables
            const int nt = xcd_remap(lin + (int)gridDim.x, ntiles);
            make_wv((nt % p.tiles_n) * BN_OUT);
            make_xe((nt / p.tiles_n) * BM);
            ik0 = kbeg;
          }
          issue_next(islot);
        }
      }
    }
    const int slot = (sbase + kt) % NSTAGE;
    const T* xs = ring + slot * STAGE + (wave_m * TM * 16 + frow) * BK;
    const T* ws = ring + slot * STAGE + BM * BK + (wave_n * TN * 16 + frow) * BK;
    // all fragment reads of the K-step go out first; the MFMAs of the first half then run while the
    // second half's reads are still landing (counted lgkmcnt waits, reads return in order)
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int cofs = ((fchunk + 4 * ks) ^ fswz) << 3;
#pragma unroll
      for (int i = 0; i < TN; ++i) wf[ks][i] = dd_as_v8<T>(dd_ld16(ws + i * 16 * BK + cofs));
#pragma unroll
      for (int j = 0; j < TM; ++j) xf[ks][j] = dd_as_v8<T>(dd_ld16(xs + j * 16 * BK + cofs));
    }
    __builtin_amdgcn_sched_barrier(0);
    mfma_step();
  };
  const bool persist = !CONV && p.persist != 0;
  for (;;) {
  have_next = persist && lin + (int)gridDim.x < ntiles;
  for (int kt = 0; kt < nk; kt += 2) {
    kstep(kt);
    DD_STAMP_IF(kt == 0, 3);                   // after the first K-step
    if (kt + 1 < nk) kstep(kt + 1);
  }
  DD_STAMP(4);
  if constexpr (!CONV && !GEGLU && WAVES_M == 1 && WAVES_N == 10 && TM == 5 && TN == 2) {
    if (p.ln_out) {                       // whole rows in this workgroup: store out AND LayerNorm(out)
      store_tile_ln<T>(p, acc, block_m0, wave_n, lane, reinterpret_cast<float*>(smem));
      return;
    }
  }
  const bool ln = !CONV && p.ln_colsum;
  if constexpr (UPF) {                    // rows go to their output pixels; padding rows nowhere
    int rowmap[TM];
#pragma unroll
    for (int tm = 0; tm < TM; ++tm) {
      int inst, oy, ox;
      const bool uv = u_pixel(block_m0 + wave_m * (TM * 16) + tm * 16 + (lane & 15), inst, oy, ox);
      rowmap[tm] = uv ? (inst * p.hout + oy) * p.wout + ox : p.rows;
    }
    store_tile<T, TM, TN, false, true>(p, acc, block_m0, block_n0, wave_m, wave_n, lane, p.rows, nullptr, nullptr, rowmap);
    break;                                // (no persistent walk in the conv forms)
  }
  store_tile<T, TM, TN, GEGLU>(p, acc, block_m0, block_n0, wave_m, wave_n, lane, p.rows,
                               ln ? s_ln_mean : nullptr, ln ? s_ln_rstd : nullptr);
  if (!have_next) break;
  lin += (int)gridDim.x;                   // next tile of this workgroup; its first stages are already in flight
  tile = xcd_remap(lin, ntiles);
  block_m0 = (tile / p.tiles_n) * BM;
  block_n0 = (tile % p.tiles_n) * BN_OUT;
  sbase = (sbase + nk) % NSTAGE;
#pragma unroll
  for (int i = 0; i < TN; ++i)
#pragma unroll
    for (int j = 0; j < TM; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  DD_STAMP_FLUSH(p);
}

template <typename T, int WAVES_M, int WAVES_N, int TM, int TN, int NSTAGE, bool CONV, bool GEGLU>
__global__ __launch_bounds__(64 * WAVES_M * WAVES_N, (gemm2_min_blocks<WAVES_M * WAVES_N, TM, TN, NSTAGE, CONV>()))
void dd_gemm2_kernel(const GemmParams p) {
  dd_gemm2_body<T, WAVES_M, WAVES_N, TM, TN, NSTAGE, CONV, GEGLU, false>(p, nullptr);
}

template <typename T, int WAVES_M, int WAVES_N, int TM, int TN, int NSTAGE>
__global__ __launch_bounds__(64 * WAVES_M * WAVES_N, (gemm2_min_blocks<WAVES_M * WAVES_N, TM, TN, NSTAGE, true>()))
void dd_gemm2u_kernel(const GemmParams p, const UpfoldTab u) {
  dd_gemm2_body<T, WAVES_M, WAVES_N, TM, TN, NSTAGE, true, false, true>(p, &u);
}

struct Gemm2 {
  static constexpr Family family = FAM_RING;
  static constexpr unsigned needs = 0;
  template <typename T, size_t I, unsigned FORM>
  static int run(const GemmParams& p, const Plan& pl, hipStream_t s) {
    constexpr const TileCfg& t = kTiles[I];
    constexpr size_t smem = (size_t)t.depth * (tile_bm(t) + tile_bn(t)) * BK * sizeof(T);
    static_assert(smem <= 160 * 1024, "LDS");
    constexpr auto kern = dd_gemm2_kernel<T, t.wm, t.wn, t.tm, t.tn, t.depth, FORM == F_CONV, FORM == F_GEGLU>;
    dim3 grid(pl.tiles_m * pl.tiles_n, 1, pl.split);
    GemmParams q = p;
    if (pl.persist_ok) {                 // more tiles than resident workgroups: walk them with the ring running ahead
      static std::atomic<int> resident{0};
      int per_cu = resident.load(std::memory_order_relaxed);
      if (per_cu == 0) {
        raise_lds_limit<kern>(smem);     // the occupancy query counts with the limit in force
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, 64 * t.wm * t.wn, smem) != hipSuccess || per_cu < 1)
          per_cu = 1;
        resident.store(per_cu, std::memory_order_relaxed);
      }
      if ((int)grid.x > kNumCU * per_cu) {
        q.persist = 1;
        grid.x = kNumCU * per_cu;
      }
    }
    return launch_kernel<kern>(grid, 64 * t.wm * t.wn, smem, s, q);
  }
};


struct Gemm2U {
  static constexpr Family family = FAM_RING;
  static constexpr unsigned needs = 0;
  template <typename T, size_t I, unsigned FORM>
  static int run(const GemmParams& p, const Plan& pl, hipStream_t s) {
    constexpr const TileCfg& t = kTiles[I];
    constexpr size_t smem = (size_t)t.depth * (tile_bm(t) + tile_bn(t)) * BK * sizeof(T);
    static_assert(smem <= 160 * 1024, "LDS");
    constexpr auto kern = dd_gemm2u_kernel<T, t.wm, t.wn, t.tm, t.tn, t.depth>;
    raise_lds_limit<kern>(smem);
    hipLaunchKernelGGL(kern, dim3(pl.tiles_m * pl.tiles_n, 1, pl.split), dim3(64 * t.wm * t.wn), smem, s, p, pl.upf);
    return dd_check_launch();
  }
};

}  // namespace
