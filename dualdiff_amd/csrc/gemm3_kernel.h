// Compiled by gemm23.hip, next to the dense dd_gemm2_kernel instantiations.
#pragma once
#include "gemm_device.h"

namespace {

// =============================================================================================
// Kernel family 2p (round 5): the LDS-DMA ring with an UN-SERIALISED K-step.  Dense GEMMs only.
//
// dd_gemm2_kernel runs every K-step as the serial chain  vmcnt wait -> barrier -> DMA issue -> fragment reads ->
// MFMAs: with one wave per SIMD (every dominant shape: <= 256 workgroups) nothing overlaps that chain and the matrix
// pipe is busy 192 of ~800 cycles (profiles/r04_gemm2_timeline.txt).  Here the fragments of K-step
// c+1 are read while the MFMAs of K-step c run, in two HALVES so that no second register set is needed:
//
//   barrier(c)  |  MFMAs on the ks=0 fragments of c   (the DMAs of stage c+D are issued between them)
//               |  ds_reads of the ks=0 fragments of c+1  ||  MFMAs on the ks=1 fragments of c
//               |  ds_reads of the ks=1 fragments of c+1  ||  (next step's wait + barrier + first MFMAs)
//
// The barrier at the top of step c therefore certifies stage c+1 (not c), and the first MFMA after it never waits
// for LDS.  TIGHT (NSTAGE <= 3): the DMA of step c refills the slot of stage c itself, whose last fragment reads
// (ks=1, issued at the end of step c-1) every wave retires with lgkmcnt(0) before the barrier; NSTAGE >= 4: it refills
// the slot of stage c-1, and the only LDS wait of a step is the compiler's counted one in front of the MFMAs.
// Same arithmetic in the same order per accumulator as dd_gemm2_kernel -> bit-identical results.
// No persistent walk (the epilogue's stores would count in the vmcnt window of the next tile's stages), no LayerNorm
// fold, no conv: those stay with dd_gemm2_kernel.
// =============================================================================================
template <typename T, int WAVES_M, int WAVES_N, int TM, int TN, int NSTAGE, bool GEGLU>
__global__ __launch_bounds__(64 * WAVES_M * WAVES_N, (gemm3_min_waves<WAVES_M, WAVES_N>()))
void dd_gemm3_kernel(const GemmParams p) {
  using V8 = typename dd_vec<T>::v8;
  constexpr int NW = WAVES_M * WAVES_N;
  constexpr int BM = WAVES_M * TM * 16;
  constexpr int BN = WAVES_N * TN * 16;
  constexpr int BN_OUT = GEGLU ? BN / 2 : BN;
  constexpr int XI = BM / 8 / NW;                 // DMA wave-instructions (8 rows x 128 B) per wave
  constexpr int WI = BN / 8 / NW;
  constexpr int LPS = XI + WI;                    // DMA instructions per thread per stage
  constexpr int STAGE = (BM + BN) * BK;           // elements per ring slot
  constexpr bool TIGHT = NSTAGE <= 3;
  constexpr int D = TIGHT ? NSTAGE : NSTAGE - 1;  // the DMA of step c carries stage c + D
  // FAST EPILOGUE (plain T output with bias / alpha / residual / SiLU / accumulate): its operands are loaded through
  // buffer descriptors whose extent is ZERO for an absent operand (the range check returns 0.0f: nothing is predicated,
  // no branch per operand) and the loads are issued right behind the LAST DMA of the K loop, D-1 K-steps before the
  // accumulators are complete — so that the epilogue starts with its operands in registers instead of paying a
  // dependent global round trip (measured before: 1.7 us from the last MFMA to the last store of a 96x64 tile).
  // They are ordinary loads counted in the same in-order vmcnt queue as the DMAs and YOUNGER than every DMA, so the
  // remaining stage waits of the drain simply allow EPI more operations in flight.
  // Register budget: 16-byte operands per lane — tiles of more than 6 (and the 10-wave tiles, 168 registers) keep the
  // general epilogue; the accumulate target is preloaded up to 4.
  constexpr int NG = GEGLU ? 1 : TN / 2;                           // 8-column groups per lane
  constexpr bool FASTEPI = !GEGLU && NW <= 8 && TM * NG <= 6;
  constexpr bool PRE_ACC = FASTEPI && TM * NG <= 4;
  constexpr int EPI = FASTEPI ? NG + TM * NG + (PRE_ACC ? TM * NG : 0) : 0;
  static_assert(BM % (8 * NW) == 0 && BN % (8 * NW) == 0, "tile/waves mismatch");
  static_assert(NW % 2 == 0, "swizzle must not depend on the instruction index");
  static_assert(TN % 2 == 0 && (!GEGLU || TN % 4 == 0), "TN");
  static_assert(NSTAGE >= 3 && NSTAGE <= 8 && D >= 2, "NSTAGE");
  static_assert((D - 1) * LPS <= 63 && (D - 2) * LPS + EPI <= 63, "vmcnt is a 6-bit counter");

  DD_STAMP_DECL();
  DD_STAMP(0);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  T* ring = reinterpret_cast<T*>(smem);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wave_m = wave / WAVES_N;
  const int wave_n = wave % WAVES_N;

  const int ntiles = p.tiles_m * p.tiles_n;
  const int tile = xcd_remap(blockIdx.x, ntiles);
  const int tm_i = tile / p.tiles_n;
  const int block_m0 = tm_i * BM;
  const int block_n0 = (tile - tm_i * p.tiles_n) * BN_OUT;

  const int kbeg = blockIdx.z * p.k_per_split;
  const int kend = min(p.k, kbeg + p.k_per_split);
  const int nk = (kend - kbeg + BK - 1) / BK;

  // DMA mapping as in dd_gemm2_kernel: instruction j of this wave fills tile rows (j*NW + wave)*8 .. +7; lane l
  // writes row (l >> 3), chunk position (l & 7); logical chunk = position ^ ((row >> 1) & 7)
  const int lrow = lane >> 3;
  const int lc = (lane & 7) ^ ((((wave & 1) << 2) + (lane >> 4)) & 7);
  const uint32_t lcb = (uint32_t)lc * 16u;

  uint32_t wv[WI];
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
      const int col = block_n0 + wvi * (TH * 16) + (r >> 2) * (4 * TH) + t * 4 + (r & 3);
      n_glob = (col < p.n) ? col + (tn >= TH ? p.n : 0) : -1;
    } else {
      const int col = block_n0 + wvi * (TN * 16) + (r >> 2) * (4 * TN) + tn * 4 + (r & 3);
      n_glob = (col < p.n) ? col : -1;
    }
    wv[j] = n_glob >= 0 ? (uint32_t)n_glob * (uint32_t)p.k * 2u + lcb : DD_OOB;
  }
  const __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.w), 0, p.w_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_a = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.a), 0, p.a_bytes, 0x00020000);

  // Issue cursor (all scalar).  The activation source is `a` for K < k1 and `a2` behind it (the up path's concat); the
  // switch is ONE scalar branch without a DMA inside, taken at most once per workgroup and placed behind the K-step's
  // schedule (a branch around the DMAs would cut the step into separate scheduling regions).
  int ik0 = kbeg;
  int islot = 0;                                   // ring slot the next stage goes to
  int kbase = 0;
  int seam_k = p.a2 ? p.k1 : 0x7fffffff;           // first K offset served by a2
  __amdgpu_buffer_rsrc_t rs_x = rs_a;
  uint32_t xe[XI];
  auto make_xe = [&](const int64_t ld) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < XI; ++j) {
      const int r = block_m0 + (j * NW + wave) * 8 + lrow;
      xe[j] = r < p.rows ? (uint32_t)r * (uint32_t)ld * 2u + lcb : DD_OOB;
    }
  };
  auto seam = [&]() __attribute__((always_inline)) {
    if (ik0 >= seam_k) {
      make_xe(p.lda2);
      rs_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.a2), 0, p.a2_bytes, 0x00020000);
      kbase = p.k1;
      seam_k = 0x7fffffff;
    }
  };
  make_xe(p.lda);
  seam();                                          // a split-K slice that starts behind the seam
  auto issue_next = [&]() __attribute__((always_inline)) {
    T* xs = ring + islot * STAGE;
    T* ws = xs + BM * BK;
#pragma unroll
    for (int j = 0; j < WI; ++j) bdma16(rs_w, wv[j], (uint32_t)ik0 * 2u, ws + (j * NW + wave) * 8 * BK);
#pragma unroll
    for (int j = 0; j < XI; ++j) bdma16(rs_x, xe[j], (uint32_t)(ik0 - kbase) * 2u, xs + (j * NW + wave) * 8 * BK);
    ik0 += BK;
    islot = islot + 1 == NSTAGE ? 0 : islot + 1;
  };

  f32x4 acc[TN][TM];
#pragma unroll
  for (int i = 0; i < TN; ++i)
#pragma unroll
    for (int j = 0; j < TM; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int frow = lane & 15;
  const int fswz = (lane >> 1) & 7;
  const int fchunk = lane >> 4;
  const int cofs0 = ((fchunk + 0) ^ fswz) << 3, cofs1 = ((fchunk + 4) ^ fswz) << 3;
  const T* xbase = ring + (wave_m * TM * 16 + frow) * BK;
  const T* wbase = ring + BM * BK + (wave_n * TN * 16 + frow) * BK;

  DD_STAMP(1);
  // prologue: stages 0 and 1 first; the remaining D-2 go out behind the first fragment reads (issuing all D up front
  // kept the wave at the address path for 0.7 us before it even looked at stage 0)
#pragma unroll
  for (int s0 = 0; s0 < 2; ++s0)
    if (s0 < nk) { issue_next(); seam(); }

  V8 wf[2][TN], xf[2][TM];
  int rslot = 0;                                   // ring slot of the stage whose fragments are read next
  auto read_half = [&](auto ks_c) __attribute__((always_inline)) {
    constexpr int ks = decltype(ks_c)::value;
    const int cofs = ks ? cofs1 : cofs0;
    const T* ws = wbase + rslot * STAGE + cofs;
    const T* xs = xbase + rslot * STAGE + cofs;
#pragma unroll
    for (int i = 0; i < TN; ++i) wf[ks][i] = dd_as_v8<T>(dd_ld16(ws + i * 16 * BK));
#pragma unroll
    for (int j = 0; j < TM; ++j) xf[ks][j] = dd_as_v8<T>(dd_ld16(xs + j * 16 * BK));
  };
  auto mfma_half = [&](auto ks_c) __attribute__((always_inline)) {
    constexpr int ks = decltype(ks_c)::value;
#pragma unroll
    for (int i = 0; i < TN; ++i)
#pragma unroll
      for (int j = 0; j < TM; ++j) acc[i][j] = dd_mfma16(wf[ks][i], xf[ks][j], acc[i][j]);
  };
  // all but the `ahead` youngest stages (and the EXTRA operations issued behind them) have landed
  auto wait_stages = [&](const int ahead, auto extra_c) __attribute__((always_inline)) {
    constexpr int X = decltype(extra_c)::value;
    if (ahead <= 0) wait_vmcnt<X>();
    else if (ahead == 1 || D <= 2) wait_vmcnt<(D > 1 ? 1 : 0) * LPS + X>();
    else if (ahead == 2 || D <= 3) wait_vmcnt<(D > 2 ? 2 : 0) * LPS + X>();
    else if (ahead == 3 || D <= 4) wait_vmcnt<(D > 3 ? 3 : 0) * LPS + X>();
    else if (ahead == 4 || D <= 5) wait_vmcnt<(D > 4 ? 4 : 0) * LPS + X>();
    else if (ahead == 5 || D <= 6) wait_vmcnt<(D > 5 ? 5 : 0) * LPS + X>();
    else wait_vmcnt<(D > 6 ? 6 : 0) * LPS + X>();
  };
  using K0 = std::integral_constant<int, 0>;
  using K1 = std::integral_constant<int, 1>;
  constexpr int NMF = TN * TM, NRD = TN + TM;

  // stage 0 -> registers
  wait_stages(min(2, nk) - 1, K0{});
  __builtin_amdgcn_s_barrier();
  read_half(K0{});
  read_half(K1{});
  rslot = 1;
#pragma unroll
  for (int s0 = 2; s0 < D; ++s0)
    if (s0 < nk) { issue_next(); seam(); }
  DD_STAMP(2);

  // One K-step in EXPLICIT issue order (pinned with sched_barrier(0) after every unit: sched_group_barrier patterns were
  // only loosely followed): the DMAs one by one behind the first half's MFMAs, the ks=0 reads behind the second half's,
  // the ks=1 reads last.  MEASURED AND REMOVED: a staggered form in which the upper half of the waves issued its DMAs
  // beside the second half's MFMAs (so that the four waves do not queue at the CU's address path together) — 8.7 us
  // either way on 1092x1280x1280, 0.25-0.26 us per K-step (profiles/r05_experiments.txt).
  auto steady = [&](auto issue_c) __attribute__((always_inline)) {
    constexpr bool ISSUE = decltype(issue_c)::value;
    const T* wp0 = wbase + rslot * STAGE + cofs0;
    const T* xp0 = xbase + rslot * STAGE + cofs0;
    const T* wp1 = wbase + rslot * STAGE + cofs1;
    const T* xp1 = xbase + rslot * STAGE + cofs1;
    T* xs = ring + islot * STAGE;
    T* ws = xs + BM * BK;
    const uint32_t so_w = (uint32_t)ik0 * 2u, so_x = (uint32_t)(ik0 - kbase) * 2u;
    auto dma = [&](const int u) __attribute__((always_inline)) {
      if (u < WI) bdma16(rs_w, wv[u], so_w, ws + (u * NW + wave) * 8 * BK);
      else bdma16(rs_x, xe[u - WI], so_x, xs + ((u - WI) * NW + wave) * 8 * BK);
    };
    auto rd = [&](const int ks, const int u) __attribute__((always_inline)) {
      if (u < TN) wf[ks][u] = dd_as_v8<T>(dd_ld16((ks ? wp1 : wp0) + u * 16 * BK));
      else xf[ks][u - TN] = dd_as_v8<T>(dd_ld16((ks ? xp1 : xp0) + (u - TN) * 16 * BK));
    };
    auto mf = [&](const int ks, const int u) __attribute__((always_inline)) {
      const int i = u / TM, j = u % TM;
      acc[i][j] = dd_mfma16(wf[ks][i], xf[ks][j], acc[i][j]);
    };
    constexpr int NDM = ISSUE ? LPS : 0;
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int u = 0; u < (NMF > NDM ? NMF : NDM); ++u) {
      if (u < NMF) mf(0, u);
      if (u < NDM) dma(u);
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int u = 0; u < (NMF > NRD ? NMF : NRD); ++u) {
      if (u < NRD) rd(0, u);
      if (u < NMF) mf(1, u);
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int u = 0; u < NRD; ++u) rd(1, u);
    __builtin_amdgcn_s_setprio(0);
    if constexpr (ISSUE) {
      ik0 += BK;
      islot = islot + 1 == NSTAGE ? 0 : islot + 1;
    }
    rslot = rslot + 1 == NSTAGE ? 0 : rslot + 1;
  };
  int c = 0;
  for (; c + D < nk; ++c) {                        // steady state: stage c+1 certified, stage c+D issued
    wait_vmcnt<(D - 2) * LPS>();
    if (TIGHT) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    steady(std::true_type{});
    seam();
    DD_STAMP_IF(c == 0, 3);
  }

  // ---- epilogue operands: issued behind the last DMA -------------------------------------------------------------
  const int q4 = lane >> 4, c16 = lane & 15;
  const int erow0 = block_m0 + wave_m * (TM * 16) + c16;
  const int ecol0 = block_n0 + wave_n * (TN * 16) + q4 * (4 * TN);
  const bool fast = FASTEPI && !p.partial && !p.hm_d && !p.out_f32 && !p.stat_out && !p.rowvec && (PRE_ACC || !p.accumulate) &&
                    p.out_bytes != 0;
  u32x4 pb[NG], pr[TM][NG], pa[PRE_ACC ? TM : 1][NG];
  uint32_t off_o[TM][NG];
  if constexpr (FASTEPI) {
    const uint32_t e_bias = fast && p.bias ? (uint32_t)p.n * 2u : 0u;
    const uint32_t e_res = fast && p.res ? p.res_bytes : 0u;
    const uint32_t e_acc = fast && p.accumulate ? p.out_bytes : 0u;
    const __amdgpu_buffer_rsrc_t rs_b = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.bias), 0, e_bias, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_r = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.res), 0, e_res, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_o = __builtin_amdgcn_make_buffer_rsrc(p.out, 0, e_acc, 0x00020000);
#pragma unroll
    for (int g8 = 0; g8 < NG; ++g8) {
      const int col = ecol0 + g8 * 8;
      pb[g8] = __builtin_amdgcn_raw_buffer_load_b128(rs_b, col < p.n ? (uint32_t)col * 2u : DD_OOB, 0, 0);
    }
#pragma unroll
    for (int tm = 0; tm < TM; ++tm) {
      const int row = erow0 + tm * 16;
#pragma unroll
      for (int g8 = 0; g8 < NG; ++g8) {
        const int col = ecol0 + g8 * 8;
        const bool ok = row < p.rows && col < p.n;
        off_o[tm][g8] = ok ? ((uint32_t)row * (uint32_t)p.ldc + (uint32_t)col) * 2u : DD_OOB;
        pr[tm][g8] = __builtin_amdgcn_raw_buffer_load_b128(rs_r, ok ? ((uint32_t)row * (uint32_t)p.ldres + (uint32_t)col) * 2u : DD_OOB, 0, 0);
        if constexpr (PRE_ACC) pa[tm][g8] = __builtin_amdgcn_raw_buffer_load_b128(rs_o, off_o[tm][g8], 0, 0);
      }
    }
  }
  using EX = std::integral_constant<int, EPI>;

  for (; c + 1 < nk; ++c) {                        // drain: nothing left to issue
    wait_stages(nk - 2 - c, EX{});
    if (TIGHT) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    steady(std::false_type{});
  }
  if (nk > 0) {                                    // last K-step: its fragments are in registers
    __builtin_amdgcn_s_setprio(1);
    mfma_half(K0{});
    mfma_half(K1{});
    __builtin_amdgcn_s_setprio(0);
  }
  DD_STAMP(4);
  bool done = false;
  if constexpr (!GEGLU && WAVES_M == 1 && WAVES_N == 10 && TM == 5 && TN == 2) {
    if (p.ln_out) {                       // whole rows in this workgroup: store out AND LayerNorm(out) (store_tile_ln syncs)
      store_tile_ln<T>(p, acc, block_m0, wave_n, lane, reinterpret_cast<float*>(smem));
      done = true;
    }
  }
  if constexpr (FASTEPI) {
    if (fast) {
      const __amdgpu_buffer_rsrc_t rs_st = __builtin_amdgcn_make_buffer_rsrc(p.out, 0, p.out_bytes, 0x00020000);
      const bool silu = p.act == DD_EPI_SILU;
#pragma unroll
      for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int g8 = 0; g8 < NG; ++g8) {
          float v[8], b[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = acc[g8 * 2 + (e >> 2)][tm][e & 3];
          dd_unpack8<T>(pb[g8], b);
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = (v[e] + b[e]) * p.alpha;
          dd_unpack8<T>(pr[tm][g8], b);
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] += b[e];
          if (silu) {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = dd_silu_f(v[e]);
          }
          if constexpr (PRE_ACC) {
            dd_unpack8<T>(pa[tm][g8], b);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] += b[e];
          }
          __builtin_amdgcn_raw_buffer_store_b128(dd_pack8<T>(v), rs_st, off_o[tm][g8], 0, 0);
        }
      done = true;
    }
  }
  if (!done) store_tile<T, TM, TN, GEGLU>(p, acc, block_m0, block_n0, wave_m, wave_n, lane, p.rows);
  DD_STAMP_FLUSH(p);
}

struct Gemm3 {
  static constexpr Family family = FAM_PIPE;
  static constexpr unsigned needs = 0;
  template <typename T, size_t I, unsigned FORM>
  static int run(const GemmParams& p, const Plan& pl, hipStream_t s) {
    constexpr const TileCfg& t = kTiles[I];
    constexpr size_t smem = (size_t)t.depth * (tile_bm(t) + tile_bn(t)) * BK * sizeof(T);
    static_assert(smem <= 160 * 1024, "LDS");
    constexpr auto kern = dd_gemm3_kernel<T, t.wm, t.wn, t.tm, t.tn, t.depth, FORM == F_GEGLU>;
    return launch_kernel<kern>(dim3(pl.tiles_m * pl.tiles_n, 1, pl.split), 64 * t.wm * t.wn, smem, s, p);
  }
};

}  // namespace
