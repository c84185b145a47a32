#include "gemm_device.h"

namespace {

// =============================================================================================
// Kernel family 3: direct 3x3 convolution for SMALL images (14x25 and deeper: H*W <= 384).
// The implicit-GEMM kernels stage the activation tile once per TAP (9 x per 64 input channels); at
// the deep levels (336 / 1092 rows x 1280 channels x 29-59 MB of weights) that makes the kernel
// bytes-in-flight bound.  Here a workgroup owns G whole instances (G*H*W <= BM rows): per 64-channel
// chunk the RAW pixels of its instances are DMA'd into LDS once, and the 9 taps are 9 different
// per-lane LDS row gathers (a padding tap points at a row the range check filled with zeros).
// Staged bytes drop ~5x; the weight matrix is streamed once per row tile through a 3-slot ring.
// Requirements (host-checked): stride 1, no resize, Cin % 64 == 0.  Split-K is over channel chunks.
// =============================================================================================
// BAND = true: images LARGER than the tile (the 28x50 level).  A workgroup owns a band of p.band_rows consecutive output
// pixels (whole image rows) of one instance; its slab holds those pixels plus a halo of W + 1 pixels on either side, so
// the activation is still staged once per 64-channel chunk (the implicit-GEMM kernels stage it once per tap).  LDS rows
// 0..15 are the zero rows, slab pixel s sits in row 16 + s; halo pixels outside the image are out-of-range DMAs = zeros.
// (C3_MFMA / C3_BARRIER / C3_SEG / dd_dbg::C3_*: hooks of tools/conv3s_bound.sh's diagnostic builds, dd_debug.h)
template <typename T, int WAVES_M, int WAVES_N, int TM, int TN, int NSW, int GRP = 1, bool BAND = false>
__global__ __launch_bounds__(64 * WAVES_M * WAVES_N)
void dd_conv3s_kernel(const GemmParams p) {
  // GRP = 3: the weight ring is two GROUPS of three taps; a workgroup synchronises (DMA wait + barrier)
  // once per group instead of once per tap — 72 MFMAs per wave between barriers instead of 24 — and the
  // next group's three weight tiles are in flight under them.
  static_assert(GRP == 1 || (GRP == 3 && NSW == 6), "grouped taps: 2 groups of 3 slots");
  using V8 = typename dd_vec<T>::v8;
  constexpr int NW = WAVES_M * WAVES_N;
  constexpr int BM = WAVES_M * TM * 16;
  constexpr int BN = WAVES_N * TN * 16;
  constexpr int AROWS = BAND ? BM + 88 : BM + 64;   // rows >= BM are never valid pixels -> always zeros (BAND: see above)
  // LOADER waves: in the staggered 8-wave tiles only the early half (waves 0-3) issues LDS-DMAs — an LDS-DMA blocks the
  // issuing wave for 60-185 cycles while the texture path is busy, and the early waves have that time: they cannot start
  // their MFMAs before the late waves' block has left the matrix pipe.  The late waves never wait on vmcnt; the barrier
  // behind the loaders' counted wait publishes the data.  (Round 5; all waves loading, each blocked ~220 cycles per step
  // at the same time with the matrix pipe idle, cost 18 % of the step: profiles/r05_conv3s_segments.txt.)
  constexpr int NL = (NW == 8 && GRP == 1) ? NW / 2 : NW;
  constexpr int XA = (AROWS / 8 + NL - 1) / NL;     // activation DMA pieces per loader wave per chunk
  constexpr int XPT = (XA + 3) / 4;                 // ... issued over taps 0..3, XPT per tap (GRP == 1)
  constexpr int WI = BN / 8 / NL;              // weight DMA pieces per loader wave per (chunk, tap) step
  // NSW weight ring slots: the weights are cold (HBM, 2-3 us) while a (chunk, tap) step lasts
  // ~0.3 us, so the ring is as deep as LDS allows
  static_assert((BAND ? AROWS % 8 == 0 : AROWS % (8 * NL) == 0) && BN % (8 * NL) == 0 && NW % 2 == 0, "tile/waves mismatch");
  static_assert(TN % 2 == 0, "TN");
  static_assert(NSW >= 3 && NSW <= 10 && (NSW - 2) * WI + XA <= 63 && 9 - (NSW - 1) >= 4, "ring depth / vmcnt");

  DD_STAMP_DECL();
  DD_STAMP(0);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  T* abuf = reinterpret_cast<T*>(smem);                 // [2][AROWS][64]
  T* wring = abuf + 2 * AROWS * BK;                     // [NSW][BN][64]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wave_m = wave / WAVES_N;
  const int wave_n = wave % WAVES_N;

  // row tiles of ONE weight slice are neighbours in the remapped order -> same XCD, same L2: at these levels the
  // weight matrix (29-59 MB) is the big operand and each slice is wanted by every row tile (activations: 1-3 MB)
  const int tile = xcd_remap(blockIdx.x, p.tiles_m * p.tiles_n);
  // (the other order — column tiles of one row band as neighbours — was measured in round 5: -0.7 % for all direct convs, neutral
  //  for the band form alone)
  const int tile_n = tile / p.tiles_m;
  const int tile_m = tile % p.tiles_m;
  const int hw = p.hout * p.wout;
  const int m_inst = dd_fdiv(p.rows, p.inv_hw);
  int g0_, ng_, vrows_, row0_, band0_ = 0;
  if constexpr (BAND) {
    g0_ = dd_fdiv(tile_m, p.inv_bands);                 // instance
    band0_ = (tile_m - g0_ * p.bands) * p.band_rows;    // first pixel of the band inside the instance
    ng_ = 1;
    vrows_ = min(p.band_rows, hw - band0_);
    row0_ = g0_ * hw + band0_;
  } else {
    g0_ = tile_m * p.g_per_tile;
    ng_ = min(p.g_per_tile, m_inst - g0_);
    vrows_ = ng_ * hw;
    row0_ = g0_ * hw;
  }
  const int g0 = g0_, ng = ng_;
  const int vrows = vrows_;                             // valid rows of this tile
  const int row0 = row0_;                               // first global output row
  const int band0 = band0_;
  (void)ng; (void)g0;
  const int block_n0 = tile_n * BN;

  const int nchunks = p.cin / BK;
  const int c_beg = blockIdx.z * p.chunks_per_split;
  const int nc = min(nchunks, c_beg + p.chunks_per_split) - c_beg;
  const int nsteps = nc * 9;

  const int lrow = lane >> 3;
  const int lc = (lane & 7) ^ ((((wave & 1) << 2) + (lane >> 4)) & 7);
  const uint32_t lcb = (uint32_t)lc * 16u;

  // The activation slab is swizzled by ROW & 7 (the weight ring by (row >> 1) & 7 like the GEMM family): the tap
  // gathers read 16 consecutive slab rows starting at ANY row (r + dy*W + dx), and ds_read_b128's lane groups
  // ({0-3, 12-15} at chunk c, {4-11} at chunk c+1) are conflict-free for every such window only when the 8
  // rows of a group get 8 different chunk positions whatever the window's parity — (row >> 1) & 7 does that
  // for even shifts only (2-way conflicts on every odd tap: 34-39 % of the LDS cycles measured).
  const uint32_t lcb_a = (uint32_t)((lane & 7) ^ (lane >> 3)) * 16u;
  // ---- DMA tables -----------------------------------------------------------------------
  uint32_t av[XA];                                      // activation rows of the tile (raw pixels)
  int adst[XA];                                         // BAND: LDS row of the piece (surplus pieces rewrite the zero rows)
#pragma unroll
  for (int j = 0; j < XA; ++j) {
    if constexpr (BAND) {
      const int pc = j * NL + wave;                     // 8-row piece of the slab buffer (loader waves only)
      const bool real = pc < AROWS / 8;
      const int L = (real ? pc : 0) * 8 + lrow;         // LDS row
      const int sidx = L - 16;                          // slab pixel index
      const int pix = band0 - (p.wout + 1) + sidx;      // pixel inside the instance
      const bool ok = real && sidx >= 0 && sidx < vrows + 2 * (p.wout + 1) && pix >= 0 && pix < hw;
      av[j] = ok ? (uint32_t)(g0 * hw + pix) * (uint32_t)p.cin * 2u + lcb_a : DD_OOB;
      adst[j] = (real ? pc : 0) * 8;
    } else {
      const int r = (j * NL + wave) * 8 + lrow;
      av[j] = r < vrows ? (uint32_t)(row0 + r) * (uint32_t)p.cin * 2u + lcb_a : DD_OOB;
      adst[j] = (j * NL + wave) * 8;
    }
  }
  uint32_t wv[WI];                                      // weight rows, permuted like dd_gemm2_kernel
#pragma unroll
  for (int j = 0; j < WI; ++j) {
    const int R = (j * NL + wave) * 8 + lrow;
    const int wvi = R / (TN * 16);
    const int rho = R % (TN * 16);
    const int tn = rho >> 4, r = rho & 15;
    const int col = block_n0 + wvi * (TN * 16) + (r >> 2) * (4 * TN) + tn * 4 + (r & 3);
    wv[j] = col < p.n ? (uint32_t)col * (uint32_t)p.k * 2u + lcb : DD_OOB;
  }
  const __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.w), 0, p.w_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_a = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.a), 0, p.a_bytes, 0x00020000);

  auto issue_a = [&](int c, const int j0, const int j1) __attribute__((always_inline)) {   // chunk c (local index) -> abuf[c & 1], pieces [j0, j1)
    T* dst = abuf + (c & 1) * AROWS * BK;
    const uint32_t so = (uint32_t)((c_beg + c) * BK) * 2u;
#pragma unroll
    for (int j = 0; j < XA; ++j)
      if (j >= j0 && j < j1) bdma16(rs_a, av[j], so, dst + adst[j] * BK);
  };
  auto issue_w = [&](int c, int t, int slot) __attribute__((always_inline)) {
    T* dst = wring + slot * BN * BK;
    const uint32_t so = (uint32_t)(t * p.cin + (c_beg + c) * BK) * 2u;
#pragma unroll
    for (int j = 0; j < WI; ++j) bdma16(rs_w, wv[j], so, dst + (j * NL + wave) * 8 * BK);
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
  const bool loader = wave < NL;
  if (nc > 0 && loader) {
    issue_a(0, 0, XA);
#pragma unroll
    for (int s0 = 0; s0 < (GRP == 1 ? NSW - 1 : NSW); ++s0)
      if (s0 < nsteps) issue_w(s0 / 9, s0 % 9, s0);
  }
  DD_STAMP(2);
  // (built AFTER the prologue DMAs are in flight: ~60 entries x ~20 VALU instructions took 3.7 us of a 36 us
  //  kernel in front of the first load; now they run under the 2-3 us the cold weights need to arrive)
  // ---- per-lane tap tables: LDS row of the pixel each tap reads (BM = the zero row), 2 x 16 bit
  uint32_t tab[TM][5];
  // (entries are ABSOLUTE LDS addresses of pixel buffer 0 so that a gather is v_bfe_u32 + ds_read with the buffer as an
  //  immediate offset; the dynamic LDS of this kernel starts at 0, and a build that moved it past the 16 bits traps)
  const uint32_t lds_base = (uint32_t)(uintptr_t)((__attribute__((address_space(3))) unsigned char*)smem);
  if (lds_base + AROWS * BK * sizeof(T) > 65536u) __builtin_trap();
  // Branch-free (bit selects on 0 / ~0 masks): written with `if`s the compiler emitted 120 exec-mask regions for
  // the 60 entries and the build took 6 200 cycles of a 69 000-cycle kernel (tools/conv3s_stamps.py).
#pragma unroll
  for (int tm = 0; tm < TM; ++tm) {
    const int r = wave_m * (TM * 16) + tm * 16 + (lane & 15);
    const bool rv = r < vrows;
    const int rr = rv ? r : 0;
    const int g = BAND ? 0 : dd_fdiv(rr, p.inv_hw);
    const int rem = BAND ? band0 + rr : rr - g * hw;    // pixel inside its instance
    const int y = dd_fdiv(rem, p.inv_wout);
    const int x = rem - y * p.wout;
    const uint32_t mrv = 0u - (uint32_t)rv;
    const uint32_t my[3] = {mrv & (0u - (uint32_t)(y >= 1)), mrv, mrv & (0u - (uint32_t)(y + 1 < p.hout))};
    const uint32_t mx[3] = {0u - (uint32_t)(x >= 1), ~0u, 0u - (uint32_t)(x + 1 < p.wout)};
#pragma unroll
    for (int t2 = 0; t2 < 5; ++t2) {
      uint32_t packed = 0;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int t = t2 * 2 + h;
        // A valid tap reads slab row r + dy*W + dx (= g*hw + iy*W + ix).  A padding tap reads one of the 16 zero rows
        // BM .. BM+15, the one with the residue mod 16 the real pixel would have had: the 16 lanes of an MFMA row
        // block keep DISTINCT rows mod 16, which is what keeps ds_read_b128 conflict-free under the row & 7
        // swizzle (one shared zero row cost 34-39 % of the LDS cycles in bank conflicts at the 4x7 / 7x13 levels,
        // where a third of all taps are padding)
        // BAND: slab pixel s sits in LDS row 16 + s and output row r is slab pixel r + W + 1; zero rows are 0..15
        const uint32_t lin = (uint32_t)(r + (BAND ? 16 + p.wout + 1 : 0) + (t < 9 ? (t / 3 - 1) * p.wout + (t % 3 - 1) : 0));
        const uint32_t pad = (BAND ? 0u : (uint32_t)BM) | (lin & 15u);   // BM is a multiple of 16
        const uint32_t ok = t < 9 ? (my[t < 9 ? t / 3 : 0] & mx[t < 9 ? t % 3 : 0]) : 0u;
        uint32_t ra = (lin & ok) | (pad & ~ok);
        // the entry is the fragment's BYTE offset inside the pixel buffer: (row * 8 + swizzled chunk of k-step 0) * 16
        // (k-step 1 is the same address with bit 2 of the chunk flipped: ^ 64); AROWS * 128 < 2^16, so one v_bfe_u32
        // yields the ds_read address
        ra = (((ra << 3) | ((uint32_t)(lane >> 4) ^ (ra & 7u))) << 4) + lds_base;
        packed |= ra << (16 * h);
      }
      tab[tm][t2] = packed;
    }
  }
  int wslot = 0;                                        // ring slot of step s (scalar)
  C3_SEG_DECL();
  // One (chunk, tap) step of a wave is 24 MFMAs (~410 cycles of matrix pipe), 16 fragment reads and 1.9 LDS-DMA
  // issues (an LDS-DMA blocks the issuing wave for 100-130 cycles).  Rounds 2-4 ran them as three blocks in series per
  // wave and relied on the partner wave of the SIMD to fill the holes: 1235 cycles per step for 768 of MFMA, both waves
  // issuing their DMAs at the same time with the matrix pipe idle (tools/conv3s_stamps.py segment clocks,
  // profiles/r05_conv3s_segments.txt).  Round 5:
  //  * the activation fragments of a wave's NEXT MFMA block are gathered INSIDE the current one, output-row block j at a
  //    time, into the registers the four MFMAs of block j have just read (two ds_read_b128 per MFMA gap are nearly
  //    free: MI355X_MICROARCH.md "Issued between MFMAs"; hence the j-major MFMA order) — ONE fragment buffer, not two;
  //  * STAGGER (8-wave tiles): waves 4-7 ("late") run the MFMAs of step s-1 at the HEAD of step s, waves 0-3 ("early")
  //    those of step s at its tail, so the two waves of a SIMD alternate on the matrix pipe behind one barrier per step
  //    (MI355X_MICROARCH.md, "Two waves per SIMD");  early: weight fragments, DMA, MFMAs + gathers of step s+1;
  //    late: MFMAs + gathers of step s, DMA, weight fragments — the two DMA windows are disjoint and each lies under the
  //    other wave's MFMAs.  The role is a COMPILE-TIME parameter of the loop (two copies of it): as a run-time branch
  //    inside every step it cost in-place accumulation and 800 spilled registers.
  // Same arithmetic in the same order per accumulator as before -> bit-identical results.
  V8 xf[2][TM];                                         // [k half][output-row block]
  V8 wf[2][TN];
  const bool late = NW == 8 && GRP == 1 && wave >= NL;
  static_assert(AROWS * BK * sizeof(T) <= 65535, "16-bit gather addresses / immediate offset of buffer 1");
  auto gather_j = [&](auto buf_c, auto tap_c, const int j) __attribute__((always_inline)) {
    constexpr int t = decltype(tap_c)::value;
    constexpr uint32_t BOFF = decltype(buf_c)::value * (AROWS * BK * sizeof(T));
    using LP = const __attribute__((address_space(3))) u32x4*;
    // (volatile: the extraction stays HERE — hoisted, the 54 gather addresses of a chunk cost more registers than the
    //  kernel has, and the spill reloads wait on vmcnt(0), i.e. on the whole weight ring)
    uint32_t a0;
    asm volatile("v_bfe_u32 %0, %1, %2, 16" : "=v"(a0) : "v"(tab[j][t >> 1]), "n"(16 * (t & 1)));
    xf[0][j] = dd_as_v8<T>(*(LP)(uintptr_t)(a0 + BOFF));
    xf[1][j] = dd_as_v8<T>(*(LP)(uintptr_t)((a0 ^ 64u) + BOFF));
  };
  auto step = [&](const int c, auto tap_c, auto buf_c, auto late_c) __attribute__((always_inline)) {
    constexpr int t = decltype(tap_c)::value;
    constexpr int BUF = decltype(buf_c)::value;         // = c & 1: the pixel buffer of this chunk (chunk loop unrolled by two)
    constexpr bool LATE = decltype(late_c)::value;
    const bool more_c = c + 1 < nc;
    const int s = c * 9 + t;
    // This step's DMAs (GRP == 1, loader waves): at taps 0..3 a quarter of the next chunk's pixels, then W(s + NSW - 1)
    // into the slot step s - 1 read.  Per-wave issue order (A pieces, then W) is what the counted waits below assume.
    int dslot_ = wslot + NSW - 1;
    if (dslot_ >= NSW) dslot_ -= NSW;
    const int dslot = dslot_;
    auto step_dma = [&]() __attribute__((always_inline)) {
      if constexpr (GRP == 1 && !dd_dbg::C3_NODMA) {
        if (t < 4 && more_c) issue_a(c + 1, t * XPT, (t + 1) * XPT);
        if (s + NSW - 1 < nsteps) {
          constexpr int ta = (t + NSW - 1) % 9, ca = (t + NSW - 1) / 9;
          issue_w(c + ca, ta, dslot);
        }
      }
    };
    if constexpr (GRP == 1) {
    // W(s) (and with it, in issue order, everything older) must have landed.  Younger loads that may stay in flight:
    // W(s+1..s+NSW-2) and the pixel pieces issued in the NSW-2 steps before this one (taps 0..3 of THIS chunk only:
    // the previous chunk's last taps issue none).  The last NSW-2 steps simply drain.  A(c+1) is complete at step
    // (c, 8), whose MFMA block gathers from it: its last piece went out at tap 3 <= 8 - (NSW - 1).
    if constexpr (!LATE && !dd_dbg::C3_NOWAIT) {
      constexpr int ta0 = t - (NSW - 2) > 0 ? t - (NSW - 2) : 0, ta1 = t - 1 < 3 ? t - 1 : 3;      // taps [ta0, ta1]
      constexpr int j0 = ta0 * XPT < XA ? ta0 * XPT : XA, j1 = (ta1 + 1) * XPT < XA ? (ta1 + 1) * XPT : XA;
      constexpr int NA = ta1 >= ta0 && j1 > j0 ? j1 - j0 : 0;
      if (s + NSW - 2 < nsteps) {
        if (NA > 0 && more_c) wait_vmcnt<(NSW - 2) * WI + NA>();
        else wait_vmcnt<(NSW - 2) * WI>();
      } else {
        wait_vmcnt<0>();
      }
    }
    C3_SEG(0);
    C3_BARRIER();
    C3_SEG(1);
    } else if constexpr (t % GRP == 0) {
      // group start: this group's taps (issued one group ago; the first two groups in the prologue) must
      // have landed; only at the very first group may the second group still be in flight
      if (s == 0 && GRP < nsteps) wait_vmcnt<GRP * WI>();
      else wait_vmcnt<0>();
      C3_BARRIER();              // everyone is done with the previous group's slots
      if (t == 0 && more_c) issue_a(c + 1, 0, XA);
      if (s >= GRP && s + GRP < nsteps) {        // next group into the slots just freed
        int slot = wslot + GRP;
        if (slot >= NSW) slot -= NSW;
        constexpr int t1 = (t + GRP) % 9, c1 = (t + GRP) / 9;
#pragma unroll
        for (int u = 0; u < GRP; ++u) issue_w(c + c1, t1 + u, slot + u);
      }
    }
    const T* ws = wring + wslot * BN * BK + (wave_n * TN * 16 + frow) * BK;
    if (++wslot == NSW) wslot = 0;
    auto wread = [&]() __attribute__((always_inline)) {
      if (dd_dbg::C3_NOWREAD && s != 0) return;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const int cofs = ((fchunk + 4 * ks) ^ fswz) << 3;
#pragma unroll
        for (int i = 0; i < TN; ++i) wf[ks][i] = dd_as_v8<T>(dd_ld16(ws + i * 16 * BK + cofs));
      }
    };
    auto mfma_j = [&](const int j) __attribute__((always_inline)) {
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int i = 0; i < TN; ++i) acc[i][j] = C3_MFMA(wf[ks][i], xf[ks][j], acc[i][j]);
    };
    if constexpr (LATE) {
      // head: the MFMAs of step s-1; block j's registers are refilled with THIS step's fragments as soon as it is done
      if (s > 0) {
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int j = 0; j < TM; ++j) {
          mfma_j(j);
          if constexpr (!dd_dbg::C3_NOGATHER) gather_j(buf_c, tap_c, j);
          __builtin_amdgcn_sched_barrier(0);
        }
        __builtin_amdgcn_s_setprio(0);
      } else {
#pragma unroll
        for (int j = 0; j < TM; ++j) gather_j(buf_c, tap_c, j);
      }
      C3_SEG(2);
      C3_SEG(3);
      wread();
      // the weight slot and the pixel buffer these reads touch are refilled by the loader waves right after the next barrier
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    } else {
      C3_SEG(2);
      wread();
      if (s == 0) {                                   // first step only: nothing was gathered under a previous block
#pragma unroll
        for (int j = 0; j < TM; ++j) gather_j(std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{}, j);
      }
      __builtin_amdgcn_sched_barrier(0);
      step_dma();
      C3_SEG(3);
      __builtin_amdgcn_sched_barrier(0);
      // the MFMAs of step s; block j's registers are refilled with the fragments of step s+1 (same resident chunk; at
      // t == 8 the next chunk, landed since step NSW-1)
      const bool have_next = t < 8 || more_c;
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int j = 0; j < TM; ++j) {
        mfma_j(j);
        if constexpr (!dd_dbg::C3_NOGATHER)
          if (have_next) gather_j(std::integral_constant<int, (t < 8 ? BUF : BUF ^ 1)>{}, std::integral_constant<int, (t + 1) % 9>{}, j);
        __builtin_amdgcn_sched_barrier(0);
      }
      __builtin_amdgcn_s_setprio(0);
    }
    C3_SEG(4);
  };
  auto chunk = [&](const int c, auto buf_c, auto late_c) __attribute__((always_inline)) {
    step(c, std::integral_constant<int, 0>{}, buf_c, late_c);
    step(c, std::integral_constant<int, 1>{}, buf_c, late_c);
    step(c, std::integral_constant<int, 2>{}, buf_c, late_c);
    step(c, std::integral_constant<int, 3>{}, buf_c, late_c);
    step(c, std::integral_constant<int, 4>{}, buf_c, late_c);
    step(c, std::integral_constant<int, 5>{}, buf_c, late_c);
    step(c, std::integral_constant<int, 6>{}, buf_c, late_c);
    step(c, std::integral_constant<int, 7>{}, buf_c, late_c);
    step(c, std::integral_constant<int, 8>{}, buf_c, late_c);
  };
  auto main_loop = [&](auto late_c) __attribute__((always_inline)) {
    for (int c = 0; c < nc; c += 2) {
      chunk(c, std::integral_constant<int, 0>{}, late_c);
      DD_STAMP_IF(c == 0, 3);                                        // after the first 9 steps
      if (c + 1 < nc) chunk(c + 1, std::integral_constant<int, 1>{}, late_c);
    }
  };
  if constexpr (NW == 8 && GRP == 1) {
    if (late) main_loop(std::true_type{});
    else main_loop(std::false_type{});
  } else {
    main_loop(std::false_type{});
  }
  DD_STAMP(4);
  if (late && nsteps > 0) {                               // staggered waves: the last step's MFMAs are still due
#pragma unroll
    for (int j = 0; j < TM; ++j)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int i = 0; i < TN; ++i) acc[i][j] = C3_MFMA(wf[ks][i], xf[ks][j], acc[i][j]);
  }
  // rows past the tile's instances are padding
  store_tile<T, TM, TN, false>(p, acc, row0, block_n0, wave_m, wave_n, lane, min(p.rows, row0 + vrows));
  DD_STAMP_FLUSH(p);
  C3_SEG_FLUSH(p, wave, lane, nsteps);
}

struct Conv3s {
  static constexpr Family family = FAM_DIRECT;
  static constexpr unsigned needs = 0;
  template <typename T, size_t I, unsigned FORM>
  static int run(const GemmParams& p, const Plan& pl, hipStream_t s) {
    constexpr const TileCfg& t = kTiles[I];
    constexpr size_t smem = (size_t)(2 * (tile_bm(t) + (t.band ? 88 : 64)) + t.depth * tile_bn(t)) * BK * sizeof(T);
    static_assert(smem <= 160 * 1024 - 64, "LDS");
    constexpr auto kern = dd_conv3s_kernel<T, t.wm, t.wn, t.tm, t.tn, t.depth, t.grp, t.band>;
    return launch_kernel<kern>(dim3(pl.tiles_m * pl.tiles_n, 1, pl.split), 64 * t.wm * t.wn, smem, s, p);
  }
};

}  // namespace

int ddg::launch_conv3s(int dtype, unsigned form, const GemmParams& p, const Plan& pl, hipStream_t s) {
  return dispatch<Conv3s, F_CONV>(dtype, form, p, pl, s);
}
