// Kernel family 1: register-staged software pipeline (dd_gemm_kernel, dd_gemm_pad0_kernel) and its launcher.
#include "gemm_device.h"

namespace {

// PAD_LO: top / left zero padding of the conv gather — output pixel o reads input rows / columns o*stride - PAD_LO + 0..2.
// 1 is nn.Conv2d(padding=1); 0 (stride 2 only) is diffusers' Downsample2D(padding=0), F.pad(x, (0, 1, 0, 1)) then a
// 3x3 / stride 2 / pad 0 conv: its bottom / right pad is the "outside the stored image reads zero" rule every conv has.
// The kernels are thin __global__ wrappers around this body, so the PAD_LO = 1 symbols are the ones of before.
template <typename T, int WAVES_M, int WAVES_N, int TM, int TN, bool CONV, bool GEGLU, int PAD_LO>
__device__ __forceinline__ void gemm1_body(const GemmParams& p) {
  using V8 = typename dd_vec<T>::v8;
  constexpr int NT = 64 * WAVES_M * WAVES_N;
  constexpr int BM = WAVES_M * TM * 16;
  constexpr int BN = WAVES_N * TN * 16;           // weight-tile rows
  constexpr int BN_OUT = GEGLU ? BN / 2 : BN;     // output columns per block
  constexpr int XI = BM * 8 / NT;                 // 16-B chunks per thread, activation tile
  constexpr int WI = BN * 8 / NT;
  static_assert(BM * 8 % NT == 0 && BN * 8 % NT == 0, "tile/threads mismatch");
  static_assert(TN % 2 == 0 && (!GEGLU || TN % 4 == 0), "TN");

  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  T* Xs = reinterpret_cast<T*>(smem);                         // [2][BM][64]
  T* Ws = Xs + 2 * BM * BK;                                   // [2][BN][64]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wave_m = wave / WAVES_N;
  const int wave_n = wave % WAVES_N;

  const int ntiles = p.tiles_m * p.tiles_n;
  const int tile = xcd_remap(blockIdx.x, ntiles);
  const int tile_m = tile / p.tiles_n;
  const int tile_n = tile % p.tiles_n;
  const int block_m0 = tile_m * BM;
  const int block_n0 = tile_n * BN_OUT;

  const int kbeg = blockIdx.z * p.k_per_split;
  const int kend = min(p.k, kbeg + p.k_per_split);
  const int nk = (kend - kbeg + BK - 1) / BK;

  // ---- per-thread loader state --------------------------------------------------------
  const int lchunk = tid & 7;        // which 16-B chunk of the 128-B tile row
  const int lrow0 = tid >> 3;        // first tile row handled by this thread
  constexpr int LROW_STEP = NT / 8;

  // activation rows
  int xm[XI];          // dense: global row (or -1).  conv: instance pixel base (or -1)
  int xiy[XI], xix[XI];
#pragma unroll
  for (int i = 0; i < XI; ++i) {
    const int r = block_m0 + lrow0 + i * LROW_STEP;
    if (r < p.rows) {
      if (CONV) {
        const int hw = p.hout * p.wout;
        const int inst = dd_fdiv(r, p.inv_hw);
        const int rem = r - inst * hw;
        const int oy = dd_fdiv(rem, p.inv_wout);
        const int ox = rem - oy * p.wout;
        xm[i] = inst;
        xiy[i] = oy * p.stride - PAD_LO;
        xix[i] = ox * p.stride - PAD_LO;
      } else {
        xm[i] = r; xiy[i] = 0; xix[i] = 0;
      }
    } else {
      xm[i] = -1; xiy[i] = 0; xix[i] = 0;
    }
  }
  // weight rows (permuted so each lane owns consecutive output channels)
  int64_t wofs[WI];    // element offset of the weight row, or -1
#pragma unroll
  for (int i = 0; i < WI; ++i) {
    const int R = lrow0 + i * LROW_STEP;           // LDS row in weight tile
    const int wv = R / (TN * 16);
    const int rho = R % (TN * 16);
    const int tn = rho >> 4, r = rho & 15;
    int n_glob;
    if (GEGLU) {
      constexpr int TH = TN / 2;
      const int t = tn % TH;
      const int loc = wv * (TH * 16) + (r >> 2) * (4 * TH) + t * 4 + (r & 3);
      const int col = block_n0 + loc;
      n_glob = (col < p.n) ? col + (tn >= TH ? p.n : 0) : -1;
    } else {
      const int loc = wv * (TN * 16) + (r >> 2) * (4 * TN) + tn * 4 + (r & 3);
      const int col = block_n0 + loc;
      n_glob = (col < p.n) ? col : -1;
    }
    wofs[i] = (n_glob >= 0) ? (int64_t)n_glob * p.k : -1;
  }

  u32x4 xreg[XI], wreg[WI];

  auto load_tiles = [&](int kt) {
    const int k = kbeg + kt * BK + lchunk * 8;
    const bool kok = k < kend;
    // weights
#pragma unroll
    for (int i = 0; i < WI; ++i) {
      u32x4 v = {0u, 0u, 0u, 0u};
      if (kok && wofs[i] >= 0) v = dd_ld16(reinterpret_cast<const T*>(p.w) + wofs[i] + k);
      wreg[i] = v;
    }
    // activations
    if (CONV) {
      const int tap = k / p.cin;
      const int ci = k - tap * p.cin;
      const int ky = tap / 3;
      const int kx = tap - ky * 3;
#pragma unroll
      for (int i = 0; i < XI; ++i) {
        u32x4 v = {0u, 0u, 0u, 0u};
        int iy = xiy[i] + ky, ix = xix[i] + kx;
        if (kok && xm[i] >= 0 && iy >= 0 && iy < p.hv && ix >= 0 && ix < p.wv) {
          if (p.upsample) {
            iy = min((int)floorf(iy * p.scale_h), p.hin - 1);
            ix = min((int)floorf(ix * p.scale_w), p.win - 1);
          }
          const int64_t off = (((int64_t)xm[i] * p.hin + iy) * p.win + ix) * p.cin + ci;
          v = dd_ld16(reinterpret_cast<const T*>(p.a) + off);
        }
        xreg[i] = v;
      }
    } else {
      const bool second = k >= p.k1;
#pragma unroll
      for (int i = 0; i < XI; ++i) {
        u32x4 v = {0u, 0u, 0u, 0u};
        if (kok && xm[i] >= 0) {
          const T* src = second
              ? reinterpret_cast<const T*>(p.a2) + (int64_t)xm[i] * p.lda2 + (k - p.k1)
              : reinterpret_cast<const T*>(p.a) + (int64_t)xm[i] * p.lda + k;
          v = dd_ld16(src);
        }
        xreg[i] = v;
      }
    }
  };

  auto store_tiles = [&](int buf) {
    T* xs = Xs + buf * BM * BK;
    T* ws = Ws + buf * BN * BK;
#pragma unroll
    for (int i = 0; i < XI; ++i) {
      const int R = lrow0 + i * LROW_STEP;
      dd_st16(xs + R * BK + ((lchunk ^ ((R >> 1) & 7)) << 3), xreg[i]);
    }
#pragma unroll
    for (int i = 0; i < WI; ++i) {
      const int R = lrow0 + i * LROW_STEP;
      dd_st16(ws + R * BK + ((lchunk ^ ((R >> 1) & 7)) << 3), wreg[i]);
    }
  };

  f32x4 acc[TN][TM];
#pragma unroll
  for (int i = 0; i < TN; ++i)
#pragma unroll
    for (int j = 0; j < TM; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // fragment addressing: LDS row = base + (lane & 15); chunk = (lane >> 4) + 4*ks, swizzled
  const int frow = lane & 15;
  const int fswz = (lane >> 1) & 7;     // == ((row >> 1) & 7) because tile bases are multiples of 16
  const int fchunk = lane >> 4;

  if (nk > 0) {
    load_tiles(0);
    store_tiles(0);
  }
  __syncthreads();

  int buf = 0;
  for (int kt = 0; kt < nk; ++kt) {
    if (kt + 1 < nk) load_tiles(kt + 1);
    const T* xs = Xs + buf * BM * BK + (wave_m * TM * 16 + frow) * BK;
    const T* ws = Ws + buf * BN * BK + (wave_n * TN * 16 + frow) * BK;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int cofs = ((fchunk + 4 * ks) ^ fswz) << 3;
      V8 wf[TN], xf[TM];
#pragma unroll
      for (int i = 0; i < TN; ++i) wf[i] = dd_as_v8<T>(dd_ld16(ws + i * 16 * BK + cofs));
#pragma unroll
      for (int j = 0; j < TM; ++j) xf[j] = dd_as_v8<T>(dd_ld16(xs + j * 16 * BK + cofs));
#pragma unroll
      for (int i = 0; i < TN; ++i)
#pragma unroll
        for (int j = 0; j < TM; ++j) acc[i][j] = dd_mfma16(wf[i], xf[j], acc[i][j]);
    }
    if (kt + 1 < nk) store_tiles(buf ^ 1);
    __syncthreads();
    buf ^= 1;
  }

  store_tile<T, TM, TN, GEGLU>(p, acc, block_m0, block_n0, wave_m, wave_n, lane, p.rows);
}

template <typename T, int WAVES_M, int WAVES_N, int TM, int TN, bool CONV, bool GEGLU>
__global__ __launch_bounds__(64 * WAVES_M * WAVES_N)
void dd_gemm_kernel(const GemmParams p) {
  gemm1_body<T, WAVES_M, WAVES_N, TM, TN, CONV, GEGLU, 1>(p);
}

// conv with PAD_LO = 0 (Downsample2D(padding=0) of the VAE encoder's down blocks)
template <typename T, int WAVES_M, int WAVES_N, int TM, int TN>
__global__ __launch_bounds__(64 * WAVES_M * WAVES_N)
void dd_gemm_pad0_kernel(const GemmParams p) {
  gemm1_body<T, WAVES_M, WAVES_N, TM, TN, true, false, 0>(p);
}

// conv with pad_lo = 0 (dd_gemm_conv_pad): the register-staged tiles only.  The LDS-DMA family keeps its one body: a
// PAD_LO template parameter there (a shared __forceinline__ body behind two __global__ wrappers) changed the register
// allocation of every existing dd_gemm2_kernel instantiation — its kernel-argument loads are rematerialised, not spilled,
// only while the body IS the kernel.  No other family's rows carry F_PAD0, so the planner reports them "unsupported".
template <typename T, size_t I, unsigned FORM>
constexpr auto gemm1_kernel() {
  constexpr const TileCfg& t = kTiles[I];
  if constexpr (FORM == F_PAD0) return dd_gemm_pad0_kernel<T, t.wm, t.wn, t.tm, t.tn>;
  else return dd_gemm_kernel<T, t.wm, t.wn, t.tm, t.tn, FORM == F_CONV, FORM == F_GEGLU>;
}

struct Gemm1 {
  static constexpr Family family = FAM_REG;
  static constexpr unsigned needs = 0;
  template <typename T, size_t I, unsigned FORM>
  static int run(const GemmParams& p, const Plan& pl, hipStream_t s) {
    constexpr const TileCfg& t = kTiles[I];
    constexpr size_t smem = (size_t)2 * (tile_bm(t) + tile_bn(t)) * BK * sizeof(T);
    return launch_kernel<gemm1_kernel<T, I, FORM>()>(dim3(pl.tiles_m * pl.tiles_n, 1, pl.split), 64 * t.wm * t.wn, smem, s, p);
  }
};

}  // namespace

int ddg::launch_gemm1(int dtype, unsigned form, const GemmParams& p, const Plan& pl, hipStream_t s) {
  return dispatch<Gemm1, F_DENSE, F_CONV, F_GEGLU, F_PAD0>(dtype, form, p, pl, s);
}
