// VAE encoder posterior: quant_conv + DiagonalGaussianDistribution in one pass over the latent pixels.
//
// diffusers AutoencoderKL.encode ends in  moments = quant_conv(encoder(x))  (1x1, 8 -> 8) and
// DiagonalGaussianDistribution(moments): mean | logvar = chunk(moments, 2), logvar clamped to [-30, 20],
// sample() = mean + exp(0.5 logvar) * noise, mode() = mean.  The reference scales the result by
// vae.config.scaling_factor (runner/base_runner.py:469-475).  Here one thread owns one latent pixel: it reads the
// 8 channels conv_out left in an NHWC row (16 bytes), applies quant_conv, the clamp and the reparameterisation in fp32,
// and writes scale * z as NCHW (m, 4, h, w) — the layout BEVDenoiser.set_inputs(conditional_latents=...) takes.
#include "dd_common.h"

namespace {

template <typename T, typename TO>
__global__ __launch_bounds__(256)
void dd_vae_posterior_kernel(const T* __restrict__ moments, const float* __restrict__ wq, const float* __restrict__ bq,
                             const T* __restrict__ noise, TO* __restrict__ z, int64_t pixels, int32_t hw, float scale) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= pixels) return;
  float x[8];
  dd_unpack8<T>(dd_ld16(moments + i * 8), x);
  float p[8];
#pragma unroll
  for (int o = 0; o < 8; ++o) {                  // quant_conv, in a fixed order: bias, then input channels 0..7
    float acc = bq[o];
#pragma unroll
    for (int c = 0; c < 8; ++c) acc = fmaf(wq[o * 8 + c], x[c], acc);
    p[o] = acc;
  }
  const int64_t inst = i / hw;
  const int64_t pix = i - inst * hw;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    float v = p[c];
    if (noise) {
      const float lv = fminf(fmaxf(p[4 + c], -30.0f), 20.0f);
      const float sd = expf(0.5f * lv);
      v = fmaf(sd, (float)noise[(inst * 4 + c) * hw + pix], v);
    }
    z[(inst * 4 + c) * hw + pix] = (TO)(scale * v);
  }
}

template <typename T>
int launch_posterior(const void* moments, const float* wq, const float* bq, const void* noise, void* z, int64_t pixels,
                     int32_t hw, float scale, int32_t out_f32, hipStream_t s) {
  const dim3 grid((unsigned)((pixels + 255) / 256));
  if (out_f32)
    hipLaunchKernelGGL((dd_vae_posterior_kernel<T, float>), grid, dim3(256), 0, s, (const T*)moments, wq, bq,
                       (const T*)noise, (float*)z, pixels, hw, scale);
  else
    hipLaunchKernelGGL((dd_vae_posterior_kernel<T, T>), grid, dim3(256), 0, s, (const T*)moments, wq, bq,
                       (const T*)noise, (T*)z, pixels, hw, scale);
  return dd_check_launch();
}

}  // namespace

extern "C" int dd_vae_posterior(const void* moments, const float* wq, const float* bq, const void* noise, void* z,
                                int32_t m, int32_t h, int32_t w, float scale, int32_t out_f32, int32_t dtype,
                                dd_stream_t stream) {
  if (!moments || !wq || !bq || !z || m <= 0 || h <= 0 || w <= 0) return DD_ERR_BAD_ARG;
  if (dtype != DD_F16 && dtype != DD_BF16) return DD_ERR_BAD_ARG;
  if (!dd_aligned16(moments)) return DD_ERR_BAD_ARG;
  const int64_t hw = (int64_t)h * w, pixels = (int64_t)m * hw;
  if (hw >= ((int64_t)1 << 31) || (pixels + 255) / 256 >= ((int64_t)1 << 31)) return DD_ERR_UNSUPPORTED;
  dd_clear_error();
  return dd_dispatch16(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    return launch_posterior<T>(moments, wq, bq, noise, z, pixels, (int32_t)hw, scale, out_f32, dd_stream(stream));
  });
}
