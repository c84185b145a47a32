"""VAE encode on the HIP path — camera images to the clean latents given-view sampling holds.

The reference turns images into latents in one form only (runner/base_runner.py:469-475, runner/multiview_runner.py:385-391):
`vae.encode(pixel_values).latent_dist.sample() * vae.config.scaling_factor`, with pixel_values in [-1, 1]
(configs/dataset/Nuscenes.yaml:152-153).  `AutoencoderKLEncoder` carries diffusers 0.17.1's parameter names for the
encode half of `AutoencoderKL` (`encoder.conv_in`, `encoder.down_blocks.*`, `encoder.mid_block.*`,
`encoder.conv_norm_out`, `encoder.conv_out`, `quant_conv`), so the stock SD-v1.5 `vae/diffusion_pytorch_model.bin` loads
with `load_state_dict(strict=False)` (the decoder keys are simply unused, as the encoder keys are for
`AutoencoderKLDecoder`).

Everything runs on the denoising path's kernels plus two pieces:
  * Downsample2D(padding=0) of the first three down blocks — F.pad(x, (0, 1, 0, 1)) then a 3x3 / stride 2 / pad 0 conv —
    is `ops.conv3x3(..., pad=0)` (dd_gemm_conv_pad: the implicit-GEMM gather with its origin at 2o instead of 2o - 1);
  * quant_conv and DiagonalGaussianDistribution (mean | logvar split, logvar clamp, mean + exp(0.5 logvar) * noise, the
    scaling factor) are one launch over the latent pixels (`ops.vae_posterior`, dd_vae_posterior) that reads conv_out's
    NHWC rows and writes NCHW latents.
The resnets and the mid block (with its 512-wide single-head attention) are vae_decoder.py's.
"""
import torch
import torch.nn as nn

from .. import ops as O
from .layers import Conv3x3, GroupNorm, Linear, derived
from .vae_decoder import SCALING_FACTOR, VaeMidBlock, VaeResnetBlock2D


def randn_tensor(shape, generator=None, device=None, dtype=None):
    """diffusers 0.17.1 `utils.randn_tensor`: a CPU generator draws on the CPU and the result moves to `device`; a list
    of generators draws one batch entry from each."""
    rand_device = device
    if generator is not None:
        gen_type = generator.device.type if not isinstance(generator, list) else generator[0].device.type
        if gen_type != device.type and gen_type == "cpu":
            rand_device = "cpu"
        elif gen_type != device.type and gen_type == "cuda":
            raise ValueError("Cannot generate a %s tensor from a generator of type %s." % (device, gen_type))
    if isinstance(generator, list):
        one = (1,) + tuple(shape[1:])
        lat = [torch.randn(one, generator=generator[i], device=rand_device, dtype=dtype) for i in range(shape[0])]
        return torch.cat(lat, dim=0).to(device)
    return torch.randn(shape, generator=generator, device=rand_device, dtype=dtype).to(device)


class Downsample2D(nn.Module):
    """diffusers Downsample2D(use_conv=True, padding=0): F.pad(x, (0, 1, 0, 1)) + conv 3x3 / stride 2 / pad 0."""

    def __init__(self, channels):
        super().__init__()
        self.conv = Conv3x3(channels, channels, stride=2)

    def run(self, x, m, h, w):
        c = self.conv
        y = O.conv3x3(x, c.packed, c.bias, m, h, w, stride=2, pad=0)
        return y, (h - 2) // 2 + 1, (w - 2) // 2 + 1


class DownEncoderBlock2D(nn.Module):
    def __init__(self, cin, cout, add_downsample, eps, layers=2):
        super().__init__()
        self.resnets = nn.ModuleList([VaeResnetBlock2D(cin if i == 0 else cout, cout, eps=eps) for i in range(layers)])
        self.downsamplers = nn.ModuleList([Downsample2D(cout)]) if add_downsample else None

    def run(self, x, m, h, w):
        for r in self.resnets:
            x = r.run(x, m, h, w)
        if self.downsamplers is not None:
            x, h, w = self.downsamplers[0].run(x, m, h, w)
        return x, h, w


class Encoder(nn.Module):
    def __init__(self, block_out_channels=(128, 256, 512, 512), in_channels=3, latent_channels=4, eps=1e-6):
        super().__init__()
        self.conv_in = Conv3x3(in_channels, block_out_channels[0])
        blocks, prev = [], block_out_channels[0]
        for i, c in enumerate(block_out_channels):
            blocks.append(DownEncoderBlock2D(prev, c, add_downsample=i != len(block_out_channels) - 1, eps=eps))
            prev = c
        self.down_blocks = nn.ModuleList(blocks)
        self.mid_block = VaeMidBlock(block_out_channels[-1], eps)
        self.conv_norm_out = GroupNorm(32, block_out_channels[-1], eps)
        self.conv_out = Conv3x3(block_out_channels[-1], 2 * latent_channels)       # double_z: mean | logvar


class DiagonalGaussian:
    """`latent_dist` of `AutoencoderKLEncoder.encode`: diffusers' DiagonalGaussianDistribution over the moments conv_out
    wrote (quant_conv not applied yet: the posterior launch does it).  sample() / mode() return unscaled (m, 4, h, w)
    latents in the model dtype, as diffusers does."""

    def __init__(self, vae, moments, m, h, w):
        self.vae, self.moments, self.m, self.h, self.w = vae, moments, m, h, w

    def latents(self, generator=None, sample=True, scale=1.0, out_f32=False):
        noise = None
        if sample:
            noise = randn_tensor((self.m, 4, self.h, self.w), generator=generator, device=self.moments.device,
                                 dtype=self.moments.dtype)
        wq, bq = self.vae._q()
        return O.vae_posterior(self.moments, wq, bq, self.m, self.h, self.w, noise=noise, scale=scale, out_f32=out_f32)

    def sample(self, generator=None):
        return self.latents(generator, True)

    def mode(self):
        return self.latents(None, False)


class EncoderOutput:
    def __init__(self, latent_dist):
        self.latent_dist = latent_dist


class AutoencoderKLEncoder(nn.Module):
    def __init__(self, block_out_channels=(128, 256, 512, 512), latent_channels=4, scaling_factor=SCALING_FACTOR):
        super().__init__()
        if latent_channels != 4:
            raise ValueError("the posterior kernel takes 2 x 4 moment channels")
        self.encoder = Encoder(block_out_channels, latent_channels=latent_channels)
        self.quant_conv = Linear(2 * latent_channels, 2 * latent_channels, conv=True)
        self.scaling_factor = scaling_factor

    @property
    def dtype(self):
        return self.encoder.conv_in.weight.dtype

    def _q(self):
        """quant_conv as the posterior kernel reads it: fp32 (8, 8) weight and (8,) bias."""
        q = self.quant_conv
        return derived(q, "q32", [q.weight, q.bias], lambda: (q.weight.detach().reshape(8, 8).float().contiguous(),
                                                              q.bias.detach().float().contiguous()))

    @torch.no_grad()
    def encode(self, x):
        """x: (m, 3, H, W) images in [-1, 1] on the GPU, H and W multiples of 8 -> EncoderOutput with `.latent_dist`."""
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError("encode takes (m, 3, H, W) images, got %s" % (tuple(x.shape),))
        m, _, h, w = x.shape
        if h % 8 or w % 8:
            raise ValueError("image height and width must be multiples of 8, got %d x %d" % (h, w))
        if not x.is_cuda:
            raise RuntimeError("the VAE encoder runs on the GPU only")
        x8 = O.nchw_to_nhwc(x.to(self.dtype).contiguous(), 8)          # (m*h*w, 8), channels 3..7 zero
        return self.encode_nhwc8(x8, m, h, w)

    @torch.no_grad()
    def encode_nhwc8(self, x8, m, h, w):
        """The encoder behind `nchw_to_nhwc(x, 8)`: x8 (m*h*w, 8) channels-last rows in the model dtype, channels 3..7
        zero — what `ops.image_load_u8(..., layout="nhwc8")` writes — -> EncoderOutput."""
        if x8.dim() != 2 or tuple(x8.shape) != (m * h * w, 8) or x8.dtype != self.dtype or not x8.is_contiguous():
            raise ValueError("encode_nhwc8 takes a contiguous (%d, 8) %s tensor, got %s %s"
                             % (m * h * w, self.dtype, tuple(x8.shape), x8.dtype))
        if h % 8 or w % 8:
            raise ValueError("image height and width must be multiples of 8, got %d x %d" % (h, w))
        if not x8.is_cuda:
            raise RuntimeError("the VAE encoder runs on the GPU only")
        enc = self.encoder
        x = enc.conv_in.run(x8, m, h, w)
        for blk in enc.down_blocks:
            x, h, w = blk.run(x, m, h, w)
        x = enc.mid_block.run(x, m, h, w)
        x = enc.conv_norm_out.run(x, m, h * w, True)
        moments = enc.conv_out.run(x, m, h, w)                          # (m*h*w, 8) NHWC rows
        return EncoderOutput(DiagonalGaussian(self, moments, m, h, w))


@torch.no_grad()
def encode_pixel_values(vae: AutoencoderKLEncoder, pixel_values, generator=None, sample_posterior=True, given=None):
    """runner/base_runner.py:469-475 on the GPU: pixel_values (b, n, 3, H, W) in [-1, 1] -> latents (b, n, 4, H/8, W/8)
    fp32, `latent_dist.sample() * scaling_factor` (or the mode with sample_posterior=False).

    given: optional (b, n) bool — only those view-instances are encoded, the other entries are zero; the result and
    `given` go to BEVDenoiser.set_inputs(..., conditional_latents=lat, conditional_mask=given) as they are."""
    if pixel_values.dim() != 5 or pixel_values.shape[2] != 3:
        raise ValueError("pixel_values must be (b, n, 3, H, W), got %s" % (tuple(pixel_values.shape),))
    if not pixel_values.is_floating_point():
        raise ValueError("pixel_values must be a float tensor, got %s" % pixel_values.dtype)
    b, n, _, hh, ww = pixel_values.shape
    if hh % 8 or ww % 8:
        raise ValueError("image height and width must be multiples of 8, got %d x %d" % (hh, ww))
    if given is not None and (tuple(given.shape) != (b, n) or given.dtype != torch.bool):
        raise ValueError("given must be a (%d, %d) bool tensor" % (b, n))
    if not pixel_values.is_cuda:
        raise RuntimeError("the VAE encoder runs on the GPU only")
    x = pixel_values.flatten(0, 1)
    idx = None
    if given is not None:
        idx = given.reshape(-1).nonzero().flatten().to(x.device)
        x = x.index_select(0, idx)
    out = torch.zeros((b * n, 4, hh // 8, ww // 8), dtype=torch.float32, device=pixel_values.device)
    if x.shape[0] > 0:
        dist = vae.encode(x.to(vae.dtype)).latent_dist
        lat = dist.latents(generator, sample_posterior, scale=vae.scaling_factor, out_f32=True)
        if idx is None:
            out = lat
        else:
            out.index_copy_(0, idx, lat)
    return out.view(b, n, 4, hh // 8, ww // 8)
