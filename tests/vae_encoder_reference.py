"""CPU restatement of the SD-v1.5 VAE encoder (`AutoencoderKL.encode`) — TEST INFRASTRUCTURE ONLY.

The reference encodes camera images in one form (runner/base_runner.py:469-475, runner/multiview_runner.py:385-391):
`vae.encode(pixel_values).latent_dist.sample() * vae.config.scaling_factor`.

PARITY UNPINNED, as for oracle/vae_decoder.py: neither diffusers 0.17.1 nor the SD-v1.5 weights are available here.
The architecture below is restated from diffusers' published `Encoder` / `DownEncoderBlock2D` / `Downsample2D` /
`DiagonalGaussianDistribution`, with its parameter names (so a real `vae/diffusion_pytorch_model.bin` would load):
  encoder.conv_in 3x3 pad 1 (3 -> 128); four down blocks of two resnets (no time embedding, eps 1e-6, 32 groups) at
  channels (128, 256, 512, 512), the first three ending in Downsample2D(padding=0) = F.pad(x, (0, 1, 0, 1)) + conv 3x3 /
  stride 2 / pad 0; encoder.mid_block as the decoder's; GroupNorm(32, 512, 1e-6) -> SiLU -> conv_out 3x3 pad 1
  (512 -> 8); quant_conv 1x1 (8 -> 8); mean | logvar = chunk(moments, 2), logvar clamped to [-30, 20],
  sample = mean + exp(0.5 logvar) * noise, mode = mean.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle.diffusers_restated import ResnetBlock2D
from oracle.vae_decoder import SCALING_FACTOR, MidBlock


class Downsample2D(nn.Module):
    """diffusers Downsample2D(use_conv=True, padding=0, name="op"): the conv is stored as `conv`."""

    def __init__(self, channels):
        super().__init__()
        self.conv = nn.Conv2d(channels, channels, 3, stride=2, padding=0)

    def forward(self, x):
        return self.conv(F.pad(x, (0, 1, 0, 1), mode="constant", value=0))


class DownEncoderBlock2D(nn.Module):
    def __init__(self, cin, cout, add_downsample, eps, layers=2):
        super().__init__()
        self.resnets = nn.ModuleList([ResnetBlock2D(in_channels=cin if i == 0 else cout, out_channels=cout,
                                                    temb_channels=None, eps=eps) for i in range(layers)])
        self.downsamplers = nn.ModuleList([Downsample2D(cout)]) if add_downsample else None

    def forward(self, x):
        for r in self.resnets:
            x = r(x, None)
        if self.downsamplers is not None:
            x = self.downsamplers[0](x)
        return x


class Encoder(nn.Module):
    def __init__(self, block_out_channels=(128, 256, 512, 512), in_channels=3, latent_channels=4, eps=1e-6):
        super().__init__()
        self.conv_in = nn.Conv2d(in_channels, block_out_channels[0], 3, padding=1)
        blocks, prev = [], block_out_channels[0]
        for i, c in enumerate(block_out_channels):
            blocks.append(DownEncoderBlock2D(prev, c, add_downsample=i != len(block_out_channels) - 1, eps=eps))
            prev = c
        self.down_blocks = nn.ModuleList(blocks)
        self.mid_block = MidBlock(block_out_channels[-1], eps)
        self.conv_norm_out = nn.GroupNorm(32, block_out_channels[-1], eps=eps)
        self.conv_out = nn.Conv2d(block_out_channels[-1], 2 * latent_channels, 3, padding=1)

    def forward(self, x):
        x = self.conv_in(x)
        for b in self.down_blocks:
            x = b(x)
        x = self.mid_block(x)
        return self.conv_out(F.silu(self.conv_norm_out(x)))


def posterior(moments, noise=None):
    """DiagonalGaussianDistribution(moments).sample() with the given noise, or .mode() when noise is None."""
    mean, logvar = torch.chunk(moments, 2, dim=1)
    if noise is None:
        return mean
    logvar = torch.clamp(logvar, -30.0, 20.0)
    return mean + torch.exp(0.5 * logvar) * noise


class AutoencoderKLEncoder(nn.Module):
    """The encode half of AutoencoderKL: moments = quant_conv(encoder(x))."""

    def __init__(self, block_out_channels=(128, 256, 512, 512), latent_channels=4):
        super().__init__()
        self.encoder = Encoder(block_out_channels, latent_channels=latent_channels)
        self.quant_conv = nn.Conv2d(2 * latent_channels, 2 * latent_channels, 1)

    def forward(self, x):
        return self.quant_conv(self.encoder(x))

    def encode(self, x, noise=None):
        """Unscaled latents: the posterior's sample with `noise`, or its mode."""
        return posterior(self(x), noise)


def encode_pixel_values(vae, pixel_values, noise=None):
    """runner/base_runner.py:469-475: (b, n, 3, H, W) -> scaling_factor * latents (b, n, 4, H/8, W/8)."""
    b, n = pixel_values.shape[:2]
    lat = vae.encode(pixel_values.flatten(0, 1), noise) * SCALING_FACTOR
    return lat.view(b, n, *lat.shape[1:])
