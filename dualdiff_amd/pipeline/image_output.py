"""Image output on the GPU: the decoded views as the uint8 frames the reference saves.

What the reference does after `decode_latents` in the run that produces its generated validation set
(perception/data_prepare/val_set_gen.py):

1. `image.cpu().permute(0, 2, 3, 1).float().numpy()` (pipeline/pipeline_bev_controlnet.py:112),
2. diffusers' `numpy_to_pil`, `(images * 255).round().astype("uint8")` (:540, `numpy_to_pil_double` :72-80),
3. per view `torchvision.transforms.Resize(cfg.fid.resize, interpolation=BICUBIC)` and `Pad(cfg.fid.padding)` on the PIL
   image (val_set_gen.py:147-159, applied at :44) — `dataset.back_resize` / `back_pad`, by default 224 x 400 -> 896 x 1600
   and four rows on top (configs/dataset/Nuscenes.yaml:35-36).

Here that is one launch per batch of views (`ops.image_resample_u8`, or `ops.image_quantize_u8` for `raw_output: true`), byte
for byte: PIL resamples 8-bit images in integer arithmetic over fixed-point coefficient tables, and the only floating
point, the construction of those tables, is done here in Python float64 exactly as PIL's C does it in double.

    post = ImagePostProcess.from_config(cfg)              # cfg.fid.resize / cfg.fid.padding / cfg.fid.raw_output
    frames = decode_images(vae, latents, post)            # (b, n_cam, H, W, 3) uint8, on the GPU
    pil = to_pil(frames)                                  # the 2-level list numpy_to_pil_double returns

Writing files, encoding and FID stay with the caller.
"""
import math

import torch

from .. import ops as O

PRECISION_BITS = 32 - 8 - 2            # PIL's fixed point for 8-bit pixels
INTERPOLATIONS = ("bicubic",)

_TABLES = {}                           # (in, out) -> (kk int32 (out, ksize), bounds int32 (out, 2))
_DEVICE_TABLES = {}                    # (in, out, device) -> the same on the device


def _bicubic(x):
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def resample_tables(in_size, out_size):
    """PIL's precompute_coeffs + normalize_coeffs_8bpc for the bicubic filter (src/libImaging/Resample.c), operation for
    operation in float64: -> (kk int32 (out_size, ksize), bounds int32 (out_size, 2) = [xmin, count]).  Output xx is
    `sum_j pixel[xmin + j] * kk[xx, j]` over `count` taps in 22-bit fixed point; kk is zero beyond `count`."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size <= 0 or out_size <= 0:
        raise ValueError("sizes must be positive, got %d -> %d" % (in_size, out_size))
    key = (in_size, out_size)
    if key in _TABLES:
        return _TABLES[key]
    scale = filterscale = in_size / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    rows, bnd = [], []
    one = float(1 << PRECISION_BITS)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = int(center - support + 0.5)
        if xmin < 0:
            xmin = 0
        xmax = int(center + support + 0.5)
        if xmax > in_size:
            xmax = in_size
        xmax -= xmin
        w = []
        ww = 0.0
        for x in range(xmax):
            v = _bicubic((x + xmin - center + 0.5) * ss)
            w.append(v)
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        row = [int(-0.5 + v * one) if v < 0 else int(0.5 + v * one) for v in w]
        rows.append(row + [0] * (ksize - xmax))
        bnd.append((xmin, xmax))
    _TABLES[key] = (torch.tensor(rows, dtype=torch.int32), torch.tensor(bnd, dtype=torch.int32))
    return _TABLES[key]


def device_tables(in_size, out_size, device):
    """The tables of one axis on `device`, cached.  An axis that keeps its size gets the one-tap identity table: PIL skips
    that pass, and since its table there is exactly [0, 1, 0, 0] the bytes are the same."""
    device = torch.device(device)
    key = (int(in_size), int(out_size), device.type, device.index if device.index is not None else torch.cuda.current_device())
    if key not in _DEVICE_TABLES:
        if key[0] == key[1]:
            kk = torch.full((key[0], 1), 1 << PRECISION_BITS, dtype=torch.int32)
            bounds = torch.stack([torch.arange(key[0], dtype=torch.int32), torch.ones(key[0], dtype=torch.int32)], dim=1)
        else:
            kk, bounds = resample_tables(*key[:2])
        _DEVICE_TABLES[key] = (kk.contiguous().to(device), bounds.contiguous().to(device))
    return _DEVICE_TABLES[key]


def _get(cfg, name, default=None):
    if hasattr(cfg, "get"):
        return cfg.get(name, default)
    return getattr(cfg, name, default)


class ImagePostProcess:
    """The reference's `post_trans` (val_set_gen.py:147-159) on GPU tensors: images (b, n, 3, h, w) or (m, 3, h, w) in
    [0, 1] -> uint8 (b, n, H, W, 3) / (m, H, W, 3).  resize = (h, w) or None (`raw_output: true`: quantise only, padding
    is not applied either, as in the reference); padding = torchvision.transforms.Pad's int / pair / (left, top, right,
    bottom)."""

    def __init__(self, resize=None, padding=None, interpolation="bicubic"):
        if str(interpolation).lower() not in INTERPOLATIONS:
            raise ValueError("interpolation %r is not built; available: %s" % (interpolation, ", ".join(INTERPOLATIONS)))
        if resize is not None:
            if isinstance(resize, int):
                raise ValueError("resize must be (h, w); the shorter-edge form of Resize(int) is not built")
            resize = tuple(int(v) for v in resize)
            if len(resize) != 2 or min(resize) <= 0:
                raise ValueError("resize must be a positive (h, w), got %r" % (resize,))
        elif padding is not None:
            raise ValueError("padding without resize: raw output is not padded (val_set_gen.py:147-148)")
        self.resize = resize
        self.padding = O.image_padding(0 if padding is None else padding)

    @classmethod
    def from_config(cls, cfg):
        """cfg: any mapping (or object) with `fid.resize`, `fid.padding`, `fid.raw_output` — the reference's test config."""
        fid = _get(cfg, "fid")
        if fid is None:
            raise ValueError("config has no `fid` section")
        if _get(fid, "raw_output", False):
            return cls()
        resize = _get(fid, "resize")
        if resize is None:
            raise ValueError("config has no fid.resize (and fid.raw_output is false)")
        padding = _get(fid, "padding")
        return cls(resize=list(resize), padding=None if padding is None else (padding if isinstance(padding, int) else list(padding)))

    def __call__(self, images, m11=False):
        if images.dim() not in (4, 5):
            raise ValueError("images must be (b, n, 3, h, w) or (m, 3, h, w), got %s" % (tuple(images.shape),))
        x = images.flatten(0, 1) if images.dim() == 5 else images
        x = x.contiguous()
        if self.resize is None:
            y = O.image_quantize_u8(x, m11=m11)
        else:
            y = O.image_resample_u8(x, self.resize, self.padding, m11=m11)
        return y.view(*images.shape[:2], *y.shape[1:]) if images.dim() == 5 else y


@torch.no_grad()
def decode_images(vae, latents, post=None):
    """latents (b, n_cam, 4, h, w) -> uint8 frames (b, n_cam, H, W, 3) on the GPU: `post(decode_latents(vae, latents))`
    byte for byte, with the decoder's output going straight into the kernel (its `/ 2 + 0.5`, clamp and quantisation
    happen on load; neither the fp32 images nor a uint8 copy at the decoder's size is written)."""
    post = ImagePostProcess() if post is None else post
    b = latents.shape[0]
    img = vae.decode(latents.flatten(0, 1), pre_scale=1.0 / vae.scaling_factor)
    return post(img.view(b, -1, *img.shape[1:]), m11=True)


def to_pil(u8):
    """uint8 frames (b, n, H, W, 3) -> the 2-level list of PIL images `numpy_to_pil_double` returns
    (pipeline_bev_controlnet.py:72-80); (m, H, W, 3) -> a flat list.  The one place that needs PIL."""
    try:
        from PIL import Image
    except ImportError as e:
        raise ImportError("to_pil needs Pillow (PIL), which is not installed; the uint8 frames themselves do not") from e
    if u8.dtype != torch.uint8 or u8.dim() not in (4, 5) or u8.shape[-1] != 3:
        raise ValueError("to_pil takes uint8 frames (b, n, H, W, 3) or (m, H, W, 3), got %s %s" % (tuple(u8.shape), u8.dtype))
    arr = u8.cpu().numpy()
    if arr.ndim == 4:
        return [Image.fromarray(a) for a in arr]
    return [[Image.fromarray(a) for a in scene] for scene in arr]
