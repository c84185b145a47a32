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

The reference then saves every view with `post_trans(img).save(<nuScenes name>.jpg)` and no options (val_set_gen.py:44,
tools/downstream_v3_batched.py:244-252): libjpeg's baseline encoder at quality 75, 4:2:0 chroma, the standard Huffman
tables.  That is integer arithmetic too, and `ops.jpeg_encode_u8` produces the same bytes on the device:

    files = encode_jpeg(frames)                           # the 2-level list of `bytes`, one .jpg file each
    save_jpeg(frames, paths)                              # ... written to `paths` (same nesting), directories created

The way back, .jpg files to uint8 frames, is pipeline/jpeg_input.py.

The reference's demo and validation path saves its results as .png instead (tools/test.py:74-97): the 2 x 3 grids of
the six views that `concat_6_views` builds (runner/img_utils.py:5-40).  PNG is lossless, so the guarantee is not PIL's
bytes (zlib's match search is one sequential chain) but a valid file that decodes to exactly the frame, encoded on the
device in a format of independent 16 KiB chunks (`ops.png_encode_u8`):

    grids = concat_views(frames)                          # (b, 2 H, 3 W, 3): views 0-2 over views 3-5
    files = encode_png(grids)                             # a list of `bytes`, one .png file each
    save_png(grids, paths)

FID stays with the caller.
"""
import os

import torch

from .. import ops as O
from ..image_tables import (JPEG_BASE_CHROMA, JPEG_BASE_LUMA, JPEG_HUFFMAN, JPEG_MODES, JPEG_ZIGZAG,  # noqa: F401
                            PNG_MODES, PRECISION_BITS, device_jpeg_tables, device_tables, jpeg_header, jpeg_quant_tables,
                            jpeg_tables, resample_tables)

INTERPOLATIONS = ("bicubic",)


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


def _jpeg_options(options):
    for name, value in options.items():
        raise ValueError("JPEG option %s=%r is not built; available: %s" % (name, value, JPEG_MODES))


@torch.no_grad()
def encode_jpeg(u8, quality=75, **options):
    """uint8 frames (b, n, H, W, 3) -> the 2-level list of `bytes` (one .jpg file per view, nested as to_pil nests its
    images), (m, H, W, 3) -> a flat list: what `Image.fromarray(frame).save(f, "JPEG", quality=quality)` writes, byte
    for byte, encoded on the GPU.  One readback of the lengths and one copy of the files' bytes; should a file not fit
    the default capacity (header + H * W bytes), the call is repeated once with the capacity the lengths ask for."""
    _jpeg_options(options)
    if u8.dtype != torch.uint8 or u8.dim() not in (4, 5) or u8.shape[-1] != 3:
        raise ValueError("encode_jpeg takes uint8 frames (b, n, H, W, 3) or (m, H, W, 3), got %s %s" % (tuple(u8.shape), u8.dtype))
    frames = (u8.flatten(0, 1) if u8.dim() == 5 else u8).contiguous()
    buf, lengths = O.jpeg_encode_u8(frames, quality)
    n = lengths.cpu().tolist()
    if max(n) > buf.shape[1]:
        buf, lengths = O.jpeg_encode_u8(frames, quality, capacity=max(n))
        n = lengths.cpu().tolist()
    raw = buf[:, :max(n)].cpu().numpy()
    files = [raw[i, :k].tobytes() for i, k in enumerate(n)]
    if u8.dim() == 4:
        return files
    per = u8.shape[1]
    return [files[i * per:(i + 1) * per] for i in range(u8.shape[0])]


def save_jpeg(u8, paths, quality=75, **options):
    """encode_jpeg, each file written to its path: `paths` nested as the frames are ((b, n) names, or m names).  Missing
    directories are created, as the reference's `mkdir -p` does.  Returns the files' sizes, nested the same way."""
    return _save(encode_jpeg(u8, quality, **options), u8, paths, "save_jpeg")


def _save(files, u8, paths, what):
    nested = u8.dim() == 5
    rows = list(zip(files, paths)) if nested else [(files, paths)]
    if len(paths) != len(files) or any(len(p) != len(f) for f, p in rows):
        raise ValueError("%s takes one path per frame, nested as the frames are" % what)
    sizes = []
    for fs, ps in rows:
        for data, path in zip(fs, ps):
            path = os.fspath(path)
            if os.path.dirname(path):
                os.makedirs(os.path.dirname(path), exist_ok=True)
            with open(path, "wb") as f:
                f.write(data)
        sizes.append([len(d) for d in fs])
    return sizes if nested else sizes[0]


def _png_options(options):
    for name, value in options.items():
        raise ValueError("PNG option %s=%r is not built; available: %s" % (name, value, PNG_MODES))


@torch.no_grad()
def encode_png(u8, **options):
    """uint8 frames (b, n, H, W, 3) -> the 2-level list of `bytes` (one .png file per frame, nested as encode_jpeg nests
    its files), (m, H, W, 3) -> a flat list: lossless files that decode to exactly the frames, encoded on the GPU.  One
    readback of the lengths and one copy of the files' bytes; the default capacity holds any content."""
    _png_options(options)
    if u8.dtype != torch.uint8 or u8.dim() not in (4, 5) or u8.shape[-1] != 3 or u8.numel() == 0:
        raise ValueError("encode_png takes uint8 frames (b, n, H, W, 3) or (m, H, W, 3) (%s), got %s %s"
                         % (PNG_MODES, tuple(u8.shape), u8.dtype))
    frames = (u8.flatten(0, 1) if u8.dim() == 5 else u8).contiguous()
    buf, lengths = O.png_encode_u8(frames)
    n = lengths.cpu().tolist()
    raw = buf[:, :max(n)].cpu().numpy()
    files = [raw[i, :k].tobytes() for i, k in enumerate(n)]
    if u8.dim() == 4:
        return files
    per = u8.shape[1]
    return [files[i * per:(i + 1) * per] for i in range(u8.shape[0])]


@torch.no_grad()
def encode_png_rgba(u8):
    """encode_png for RGBA frames, (b, n, H, W, 4) or (m, H, W, 4) uint8 — the transparent box overlays of
    pipeline/box_output.py: colour type 6, otherwise the same format (`ops.png_encode_u8c`).  The files open as mode
    "RGBA" and decode to exactly the frames."""
    if u8.dtype != torch.uint8 or u8.dim() not in (4, 5) or u8.shape[-1] != 4 or u8.numel() == 0:
        raise ValueError("encode_png_rgba takes uint8 frames (b, n, H, W, 4) or (m, H, W, 4), got %s %s" % (tuple(u8.shape), u8.dtype))
    frames = (u8.flatten(0, 1) if u8.dim() == 5 else u8).contiguous()
    buf, lengths = O.png_encode_u8c(frames)
    n = lengths.cpu().tolist()
    raw = buf[:, :max(n)].cpu().numpy()
    files = [raw[i, :k].tobytes() for i, k in enumerate(n)]
    if u8.dim() == 4:
        return files
    per = u8.shape[1]
    return [files[i * per:(i + 1) * per] for i in range(u8.shape[0])]


def save_png_rgba(u8, paths):
    """encode_png_rgba, each file written to its path, as save_png does."""
    return _save(encode_png_rgba(u8), u8, paths, "save_png_rgba")


def save_png(u8, paths, **options):
    """encode_png, each file written to its path: `paths` nested as the frames are ((b, n) names, or m names).  Missing
    directories are created.  Returns the files' sizes, nested the same way."""
    return _save(encode_png(u8, **options), u8, paths, "save_png")


def concat_views(u8, oneline=False):
    """The reference's `concat_6_views` (runner/img_utils.py:5-40) for equal-sized views, on the tensor's device: frames
    (b, 6, H, W, 3) -> (b, 2 H, 3 W, 3), views 0-2 over views 3-5; oneline=True: (b, n, H, W, 3), n >= 2 -> (b, H, n W, 3).
    A last dimension of 4 (the RGBA box overlays) is kept."""
    if u8.dim() != 5 or u8.shape[-1] not in (3, 4):
        raise ValueError("concat_views takes frames (b, n, H, W, 3) or (b, n, H, W, 4), got %s" % (tuple(u8.shape),))
    b, n, h, w, c = u8.shape
    if oneline:
        if n < 2:
            raise ValueError("concat_views(oneline=True) takes at least 2 views, got %d" % n)
        return u8.permute(0, 2, 1, 3, 4).reshape(b, h, n * w, c)
    if n != 6:
        raise ValueError("concat_views takes 6 views for the 2 x 3 grid, got %d (oneline=True takes any n >= 2)" % n)
    return u8.reshape(b, 2, 3, h, w, c).permute(0, 1, 3, 2, 4, 5).reshape(b, 2 * h, 3 * w, c)
