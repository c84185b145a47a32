"""numpy restatement of what the reference does to a decoded image before it saves it: diffusers' numpy_to_pil
quantisation, PIL's `Image.resize(..., BICUBIC)` on 8-bit pixels (src/libImaging/Resample.c: precompute_coeffs,
normalize_coeffs_8bpc, ImagingResampleHorizontal_8bpc / Vertical_8bpc) and torchvision's Pad.

Written from PIL's algorithm, independent of dualdiff_amd: tests/test_image_output_cpu.py pins it to PIL itself (where
PIL is installed) and to tests/golden/pil_resample.npz; the GPU tests compare the kernels with it byte for byte."""
import math

import numpy as np

PB = 22                                  # PRECISION_BITS = 32 - 8 - 2


def _cubic(x, a=-0.5):
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


_COEFFS = {}


def coeffs(in_size, out_size):
    """-> (kk int32 (out, ksize), bounds int32 (out, 2) = [xmin, count]) of one axis, in Python float64."""
    key = (in_size, out_size)
    if key in _COEFFS:
        return _COEFFS[key]
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    kk = np.zeros((out_size, ksize), dtype=np.int32)
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    for xx in range(out_size):
        c = (xx + 0.5) * scale
        xmin = max(int(c - support + 0.5), 0)
        n = min(int(c + support + 0.5), in_size) - xmin
        w = [_cubic((x + xmin - c + 0.5) * ss) for x in range(n)]
        tot = 0.0
        for v in w:
            tot += v
        for x in range(n):
            v = w[x] / tot if tot != 0.0 else w[x]
            kk[xx, x] = int(v * (1 << PB) - 0.5) if v < 0 else int(v * (1 << PB) + 0.5)
        bounds[xx] = (xmin, n)
    _COEFFS[key] = (kk, bounds)
    return _COEFFS[key]


def pass1d(img, kk, bounds, axis):
    """One pass along `axis` of a uint8 array: clip8(((1 << 21) + sum_j px[xmin + j] * kk[xx, j]) >> 22), rounded and
    clipped to uint8 as PIL does after EACH pass."""
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((kk.shape[0],) + src.shape[1:], dtype=np.uint8)
    for xx in range(kk.shape[0]):
        xmin, n = int(bounds[xx, 0]), int(bounds[xx, 1])
        k = kk[xx, :n].astype(np.int64).reshape((n,) + (1,) * (src.ndim - 1))
        acc = (1 << (PB - 1)) + (src[xmin:xmin + n] * k).sum(axis=0)
        out[xx] = np.clip(acc >> PB, 0, 255).astype(np.uint8)
    return np.moveaxis(out, 0, axis)


def resize(img, size):
    """img (h, w, c) uint8, size = (oh, ow) -> (oh, ow, c): the horizontal pass, then the vertical one; an axis that keeps
    its size is skipped (ImagingResample's need_horizontal / need_vertical)."""
    oh, ow = size
    h, w = img.shape[:2]
    if ow != w:
        img = pass1d(img, *coeffs(w, ow), axis=1)
    if oh != h:
        img = pass1d(img, *coeffs(h, oh), axis=0)
    return img


def pad(img, padding, fill=0):
    """torchvision.transforms.Pad on (h, w, c): padding = (left, top, right, bottom), constant fill."""
    left, top, right, bottom = padding
    h, w, c = img.shape
    out = np.full((top + h + bottom, left + w + right, c), fill, dtype=np.uint8)
    out[top:top + h, left:left + w] = img
    return out


def quantize(x, m11=False):
    """float32 array -> uint8: diffusers' numpy_to_pil, `(x * 255).round().astype("uint8")`, behind the [0, 1] clamp of
    decode_latents; m11: x is in [-1, 1] and goes through decode_latents' `(x / 2 + 0.5).clamp(0, 1)` in fp32 first."""
    x = np.asarray(x, dtype=np.float32)
    if m11:
        x = x / np.float32(2) + np.float32(0.5)
    x = np.clip(x, np.float32(0), np.float32(1))
    return (x * np.float32(255)).round().astype(np.uint8)


def frames(x, size=None, padding=(0, 0, 0, 0), fill=0, m11=False):
    """NCHW float images (m, 3, h, w) -> (m, H, W, 3) uint8 frames: quantize, then resize + pad per image if size is given."""
    q = quantize(np.transpose(np.asarray(x, dtype=np.float32), (0, 2, 3, 1)), m11)
    if size is None:
        return q
    return np.stack([pad(resize(im, size), padding, fill) for im in q])


# (h, w) -> (oh, ow) of the small cases: up in both axes, down in both (ksize 11 / 11), each axis alone kept, a tiny source
# whose every window is clipped by the border, and the production 4x ratio over several tiles
SMALL_SHAPES = [((8, 12), (19, 31)), ((16, 20), (7, 9)), ((9, 13), (9, 29)), ((5, 7), (23, 7)), ((3, 2), (11, 9)),
                ((24, 40), (96, 160))]
# dataset.back_resize of the reference's four configurations: (h, w) -> (oh, ow), pad (left, top, right, bottom)
PRODUCTION = [((224, 400), (896, 1600), (0, 4, 0, 0)), ((256, 704), (533, 1466), (67, 367, 67, 0)),
              ((432, 768), (900, 1600), (0, 0, 0, 0)), ((192, 384), (800, 1600), (0, 100, 0, 0))]


def noise_u8(shape, kind, seed):
    """Seeded uint8 test images: 'uniform' noise or '0/255' noise (every overshoot clips, at both ends and between the
    passes)."""
    rng = np.random.RandomState(seed)
    if kind == "uniform":
        return rng.randint(0, 256, size=shape).astype(np.uint8)
    return (rng.randint(0, 2, size=shape) * 255).astype(np.uint8)
