"""The image-mode ORS condition with a resize (`crop_drivewm`, dataset/utils.py:355-358, 374-388) restated twice.

`restatement` is the definition of the feature's arithmetic in numpy: per view a zero pad on top, a bilinear resize without
antialias at half-pixel centres, and a crop, every operation rounded to float32 and every fused multiply-add a real one
(`fma32`: the product and the sum exact, one rounding).  `torch_crop_drivewm` is the reference's own sequence of torch calls,
with switches for the faults the tests plant.  Neither imports the package under test.
"""
import numpy as np

F32 = np.float32

# (views, h, w of one view, pad_top, resize, top, left, size): the reference's geometry, then small ones that keep resized row 0 (the
# pad's side and value), crop on both axes, upscale, and keep every size
TRUE = (6, 224, 400, 1, (216, 384), 24, 0, (192, 384))
GEOMETRIES = (
    TRUE,
    (3, 9, 16, 1, (8, 14), 0, 0, (8, 14)),
    (3, 9, 16, 1, (8, 14), 2, 1, (5, 11)),
    (2, 3, 7, 2, (7, 9), 0, 0, (7, 9)),
    (6, 28, 50, 1, (27, 48), 3, 0, (24, 48)),
    (1, 5, 5, 0, (5, 5), 1, 1, (3, 3)),
)
IDENTITY = GEOMETRIES[5]
BOUND = 2.0 ** -21


def geometry_id(g):
    return "v%d_%dx%d_pad%d_to%dx%d_at%d_%d_%dx%d" % (g[0], g[1], g[2], g[3], g[4][0], g[4][1], g[5], g[6], g[7][0], g[7][1])


def fma32(a, b, c):
    """float32(a * b + c) with one rounding, for float32 arrays.  The product of two float32 is exact in float64; the sum
    is taken in float64 with its rounding error (Knuth's TwoSum) and, where it is inexact and its last bit even, moved to
    the odd neighbour on the error's side — rounding to odd at 53 bits, after which the rounding to 24 is the correct one."""
    a, b, c = (np.asarray(v, dtype=F32).astype(np.float64) for v in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    fix = (err != 0) & even
    s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(F32)


def axis_tables(n_in, n_out):
    """(i0, i1 int64, lam0, lam1 float32), each (n_out,): the two taps of every output position and their weights"""
    scale = F32(n_in) / F32(n_out)
    dst = np.arange(n_out, dtype=F32) + F32(0.5)
    src = fma32(np.full(n_out, scale, dtype=F32), dst, np.full(n_out, -0.5, dtype=F32))
    src = np.where(src < 0, F32(0), src).astype(F32)
    i0 = src.astype(np.int64)
    i1 = i0 + (i0 < n_in - 1)
    lam1 = np.clip((src - i0.astype(F32)).astype(F32), F32(0), F32(1)).astype(F32)
    lam0 = (F32(1) - lam1).astype(F32)
    return i0, i1, lam0, lam1


def restatement(frames, views, pad_top, resize, top, left, size):
    """uint8 (b, h, w, 3) -> float32 (b, 3, oh, views * ow)"""
    frames = np.asarray(frames)
    b, h, w, _ = frames.shape
    pw = w // views
    (rh, rw), (oh, ow) = resize, size
    x = frames.astype(F32) / F32(255)                                    # ToTensor
    x = x.transpose(0, 3, 1, 2).reshape(b, 3, h, views, pw)
    x = np.concatenate([np.zeros((b, 3, pad_top, views, pw), dtype=F32), x], axis=2)    # pad_top
    y0, y1, a0, a1 = (t[top:top + oh] for t in axis_tables(h + pad_top, rh))
    x0, x1, b0, b1 = (t[left:left + ow] for t in axis_tables(pw, rw))
    b0, b1 = b0[None, None, None, None, :], b1[None, None, None, None, :]
    a0, a1 = a0[None, None, :, None, None], a1[None, None, :, None, None]
    r0, r1 = x[:, :, y0], x[:, :, y1]                                    # (b, 3, oh, views, pw)
    t = fma32(b0, r0[..., x0], (b1 * r0[..., x1]).astype(F32))
    u = fma32(b0, r1[..., x0], (b1 * r1[..., x1]).astype(F32))
    out = fma32(a0, t, (a1 * u).astype(F32))
    return out.reshape(b, 3, oh, views * ow)


def torch_crop_drivewm(frames, views, pad_top, resize, top, left, size, fault=None):
    """The reference's calls: per view pad_top, Resize (F.interpolate bilinear, align_corners=False, no antialias: the
    reference's torchvision 0.11.3 on a tensor), the crop, cat.  fault: None, or one planted mistake out of FAULTS."""
    import torch
    import torch.nn.functional as TF
    x = torch.tensor(np.asarray(frames)).permute(0, 3, 1, 2).float().div(255)        # a copy: the caller's may be read-only
    b, _, h, w = x.shape
    pw = w // views
    (rh, rw), (oh, ow) = resize, size

    def pad(v):
        out = torch.zeros(b, 3, h + pad_top, v.shape[-1])
        if fault == "pad_bottom":
            out[..., :h, :] = v
        else:
            out[..., pad_top:, :] = v
        return out

    def resized(v, width):
        return TF.interpolate(v, size=(rh, width), mode="bilinear", align_corners=fault == "align_corners",
                              antialias=fault == "antialias")

    def rows(v):
        return v[..., :oh, :] if fault == "crop_bottom" else v[..., top:top + oh, :]
    if fault == "whole_panorama":
        y = rows(resized(pad(x), views * rw))
        return torch.cat([y[..., v * rw + left:v * rw + left + ow] for v in range(views)], dim=-1).numpy()
    parts = [rows(resized(pad(x[..., v * pw:(v + 1) * pw]), rw))[..., left:left + ow] for v in range(views)]
    return torch.cat(parts, dim=-1).numpy()


FAULTS = ("whole_panorama", "pad_bottom", "align_corners", "antialias", "crop_bottom")


def random_frames(g, b, seed):
    """b panoramas of g's views: uint8 (b, h, views * w, 3)"""
    return np.random.RandomState(seed).randint(0, 256, (b, g[1], g[0] * g[2], 3)).astype(np.uint8)
