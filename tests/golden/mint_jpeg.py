"""Mints tests/golden/jpeg_output.npz: the bytes PIL's `Image.fromarray(a).save(buf, "JPEG", quality=q)` writes for small
seeded frames, so that the numpy restatement (tests/jpeg_reference.py) and the GPU encoder stay pinned to PIL's bytes
where PIL is not installed.  Needs Pillow:  python -m tests.golden.mint_jpeg

The shapes are the edge cases of the encoder's geometry, the contents the code paths of its entropy coder; main()
asserts that the paths the cases are there for do occur."""
import io
import os

import numpy as np

from tests import jpeg_reference as J

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "jpeg_output.npz")

# (H, W) -> contents at quality 75
SHAPES = (
    ((1, 1), ("uniform",)),                              # single block / single MCU
    ((8, 8), ("uniform",)),
    ((16, 16), ("saturated",)),
    ((9, 17), ("uniform", "smooth")),                    # both dummy kinds at once
    ((17, 31), ("saturated", "lone")),
    ((24, 40), ("uniform", "smooth")),                   # bottom dummy row only
    ((40, 24), ("uniform", "flat")),                     # right dummy column only
    ((20, 32), ("uniform", "saturated", "lone")),        # 900 x 1600 in small: H mod 16 = 4
    ((37, 53), ("uniform", "smooth")),                   # edges on both axes
    ((45, 80), ("uniform", "lone")),                     # odd H
    ((90, 160), ("smooth", "lone")),                     # chroma row replication
    ((57, 100), ("saturated", "uniform")),
)
QUALITIES = (1, 50, 95, 100)                             # ... of these shapes, uniform noise
QUALITY_SHAPES = ((20, 32), (37, 53), (57, 100))
TILE_SHAPES = ((37, 53), (20, 32))                       # 16-pixel tiles of 0 / 255 at quality 100


def content(kind, h, w, seed):
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "uniform":
        return rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
    if kind == "saturated":                              # many 0xFF bytes, the largest coefficients
        return (rs.randint(0, 2, (h, w, 3)) * 255).astype(np.uint8)
    if kind == "flat":                                   # DC difference 0 throughout
        return np.full((h, w, 3), 128, dtype=np.uint8)
    if kind == "tiles":                                  # DC differences of size 11 at quality 100
        return np.repeat((((yy // 16 + xx // 16) % 2) * 255).astype(np.uint8)[..., None], 3, axis=2)
    smooth = np.stack([40 + 150 * yy / max(h - 1, 1), 60 + 120 * xx / max(w - 1, 1),
                       200 - 90 * (yy + xx) / max(h + w - 2, 1)], axis=-1)
    if kind == "smooth":                                 # EOB-heavy
        return np.round(smooth).astype(np.uint8)
    if kind == "lone":
        # a faint pattern at the pixel rate on a flat field: 8 x 8 blocks in turn get a checkerboard, alternating rows
        # or alternating columns, i.e. one high-frequency coefficient behind a long run of zeros
        which = (yy // 8 + 2 * (xx // 8)) % 4
        sign = np.select([which == 0, which == 1, which == 2], [(yy + xx) % 2, yy % 2, xx % 2], 0) * 2 - 1
        amp = np.select([which == 0, which == 1, which == 2], [60, 40, 40], 0)
        base = np.array([120, 130, 110]) + 0 * smooth
        return np.clip(np.round(base + (amp * sign)[..., None]), 0, 255).astype(np.uint8)
    raise ValueError(kind)


def cases():
    """-> (name, quality, frame)"""
    seed = 500
    for (h, w), kinds in SHAPES:
        for kind in kinds:
            seed += 1
            yield "%dx%d_%s_q75" % (h, w, kind), 75, content(kind, h, w, seed)
    for h, w in QUALITY_SHAPES:
        for q in QUALITIES:
            seed += 1
            yield "%dx%d_uniform_q%d" % (h, w, q), q, content("uniform", h, w, seed)
    for h, w in TILE_SHAPES:
        yield "%dx%d_tiles_q100" % (h, w), 100, content("tiles", h, w, 0)


def shape_cases(h, w, quality=75):
    return [c for c in cases() if c[2].shape[:2] == (h, w) and c[1] == quality]


def main():
    import PIL
    from PIL import Image
    out = {"pil_version": np.array(PIL.__version__)}
    stats, stuffed = {}, 0
    for name, q, img in cases():
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, "JPEG", quality=q)
        data = buf.getvalue()
        out["in_" + name] = img
        out["out_" + name] = np.frombuffer(data, dtype=np.uint8)
        assert J.encode(img, q, stats) == data, name
        stuffed += data[len(J.header(img.shape[0], img.shape[1], q)):].count(b"\xff\x00")
    assert stuffed > 0, "no FF 00 pair in any scan"
    assert stats["zrl"] >= {1, 2, 3}, stats["zrl"]
    assert stats["dc_sizes"] == set(range(12)), stats["dc_sizes"]
    np.savez_compressed(PATH, **out)
    print("wrote %s (PIL %s, %d cases, %d bytes; %d stuffed bytes, ZRL runs %s, DC sizes %s)"
          % (PATH, PIL.__version__, (len(out) - 1) // 2, os.path.getsize(PATH), stuffed, sorted(stats["zrl"]),
             sorted(stats["dc_sizes"])))


if __name__ == "__main__":
    main()
