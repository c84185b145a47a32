"""Mints tests/golden/png_output.npz: the inputs of the PNG tests (tests/png_cases.py) and, for each, the length of the
file PIL writes by default and with compress_level=0, so that the size conditions hold where PIL is not installed.  Needs
Pillow and the reference's media directory for the two natural crops:

    python -m tests.golden.mint_png <reference>/media

Stored: `in_<name>` (every synthetic case and the two 64 x 96 crops of media/day_object_case.png and
media/day_road_case.png — data only), `pil_<name>` = [default length, compress_level=0 length] (also for "large", the
900 x 1600 frame, whose pixels are generated and pinned by `crc_large`), `pil_version`."""
import io
import os
import sys
import zlib

import numpy as np

from tests import png_cases as C

CROP = {"crop_object": ("day_object_case.png", 200, 250), "crop_road": ("day_road_case.png", 300, 100)}   # file, top, left
CROP_SHAPE = (64, 96)


def pil_lengths(img):
    from PIL import Image
    out = []
    for kw in ({}, {"compress_level": 0}):
        buf = io.BytesIO()
        Image.fromarray(np.asarray(img)).save(buf, "PNG", **kw)
        out.append(len(buf.getvalue()))
    return np.array(out, dtype=np.int64)


def main():
    import PIL
    from PIL import Image
    media, = sys.argv[1:]
    out = {"pil_version": np.array(PIL.__version__)}
    inputs = [(c.name, c.img) for c in C.synthetic()]
    for name, (fname, top, left) in CROP.items():
        full = np.array(Image.open(os.path.join(media, fname)).convert("RGB"))
        assert full.shape[0] >= top + CROP_SHAPE[0] and full.shape[1] >= left + CROP_SHAPE[1], (name, full.shape)
        inputs.append((name, np.ascontiguousarray(full[top:top + CROP_SHAPE[0], left:left + CROP_SHAPE[1]])))
    for name, img in inputs:
        out["in_" + name] = img
        out["pil_" + name] = pil_lengths(img)
    out["pil_large"] = pil_lengths(C.large())
    out["crc_large"] = np.array(zlib.crc32(C.large().tobytes()), dtype=np.int64)
    np.savez_compressed(C.GOLDEN, **out)
    print("wrote %s (PIL %s, %d inputs, %d bytes)" % (C.GOLDEN, PIL.__version__, len(inputs), os.path.getsize(C.GOLDEN)))


if __name__ == "__main__":
    main()
