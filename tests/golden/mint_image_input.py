"""Mints tests/golden/image_input.npz: PIL's own `Image.resize((w, h)).crop(box)` (the default filter for RGB: bicubic) on
the cases of tests/image_input_reference.py (seeded uniform and 0/255 noise), so that the restatement stays pinned to
PIL's bytes where PIL is not installed.  The inputs are not stored, only their CRC-32 (a drift of the generator then
shows as an input mismatch, not as a resample error).  Needs Pillow:  python -m tests.golden.mint_image_input"""
import os
import zlib

import numpy as np

from tests import image_input_reference as RI

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "image_input.npz")


def cases():
    for name, hw, size, box in RI.CASES:
        for kind in RI.KINDS:
            yield "%s_%s" % (name, kind.replace("/", "_")), size, box, RI.frame(name, hw, kind)[0]


def pil_crop(img, size, box):
    from PIL import Image
    return np.asarray(Image.fromarray(img).resize((size[1], size[0])).crop(box))


def main():
    import PIL
    out = {"pil_version": np.array(PIL.__version__)}
    for name, size, box, img in cases():
        out["crc_" + name] = np.array(zlib.crc32(img.tobytes()), dtype=np.uint32)
        out["out_" + name] = pil_crop(img, size, box)
    np.savez_compressed(PATH, **out)
    print("wrote %s (PIL %s, %d cases, %d bytes)" % (PATH, PIL.__version__, (len(out) - 1) // 2, os.path.getsize(PATH)))


if __name__ == "__main__":
    main()
