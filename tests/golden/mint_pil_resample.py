"""Mints tests/golden/pil_resample.npz: PIL's own `Image.resize(..., BICUBIC)` on the small cases of
tests/pil_resample_reference.py (seeded uniform and 0/255 noise), so that the numpy restatement stays pinned to PIL's
bytes where PIL is not installed.  Needs Pillow:  python -m tests.golden.mint_pil_resample"""
import os

import numpy as np

from tests import pil_resample_reference as R

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "pil_resample.npz")
KINDS = ("uniform", "0/255")


def cases():
    for i, ((h, w), (oh, ow)) in enumerate(R.SMALL_SHAPES):
        for j, kind in enumerate(KINDS):
            yield "%dx%d_%dx%d_%s" % (h, w, oh, ow, kind.replace("/", "_")), (oh, ow), R.noise_u8((h, w, 3), kind, 100 + 10 * i + j)


def main():
    import PIL
    from PIL import Image
    out = {"pil_version": np.array(PIL.__version__)}
    for name, (oh, ow), img in cases():
        out["in_" + name] = img
        out["out_" + name] = np.asarray(Image.fromarray(img).resize((ow, oh), Image.BICUBIC))
    np.savez_compressed(PATH, **out)
    print("wrote %s (PIL %s, %d cases, %d bytes)" % (PATH, PIL.__version__, (len(out) - 1) // 2, os.path.getsize(PATH)))


if __name__ == "__main__":
    main()
