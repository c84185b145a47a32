"""Mints tests/golden/png_input.npz: the .png files a real encoder wrote, and PIL's pixels for them, so that the PNG input
tests pin PIL's result where PIL is not installed.  Needs Pillow:

    python -m tests.golden.mint_png_input

Stored: `file_<name>` (the bytes PIL's `.save` wrote) and `pix_<name>` (`np.asarray(Image.open(file).convert("RGB"))`) for
the two 64 x 96 crops of tests/golden/png_output.npz (`in_crop_object`, `in_crop_road`) and for `panorama`, a 12 x 60 RGBA
flat-colour image of six views with non-opaque alpha in places — what the image-mode ORS condition looks like in small;
`pil_version`."""
import io
import os

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "png_input.npz")
OUTPUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "png_output.npz")
NAMES = ("crop_object", "crop_road", "panorama")
PANORAMA_HW, VIEWS = (12, 60), 6


def panorama():
    """(12, 60, 4) uint8: per view a few flat patches of class colours, alpha 255 but for a band of 0 and a patch of 128"""
    rs = np.random.RandomState(1260)
    h, w = PANORAMA_HW
    img = np.zeros((h, w, 4), dtype=np.uint8)
    img[..., 3] = 255
    colours = rs.randint(0, 256, (8, 3)).astype(np.uint8)
    for v in range(VIEWS):
        x0 = v * (w // VIEWS)
        img[:, x0:x0 + 10, :3] = colours[v % 8]
        img[3:8, x0 + 2:x0 + 7, :3] = colours[(v + 3) % 8]
        img[9:, x0 + 5:x0 + 10, :3] = colours[(v + 5) % 8]
    img[:2, :, 3] = 0
    img[5:9, 20:33, 3] = 128
    return img


def load():
    return np.load(PATH)


def files(z=None):
    """[(name, file bytes, PIL's pixels)]"""
    z = load() if z is None else z
    return [(n, z["file_" + n].tobytes(), z["pix_" + n]) for n in NAMES]


def main():
    import PIL
    from PIL import Image
    src = np.load(OUTPUT)
    inputs = {"crop_object": src["in_crop_object"], "crop_road": src["in_crop_road"], "panorama": panorama()}
    out = {"pil_version": np.array(PIL.__version__)}
    for name, img in inputs.items():
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, "PNG")
        data = buf.getvalue()
        pix = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
        assert np.array_equal(pix, img[..., :3])
        out["file_" + name] = np.frombuffer(data, dtype=np.uint8)
        out["pix_" + name] = pix
    np.savez_compressed(PATH, **out)
    size = os.path.getsize(PATH)
    assert size < 100 * 1000, size
    print("wrote %s (PIL %s, %d bytes)" % (PATH, PIL.__version__, size))


if __name__ == "__main__":
    main()
