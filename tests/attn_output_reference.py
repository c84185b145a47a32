"""The reference's attention-map pictures restated on the host (tools/explore_attn.py:114-151 and view_images :25-53), for
the tests of dualdiff_amd/pipeline/attn_output.py.  Built on matplotlib's own `cmap(...)` and PIL's own `resize`; np.float64
stands where the reference has the removed `np.float`; there is no `putText` (the label strip stays white unless strips
are handed in).  matplotlib is imported when a colour is first asked for, so that the layout arithmetic needs none."""
import functools

import numpy as np


@functools.lru_cache(maxsize=None)
def colormap(name="coolwarm"):
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    return plt.get_cmap(name)


def normalise(column, hw):
    """:118-122: one context column (h * w,) float32 -> (h, w, 1) float64 in [0, 1]; 0 / 0 = NaN for a constant column."""
    image = np.asarray(column).reshape(hw[0], hw[1], -1).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (image - image.min()) / (image.max() - image.min())


def colour_loop(image, cmap=None):
    """:123-128, as the reference has it: one `cmap(...)` call per pixel -> (h, w, 3) uint8."""
    cmap = colormap() if cmap is None else cmap
    coloured = np.zeros((image.shape[0], image.shape[1], 4), dtype=np.float64)
    for j in range(image.shape[0]):
        for k in range(image.shape[1]):
            coloured[j, k] = cmap(image[j, k])
    return (coloured[:, :, :3] * 255).astype(np.uint8)


def colour(image, cmap=None):
    """The same bytes with one `cmap(...)` call per tile (matplotlib's __call__ is elementwise): what the GPU tests use,
    tests/test_attn_output_cpu.py holds it against colour_loop."""
    cmap = colormap() if cmap is None else cmap
    return (cmap(image[:, :, 0])[:, :, :3] * 255).astype(np.uint8)


def colour_by_table(image, table):
    """The formula the kernel implements: index min(int(X * 256), 255) into a (256, 3) byte table, black for NaN."""
    x = image[:, :, 0]
    with np.errstate(invalid="ignore"):
        k = np.minimum((x * 256.0).astype(np.int64), 255)
    k = np.where(np.isnan(x), 256, k)
    full = np.concatenate([np.asarray(table, dtype=np.uint8), np.zeros((1, 3), dtype=np.uint8)])
    return full[k]


def resized(rgb, size):
    """:129: PIL's default resize (bicubic) to size = (height, width)."""
    from PIL import Image
    return np.array(Image.fromarray(rgb).resize((size[1], size[0])))


def with_strip(image, label_ratio=.2, strip=None):
    """text_under_image (:13-23) without the text: `int(h * .2)` white rows below the tile, or the given strip."""
    h, w, c = image.shape
    offset = int(h * label_ratio)
    img = np.ones((h + offset, w, c), dtype=np.uint8) * 255
    img[:h] = image
    if strip is not None:
        img[h:] = strip
    return img


def layout(n, num_rows):
    """view_images' counts (:27-40) -> (num_empty, num_items, num_cols)."""
    num_empty = n % num_rows
    num_items = n + num_empty
    return num_empty, num_items, num_items // num_rows


def view_images(images, num_rows=1, offset_ratio=0.02):
    """:25-53 for an (N, h, w, 3) stack -> the sheet."""
    num_empty, num_items, num_cols = layout(images.shape[0], num_rows)
    empty = np.ones(images[0].shape, dtype=np.uint8) * 255
    images = [im.astype(np.uint8) for im in images] + [empty] * num_empty
    h, w, c = images[0].shape
    offset = int(h * offset_ratio)
    sheet = np.ones((h * num_rows + offset * (num_rows - 1), w * num_cols + offset * (num_cols - 1), 3), dtype=np.uint8) * 255
    for i in range(num_rows):
        for j in range(num_cols):
            sheet[i * (h + offset): i * (h + offset) + h, j * (w + offset): j * (w + offset) + w] = images[i * num_cols + j]
    return sheet


@functools.lru_cache(maxsize=None)
def _tile(key, hw, size):
    return resized(colour(normalise(np.frombuffer(key, dtype=np.float32), hw)), size)


def tile(column, hw, size):
    """The resized heat map of one column, computed once per distinct column."""
    out = _tile(np.ascontiguousarray(column, dtype=np.float32).tobytes(), tuple(hw), tuple(size))
    out.setflags(write=False)
    return out


def text_sheet(view_map, n_text, hw, size, strips=None, num_rows=4):
    """:114-132 for one view's (h * w, n) map -> view_images_{view}.png's pixels (label strips white or `strips[i]`)."""
    images = [with_strip(tile(view_map[:, i], hw, size), strip=None if strips is None else strips[i - 1])
              for i in range(1, n_text + 1)]
    return view_images(np.stack(images, axis=0), num_rows=num_rows)


def box_sheet(view_map, hw, size, first=78, num_rows=1):
    """:134-151 for one view's map -> view_images_{view}box.png's pixels."""
    images = [tile(view_map[:, i], hw, size) for i in range(first, view_map.shape[-1])]
    return view_images(np.stack(images, axis=0), num_rows=num_rows)
