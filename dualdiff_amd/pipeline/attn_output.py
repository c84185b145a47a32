"""Attention-map pictures on the GPU: the per-token heat-map sheets the reference's analysis script saves per view.

tools/explore_attn.py:114-151 turns `gather_layer` (the `mean_map` of networks/attn_maps.py, (views, h * w, n) float32) into
`view_images_{view}.png`, one heat map per prompt token, and `view_images_{view}box.png`, one per box token:

1. per view and context column the min-max normalisation in float64 (:118-122, :138-142); a constant column is 0 / 0 = NaN;
2. matplotlib's `coolwarm` per pixel, a Python loop of `cmap(...)` calls, and `(rgba[:3] * 255).astype(uint8)` (:123-128,
   :143-148): index `min(int(X * 256), 255)` into the 256 colours, black for NaN;
3. `Image.resize((400, 224))`, PIL's default bicubic (:129, :149);
4. text tiles only: `text_under_image` (:13-23), a white strip of `int(h * .2)` rows below the tile with the token's text;
5. `view_images` (:25-53): the tiles in row-major cells on a white canvas with a gutter of `int(tile_h * 0.02)` pixels;
   `num_empty = N % num_rows` white tiles are appended, `num_cols = (N + num_empty) // num_rows`, and tiles beyond
   `rows * cols` are dropped (N = 5 on 4 rows gives one column: the fifth tile is lost).  Kept as it is.

Here 1-5 are three launches per call (`ops.attn_heat`, the PIL-exact `ops.image_resample_u8` whose bottom pad is the white
strip, `ops.attn_sheet_u8`) with no host synchronisation, byte for byte:

    render = AttnMapRender()                               # hw (28, 50), tiles of 224 x 400, coolwarm
    text, box = render(capture, n_text, labels=words)      # capture: a CrossAttnMapCapture, or the (views, h * w, n) map
    render.save(directory, text, box)                      # view_images_{v}.png / view_images_{v}box.png, through save_png

The one difference from the reference's pictures: the GLYPH PIXELS of the label strip, and nothing else.  The reference
draws the token text with `cv2.putText` in the Hershey font; cv2's glyphs are not reproduced.  `labels=None` leaves the
strips white; a list of strings is drawn with PIL's default font, centred by the reference's formula (:20-21); a uint8
tensor of strips is pasted as it is (draw them with cv2 for the reference's own bytes).
"""
import os

import numpy as np
import torch

from .. import ops as O
from .._consts import device_const
from ..image_tables import cmap_bytes, device_cmap_table
from .image_output import save_png

FIRST_BOX_COLUMN = 78                   # :137: one camera token and the 77 prompt tokens come first

_STRIPS = {}                            # (text, lh, tw) -> (lh, tw, 3) uint8 ndarray, drawn once per process


def sheet_layout(n, num_rows):
    """`view_images`' arithmetic (:27-40, :46-49) for n tiles -> (rows, cols, index): index[r * cols + c] is the tile of
    cell (r, c), or -1 for one of the appended all-255 tiles.  Tiles from rows * cols on are in no cell."""
    for name, v in (("n", n), ("num_rows", num_rows)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError("%s must be an int, got %r" % (name, v))
    if n <= 0:
        raise ValueError("a sheet of %d tiles: the reference fails there too (images[0])" % n)
    if num_rows <= 0:
        raise ValueError("num_rows must be positive, got %d" % num_rows)
    num_empty = n % num_rows                                # a remainder, not a complement
    cols = (n + num_empty) // num_rows
    if cols == 0:
        raise ValueError("%d tiles on %d rows give no column: the reference fails there too" % (n, num_rows))
    return num_rows, cols, [i if i < n else -1 for i in range(num_rows * cols)]


def draw_label(text, lh, tw):
    """The strip of one token: black text on white, (lh, tw, 3) uint8, drawn with PIL's default font where the reference
    calls cv2.putText.  Placed by the reference's formula (:20-21) with the text's own box in place of cv2.getTextSize:
    left edge at (tw - text_w) // 2, bottom edge text_h // 2 above the strip's bottom.  Cached per (text, lh, tw)."""
    key = (text, lh, tw)
    if key not in _STRIPS:
        from PIL import Image, ImageDraw, ImageFont
        im = Image.new("RGB", (tw, lh), (255, 255, 255))
        draw = ImageDraw.Draw(im)
        font = ImageFont.load_default()
        left, top, right, bottom = draw.textbbox((0, 0), text, font=font)
        x, y = (tw - (right - left)) // 2, lh - (bottom - top) // 2
        draw.text((x - left, y - bottom), text, fill=(0, 0, 0), font=font)
        _STRIPS[key] = np.asarray(im, dtype=np.uint8)
    return _STRIPS[key]


def _ratio_rows(h, ratio, what):
    rows = int(h * ratio)
    if not 0 <= rows:
        raise ValueError("%s %r gives %d rows of a tile of %d" % (what, ratio, rows, h))
    return rows


class AttnMapRender:
    """tools/explore_attn.py:114-151 on the GPU.  hw: the (h, w) of the attention layer's queries; size: the (height,
    width) every heat map is resized to (the reference's `resize((400, 224))` is width first); cmap: "coolwarm" or any
    (256, 3) uint8 table; label_ratio / gap_ratio: text_under_image's .2 and view_images' offset_ratio.

    The pictures equal the reference's byte for byte except in the glyph pixels of the label strip (module docstring)."""

    def __init__(self, hw=(28, 50), size=(224, 400), cmap="coolwarm", label_ratio=0.2, gap_ratio=0.02):
        try:
            self.hw = tuple(int(v) for v in hw)
            self.size = tuple(int(v) for v in size)
        except (TypeError, ValueError):
            raise ValueError("hw and size must be (h, w), got %r / %r" % (hw, size))
        if len(self.hw) != 2 or len(self.size) != 2 or min(self.hw + self.size) <= 0:
            raise ValueError("hw and size must be two positive ints each, got %r / %r" % (hw, size))
        self.cmap = cmap if isinstance(cmap, str) else cmap_bytes(cmap)
        cmap_bytes(self.cmap)                               # an unknown name fails here, not at the first call
        self.label_ratio, self.gap_ratio = float(label_ratio), float(gap_ratio)
        self.strip = _ratio_rows(self.size[0], self.label_ratio, "label_ratio")      # :15
        _ratio_rows(self.size[0] + self.strip, self.gap_ratio, "gap_ratio")

    def gap(self, tile_h):
        return _ratio_rows(tile_h, self.gap_ratio, "gap_ratio")                      # :39

    # ---------------------------------------------------------------------------- tiles ----
    def _maps(self, maps):
        if hasattr(maps, "mean_map"):                       # a CrossAttnMapCapture: `gather_layer` (:97-105)
            maps = maps.mean_map(self.hw)
        if not isinstance(maps, torch.Tensor) or maps.dim() != 3 or maps.numel() == 0 \
                or maps.shape[1] != self.hw[0] * self.hw[1]:
            raise ValueError("maps must be (views, %d, n) for hw %s, got %s"
                             % (self.hw[0] * self.hw[1], self.hw,
                                tuple(maps.shape) if isinstance(maps, torch.Tensor) else type(maps).__name__))
        if maps.dtype != torch.float32:
            raise ValueError("maps must be float32 (the capture's own type), got %s" % (maps.dtype,))
        if maps.stride(2) != 1 or maps.stride(1) < maps.shape[2] or maps.stride(0) < 0:
            maps = maps.contiguous()
        return maps

    def _tiles(self, maps, cols, strip):
        n, dev = maps.shape[2], maps.device
        if isinstance(cols, torch.Tensor):
            if cols.dtype != torch.int32 or cols.dim() != 1 or cols.numel() == 0:
                raise ValueError("cols must be a non-empty int32 vector, got %s %s" % (cols.dtype, tuple(cols.shape)))
            cols = cols.contiguous()
        else:
            cols = tuple(cols)
            if not cols or any(isinstance(c, bool) or not isinstance(c, int) or not 0 <= c < n for c in cols):
                raise ValueError("cols must be context columns in [0, %d), got %r" % (n, cols))
            cols = device_const(("attn_cols", cols), dev, lambda: torch.tensor(cols, dtype=torch.int32))
        img = O.attn_heat(maps, cols, device_cmap_table(self.cmap, dev), self.hw)
        u8 = O.image_resample_u8(img, self.size, padding=(0, 0, 0, self.strip if strip else 0), fill=255)
        return u8, cols.shape[0]

    @torch.no_grad()
    def tiles(self, maps, cols, strip=True):
        """maps (views, h * w, n) float32 on the device (any row pitch), cols: the context columns to draw (ints, or an
        int32 device tensor) -> (views, t, th, tw, 3) uint8: the resized heat maps (:118-129), with the white strip of
        text_under_image below them for strip=True (th = size[0] + int(size[0] * label_ratio)).  Two launches."""
        maps = self._maps(maps)
        u8, t = self._tiles(maps, cols, strip)
        return u8.reshape(maps.shape[0], t, u8.shape[1], u8.shape[2], 3)

    # --------------------------------------------------------------------------- sheets ----
    def _sheets(self, maps, cols, strip, labels, num_rows):
        views, dev = maps.shape[0], maps.device
        u8, t = self._tiles(maps, cols, strip)
        rows, ncols, cells = sheet_layout(t, num_rows)
        index = device_const(("attn_sheet_index", views, t, rows, ncols), dev, lambda: torch.tensor(
            [[c + v * t if c >= 0 else -1 for c in cells] for v in range(views)], dtype=torch.int32))
        return O.attn_sheet_u8(u8, index, rows, ncols, self.gap(u8.shape[1]), labels)

    def _labels(self, labels, views, t, dev):
        lh, tw = self.strip, self.size[1]
        if labels is None or lh == 0:
            return None
        if isinstance(labels, torch.Tensor):
            if labels.dtype != torch.uint8 or labels.dim() not in (4, 5) or tuple(labels.shape[-4:]) != (t, lh, tw, 3) \
                    or (labels.dim() == 5 and labels.shape[0] != views):
                raise ValueError("label strips must be uint8 (%d, %d, %d, 3) or (%d, %d, %d, %d, 3), got %s %s"
                                 % (t, lh, tw, views, t, lh, tw, labels.dtype, tuple(labels.shape)))
            if labels.dim() == 4:
                labels = labels[None].expand(views, t, lh, tw, 3)
            return labels.to(dev).contiguous().reshape(views * t, lh, tw, 3)
        labels = tuple(labels)
        if len(labels) != t or not all(isinstance(s, str) for s in labels):
            raise ValueError("labels must be %d strings (one per text token), got %r" % (t, labels))

        def build():
            strips = np.stack([draw_label(s, lh, tw) for s in labels])
            return torch.from_numpy(np.ascontiguousarray(np.broadcast_to(strips, (views,) + strips.shape))
                                    .reshape(views * t, lh, tw, 3))
        return device_const(("attn_labels", labels, views, lh, tw), dev, build)

    @torch.no_grad()
    def text_sheets(self, maps, n_text, labels=None, num_rows=4):
        """`view_images_{view}.png` (:114-132) of every view -> (views, H, W, 3) uint8 on the device: columns 1 .. n_text
        (column 0 is the camera token; n_text = len(tokenizer.encode(prompt)), BOS and EOS included), each with its label
        strip, on `num_rows` rows.  labels: None (white strips), n_text strings (PIL's default font, drawn once per
        distinct string and kept on the device), or a uint8 tensor of strips (n_text, lh, tw, 3) / (views, n_text, lh, tw,
        3).  Three launches, no host synchronisation."""
        maps = self._maps(maps)
        if isinstance(n_text, bool) or not isinstance(n_text, int) or not 0 < n_text < maps.shape[2]:
            raise ValueError("n_text must be in 1..%d (the map has %d context columns), got %r"
                             % (maps.shape[2] - 1, maps.shape[2], n_text))
        strips = self._labels(labels, maps.shape[0], n_text, maps.device)
        return self._sheets(maps, range(1, n_text + 1), True, strips, num_rows)

    @torch.no_grad()
    def box_sheets(self, maps, first=FIRST_BOX_COLUMN, num_rows=1):
        """`view_images_{view}box.png` (:134-151) of every view -> (views, H, W, 3) uint8: columns first .. n - 1 without a
        label strip, or None when the map has no box column (the reference fails on the empty list there)."""
        maps = self._maps(maps)
        if isinstance(first, bool) or not isinstance(first, int) or first < 0:
            raise ValueError("first must be a non-negative int, got %r" % (first,))
        if first >= maps.shape[2]:
            return None
        return self._sheets(maps, range(first, maps.shape[2]), False, None, num_rows)

    @torch.no_grad()
    def __call__(self, maps, n_text, labels=None):
        """maps: (views, h * w, n) float32 on the device, or a CrossAttnMapCapture (its `mean_map(hw)` is taken once)
        -> (text_sheets, box_sheets)."""
        maps = self._maps(maps)
        return self.text_sheets(maps, n_text, labels), self.box_sheets(maps)

    def save(self, directory, text, box=None):
        """`view_images_{v}.png` of text[v] and `view_images_{v}box.png` of box[v] under `directory` (:53), through
        save_png.  Returns the paths."""
        paths = [os.path.join(os.fspath(directory), "view_images_%d.png" % v) for v in range(text.shape[0])]
        save_png(text, paths)
        if box is not None:
            more = [os.path.join(os.fspath(directory), "view_images_%dbox.png" % v) for v in range(box.shape[0])]
            save_png(box, more)
            paths += more
        return paths
