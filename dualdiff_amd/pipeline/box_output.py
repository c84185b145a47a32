"""Box output on the GPU: the 3D-box overlays of the reference's demo and validation path.

The reference's `run_one_batch` (misc/test_utils.py:324-387) draws the boxes of a sample over its original and its
generated views with `draw_box_on_imgs` (:48-65) -> `show_box_on_views` (runner/box_visualizer.py:89-114), and
tools/test.py:86-97 saves the results as `{n}_ori_box.png` and `{n}_gen{t}_box.png` (`show_box: true`,
configs/test_config.yaml:11).  Per view:

1. the corners of the boxes re-centred to (0.5, 0.5, 0.5) (:94) go through `img_aug_matrix @ lidar2image` (:102-104) in
   float64; a box is drawn iff all eight corners have z > 0; the boxes are drawn farthest first;
2. the image point is (x, y) / clip(z, 1e-5, 1e5) truncated toward zero; a box is 12 lines in its class colour;
3. with `transparent_bg` (tools/test.py:26) the boxes are drawn on black and every pixel that is not black gets A = 255.

Here that is two launches with no host synchronisation (`ops.box_edges`: project, filter, order; `ops.box_draw_u8`: every
pixel asks the boxes of its tile, last one first, whether one of their edges covers it), on the frames `decode_images`
left on the device, with the corners and matrices `box_input.reference_corners` / `compose_transforms` make:

    overlay = BoxOverlay.from_config(cfg, transparent_bg=True)        # cfg.dataset.object_classes
    pay, flt = zip(*(reference_corners(ex["gt_bboxes_3d"].data) for ex in examples))
    trans = compose_transforms([ex["lidar2image"].data for ex in examples], [ex["img_aug_matrix"].data for ex in examples])
    boxes = overlay(frames, flt, [ex["gt_labels_3d"].data for ex in examples], trans)     # (b, n, H, W, 4) uint8
    concat_views(boxes)                                               # the 2 x 3 grid, as for the frames

WHAT DIFFERS FROM THE REFERENCE: the geometry above is the reference's, the line is not.  The reference draws through
mmdet3d's `visualize_camera` with `cv2.line(..., thickness=1, cv2.LINE_AA)`; here an edge is PIL's thin line
(`ImageDraw.line(..., width=1)`), every pixel of it in the full class colour.  The pictures differ in the anti-aliasing
fringe of the 1-pixel lines and nowhere else.  (The reference makes the same trade for its own projections:
dataset/pipeline.py:176-179.)  Line widths other than 1 and the legend are not built.
"""
import numpy as np
import torch

from .. import ops as O
from .._consts import device_const
from .box_input import _np
from .image_output import _get
from .map_output import COLORS

# the nuScenes object classes of map_output.COLORS: the default palette, name -> RGB
OBJECT_COLORS = {name: COLORS[name] for name in ("car", "truck", "construction_vehicle", "bus", "trailer", "barrier",
                                                 "motorcycle", "bicycle", "pedestrian", "traffic_cone")}


class BoxOverlay:
    """`draw_box_on_imgs` on the GPU.  object_classes: the list of `cfg.dataset` that the labels index; palette: a mapping
    class name -> (r, g, b), default OBJECT_COLORS; transparent_bg: RGBA boxes on a transparent canvas instead of the
    boxes over the frames."""

    def __init__(self, object_classes, palette=None, transparent_bg=False):
        if object_classes is None or isinstance(object_classes, str) or len(tuple(object_classes)) == 0:
            raise ValueError("object_classes must be a non-empty list of class names, got %r" % (object_classes,))
        self.object_classes = tuple(object_classes)
        palette = OBJECT_COLORS if palette is None else palette
        rows = []
        for name in self.object_classes:
            if name not in palette:
                raise ValueError("object class %r has no colour in the palette (%s)" % (name, ", ".join(map(str, palette))))
            rgb = tuple(palette[name])
            if len(rgb) != 3 or any(isinstance(c, bool) or int(c) != c or not 0 <= c <= 255 for c in rgb):
                raise ValueError("the colour of %r must be three bytes (r, g, b), got %r" % (name, palette[name]))
            rows.append(tuple(int(c) for c in rgb))
        self.colors = tuple(rows)
        self.transparent_bg = bool(transparent_bg)

    @classmethod
    def from_config(cls, cfg, transparent_bg=False, palette=None):
        """cfg: any mapping (or object) with `dataset.object_classes`."""
        ds = _get(cfg, "dataset")
        if ds is None or _get(ds, "object_classes") is None:
            raise ValueError("config has no dataset.object_classes")
        return cls(list(_get(ds, "object_classes")), palette=palette, transparent_bg=transparent_bg)

    def palette_table(self):
        """(n, 3) uint8: RGB per class, in the order of object_classes."""
        return np.asarray(self.colors, dtype=np.uint8).reshape(len(self.colors), 3)

    def _device(self, frames):
        if frames is not None:
            if not isinstance(frames, torch.Tensor) or frames.dim() != 5 or frames.shape[-1] != 3 or frames.dtype != torch.uint8:
                raise ValueError("frames must be a uint8 (b, n, H, W, 3) tensor, got %s"
                                 % ("%s %s" % (frames.dtype, tuple(frames.shape)) if isinstance(frames, torch.Tensor)
                                    else type(frames).__name__,))
            O._need_gpu(frames)
            return frames.device
        return torch.device("cuda", torch.cuda.current_device())

    @torch.no_grad()
    def edges(self, corners, labels, transforms, offsets=None, device=None):
        """corners / labels: per-scene lists of (N_i, 8, 3) / (N_i,) arrays or tensors, N_i >= 0 — or, with `offsets`
        (scenes + 1 host integers), the concatenated (total, 8, 3) / (total,) ones, which may already be device tensors —
        as `BoxPreProcess.__call__` takes them; transforms: (b, n, 4, 4) of compose_transforms.
        -> (pts (b, n, cap, 8, 2) int32, cls (b, n, cap) int32, counts (b, n) int32, flags (1,) int32) on the device, cap
        = the largest scene's box count (at least 1): what `ops.box_edges` writes.  One upload, one launch, no readback."""
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else device
        if offsets is None:
            sizes = [int(len(c)) for c in corners]
            if len(labels) != len(sizes):
                raise ValueError("corners and labels must have one entry per scene")
            offs = np.zeros(len(sizes) + 1, dtype=np.int64)
            np.cumsum(sizes, out=offs[1:])

            def cat(parts, tail, dtype):
                parts = [_np(p, dtype).reshape((-1,) + tail) for p in parts]
                return np.concatenate(parts, axis=0) if parts else np.zeros((0,) + tail, dtype)
            corners, labels = cat(corners, (8, 3), np.float32), cat(labels, (), np.int64)
        else:
            offs = np.asarray(offsets.cpu() if isinstance(offsets, torch.Tensor) else offsets, dtype=np.int64).reshape(-1)
        scenes = offs.shape[0] - 1
        if scenes < 1 or offs[0] != 0 or np.any(np.diff(offs) < 0) or offs[-1] != len(corners):
            raise ValueError("offsets must rise from 0 to the number of boxes (%d) over at least one scene, got %s"
                             % (len(corners), offs.tolist()))
        if transforms is None:
            raise ValueError("transforms (b, n, 4, 4) are needed")
        if not (isinstance(transforms, torch.Tensor) and transforms.is_cuda):
            transforms = _np(transforms, np.float32)
        if transforms.ndim != 4 or tuple(transforms.shape[0:1] + transforms.shape[2:]) != (scenes, 4, 4):
            raise ValueError("transforms must be (%d, n, 4, 4), got %s" % (scenes, tuple(transforms.shape)))
        cap = max(int(np.diff(offs).max()), 1)
        if cap > O.BOX_EDGES_MAX:
            raise O._native.Unsupported("dualdiff_amd.BoxOverlay: a scene holds at most %d boxes, got %d"
                                        % (O.BOX_EDGES_MAX, cap))
        # one upload: every host array of the call in one byte buffer, 16-byte aligned parts (as BoxPreProcess does)
        items = {"corners": (corners, np.float32), "labels": (labels, np.int64), "offsets": (offs, np.int32),
                 "transforms": (transforms, np.float32)}
        host, on_dev, size = {}, {}, 0
        for name, (x, dtype) in items.items():
            if isinstance(x, torch.Tensor) and x.is_cuda:
                on_dev[name] = x.to(getattr(torch, np.dtype(dtype).name)).contiguous()
            else:
                arr = _np(x, dtype)
                host[name] = (size, arr)
                size += (arr.nbytes + 15) & ~15
        buf = np.zeros(max(size, 16), dtype=np.uint8)
        for start, arr in host.values():
            buf[start:start + arr.nbytes] = arr.reshape(-1).view(np.uint8)
        dbuf = torch.from_numpy(buf).to(dev)
        for name, (start, arr) in host.items():
            on_dev[name] = dbuf[start:start + arr.nbytes].view(getattr(torch, arr.dtype.name)).view(arr.shape)
        return O.box_edges(on_dev["corners"], on_dev["labels"], on_dev["offsets"], on_dev["transforms"], cap,
                           len(self.object_classes))

    @torch.no_grad()
    def __call__(self, frames, corners, labels, transforms, offsets=None, check=True, size=None):
        """frames: uint8 (b, n, H, W, 3) on the device, or None with transparent_bg and size=(H, W); the other arguments
        as `edges` takes them.  -> uint8 (b, n, H, W, 3): the boxes over the frames, or (b, n, H, W, 4) with transparent_bg:
        the boxes alone.  A new tensor: the frames are never written.  Two launches.  check=True reads the 4-byte flags
        word back and raises ValueError naming what it reports; check=False performs no host synchronisation."""
        if frames is None and not self.transparent_bg:
            raise ValueError("frames may be None with transparent_bg only")
        dev = self._device(frames)
        if frames is None:
            try:
                h, w = (int(v) for v in size)
            except (TypeError, ValueError):
                raise ValueError("without frames pass size=(H, W), got %r" % (size,))
        else:
            h, w = frames.shape[2], frames.shape[3]
        pts, cls, counts, flags = self.edges(corners, labels, transforms, offsets, device=dev)
        b, n = counts.shape
        if frames is not None and tuple(frames.shape[:2]) != (b, n):
            raise ValueError("frames are %d x %d views, the transforms %d x %d" % (frames.shape[0], frames.shape[1], b, n))
        table = device_const(("box_palette", self.colors), dev, lambda: torch.from_numpy(self.palette_table()))
        flat = None if frames is None or self.transparent_bg else frames.contiguous().flatten(0, 1)
        out = O.box_draw_u8(flat, pts, cls, counts, table, transparent=self.transparent_bg, size=(h, w))
        if check:
            word = int(flags.item())                                   # the one readback: 4 bytes
            if word:
                raise ValueError("box overlay: " + "; ".join("bit %d: %s" % (bit.bit_length() - 1, text)
                                                               for bit, text in O.BOX_FLAGS if word & bit))
        return out.view(b, n, h, w, out.shape[-1])
