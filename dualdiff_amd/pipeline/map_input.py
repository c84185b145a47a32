"""Map input on the GPU: the BEV object layers and aux channels from the 3D boxes.

The reference's `LoadBEVSegmentationM` (magicdrive/dataset/pipeline.py) makes the BEV map of a sample on the host: the
static layers from the nuScenes map (or from the h5 cache, as int32 bit fields: `one_hot_decode`, dataset/
pipeline_utils.py:34-49), one object layer per class by PIL's `ImageDraw.polygon(fill=1)` over every box's bottom
rectangle on the 200 x 200 canvas (`_project_dynamic_bbox`, :176-200), and up to eight float channels per pixel from the
last box that covers it (`_get_dynamic_aux_bbox`, :88-152).  That is `gt_masks_bev` (8 + 10 channels with the default
`configs/dataset/Nuscenes.yaml`) and `gt_aux_bev`.  Here the whole line runs on the device, in two launches:

    mi = BevMapInput.from_config(cfg)
    out = mi(static, corners, labels, bottom_center=bc, height=h, visibility=vis)
    out.masks                       # (b, ns + nd, S, S) uint8: gt_masks_bev per sample; MapRender.render takes it as it is
    out.aux                         # (b, aux_ch, S, S) float32: gt_aux_bev, or None
    mi.collate(out, channels=8)     # float32 (b, 8, S, S): collate_fn's bev_map_with_aux (dataset/utils.py:341-345)

REACH: DualDiff's own `collate_fn` keeps `gt_masks_bev[:8]`, the static layers.  The object layers feed the map picture
(`MapRender`, `{n}_map.png`) and the 18 / 26-channel maps of vanilla MagicDrive, not DualDiff's condition.

The corners are the caller's `box.corners` — mmdet3d's corner order differs between versions, so
they are never restated here; the bottom rectangle is corners 0, 3, 7, 4 and the front edge corners 4, 7, as the
reference indexes them.  PIL is not imported: its polygon fill is restated in csrc/bev_map_core.h.

ONE FAMILY OF QUADS IS NOT DRAWN: a rounded quad with two OPPOSITE vertices equal, the other two distinct from them and
from each other, and one of those two more than one pixel away from the repeated vertex, e.g. ((0, 0), (2, 1), (0, 0),
(1, 3)).  No rectangle rounds to such a quad (a rectangle whose diagonal collapses has all four vertices within one
pixel of each other), Pillow's result for it was not reproduced, and such boxes are counted in `out.flags`; with
`check=True` the call raises ValueError naming the count.  Every other quad with repeated vertices — triangle-like,
segment-like, a point, the collapsed diagonal of a tiny box — equals Pillow pixel for pixel.
"""
from collections import namedtuple

import torch

from .. import ops as O

__all__ = ["BevMapInput", "BevMapOutput", "AUX_DATA_CH"]

AUX_DATA_CH = {name: ch for name, _, ch in O.BEV_MAP_AUX}               # pipeline.py:43-48
BevMapOutput = namedtuple("BevMapOutput", ["masks", "aux", "flags"])


def _get(node, key):
    if node is None:
        return None
    if isinstance(node, dict):
        return node.get(key)
    try:
        return node[key]
    except (KeyError, TypeError, IndexError, AttributeError):
        return getattr(node, key, None)


def _bound(bound, what):
    try:
        lo, hi, step = (float(v) for v in bound)
    except (TypeError, ValueError):
        raise ValueError("%s must be (low, high, step), got %r" % (what, bound))
    if not hi > lo or not step > 0:
        raise ValueError("%s must have high > low and step > 0, got %r" % (what, bound))
    return lo, hi, step


class BevMapInput:
    """xbound, ybound: (low, high, step) in metres, `cfg.dataset.map_bound.x / .y`; n_static, n_object: the numbers of
    map and object classes; aux_data: names out of visibility, center_offset, center_ohw, height (any order: the
    channels keep the reference's fixed order), or None."""

    def __init__(self, xbound=(-50.0, 50.0, 0.5), ybound=(-50.0, 50.0, 0.5), n_static=8, n_object=10,
                 aux_data=("visibility", "center_offset", "center_ohw", "height"), device="cuda"):
        xlo, xhi, xstep = _bound(xbound, "xbound")
        ylo, yhi, ystep = _bound(ybound, "ybound")
        patch_h, patch_w = yhi - ylo, xhi - xlo                         # pipeline.py:61-66
        canvas_h, canvas_w = int(patch_h / ystep), int(patch_w / xstep)
        if canvas_h != canvas_w:
            raise ValueError("a non-square canvas is not built (%d x %d): the reference's transposes only make sense for "
                             "a square one, and MapRender refuses it too" % (canvas_h, canvas_w))
        if canvas_h <= 0:
            raise ValueError("the bounds %r, %r leave no canvas" % (xbound, ybound))
        for what, n in (("n_static", n_static), ("n_object", n_object)):
            if isinstance(n, bool) or int(n) != n or n < 0:
                raise ValueError("%s must be a non-negative int, got %r" % (what, n))
        self.ns, self.nd = int(n_static), int(n_object)
        if self.ns + self.nd > O.BEV_MAP_MAX_LAYERS:
            raise ValueError("more than %d layers do not fit the int32 bit fields of the cache (one_hot_encode), got %d "
                             "+ %d" % (O.BEV_MAP_MAX_LAYERS, self.ns, self.nd))
        if self.ns + self.nd == 0:
            raise ValueError("n_static and n_object are both 0: there is no layer to make")
        aux_data = () if aux_data is None else ((aux_data,) if isinstance(aux_data, str) else tuple(aux_data))
        unknown = [a for a in aux_data if a not in AUX_DATA_CH]
        if unknown:
            raise ValueError("unknown aux_data %r: the names are %s" % (unknown, ", ".join(AUX_DATA_CH)))
        self.aux_sel = sum(bit for name, bit, _ in O.BEV_MAP_AUX if name in aux_data)
        self.aux_channels = O.bev_map_aux_channels(self.aux_sel)
        self.size = canvas_h
        # lidar2canvas (:70-74): x * (canvas_h / patch_h) + canvas_h / 2, y * (canvas_w / patch_w) + canvas_w / 2
        self.l2c = (canvas_h / patch_h, canvas_h / 2, canvas_w / patch_w, canvas_w / 2)
        self.device = torch.device(device)

    @classmethod
    def from_config(cls, cfg, **kw):
        """cfg: any mapping (or object) with `dataset.map_bound.x / .y`, `.map_classes`, `.object_classes`, `.aux_data`."""
        ds = _get(cfg, "dataset")
        if ds is None:
            raise ValueError("config has no `dataset` section")
        mb = _get(ds, "map_bound")
        if mb is None or _get(mb, "x") is None or _get(mb, "y") is None:
            raise ValueError("config has no `dataset.map_bound.x / .y`")
        mc, oc, aux = _get(ds, "map_classes"), _get(ds, "object_classes"), _get(ds, "aux_data")
        return cls(tuple(_get(mb, "x")), tuple(_get(mb, "y")), n_static=0 if mc is None else len(mc),
                   n_object=0 if oc is None else len(oc), aux_data=None if aux is None else tuple(aux), **kw)

    # ------------------------------------------------------------------------------------------------- the boxes
    _FIELDS = (("corners", torch.float32, (8, 3)), ("bottom_center", torch.float32, (3,)), ("height", torch.float32, ()),
               ("visibility", torch.float32, ()), ("labels", torch.int64, ()))

    def _boxes(self, b, fields, offsets):
        """-> the five concatenated device tensors and the int32 offsets on the device"""
        lists = [isinstance(v, (list, tuple)) for v in fields.values()]
        if any(lists) and not all(lists):
            raise ValueError("the box fields must be all per-scene lists or all concatenated tensors")
        if all(lists):
            if offsets is not None:
                raise ValueError("offsets go with concatenated tensors, not with per-scene lists")
            if any(len(v) != b for v in fields.values()):
                raise ValueError("per-scene lists must have one entry per sample (%d), got %s"
                                 % (b, {k: len(v) for k, v in fields.items()}))
            counts = [int(torch.as_tensor(c).shape[0]) if torch.as_tensor(c).dim() else 0 for c in fields["labels"]]
            off = [0]
            for c in counts:
                off.append(off[-1] + c)
            cat = {}
            for (name, dt, tail) in self._FIELDS:
                parts = [torch.as_tensor(p).reshape((-1,) + tail) for p in fields[name]]
                cat[name] = torch.cat(parts) if parts else torch.zeros((0,) + tail)
            fields, offsets = cat, torch.tensor(off, dtype=torch.int32)
        else:
            fields = {k: torch.as_tensor(v) for k, v in fields.items()}
            if offsets is None:
                if b != 1:
                    raise ValueError("concatenated box tensors of a batch of %d need offsets (b + 1,)" % b)
                offsets = torch.tensor([0, fields["labels"].shape[0]], dtype=torch.int32)
            offsets = torch.as_tensor(offsets)
            if offsets.dim() != 1 or offsets.shape[0] != b + 1 or offsets.dtype.is_floating_point:
                raise ValueError("offsets must be %d integers, got %s %s" % (b + 1, offsets.dtype, tuple(offsets.shape)))
        total = fields["labels"].reshape(-1).shape[0]
        for name, dt, tail in self._FIELDS:
            t = fields[name]
            if tuple(t.shape) != (total,) + tail:
                if t.numel() == 0 and total == 0:
                    fields[name] = t.reshape((0,) + tail)
                else:
                    raise ValueError("%s must be %s for %d boxes, got %s" % (name, (total,) + tail, total, tuple(t.shape)))
        if total == 0:
            dev = offsets.device if offsets.is_cuda else self.device
            out = [torch.zeros((0,) + tail, dtype=dt, device=dev) for _, dt, tail in self._FIELDS]
            return out, offsets.to(device=dev, dtype=torch.int32).contiguous()
        where = {t.is_cuda for t in fields.values()}
        if len(where) == 2:
            raise RuntimeError("the box fields are partly on the host and partly on the device: pass them all on one side")
        if where == {True}:
            dev = fields["corners"].device
            out = [fields[name].to(device=dev, dtype=dt).contiguous() for name, dt, _ in self._FIELDS]
            return out, offsets.to(device=dev, dtype=torch.int32).contiguous()
        if offsets.is_cuda:
            raise RuntimeError("offsets are on the device and the box fields on the host: pass them all on one side")
        # host: one buffer, one upload — labels (8 bytes each) first, then the float fields, then the offsets
        parts = [fields["labels"].to(torch.int64).contiguous().view(-1).view(torch.uint8)]
        for name, dt, _ in self._FIELDS[:4]:
            parts.append(fields[name].to(dt).contiguous().view(-1).view(torch.uint8))
        parts.append(offsets.to(torch.int32).contiguous().view(torch.uint8))
        dev_buf = torch.cat(parts).to(self.device, non_blocking=True)
        out, at = {}, 0
        for (name, dt, tail), n in zip((self._FIELDS[4],) + self._FIELDS[:4], (8, 96, 12, 4, 4)):
            out[name] = dev_buf[at:at + n * total].view(dt).reshape((total,) + tail)
            at += n * total
        off_dev = dev_buf[at:at + 4 * (b + 1)].view(torch.int32)
        return [out[name] for name, _, _ in self._FIELDS], off_dev

    def _static(self, static):
        if self.ns == 0:
            return None
        if not isinstance(static, torch.Tensor):
            raise ValueError("static must be a tensor: (b, %d, S, S) layers or (b, S, S) int32 bit fields, got %s"
                             % (self.ns, type(static).__name__))
        if not static.is_cuda:
            raise RuntimeError("static must be on the device (got a %s tensor): the layers are joined there" % static.device)
        s = self.size
        if static.dim() == 3:
            if static.dtype != torch.int32 or tuple(static.shape[1:]) != (s, s):
                raise ValueError("bit fields must be int32 (b, %d, %d), got %s %s" % (s, s, static.dtype, tuple(static.shape)))
            return static.contiguous()
        if static.dim() != 4 or tuple(static.shape[1:]) != (self.ns, s, s):
            raise ValueError("static layers must be (b, %d, %d, %d), got %s" % (self.ns, s, s, tuple(static.shape)))
        if static.dtype == torch.bool:
            return static.contiguous().view(torch.uint8)
        return static.to(torch.uint8).contiguous()

    @torch.no_grad()
    def __call__(self, static, corners, labels, *, bottom_center, height, visibility, offsets=None, check=True, batch=None):
        """static: (b, ns, S, S) layers of 0 / 1 or (b, S, S) int32 bit fields, on the device (None with n_static = 0, then
        pass batch=b).  Boxes as `BoxPreProcess` takes them: per-scene lists (b entries each), or concatenated tensors with
        offsets (b + 1,) — on the host (one upload for the whole call) or on the device: corners (N, 8, 3), bottom_center
        (N, 3), height (N,), visibility (N,), labels (N,).  A scene may have no box.
        -> BevMapOutput(masks, aux, flags), all on the device.  check=True reads the 4-byte flags word back and raises
        ValueError where a box's quad is of the family that is not drawn (the module's docstring); check=False performs
        no host synchronisation."""
        st = self._static(static)
        if st is not None:
            b = st.shape[0]
        elif batch is None:
            b = len(labels) if isinstance(labels, (list, tuple)) else 1
        else:
            b = int(batch)
        fields = {"corners": corners, "bottom_center": bottom_center, "height": height, "visibility": visibility,
                  "labels": labels}
        (c, bc, h, v, l), off = self._boxes(b, fields, offsets)
        if st is not None and st.device != off.device:
            raise RuntimeError("static is on %s and the boxes on %s" % (st.device, off.device))
        masks, aux, flags = O.bev_map_layers(st, c, bc, h, v, l, off, self.size, self.ns, self.nd, self.aux_sel, self.l2c)
        if check:
            n = int(flags.item())
            if n:
                raise ValueError("map input: %d box(es) round to a quad with two opposite vertices equal and the others "
                                 "apart, which no rectangle gives and which is not drawn (check=False returns the count "
                                 "in flags)" % n)
        return BevMapOutput(masks, aux, flags)

    @torch.no_grad()
    def collate(self, out, channels=8, with_aux=False):
        """`collate_fn`'s bev_map_with_aux (dataset/utils.py:341-345): the first `channels` layers as float32, (b, channels,
        S, S).  with_aux=True appends gt_aux_bev, as the lines commented out there (vanilla MagicDrive) do."""
        masks = out.masks if isinstance(out, BevMapOutput) else out
        res = masks[:, :channels].float()
        if with_aux and isinstance(out, BevMapOutput) and out.aux is not None:
            res = torch.cat([res, out.aux], dim=1)
        return res
