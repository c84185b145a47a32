"""Box input on the GPU: a batch's 3D box corners as the `bboxes_3d_data` that `BEVDenoiser.set_inputs` and
`BEVControlNetModel.forward` take.

What the reference's `collate_fn` does with `gt_bboxes_3d` / `gt_labels_3d` (dataset/utils.py:128-262, `_preprocess_bbox`,
test time: no random drop / add): per view, transform the eight corners of every box — of the box re-centred to (0.5, 0.5,
0.5), runner/box_visualizer.py:63 — by `img_aug_matrix @ lidar2camera` (`use_3d_filter`, keep a box with any corner at z >
0) or by `img_aug_matrix @ lidar2image` (project, keep a box that reaches the canvas), in float64; select the kept boxes'
corners and labels in their order; pad every (scene, view) to the batch maximum with zero points, class -1, mask False; give
`None` when nothing is visible.  With `view_shared` there is one "view" that keeps everything.

Here that is one upload and one launch (`ops.box_views`): the arrays of the batch go to the device as one buffer, the kernel
writes the rows at a capacity known on the host (`layers.box_capacity` of the largest scene: the layout the public
forward()s use), and the batch maximum stays in device memory.  `sync=True` reads that one int32 back, because the reference's
tensor shapes need it, and returns the dict element for element; `sync=False` returns the capacity layout with no host
synchronisation.

    pre = BoxPreProcess.from_config(cfg)                              # cfg.model.bbox_mode / .bbox_view_shared, image_size
    pay, flt = zip(*(reference_corners(ex["gt_bboxes_3d"].data) for ex in examples))
    trans = compose_transforms([ex["lidar2camera"].data for ex in examples], [ex["img_aug_matrix"].data for ex in examples])
    bboxes_3d_data = pre(pay, [ex["gt_labels_3d"].data for ex in examples], trans, filter_corners=flt)

The corners themselves come from the caller's box class (`reference_corners`): mmdet3d's corner order and yaw convention
differ between its versions, so they are not restated here.  `for_mask` (dataset/utils.py:533-537) is this class with
`use_3d_filter=False` on the re-centred corners, and `FgmMask` (fgm_mask.py) makes `heatmap_gt` of it.  The training-time
`bbox_add_ratio` / `bbox_drop_ratio` paths, the projected `bboxes_coord` and `_preprocess_map_vec` stay with the caller.
"""
import collections

import numpy as np
import torch

from .. import ops as O
from ..networks.layers import box_capacity
from .image_output import _get

BBOX_MODES = ("all-xyz", "cxyz")

BoxViews = collections.namedtuple("BoxViews", "bboxes classes masks counts max_len_dev")
BoxViews.__doc__ = """`BoxPreProcess(..., sync=False)`: `bboxes` (b, n, cap, P, 3) fp32, `classes` (b, n, cap) int64, `masks`
(b, n, cap) bool at the capacity `cap = box_capacity(largest scene)`, `counts` (b, n) int32 = boxes kept per (scene, view),
`max_len_dev` (1,) int32 = their maximum — all in device memory.  With `uncond_first` the first three are the (2 b, ...) CFG
layout, counts and max_len_dev describe the conditional half."""


def _np(x, dtype):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(x), dtype=dtype)


def compose_transforms(lidar2x, img_aug_matrix=None):
    """The matrices the visibility test uses, `aug @ trans` per view in numpy float32 as runner/box_visualizer.py:64-67 does
    (`lidar2x` = lidar2camera for `use_3d_filter`, lidar2image otherwise): (b, n, 4, 4) arrays / tensors, or per-scene lists
    of (n, 4, 4) -> float32 (b, n, 4, 4).  One 4 x 4 product per view on the host, with numpy's rounding."""
    trans = np.stack([_np(t, np.float32) for t in lidar2x], axis=0)
    if trans.ndim != 4 or trans.shape[2:] != (4, 4):
        raise ValueError("lidar2x must be (b, n, 4, 4), got %s" % (trans.shape,))
    if img_aug_matrix is None:
        return trans
    aug = np.stack([_np(a, np.float32) for a in img_aug_matrix], axis=0)
    if aug.shape != trans.shape:
        raise ValueError("img_aug_matrix %s does not match lidar2x %s" % (aug.shape, trans.shape))
    out = np.empty_like(trans)
    for b in range(trans.shape[0]):
        for n in range(trans.shape[1]):
            out[b, n] = aug[b, n] @ trans[b, n]
    return out


def reference_corners(boxes):
    """(payload corners, filter corners) of a box container of the caller's: `boxes.corners`, and the corners of the same
    boxes re-centred to (0.5, 0.5, 0.5) — `box_center_shift` of runner/box_visualizer.py:17-21, 63.  Duck-typed: the class
    has `.corners`, `.tensor` and a constructor `(tensor, box_dim=, origin=)` (mmdet3d's LiDARInstance3DBoxes)."""
    shifted = type(boxes)(boxes.tensor, box_dim=boxes.tensor.shape[-1], origin=(0.5, 0.5, 0.5))
    return boxes.corners, shifted.corners


def camera_param(intrinsics, camera2lidar):
    """`camera_param` of dataset/utils.py:434-437, (b, n, 3, 7): columns 0..2 the upper-left 3 x 3 of every camera's
    intrinsics, columns 3..6 the first three rows of its camera2lidar.  intrinsics / camera2lidar: (b, n, 4, 4) (intrinsics
    may be (b, n, 3, 3)) tensors or arrays, or per-scene lists of (n, ...) — every scene with the same cameras."""
    def batched(x):
        return torch.as_tensor(x) if not isinstance(x, (list, tuple)) else torch.stack([torch.as_tensor(v) for v in x])
    k, c = batched(intrinsics), batched(camera2lidar)
    if k.dim() != 4 or c.dim() != 4 or k.shape[:2] != c.shape[:2] or min(k.shape[2:]) < 3 or c.shape[2] < 3:
        raise ValueError("camera_param takes (b, n, >=3, >=3) intrinsics and (b, n, >=3, m) camera2lidar, got %s and %s"
                         % (tuple(k.shape), tuple(c.shape)))
    return torch.cat((k[..., :3, :3], c[..., :3, :]), dim=-1)


def aug_text_names(classes, object_classes):
    """The per-(scene, camera) class sentences of `use_aug_text` (dataset/utils.py:496-506) from the `classes` tensor (b, n,
    len) of `bboxes_3d_data`, with one readback: the sorted unique classes of a view WITHOUT THE FIRST, as names joined by
    ", " -> list of b * n strings, scene-major.

    The reference drops the first unique value unconditionally ("there is a -1 in the front as blank").  In a view with no
    padding — as many boxes as the batch maximum — there is no -1, and the smallest real class of that view is lost.  That
    quirk is kept, because the captions of the reference depend on it."""
    names = list(object_classes)
    host = classes.detach().cpu()
    out = []
    for scene in host:
        for view in scene:
            out.append(", ".join(names[i] for i in torch.unique(view)[1:].tolist()))
    return out


class BoxPreProcess:
    """The reference's test-time `_preprocess_bbox` on the GPU.  bbox_mode "all-xyz" (8 corners) or "cxyz" (corners 6, 5, 7,
    2); view_shared: one view that keeps every box; use_3d_filter: positive-z test on `aug @ lidar2camera`, else the canvas
    test on the projection by `aug @ lidar2image`, which needs canvas_size = (H, W) of the images."""

    def __init__(self, bbox_mode="all-xyz", view_shared=False, use_3d_filter=True, canvas_size=None):
        if bbox_mode == "owhr":
            raise NotImplementedError("Not sure how to do this.")
        if bbox_mode not in BBOX_MODES:
            raise NotImplementedError("Wrong mode %s" % (bbox_mode,))
        self.bbox_mode, self.view_shared, self.use_3d_filter = bbox_mode, bool(view_shared), bool(use_3d_filter)
        self.filter_mode = "all" if self.view_shared else "positive_z" if self.use_3d_filter else "canvas"
        self.canvas_size = None
        if self.filter_mode == "canvas":
            if canvas_size is None:
                raise ValueError("use_3d_filter=False filters on the image canvas and needs canvas_size = (H, W)")
            self.canvas_size = tuple(int(v) for v in canvas_size)
            if len(self.canvas_size) != 2 or min(self.canvas_size) <= 0:
                raise ValueError("canvas_size must be a positive (H, W), got %r" % (canvas_size,))

    @classmethod
    def from_config(cls, cfg, use_3d_filter=True, branch=None):
        """cfg: any mapping (or object) with `model.bbox_mode`, `model.bbox_view_shared` — what the reference's runners hand
        to `collate_fn` — and `dataset.image_size` (the canvas, `pixel_values.shape[-2:]`).  branch: index into a
        per-ControlNet list `bbox_view_shared` of a dual-branch config."""
        model, ds = _get(cfg, "model"), _get(cfg, "dataset")
        if model is None or _get(model, "bbox_mode") is None:
            raise ValueError("config has no model.bbox_mode")
        shared = _get(model, "bbox_view_shared", False)
        if isinstance(shared, (list, tuple)) or (hasattr(shared, "__len__") and not isinstance(shared, str)):
            if branch is None:
                raise ValueError("model.bbox_view_shared is a per-branch list %r: pass branch=" % (list(shared),))
            shared = shared[branch]
        size = None if ds is None else _get(ds, "image_size")
        return cls(bbox_mode=_get(model, "bbox_mode"), view_shared=bool(shared), use_3d_filter=use_3d_filter,
                   canvas_size=None if size is None else tuple(size))

    @property
    def points(self):
        return 8 if self.bbox_mode == "all-xyz" else 4

    def __call__(self, corners, labels, transforms, filter_corners=None, uncond_first=False, sync=True, offsets=None):
        """corners / labels (/ filter_corners): per-scene lists of (N_i, 8, 3) / (N_i,) arrays or tensors, N_i >= 0 — or,
        with `offsets` (scenes + 1 host integers), the concatenated (total, 8, 3) / (total,) ones, which may already be
        device tensors.  transforms: (b, n, 4, 4) of compose_transforms; unused (may be None) with view_shared.
        -> sync=True: {"bboxes" (b, n', max_len, P, 3) fp32, "classes" int64, "masks" bool} on the device, or None when no
        box is visible anywhere; n' = 1 with view_shared.  sync=False: a BoxViews.  uncond_first: the (2 b, ...) layout of
        `add_uncond_to_kwargs`, an all-zero half in front."""
        dev = torch.device("cuda", torch.cuda.current_device())       # the launch goes to this device's current stream
        if offsets is None:
            counts = [int(len(c)) for c in corners]
            if len(labels) != len(counts) or (filter_corners is not None and len(filter_corners) != len(counts)):
                raise ValueError("corners, labels and filter_corners must have one entry per scene")
            offs = np.zeros(len(counts) + 1, dtype=np.int64)
            np.cumsum(counts, out=offs[1:])

            def cat(parts, tail, dtype):
                parts = [_np(p, dtype).reshape((-1,) + tail) for p in parts]
                return np.concatenate(parts, axis=0) if parts else np.zeros((0,) + tail, dtype)
            corners, labels = cat(corners, (8, 3), np.float32), cat(labels, (), np.int64)
            if filter_corners is not None:
                filter_corners = cat(filter_corners, (8, 3), np.float32)
        else:
            offs = np.asarray(offsets.cpu() if isinstance(offsets, torch.Tensor) else offsets, dtype=np.int64).reshape(-1)
        scenes = offs.shape[0] - 1
        if scenes < 1 or offs[0] != 0 or np.any(np.diff(offs) < 0) or offs[-1] != len(corners):
            raise ValueError("offsets must rise from 0 to the number of boxes (%d) over at least one scene, got %s"
                             % (len(corners), offs.tolist()))
        if self.view_shared:
            views, transforms = 1, None
        else:
            if transforms is None:
                raise ValueError("transforms (b, n, 4, 4) are needed unless view_shared")
            if not (isinstance(transforms, torch.Tensor) and transforms.is_cuda):
                transforms = _np(transforms, np.float32)
            if transforms.ndim != 4 or tuple(transforms.shape[0:1] + transforms.shape[2:]) != (scenes, 4, 4):
                raise ValueError("transforms must be (%d, n, 4, 4), got %s" % (scenes, tuple(transforms.shape)))
            views = transforms.shape[1]
        # one upload: every host array of the call in one byte buffer, 16-byte aligned parts
        items = {"corners": (corners, np.float32), "labels": (labels, np.int64), "offsets": (offs, np.int32),
                 "transforms": (transforms, np.float32), "filter_corners": (filter_corners, np.float32)}
        host, on_dev, size = {}, {}, 0
        for name, (x, dtype) in items.items():
            if x is None:
                on_dev[name] = None
            elif isinstance(x, torch.Tensor) and x.is_cuda:
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
            t = dbuf[start:start + arr.nbytes].view(getattr(torch, arr.dtype.name))
            on_dev[name] = t.view(arr.shape)
        b, cap, pts = scenes, box_capacity(int(np.diff(offs).max())), self.points
        out = None
        if uncond_first:                                     # the kernel writes the second half of a zeroed batch
            full = (torch.zeros((2 * b, views, cap, pts, 3), dtype=torch.float32, device=dev),
                    torch.zeros((2 * b, views, cap), dtype=torch.int64, device=dev),
                    torch.zeros((2 * b, views, cap), dtype=torch.bool, device=dev))
            out = tuple(t[b:] for t in full) + (torch.empty((b, views), dtype=torch.int32, device=dev),
                                                torch.empty((1,), dtype=torch.int32, device=dev))
        res = O.box_views(on_dev["corners"], on_dev["labels"], on_dev["offsets"], on_dev["transforms"], views, cap,
                          points_mode=self.bbox_mode, filter_mode=self.filter_mode, canvas_size=self.canvas_size,
                          filter_corners=on_dev["filter_corners"], out=out)
        bx, cl, mk = full if uncond_first else res[:3]
        if not sync:
            return BoxViews(bx, cl, mk, res[3], res[4])
        max_len = int(res[4].item())                         # the one readback: 4 bytes
        if max_len == 0:
            return None
        return {"bboxes": bx[:, :, :max_len].contiguous(), "classes": cl[:, :, :max_len].contiguous(),
                "masks": mk[:, :, :max_len].contiguous()}
