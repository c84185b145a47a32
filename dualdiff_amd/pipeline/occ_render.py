"""ORS panorama on the GPU: occupancy volumes to the image-mode ORS condition.

The reference's default ORS condition (`use_occ_3d: false`: every single-branch config and branch 0 of the dual-branch
ones) is a folder of pre-rendered panoramas, `./occ_proj/occ_bg/{token}.png` (misc/test_utils.py:219-222,
dataset/dataset_wrapper.py:62-81).  `png_input.OccCondition` reads and collates such files; this module MAKES them from
the Occ3D labels, for a user who has the labels but not the authors' folder:

    render = OccRender.for_image_size(cfg.dataset.image_size)                 # mode="bg": the occ_bg folder
    frames = render(volumes, rigs)                                            # (b, h, 6 * w, 3) uint8, on the device
    cond = occ_condition_from_config(cfg)(frames)                             # what the ControlNet branch takes
    save_png(frames, paths)                                                   # or the folder itself

A panorama is, per ray of `OccupancyRay` (networks/occ3d_proj.py, the same rays and samples as the 3-D condition, at the
image size instead of the latent size): the first class along the ray that is not 17, painted with the Occ3D palette,
the six views side by side.  One launch per batch (`ops.ors_first_hit`); no label per sample is ever written.

WHAT IS SUPPOSED, NOT KNOWN: the reference ships no script that writes `occ_proj/occ_bg`.  The only statement of the
picture in the reference is the `__main__` block of networks/occ3d_proj.py:156-198.  The panorama here is `colored_image`
of that block, with its "filter out foregrounds" line (:157, commented out there) enabled for mode "bg", which is what
the folder's name points to.  The authors' files may have been made with another sample count, step, geometry or filter:
all of these are parameters here for that reason.  `overlay` is the one picture that block writes itself (:196-203).
"""
import torch

from .. import ops as O
from ..networks.occ3d_proj import OCC_COLORS, OccupancyRay

__all__ = ["OCC_COLORS", "OccRender"]

# cfg.dataset.image_size -> (image_shape, compress_ratio) of the render whose panorama the collate step for that size takes
_GEOMETRY = {
    (224, 400): ((896, 1600), 400 / 1600),      # the `h = 896` note of occ3d_proj.py:144: 224 x 400 per view
    (192, 384): ((896, 1600), 400 / 1600),      # crop_drivewm takes the 224 x 2400 panorama (dataset/utils.py:374-388)
    (432, 768): ((900, 1600), 768 / 1600),      # occ_bg_hd: 432 x 768 per view
    (256, 704): ((900, 1600), 768 / 1600),      # crop_hd takes the 432 x 4608 panorama (dataset/utils.py:348-372)
}


class OccRender:
    """image_shape, compress_ratio, sample_point, sample_step: `OccupancyRay`'s (a view is int(image_shape * compress_ratio)
    pixels); mode: "bg" (classes <= 10 removed first, the occ_bg folder), "fg" (classes >= 11 removed) or "all"; palette:
    18 (r, g, b) byte triples, default OCC_COLORS."""

    def __init__(self, image_shape, compress_ratio, sample_point=320, sample_step=0.2, mode="bg", palette=None,
                 device="cuda"):
        if mode not in O.ORS_MODES:
            raise ValueError("mode must be one of %s, got %r" % (", ".join(O.ORS_MODES), mode))
        if isinstance(sample_point, bool) or int(sample_point) != sample_point or sample_point <= 0:
            raise ValueError("sample_point must be a positive int, got %r" % (sample_point,))
        if not float(sample_step) > 0:
            raise ValueError("sample_step must be positive, got %r" % (sample_step,))
        palette = OCC_COLORS if palette is None else palette
        try:
            rows = tuple(tuple(int(c) for c in row) for row in palette)
        except (TypeError, ValueError):
            raise ValueError("palette must be 18 (r, g, b) byte triples, got %r" % (palette,))
        if len(rows) != 18 or any(len(r) != 3 or any(not 0 <= c <= 255 for c in r) for r in rows):
            raise ValueError("palette must be 18 (r, g, b) byte triples: one per Occ3D class 0 .. 16 and one for 17, no hit")
        self.mode, self.palette = mode, rows
        self.projector = OccupancyRay(image_shape=tuple(image_shape), sample_point=int(sample_point),
                                      sample_step=float(sample_step), compress_ratio=compress_ratio, device=device)
        if min(self.projector.image_shape_compress) <= 0:
            raise ValueError("image_shape %r at compress_ratio %r leaves no pixel" % (tuple(image_shape), compress_ratio))

    @classmethod
    def for_image_size(cls, size, **kw):
        """cfg.dataset.image_size -> the render whose panoramas `occ_condition_from_config(cfg)` takes for that size:
        [224, 400] and [192, 384]: image_shape (896, 1600), ratio 400 / 1600 (the `h = 896` note of occ3d_proj.py:144);
        [432, 768] and [256, 704]: image_shape (900, 1600), ratio 768 / 1600.  The HD geometry is THIS project's choice: the
        reference states none for occ_bg_hd; 900 x 1600 is the camera picture and gives 432 x 768 without a remainder.
        compress_ratio=...: the same cameras at another scale (a preview; such panoramas are not the size's own)."""
        scale = kw.pop("compress_ratio", None)
        try:
            key = tuple(int(v) for v in size)
        except (TypeError, ValueError):
            key = None
        if key not in _GEOMETRY:
            raise ValueError("image_size %r: the image-mode ORS condition is defined for [224, 400], [192, 384], [432, 768] "
                             "and [256, 704]" % (size,))
        shape, ratio = _GEOMETRY[key]
        if scale is not None:
            return cls(shape, scale, **kw)
        self = cls(shape, ratio, **kw)
        want = [224, 400] if key in ((224, 400), (192, 384)) else [432, 768]
        assert self.projector.image_shape_compress == want, (self.projector.image_shape_compress, want)
        return self

    @property
    def view_hw(self):
        return tuple(self.projector.image_shape_compress)

    def _rigs(self, volumes, rigs):
        b = volumes.shape[0] if torch.is_tensor(volumes) and volumes.dim() == 4 else len(volumes)
        if len(rigs) == 2 and len(rigs[0]) and len(tuple(rigs[0][0].shape if hasattr(rigs[0][0], "shape") else ())) == 2:
            return [tuple(rigs)] * b                                   # one (intrinsics, extrinsics) for the whole batch
        return rigs

    @torch.no_grad()
    def __call__(self, volumes, rigs):
        """volumes: b class volumes 200 x 200 x 16 (a list of arrays / tensors, or one (b, 200, 200, 16) tensor); rigs: a
        list of b (intrinsics, extrinsics) pairs — per camera a 3 x 3 and a 4 x 4 camera-to-ego matrix, as
        `OccupancyRay.rays` takes them, arrays or tensors — or ONE such pair for all.  -> (b, h, n * w, 3) uint8 on the
        device."""
        return self.projector.render_batch(volumes, self._rigs(volumes, rigs), mode=self.mode, palette=self.palette)[0]

    @torch.no_grad()
    def classes(self, volumes, rigs):
        """The first-hit classes themselves: (b, n, h, w) uint8, 17 where a ray hits nothing."""
        return self.projector.render_batch(volumes, self._rigs(volumes, rigs), mode=self.mode, palette=self.palette,
                                           want_frames=False, want_classes=True)[1]

    @torch.no_grad()
    def overlay(self, frames, camera_frames, check=True):
        """The panoramas blended over camera panoramas of the same shape (occ3d_proj.py:196-203; the caller resizes the
        camera pictures): uint8 (b, h, n * w, 3).  check=True reads the 4-byte flags word back and raises ValueError where a
        sample's camera picture is constant (0 / 0 in the reference); check=False performs no host synchronisation."""
        out, flags = O.ors_overlay(frames, camera_frames)
        if check:
            word = int(flags.item())
            if word:
                raise ValueError("ORS overlay: " + "; ".join("bit %d: %s" % (bit.bit_length() - 1, text)
                                                              for bit, text in O.ORS_OVERLAY_FLAGS if word & bit))
        return out
