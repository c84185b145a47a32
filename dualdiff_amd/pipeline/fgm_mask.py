"""FGM loss mask on the GPU: `heatmap_gt`, the foreground mask of DualDiff's FGM loss, and the loss that consumes it.

With `use_aug_loss` the reference's `collate_fn` (magicdrive/dataset/utils.py:530-559) makes a foreground heat map per
camera view on the host: `_preprocess_bbox(..., use_3d_filter=False, for_mask=True)` gives the per-view box corners,
`create_heatmap_gt` (magicdrive/networks/utils.py:26-39, 100-163) projects every box's corners with `lidar2image` in
float64, truncates them to latent pixels, takes scipy's `ConvexHull` and asks matplotlib's `Polygon.contains_point` once
per latent pixel in a Python double loop; a painted pixel gets the weight `1 - area / (W * H)` of its box (small objects
weigh more), a view's map is the maximum over its boxes, and `hd_crop` cuts the map to the latent size of the cropped
image sizes.  The training step then uses it in two lines (runner/multiview_runner.py:506-507):

    loss = F.mse_loss(model_pred.float(), target.float(), reduction='none')
    loss = loss.mean() + (loss * batch['heatmap_gt'][0].unsqueeze(2)).mean()

Here both run on the device: the mask in two launches with no host synchronisation (`ops.fgm_mask`), the loss and its
gradient in one pass over the prediction (`ops.fgm_loss`).

    pre = BoxPreProcess(bbox_mode, use_3d_filter=False, canvas_size=image_size)          # box_input.py
    for_mask = pre(filter_corners, labels, compose_transforms(lidar2image, img_aug_matrix))   # the re-centred corners
    fgm = FgmMask.from_config(cfg)
    heat = fgm(for_mask["bboxes"], for_mask["masks"], lidar2image)                       # heatmap_gt[0]
    loss = fgm_loss(model_pred, target, heat)                                            # the two lines above

scipy and matplotlib are not imported: the hull is computed on the device (eight points at most) and the rule is
restated in integers (csrc/fgm_mask_core.h; INTEGRATION.md §4w has it in words).

UNSUPPORTED BOXES: a box with a corner whose projection is not finite, or with a corner in front of the camera whose
latent coordinate truncates beyond 2^25 in magnitude, is not painted and is counted in `flags`.  It takes a corner within
about 1e-5 of the camera plane to get there; beyond that bound the reference's own float64 crossing test is no longer
exact and its integer cast is undefined.  `check=True` reads the count back and raises.
"""
import torch

from .. import ops as O
from .image_output import _get

__all__ = ["FgmMask", "fgm_loss", "IMAGE_SIZES"]

# dataset/utils.py:539-559: image_size (H, W) -> (resolution (W, H) of create_heatmap_gt, hd_crop's out_shape or None)
IMAGE_SIZES = {(224, 400): ((50, 28), None), (192, 384): ((48, 27), (24, 48)), (432, 768): ((96, 54), None),
               (256, 704): ((96, 54), (32, 88))}


def _pair(v, what):
    try:
        a, b = (int(x) for x in v)
    except (TypeError, ValueError):
        raise ValueError("%s must be two integers, got %r" % (what, v))
    if a < 1 or b < 1:
        raise ValueError("%s must be positive, got %r" % (what, v))
    return a, b


class FgmMask:
    """resolution: (W, H) of the latent grid the boxes are painted on; crop: (H_out, W_out) kept of it as `hd_crop` keeps
    them (the bottom rows, the middle columns), or None; source_size: (W, H) of the camera images `lidar2image` maps to."""

    def __init__(self, resolution=(50, 28), crop=None, source_size=(1600, 900)):
        self.resolution = _pair(resolution, "resolution")
        self.source_size = _pair(source_size, "source_size")
        width, height = self.resolution
        if width * height > O.FGM_MAX_PIXELS:
            raise ValueError("a grid of %d x %d is more than %d pixels" % (width, height, O.FGM_MAX_PIXELS))
        self.crop = None if crop is None else _pair(crop, "crop")
        if self.crop is not None:
            ho, wo = self.crop
            if ho > height or wo > width:
                raise ValueError("crop (H_out, W_out) = %r is larger than the grid (H, W) = %r" % (self.crop, (height, width)))
            if (width - wo) % 2:
                raise ValueError("crop %r leaves an odd number of columns of %d: hd_crop takes the same number off each side"
                                 % (self.crop, width))
        # utils.py:137-138: Python float64 quotients
        self.scale = (width / self.source_size[0], height / self.source_size[1])
        self.flags = None

    @classmethod
    def from_config(cls, cfg, **kw):
        """cfg: any mapping (or object) with `dataset.image_size` = [H, W], one of the four sizes of dataset/utils.py:539-559."""
        ds = _get(cfg, "dataset")
        size = None if ds is None else _get(ds, "image_size")
        if size is None:
            raise ValueError("config has no dataset.image_size")
        key = tuple(int(v) for v in size)
        if key not in IMAGE_SIZES:
            raise ValueError("dataset.image_size %r has no FGM mask in the reference: the sizes are %s"
                             % (list(size), ", ".join(str(list(k)) for k in IMAGE_SIZES)))
        resolution, crop = IMAGE_SIZES[key]
        return cls(resolution=resolution, crop=crop, **kw)

    @property
    def out_shape(self):
        return self.crop if self.crop is not None else (self.resolution[1], self.resolution[0])

    @torch.no_grad()
    def __call__(self, bboxes, masks=None, lidar2image=None, check=False):
        """bboxes (b, n, m, P, 3) fp32 and masks (b, n, m) bool as `BoxPreProcess(use_3d_filter=False, canvas_size=...)`
        returns them from the re-centred corners — the synced dict's tensors or the `BoxViews` capacity layout (rows past a
        view's count have mask False and paint nothing), or the dict / BoxViews itself in place of both; None: no box is
        visible anywhere.  lidar2image (b, n, 4, 4) fp32: `torch.bmm(camera_intrinsics, lidar2camera)` per scene.
        -> heat (b, n, H_out, W_out) fp32 on the device, `heatmap_gt[0]`; `.flags` holds the (1,) int32 count of unsupported
        boxes, on the device.  check=True reads those 4 bytes back and raises ValueError where the count is not 0;
        check=False performs no host synchronisation."""
        if masks is None and bboxes is not None:
            if isinstance(bboxes, dict):
                bboxes, masks = bboxes["bboxes"], bboxes["masks"]
            elif hasattr(bboxes, "bboxes") and hasattr(bboxes, "masks"):
                bboxes, masks = bboxes.bboxes, bboxes.masks
            else:
                raise ValueError("masks (b, n, m) go with bboxes (b, n, m, P, 3)")
        if not isinstance(lidar2image, torch.Tensor) or lidar2image.dim() != 4 or tuple(lidar2image.shape[2:]) != (4, 4):
            raise ValueError("lidar2image must be a (b, n, 4, 4) tensor, got %s"
                             % ((tuple(lidar2image.shape) if isinstance(lidar2image, torch.Tensor) else type(lidar2image).__name__),))
        if not lidar2image.is_cuda:
            raise RuntimeError("lidar2image must be on the device (got a %s tensor): the mask is made there" % lidar2image.device)
        b, n = lidar2image.shape[:2]
        dev = lidar2image.device
        if bboxes is None:
            self.flags = torch.zeros((1,), dtype=torch.int32, device=dev)
            return torch.zeros((b, n) + self.out_shape, dtype=torch.float32, device=dev)
        if not (isinstance(bboxes, torch.Tensor) and isinstance(masks, torch.Tensor)):
            raise ValueError("bboxes and masks must be tensors")
        if bboxes.dim() != 5 or tuple(bboxes.shape[:2]) != (b, n) or tuple(masks.shape) != tuple(bboxes.shape[:3]):
            raise ValueError("bboxes must be (%d, %d, m, P, 3) and masks (%d, %d, m), got %s and %s"
                             % (b, n, b, n, tuple(bboxes.shape), tuple(masks.shape)))
        if not (bboxes.is_cuda and masks.is_cuda):
            raise RuntimeError("bboxes and masks must be on the device: BoxPreProcess leaves them there")
        heat, self.flags = O.fgm_mask(bboxes.to(torch.float32).contiguous(), masks.to(torch.bool).contiguous(),
                                      lidar2image.to(torch.float32).contiguous(), self.resolution, self.crop, self.scale)
        if check:
            count = int(self.flags.item())
            if count:
                raise ValueError("FGM mask: %d box(es) have a corner whose projection is not finite or lies beyond 2^25 latent "
                                 "pixels (a corner within ~1e-5 of the camera plane); they are not painted (check=False returns "
                                 "the count in .flags)" % count)
        return heat


class _FgmLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, heat):
        loss, grad = O.fgm_loss(pred.contiguous(), target.contiguous(), heat, want_grad=ctx.needs_input_grad[0])
        ctx.save_for_backward(grad)
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        (grad,) = ctx.saved_tensors
        return (grad * grad_out).to(grad.dtype), None, None


def fgm_loss(pred, target, heat=None):
    """The two loss lines of runner/multiview_runner.py:506-507 with `heat = batch['heatmap_gt'][0]`:

        loss = F.mse_loss(pred.float(), target.float(), reduction='none')
        loss = loss.mean() + (loss * heat.unsqueeze(2)).mean()

    as one kernel pass, sum((pred - target)^2 (1 + heat)) / N in fp32; heat=None is the plain mean (`use_aug_loss: false`).
    pred, target (b, n, c, h, w) fp16 / bf16 / fp32, heat (b, n, h, w) fp32, on the device.  -> a () fp32 tensor; the gradient
    goes to pred only (in pred's dtype, computed in the forward pass), target and heat are constants."""
    if heat is not None and heat.requires_grad or target.requires_grad:
        raise ValueError("fgm_loss differentiates with respect to pred only: detach target and heat")
    return _FgmLoss.apply(pred, target, None if heat is None else heat.contiguous())
