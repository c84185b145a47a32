"""Image input on the GPU: uint8 camera frames as the `pixel_values` the reference's dataset hands to the VAE encoder.

What the reference's `test_pipeline` does to a camera frame (configs/dataset/Nuscenes.yaml:181-229): `ImageAug3D` with
`final_dim = image_size`, `resize_lim = augment2d.resize[0]`, `bot_pct_lim [0, 0]`, no rotation, no flip, `is_train:
false`, then `ImageNormalize` with mean and std 0.5.  In PIL and torch terms, for a frame of `ori_shape = (H, W)`,
`r = mean(resize_lim)` and `final_dim = (fH, fW)`:

    newW, newH = int(W * r), int(H * r)                                 # Python floats
    crop_h = int((1 - mean(bot_pct_lim)) * newH) - fH                   # bot_pct_lim = [0, 0]: rows cut from the TOP
    crop_w = int(max(0, newW - fW) / 2)
    box    = (crop_w, crop_h, crop_w + fW, crop_h + fH)                 # PIL box: left, top, right, bottom
    img    = pil_rgb.resize((newW, newH)).crop(box)                     # PIL's default filter for RGB: BICUBIC
    x      = ToTensor()(img)                                            # uint8 HWC -> float32 CHW, .div(255)
    x      = Normalize(mean, std)(x)                                    # (x - mean[c]) / std[c], float32

`collate_fn` stacks the views and calls `.float()` (dataset/utils.py:449-453); the runner casts to the weight dtype before
`vae.encode` (runner/base_runner.py:469-475).

Here that is one launch per batch of views (`ops.image_load_u8`), element for element: PIL's resample is integer
arithmetic over fixed-point tables (pipeline/image_output.py builds them as PIL does), the crop is a slice of those
tables, and ToTensor + Normalize have 256 possible inputs per channel, so they are a table built with torch's own
float32 ops.

    pre = ImagePreProcess.from_config(cfg, ori_shape=(900, 1600))    # cfg.dataset.image_size / .augment2d.resize
    pixel_values = pre(frames)                                       # (b, n_cam, 900, 1600, 3) uint8 -> (b, n_cam, 3, fH, fW)
    latents = encode_images(vae, frames, pre, given=given)           # == encode_pixel_values(vae, pre(frames), ...)

The frames come from the camera files through pipeline/jpeg_input.py (decode_jpeg / load_jpeg); the flip and rotation of
ImageAug3D's training mode stay with the caller.
"""
import torch

from .. import ops as O
from .image_output import _get


def aug3d_geometry(ori_shape, final_dim, resize, bot_pct=0.0):
    """ImageAug3D.sample_augmentation with `is_train: false`: -> ((newH, newW), (left, top, right, bottom))."""
    H, W = (int(v) for v in ori_shape)
    fH, fW = (int(v) for v in final_dim)
    r = float(resize)
    newW, newH = int(W * r), int(H * r)
    crop_h = int((1 - float(bot_pct)) * newH) - fH
    crop_w = int(max(0, newW - fW) / 2)
    return (newH, newW), (crop_w, crop_h, crop_w + fW, crop_h + fH)


class ImagePreProcess:
    """The reference's test-time image transform on GPU tensors: uint8 frames (b, n, H, W, 3) or (m, H, W, 3) ->
    `pixel_values` (b, n, 3, fH, fW) / (m, 3, fH, fW) in `dtype`.  resize = (newH, newW) of PIL's bicubic resize; box =
    PIL's (left, top, right, bottom) inside the resized image, default all of it; mean / std = Normalize's, one per
    channel."""

    def __init__(self, resize, box=None, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5), dtype=torch.float32):
        if isinstance(resize, int):
            raise ValueError("resize must be (h, w); the shorter-edge form of Resize(int) is not built")
        resize = tuple(int(v) for v in resize)
        if len(resize) != 2 or min(resize) <= 0:
            raise ValueError("resize must be a positive (h, w), got %r" % (resize,))
        box = (0, 0, resize[1], resize[0]) if box is None else tuple(int(v) for v in box)
        if len(box) != 4 or not (0 <= box[0] < box[2] <= resize[1] and 0 <= box[1] < box[3] <= resize[0]):
            raise ValueError("box %r is empty or leaves the %d x %d (w x h) resized image; the black border PIL's crop "
                             "would add there is not built" % (box, resize[1], resize[0]))
        self.resize, self.box, self.dtype = resize, box, dtype
        self.mean, self.std = O._image_mean_std(mean, std)

    @property
    def size(self):
        """(fH, fW) of the result."""
        return self.box[3] - self.box[1], self.box[2] - self.box[0]

    @classmethod
    def from_config(cls, cfg, ori_shape, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5), dtype=torch.float32):
        """cfg: any mapping (or object) with `dataset.image_size` = (fH, fW) and `dataset.augment2d.resize` = [[lo, hi], ..]
        — the reference's config; ori_shape = (H, W) of the camera frames."""
        ds = _get(cfg, "dataset")
        if ds is None:
            raise ValueError("config has no `dataset` section")
        image_size = _get(ds, "image_size")
        aug = _get(ds, "augment2d")
        lim = None if aug is None else _get(aug, "resize")
        if image_size is None or lim is None:
            raise ValueError("config has no dataset.image_size / dataset.augment2d.resize")
        lim = [float(v) for v in lim[0]]
        resize, box = aug3d_geometry(ori_shape, image_size, sum(lim) / len(lim))
        return cls(resize=resize, box=box, mean=mean, std=std, dtype=dtype)

    def _flat(self, frames):
        if frames.dim() not in (4, 5) or frames.shape[-1] != 3:
            raise ValueError("frames must be (b, n, H, W, 3) or (m, H, W, 3), got %s" % (tuple(frames.shape),))
        if frames.dtype != torch.uint8:
            raise ValueError("frames must be uint8, got %s" % frames.dtype)
        return (frames.flatten(0, 1) if frames.dim() == 5 else frames).contiguous()

    def __call__(self, frames):
        x = self._flat(frames)
        y = O.image_load_u8(x, self.resize, self.box, self.mean, self.std, self.dtype)
        return y.view(*frames.shape[:2], *y.shape[1:]) if frames.dim() == 5 else y

    def nhwc8(self, frames, dtype):
        """(m, H, W, 3) uint8 -> (m * fH * fW, 8) channels-last rows in `dtype`, channels 3..7 zero: conv_in's input."""
        return O.image_load_u8(self._flat(frames), self.resize, self.box, self.mean, self.std, dtype, layout="nhwc8")


@torch.no_grad()
def encode_images(vae, frames, pre, generator=None, sample_posterior=True, given=None):
    """uint8 frames (b, n_cam, H, W, 3) -> latents (b, n_cam, 4, fH/8, fW/8) fp32: `encode_pixel_values(vae, pre(frames),
    generator, sample_posterior, given)` bit for bit, with the kernel writing conv_in's channels-last input in the model
    dtype (neither the fp32 pixel_values nor the NCHW -> NHWC pass exists).  Only the `given` views are pre-processed
    and encoded; the other entries are zero."""
    if frames.dim() != 5 or frames.shape[-1] != 3 or frames.dtype != torch.uint8:
        raise ValueError("frames must be uint8 (b, n, H, W, 3), got %s %s" % (tuple(frames.shape), frames.dtype))
    b, n = frames.shape[:2]
    fh, fw = pre.size
    if fh % 8 or fw % 8:
        raise ValueError("image height and width must be multiples of 8, got %d x %d" % (fh, fw))
    if given is not None and (tuple(given.shape) != (b, n) or given.dtype != torch.bool):
        raise ValueError("given must be a (%d, %d) bool tensor" % (b, n))
    if not frames.is_cuda:
        raise RuntimeError("the VAE encoder runs on the GPU only")
    x = frames.flatten(0, 1)
    idx = None
    if given is not None:
        idx = given.reshape(-1).nonzero().flatten().to(x.device)
        x = x.index_select(0, idx)
    out = torch.zeros((b * n, 4, fh // 8, fw // 8), dtype=torch.float32, device=frames.device)
    m = x.shape[0]
    if m > 0:
        dist = vae.encode_nhwc8(pre.nhwc8(x, vae.dtype), m, fh, fw).latent_dist
        lat = dist.latents(generator, sample_posterior, scale=vae.scaling_factor, out_f32=True)
        if idx is None:
            out = lat
        else:
            out.index_copy_(0, idx, lat)
    return out.view(b, n, 4, fh // 8, fw // 8)
