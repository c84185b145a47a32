"""numpy / torch restatement of what the reference's dataset does to a camera frame before the VAE encoder sees it:
`ImageAug3D` (PIL `Image.resize` with the default bicubic filter, then `Image.crop`), torchvision's `ToTensor` and
`Normalize`, `collate_fn`'s `.float()` and the runner's cast to the weight dtype.

Independent of dualdiff_amd: the resize is tests/pil_resample_reference.py (pinned to PIL's bytes), the crop is a slice of
its result, the rest is torch's float32 arithmetic.  tests/test_image_input_cpu.py pins the whole of it to PIL and
torch (and to tests/golden/image_input.npz where PIL is absent); the GPU tests compare the kernel with it element for
element."""
import numpy as np
import torch

from tests import pil_resample_reference as R

IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
HALF = ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5))


def geometry(ori_shape, final_dim, resize_lim, bot_pct_lim=(0.0, 0.0)):
    """ImageAug3D.sample_augmentation with is_train false -> ((newH, newW), PIL box (left, top, right, bottom))."""
    H, W = ori_shape
    fH, fW = final_dim
    r = float(np.mean(resize_lim))
    newW, newH = int(W * r), int(H * r)
    crop_h = int((1 - np.mean(bot_pct_lim)) * newH) - fH
    crop_w = int(max(0, newW - fW) / 2)
    return (newH, newW), (crop_w, crop_h, crop_w + fW, crop_h + fH)


def crop_u8(img, size, box=None):
    """img (h, w, 3) uint8 -> the bytes of `Image.fromarray(img).resize(size[::-1]).crop(box)`, box inside the image."""
    out = R.resize(img, size)
    if box is None:
        return out
    left, top, right, bottom = box
    assert 0 <= left < right <= size[1] and 0 <= top < bottom <= size[0]
    return out[top:bottom, left:right]


def normalize(u8, mean, std):
    """(..., h, w, 3) uint8 -> (..., 3, h, w) float32: ToTensor's `.float().div(255)`, Normalize's `sub(mean).div(std)` with
    float32 mean / std tensors."""
    x = torch.from_numpy(np.ascontiguousarray(u8)).movedim(-1, -3).contiguous().to(torch.float32).div(255)
    m = torch.as_tensor(mean, dtype=torch.float32).view(3, 1, 1)
    s = torch.as_tensor(std, dtype=torch.float32).view(3, 1, 1)
    return x.sub(m).div(s)


def pixel_values(frames, size, box=None, mean=HALF[0], std=HALF[1], dtype=torch.float32):
    """frames (m, h, w, 3) uint8 numpy -> (m, 3, fH, fW) in `dtype` (one cast from float32, as `.to(weight_dtype)`)."""
    u8 = np.stack([crop_u8(im, size, box) for im in frames])
    return normalize(u8, mean, std).to(dtype)


def nhwc8(x):
    """(m, 3, h, w) -> (m * h * w, 8) channels-last rows, channels 3..7 zero."""
    m, c, h, w = x.shape
    out = torch.zeros((m * h * w, 8), dtype=x.dtype)
    out[:, :c] = x.permute(0, 2, 3, 1).reshape(-1, c)
    return out


# the reference's four configurations at 900 x 1600 frames: image_size, augment2d.resize[0] -> resized (h, w), box
CONFIGS = [((224, 400), (0.25, 0.25), (225, 400), (0, 1, 400, 225)),
           ((256, 704), (0.48, 0.48), (432, 768), (32, 176, 736, 432)),
           ((432, 768), (0.48, 0.48), (432, 768), (0, 0, 768, 432)),
           ((192, 384), (0.24, 0.24), (216, 384), (0, 24, 384, 216))]

# name, (h, w) of the frame, (h, w) of the resize, an off-origin box with odd offsets.  Ratio 4 (ksize 17), 1 / 0.24
# (ksize 19) and 1 / 0.48 (ksize 11) are the production ratios; every case with more than one tile of its ratio's tile
# size in both axes, or as many as its size allows.
CASES = [
    ("down4", (180, 320), (45, 80), (0, 1, 80, 45)),         # the 224 x 400 configuration, scaled down: one row off the top
    ("down4_odd", (180, 320), (45, 80), (3, 5, 71, 44)),
    ("down024", (150, 200), (36, 48), (5, 3, 48, 35)),
    ("down048", (50, 150), (24, 72), (3, 1, 70, 24)),
    ("down048_small", (50, 60), (24, 29), (1, 3, 28, 24)),
    ("down_both", (16, 20), (7, 9), (1, 1, 8, 6)),
    ("up_both", (8, 12), (19, 31), (1, 3, 30, 18)),
    ("keep_h", (9, 13), (9, 29), (3, 1, 28, 8)),
    ("keep_w", (5, 7), (23, 7), (1, 3, 6, 22)),
    ("tiny", (3, 2), (11, 9), (1, 1, 8, 10)),
]
KINDS = ("uniform", "0/255")


def frame(name, hw, kind, m=1):
    """The seeded frames of a case: (m, h, w, 3) uint8."""
    seed = 1000 + 10 * [c[0] for c in CASES].index(name) + KINDS.index(kind)
    return R.noise_u8((m, hw[0], hw[1], 3), kind, seed)
