"""FID on the GPU: what the reference's evaluation step tools/fid_score.py does with a set of generated and a set of real
camera files, from the file bytes to the distance.

    model = InceptionV3().to("cuda"); model.load_state_dict(torch.load("pt_inception-2015-12-05.pth"))
    pre = FIDPreProcess.from_config(cfg)                       # fid_score.py:477-484; FIDPreProcess() = ToTensor alone
    mu1, s1 = activation_statistics(files_a, model, pre)       # :216-241
    mu2, s2 = activation_statistics(files_b, model, pre)
    fid = frechet_distance(mu1, s1, mu2, s2)                   # :159-213
    fid = fid_given_paths([dir_a, dir_b_or_npz], model)        # :260-276, the `paths` entry point

The reference opens every file with PIL, resizes on the host, runs batches of 50 through the Inception network in fp32
and ends with np.cov and scipy.linalg.sqrtm.  Here the files are decoded on the device (pipeline/jpeg_input.py,
png_input.py), the transform is the PIL-exact ImagePreProcess, the network is networks/inception.py (16-bit
activations, fp32 accumulation, fp32 BatchNorm and fp32 pooled features) and the statistics are float64 on the device:
no frame leaves the device between the file bytes and (mu, sigma).  The distance itself is a few small float64
eigenproblems on the host, without scipy.

frechet_distance and the reference: Tr((s1 s2)^1/2) is the sum of the square roots of the eigenvalues of the symmetric
matrix s1^1/2 s2 s1^1/2 (similar to s1 s2), and those square roots are the singular values of s2^1/2 s1^1/2.  The two
roots come from two numpy.linalg.eigh calls with negative round-off eigenvalues clamped to 0, the trace from one
numpy.linalg.svd of their product.  (Taking eigh of s1^1/2 s2 s1^1/2 instead and then the square roots turns the
2^-53-relative noise of every ZERO eigenvalue into 2^-26.5: for two identical 2048-dimensional covariances of 12 samples
that form returned -1.3e-3 where this one returns 3e-11 — singular values carry the noise unsquared.)  The reference
takes scipy's sqrtm of the non-symmetric product s1 s2.  For full-rank,
well-conditioned covariances both agree to round-off (tests/test_fid_cpu.py holds this form to the reference's own
noise).  They differ where the product is singular — rank-deficient covariances, fewer samples than dims: sqrtm of a
singular matrix returns round-off noise of unpredictable size, sometimes non-finite (the reference then adds eps = 1e-6
to both diagonals and retries, fid_score.py:196-201) and sometimes with an imaginary part (:204-208).  The symmetric
form has none of these cases: zero eigenvalues contribute exactly zero, nothing is retried and nothing is complex.

Not built: the nuScenes token walk of calculate_fid_given_tokens (:297-340) — file lists are the caller's.
"""
import os

import numpy as np
import torch

from .image_input import ImagePreProcess
from .image_output import _get
from .jpeg_input import load_jpeg
from .png_input import load_png

IN_SIZE = (900, 1600)                       # fid_score.py:477: the camera frames the resize ratio applies to
JPEG_EXTENSIONS = ("jpg", "jpeg")
PNG_EXTENSIONS = ("png",)
# the other kinds the reference's IMAGE_EXTENSIONS lists have no decoder here: such a file is an error, not skipped
UNBUILT_EXTENSIONS = ("bmp", "pgm", "ppm", "tif", "tiff", "webp")


def top_center_crop_box(size, target_size):
    """PIL box of fid_score.py:363-370: size = (newH, newW) of the resized image, target_size = (fH, fW): the rows above
    the bottom fH are cut, the columns are centred."""
    newH, newW = (int(v) for v in size)
    fH, fW = (int(v) for v in target_size)
    crop_h = newH - fH
    crop_w = int(max(0, newW - fW) / 2)
    return (crop_w, crop_h, crop_w + fW, crop_h + fH)


class FIDPreProcess(ImagePreProcess):
    """The transform of fid_score.py:477-484 on uint8 device frames (m, H, W, 3) -> float32 (m, 3, fH, fW) in [0, 1]:
    PIL's bicubic resize to `resize` = (h, w), the crop `box`, ToTensor (mean 0, std 1).  FIDPreProcess() is ToTensor
    alone, the `paths` mode (:121-122)."""

    def __init__(self, resize=None, box=None):
        self.identity = resize is None
        if self.identity:
            if box is not None:
                raise ValueError("a crop box needs the resize it refers to")
            self.resize = self.box = None
            self.dtype = torch.float32
            self.mean, self.std = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
        else:
            super().__init__(resize, box, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0), dtype=torch.float32)

    @classmethod
    def from_config(cls, cfg, in_size=IN_SIZE):
        """cfg: the reference's config (mapping or object) with dataset.image_size and dataset.augment2d.resize."""
        ds = _get(cfg, "dataset")
        if ds is None:
            raise ValueError("config has no `dataset` section")
        image_size = _get(ds, "image_size")
        aug = _get(ds, "augment2d")
        lim = None if aug is None else _get(aug, "resize")
        if image_size is None or lim is None:
            raise ValueError("config has no dataset.image_size / dataset.augment2d.resize")
        r = float(np.mean([float(v) for v in lim[0]]))
        size = (int(in_size[0] * r), int(in_size[1] * r))
        return cls(resize=size, box=top_center_crop_box(size, image_size))

    def __call__(self, frames):
        if not self.identity:
            return super().__call__(frames)
        x = self._flat(frames)
        # ToTensor alone: the resize to the frame's own size is PIL's identity (every bicubic tap but the centre is zero)
        from .. import ops as O
        y = O.image_load_u8(x, (x.shape[1], x.shape[2]), None, self.mean, self.std, self.dtype)
        return y.view(*frames.shape[:2], *y.shape[1:]) if frames.dim() == 5 else y


class FIDStatistics:
    """Running collection of pooled features and their Gaussian statistics (fid_score.py:239-240)."""

    def __init__(self, dims=2048):
        self.dims = int(dims)
        self._chunks = []
        self.mu = self.sigma = None

    @property
    def count(self):
        return sum(c.shape[0] for c in self._chunks)

    def update(self, features):
        """features: (n, dims) fp32; kept where they are (on the device)."""
        if features.dim() != 2 or features.shape[1] != self.dims:
            raise ValueError("features must be (n, %d), got %s" % (self.dims, tuple(features.shape)))
        if features.dtype != torch.float32:
            raise ValueError("features must be fp32, got %s" % features.dtype)
        self._chunks.append(features.detach())
        self.mu = self.sigma = None

    def finalize(self):
        """-> (mu (dims,), sigma (dims, dims)) float64 numpy arrays: np.mean(act, axis=0) and np.cov(act, rowvar=False) —
        the mean and the centred two-pass covariance with divisor N - 1, in float64 where the features live."""
        n = self.count
        if n < 2:
            raise ValueError("a covariance needs at least 2 samples, got %d" % n)
        x = torch.cat([c.to(torch.float64) for c in self._chunks], dim=0)
        mu = x.mean(dim=0)
        x -= mu
        sigma = (x.t() @ x) / (n - 1)
        self.mu, self.sigma = mu.cpu().numpy(), sigma.cpu().numpy()
        return self.mu, self.sigma

    def save(self, path):
        """The reference's statistics file (fid_score.py:360): a compressed .npz with `mu` and `sigma`."""
        if self.mu is None:
            self.finalize()
        np.savez_compressed(path, mu=self.mu, sigma=self.sigma)

    @classmethod
    def load(cls, path):
        """-> a finalized FIDStatistics holding the `mu` / `sigma` of a statistics file (fid_score.py:246-248)."""
        with np.load(path) as f:
            mu, sigma = np.asarray(f["mu"][:], dtype=np.float64), np.asarray(f["sigma"][:], dtype=np.float64)
        if mu.ndim != 1 or sigma.shape != (mu.shape[0], mu.shape[0]):
            raise ValueError("%s: mu %s and sigma %s do not belong together" % (path, mu.shape, sigma.shape))
        st = cls(mu.shape[0])
        st.mu, st.sigma = mu, sigma
        return st


def _sqrt_psd_eigh(s):
    w, v = np.linalg.eigh(s)
    return (v * np.sqrt(np.clip(w, 0.0, None))) @ v.T


def frechet_distance(mu1, sigma1, mu2, sigma2):
    """|mu1 - mu2|^2 + Tr(s1 + s2 - 2 (s1 s2)^1/2) in float64 on the host (module docstring: the symmetric form)."""
    mu1, mu2 = np.atleast_1d(np.asarray(mu1, dtype=np.float64)), np.atleast_1d(np.asarray(mu2, dtype=np.float64))
    s1, s2 = np.atleast_2d(np.asarray(sigma1, dtype=np.float64)), np.atleast_2d(np.asarray(sigma2, dtype=np.float64))
    if mu1.shape != mu2.shape or mu1.ndim != 1:
        raise ValueError("mean vectors have different lengths: %s, %s" % (mu1.shape, mu2.shape))
    if s1.shape != s2.shape or s1.shape != (mu1.shape[0], mu1.shape[0]):
        raise ValueError("covariances %s, %s do not fit means of length %d" % (s1.shape, s2.shape, mu1.shape[0]))
    r1, r2 = _sqrt_psd_eigh((s1 + s1.T) * 0.5), _sqrt_psd_eigh((s2 + s2.T) * 0.5)
    tr_covmean = np.linalg.svd(r2 @ r1, compute_uv=False).sum()
    diff = mu1 - mu2
    return float(diff.dot(diff) + np.trace(s1) + np.trace(s2) - 2.0 * tr_covmean)


def _ext(path):
    return os.path.splitext(os.fspath(path))[1][1:].lower()


def _load_files(paths, device):
    """A batch of .jpg / .png paths -> uint8 frames (n, H, W, 3) on the device, in the order given."""
    kinds = [_ext(p) for p in paths]
    for p, k in zip(paths, kinds):
        if k not in JPEG_EXTENSIONS + PNG_EXTENSIONS:
            raise ValueError("%s: only .jpg / .jpeg / .png files are decoded on the device" % (p,))
    parts, at = [], 0
    while at < len(paths):                                   # runs of one kind keep the order
        end = at
        while end < len(paths) and (kinds[end] in PNG_EXTENSIONS) == (kinds[at] in PNG_EXTENSIONS):
            end += 1
        loader = load_png if kinds[at] in PNG_EXTENSIONS else load_jpeg
        parts.append(loader(list(paths[at:end]), device=device))
        at = end
    return parts[0] if len(parts) == 1 else torch.cat(parts, dim=0)


@torch.no_grad()
def activation_statistics(source, model, pre=None, batch_size=50, dims=2048, device="cuda", stats=None):
    """calculate_activation_statistics (fid_score.py:216-241).  source: uint8 frames (n, H, W, 3) on the device, or a
    list of .jpg / .png paths (decoded on the device, a batch at a time).  pre: FIDPreProcess (default: ToTensor alone).
    -> (mu, sigma) float64 numpy arrays.  stats: a FIDStatistics to add to (the features stay in it)."""
    pre = FIDPreProcess() if pre is None else pre
    stats = FIDStatistics(dims) if stats is None else stats
    if batch_size < 1:
        raise ValueError("batch_size must be positive")
    is_frames = torch.is_tensor(source)
    if is_frames:
        if source.dim() != 4 or source.shape[-1] != 3 or source.dtype != torch.uint8:
            raise ValueError("frames must be uint8 (n, H, W, 3), got %s %s" % (tuple(source.shape), source.dtype))
        if not source.is_cuda:
            raise RuntimeError("dualdiff_amd ops run on the GPU only (got a %s tensor); there is no CPU fallback"
                               % source.device)
    n = len(source)
    if n == 0:
        raise ValueError("no images")
    for at in range(0, n, batch_size):
        chunk = source[at:at + batch_size]
        frames = chunk if is_frames else _load_files(chunk, device)
        stats.update(model.features(pre(frames), dims))
    return stats.finalize()


def image_files(root):
    """Every image file under `root`, sorted, as compute_statistics_of_path lists them (fid_score.py:250-253)."""
    found, unbuilt = [], []
    for base, _dirs, names in os.walk(os.fspath(root)):
        for name in names:
            k = _ext(name)
            if k in JPEG_EXTENSIONS + PNG_EXTENSIONS:
                found.append(os.path.join(base, name))
            elif k in UNBUILT_EXTENSIONS:
                unbuilt.append(os.path.join(base, name))
    if unbuilt:
        raise ValueError("%s holds image kinds with no device decoder, e.g. %s" % (root, sorted(unbuilt)[0]))
    return sorted(found)


def statistics_of_path(path, model, pre=None, batch_size=50, dims=2048, device="cuda"):
    """compute_statistics_of_path (fid_score.py:244-257): a .npz statistics file, or a directory of images."""
    path = os.fspath(path)
    if path.endswith(".npz"):
        st = FIDStatistics.load(path)
        if st.dims != dims:
            raise ValueError("%s holds %d-dimensional statistics, not %d" % (path, st.dims, dims))
        return st.mu, st.sigma
    files = image_files(path)
    if not files:
        raise ValueError("%s holds no .jpg / .png file" % path)
    return activation_statistics(files, model, pre, batch_size, dims, device)


def fid_given_paths(paths, model, pre=None, batch_size=50, dims=2048, device="cuda"):
    """calculate_fid_given_paths (fid_score.py:260-276): two directories of images or .npz statistics files -> FID."""
    if len(paths) != 2:
        raise ValueError("fid_given_paths takes two paths")
    for p in paths:
        if not os.path.exists(p):
            raise RuntimeError("Invalid path: %s" % p)
    m1, s1 = statistics_of_path(paths[0], model, pre, batch_size, dims, device)
    m2, s2 = statistics_of_path(paths[1], model, pre, batch_size, dims, device)
    return frechet_distance(m1, s1, m2, s2)


def save_fid_stats(paths, model, pre=None, batch_size=50, dims=2048, device="cuda"):
    """save_fid_stats (fid_score.py:343-360): the statistics of paths[0] into the new file paths[1]."""
    if not os.path.exists(paths[0]):
        raise RuntimeError("Invalid path: %s" % paths[0])
    if os.path.exists(paths[1]):
        raise RuntimeError("Existing output file: %s" % paths[1])
    mu, sigma = statistics_of_path(paths[0], model, pre, batch_size, dims, device)
    np.savez_compressed(paths[1], mu=mu, sigma=sigma)
