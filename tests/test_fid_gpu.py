"""FID statistics on the device against numpy, and fid_given_paths end to end against the float64 restatement."""
import numpy as np
import pytest
import torch

from oracle.numerics import storage_emulation
from tests import inception_reference as R

pytestmark = pytest.mark.gpu
DTYPES = [torch.float16, torch.bfloat16]


@pytest.mark.parametrize("dims,splits", [(64, (2,)), (64, (7,)), (64, (50, 13)), (2048, (2,)), (2048, (7,)), (2048, (50, 13))])
def test_statistics_against_numpy(gpu, dims, splits):
    """finalize() against np.mean / np.cov of the same fp32 features (float64, as the reference collects them).  Per entry
    a float64 dot product of N terms is within N 2^-53 sum |a_i| |b_i| of exact, so two of them differ by at most
    N 2^-52 sum |a_i| |b_i|; a, b = the centred columns, divided by N - 1 for sigma; a = the column, b = 1 / N for mu."""
    from dualdiff_amd.pipeline.fid import FIDStatistics
    n = sum(splits)
    g = torch.Generator().manual_seed(dims + n)
    feats = (torch.rand((n, dims), generator=g) * torch.rand((1, dims), generator=g) * 3).float()
    st = FIDStatistics(dims)
    at = 0
    for k in splits:
        st.update(feats[at:at + k].cuda())
        at += k
    mu, sigma = st.finalize()
    act = feats.numpy().astype(np.float64)
    mu_ref, sigma_ref = np.mean(act, axis=0), np.cov(act, rowvar=False)
    c = np.abs(act - mu_ref)
    b_mu = n * 2.0 ** -52 * np.abs(act).sum(axis=0) / n
    b_sigma = n * 2.0 ** -52 * (c.T @ c) / (n - 1)
    assert mu.dtype == np.float64 and sigma.shape == (dims, dims)
    assert (np.abs(mu - mu_ref) <= b_mu).all(), float((np.abs(mu - mu_ref) / b_mu).max())
    assert (np.abs(sigma - sigma_ref) <= b_sigma).all(), float((np.abs(sigma - sigma_ref) / b_sigma).max())


# ---- end to end ------------------------------------------------------------------------------------------------------------
E2E_DIMS = 768                                  # rank-deficient at 12 samples like 2048, and its eigenproblems are 19 x cheaper
RESIZE, BOX = (80, 96), (2, 5, 93, 80)          # 32 x 48 files -> PIL bicubic 80 x 96 -> crop 75 x 91, the smallest input of
#                                                 the network without its own resize (tests/inception_reference.py)


def _frames(seed):
    g = torch.Generator().manual_seed(seed)
    base = torch.randint(0, 256, (12, 4, 6, 3), generator=g).float()              # blocky content with some structure
    up = torch.nn.functional.interpolate(base.permute(0, 3, 1, 2), size=(32, 48), mode="bilinear", align_corners=False)
    noise = torch.randint(-20, 21, (12, 3, 32, 48), generator=g).float()
    return (up + noise).clamp(0, 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()


@pytest.fixture(scope="module")
def directories(tmp_path_factory):
    """Two sets of 12 seeded frames; per set the float64 restatement's E2E_DIMS features of the reference transform (PIL
    bicubic resize, crop, ToTensor) and, per storage type, the emulated ones — computed once."""
    from PIL import Image
    torch.set_num_threads(16)
    net = R.InceptionV3(output_blocks=(2,), resize_input=False).eval()
    net.load_state_dict(R.seeded_state_dict(R.WEIGHT_SEED))
    net = net.double()
    sets = []
    for seed in (21, 22):
        frames = _frames(seed)
        x = torch.stack([torch.from_numpy(np.array(Image.fromarray(f.numpy()).resize(RESIZE[::-1], Image.BICUBIC).crop(BOX)))
                         for f in frames]).permute(0, 3, 1, 2).double() / 255.0
        with torch.no_grad():
            ref = net.features(x, E2E_DIMS)
            emul = {}
            for dt in DTYPES:
                with storage_emulation(net, dt):
                    emul[dt] = net.features(x, E2E_DIMS)
        sets.append((frames, ref, emul))
    return tmp_path_factory.mktemp("fid"), sets


def _stats(f):
    a = f.numpy().astype(np.float64)
    return np.mean(a, axis=0), np.cov(a, rowvar=False)


@pytest.mark.parametrize("dtype", DTYPES)
def test_fid_given_paths_end_to_end(gpu, directories, dtype):
    """fid_given_paths on two directories of .png files against frechet_distance of the float64 restatement's statistics.

    Tolerance.  The network test holds the features to ||F_hip - F|| <= B ||F|| with B = max(1e-3, 1.5 e_floor)
    (tests/test_inception_gpu.py).  The distance is evaluated at features perturbed by that bound: each set scaled by
    (1 + s B) for the four sign pairs (s_a, s_b) — a common scale error moves mean and covariance of a set together,
    the direction the distance is most sensitive to — and each set moved by B ||F|| along a seeded random direction
    and along its own per-feature deviation from the set mean (which inflates the covariance); tol is the largest change
    of the distance among them plus frechet_distance's floor dims 2^-44 (tr s1 + tr s2).
    The 768-dimensional features (block 2) are used: the 2048-dimensional ones are held to the same bound in
    tests/test_inception_gpu.py, and a 2048 x 2048 distance costs 1.5 s per evaluation, of which this test needs 15."""
    from dualdiff_amd.networks.inception import InceptionV3
    from dualdiff_amd.pipeline.fid import FIDPreProcess, fid_given_paths, frechet_distance
    from dualdiff_amd.pipeline.image_output import save_png
    root, sets = directories
    dirs = []
    for i, (frames, _, _) in enumerate(sets):
        d = root / ("%s_set%d" % (str(dtype).split(".")[-1], i))
        save_png(frames.cuda(), [str(d / "sub" / ("%02d.png" % k)) for k in range(12)])
        dirs.append(str(d))
    net = InceptionV3(resize_input=False, dtype=dtype)
    net.load_state_dict(R.seeded_state_dict(R.WEIGHT_SEED))
    net = net.to("cuda")
    pre = FIDPreProcess(resize=RESIZE, box=BOX)
    got = fid_given_paths(dirs, net, pre, batch_size=5, dims=E2E_DIMS)

    (fa, fb) = (s[1] for s in sets)
    ref = frechet_distance(*_stats(fa), *_stats(fb))
    B = max(max(1e-3, 1.5 * float((s[2][dtype] - s[1]).norm() / s[1].norm())) for s in sets)
    g = torch.Generator().manual_seed(5)

    def moved(f, kind, sign):
        if kind == "scale":
            return f * (1 + sign * B)
        d = torch.randn(f.shape, generator=g, dtype=torch.float64) if kind == "random" else f - f.mean(dim=0)
        return f + sign * B * f.norm() * d / d.norm()

    changes = []
    for kind in ("scale", "random", "spread"):
        for sa in (1, -1):
            for sb in (1, -1):
                changes.append(abs(frechet_distance(*_stats(moved(fa, kind, sa)), *_stats(moved(fb, kind, sb))) - ref))
    floor = E2E_DIMS * 2.0 ** -44 * (np.trace(_stats(fa)[1]) + np.trace(_stats(fb)[1]))
    tol = max(changes) + floor
    print("fid %s: hip %.8g reference %.8g |diff| %.3g tol %.3g (B %.3g)" % (dtype, got, ref, abs(got - ref), tol, B))
    assert abs(got - ref) <= tol

    from dualdiff_amd.pipeline.fid import statistics_of_path
    same = fid_given_paths([dirs[0], dirs[0]], net, pre, batch_size=5, dims=E2E_DIMS)
    own = statistics_of_path(dirs[0], net, pre, batch_size=5, dims=E2E_DIMS)[1]
    assert abs(same) <= E2E_DIMS * 2.0 ** -44 * 2 * np.trace(own), same           # the floor of 0: both sets are the same set


def test_fid_given_paths_takes_npz_statistics(gpu, directories, tmp_path):
    from dualdiff_amd.pipeline.fid import FIDStatistics, fid_given_paths, frechet_distance
    _, sets = directories
    files = []
    for i, s in enumerate(sets):
        st = FIDStatistics(E2E_DIMS)
        st.update(s[1].float().cuda())
        files.append(str(tmp_path / ("s%d.npz" % i)))
        st.save(files[-1])
    a, b = FIDStatistics.load(files[0]), FIDStatistics.load(files[1])
    assert fid_given_paths(files, model=None, dims=E2E_DIMS) == frechet_distance(a.mu, a.sigma, b.mu, b.sigma)
    with pytest.raises(RuntimeError, match="Invalid path"):
        fid_given_paths([files[0], str(tmp_path / "missing")], model=None)
