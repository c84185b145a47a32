"""The whole InceptionV3 on the HIP path against the float64 restatement (tests/inception_reference.py, parity unpinned,
seeded weights), under the rule the project uses for the VAEs (tests/test_vae_gpu.py):

    e(HIP) <= max(1e-3, 1.5 * e_floor)

e = relative L2 error against the float64 restatement; e_floor = the same restatement run under
oracle.numerics.storage_emulation at the storage type.  That the seeded network is alive for these inputs (at least
half of the pooled features non-zero, no constant feature map) is checked in tests/test_fid_cpu.py.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle.numerics import storage_emulation
from tests import inception_reference as R

pytestmark = pytest.mark.gpu
DTYPES = [torch.float16, torch.bfloat16]
DIMS = (64, 192, 768, 2048)


def rel_l2(y, ref):
    y, ref = y.detach().double().cpu(), ref.double()
    return ((y - ref).norm() / (ref.norm() + 1e-20)).item()


@pytest.fixture(scope="module")
def references():
    """Per case: images, the float64 feature maps and the emulated ones per storage type — computed once, never changed."""
    torch.set_num_threads(16)
    out = {}
    for name in R.NETWORK_CASES:
        net, x = R.network_case(name)
        with torch.no_grad():
            ref = net(x.double())
            emul = {}
            for dt in DTYPES:
                with storage_emulation(net, dt):
                    emul[dt] = net(x.double())
        out[name] = (x, ref, emul)
    return out


def _hip(name, dtype, blocks=(0, 1, 2, 3)):
    from dualdiff_amd.networks.inception import InceptionV3
    net = InceptionV3(output_blocks=blocks, resize_input=R.NETWORK_CASES[name][0], dtype=dtype)
    net.load_state_dict(R.seeded_state_dict(R.WEIGHT_SEED))
    return net.to("cuda")


def _check(what, y, ref, emul, dtype):
    e, fl = rel_l2(y, ref), rel_l2(emul, ref)
    bound = max(1e-3, 1.5 * fl)
    print("%-44s %-8s e_hip=%.3e e_floor=%.3e bound=%.3e" % (what, str(dtype).split(".")[-1], e, fl, bound))
    assert torch.isfinite(y).all()
    assert e <= bound, (what, e, fl)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", sorted(R.NETWORK_CASES))
def test_feature_maps_and_pooled_features(gpu, references, name, dtype):
    x, ref, emul = references[name]
    net = _hip(name, dtype)
    xd = x.cuda()
    outs = net(xd)
    assert len(outs) == 4
    for b, (y, r, em) in enumerate(zip(outs, ref, emul[dtype])):
        assert y.dtype == torch.float32 and tuple(y.shape) == tuple(r.shape), (b, y.shape, r.shape)
        _check("%s block %d map" % (name, b), y, r, em, dtype)
    for d, r, em in zip(DIMS, ref, emul[dtype]):
        f = net.features(xd, d)
        assert f.dtype == torch.float32 and tuple(f.shape) == (x.shape[0], d)
        _check("%s features dims=%d" % (name, d), f, F.adaptive_avg_pool2d(r, 1).flatten(1),
               F.adaptive_avg_pool2d(em, 1).flatten(1), dtype)
    # the same input twice gives the same bits (buffers are reused, nothing is left over from the call before)
    again = net(xd)
    for y, z in zip(outs, again):
        assert torch.equal(y, z)
    assert torch.equal(net.features(xd, 2048), net.features(xd, 2048))


@pytest.mark.parametrize("dtype", DTYPES)
def test_ragged_batch_gives_the_single_image_rows(gpu, dtype):
    """get_activations' last batch is smaller: m = 2 after m = 3 must give the rows of the single-image calls."""
    name = "noresize_3x75x91"
    x = R.seeded_images(*R.NETWORK_CASES[name][1:]).cuda()
    net = _hip(name, dtype, blocks=(3,))
    f3 = net.features(x)
    f2 = net.features(x[:2].contiguous())
    singles = torch.cat([net.features(x[i:i + 1].contiguous()) for i in range(3)])
    assert torch.equal(f3, singles) and torch.equal(f2, singles[:2])
    assert torch.equal(net.features(x), f3)                       # and the m = 3 buffers are still good afterwards


@pytest.mark.parametrize("dtype", DTYPES)
def test_statistics_from_files_equal_statistics_from_frames(gpu, tmp_path, dtype):
    """.jpg / .png bytes -> device decode -> FIDPreProcess -> features -> statistics equals the same call on the
    decoded frames: no frame leaves the device in between, and the file route adds nothing of its own."""
    from dualdiff_amd.pipeline.fid import FIDPreProcess, activation_statistics
    from dualdiff_amd.pipeline.image_output import encode_jpeg, encode_png
    from dualdiff_amd.pipeline.jpeg_input import load_jpeg
    g = torch.Generator().manual_seed(11)
    frames = torch.randint(0, 256, (6, 32, 48, 3), generator=g, dtype=torch.uint8).cuda()
    net = _hip("resize_1x37x52", dtype, blocks=(3,))
    pre = FIDPreProcess()
    for kind, files in (("png", encode_png(frames)), ("jpg", encode_jpeg(frames))):
        paths = []
        for i, data in enumerate(files):
            paths.append(str(tmp_path / ("%s_%d.%s" % (kind, i, kind))))
            with open(paths[-1], "wb") as f:
                f.write(data)
        decoded = frames if kind == "png" else load_jpeg(paths)     # PNG is lossless: the decoded frames ARE the frames
        mu_f, s_f = activation_statistics(paths, net, pre, batch_size=4)
        mu_d, s_d = activation_statistics(decoded, net, pre, batch_size=4)
        assert mu_f.shape == (2048,) and s_f.shape == (2048, 2048) and mu_f.dtype == np.float64
        assert np.array_equal(mu_f, mu_d) and np.array_equal(s_f, s_d), kind
        assert np.isfinite(mu_f).all() and float(np.abs(mu_f).sum()) > 0
