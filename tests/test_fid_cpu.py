"""CPU-side checks of the FID path: the restatement's properties, the Frechet distance against the reference's own
values (tests/golden/fid.npz, minted by tests/golden/mint_fid.py), the transform's geometry, the statistics' host logic
and the argument validation of the new entry points on a machine without a GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

from dualdiff_amd.networks import inception as N
from dualdiff_amd.pipeline import fid as FID
from tests import inception_reference as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fid.npz")


# ---- restatement properties ---------------------------------------------------------------------------------------------

def test_bn_fold_equals_the_module_in_float64():
    torch.manual_seed(3)
    layer = R.BasicConv2d(16, 24, 3, padding=1).double().eval()
    with torch.no_grad():
        layer.bn.weight.uniform_(0.8, 1.2)
        layer.bn.bias.uniform_(-0.1, 0.1)
        layer.bn.running_mean.uniform_(-0.1, 0.1)
        layer.bn.running_var.uniform_(0.5, 1.5)
        x = torch.randn(2, 16, 5, 6, dtype=torch.float64)
        conv = layer.conv(x)
        scale, shift = N.fold_bn(layer.bn.weight, layer.bn.bias, layer.bn.running_mean, layer.bn.running_var, layer.bn.eps)
        assert scale.dtype == torch.float64
        folded = torch.relu(conv * scale[None, :, None, None] + shift[None, :, None, None])
        assert torch.allclose(folded, layer(x), rtol=0, atol=1e-14)


@pytest.mark.parametrize("cin,kh,kw", [(3, 3, 3), (48, 5, 5), (128, 1, 7), (80, 3, 3)])
def test_weight_packing_round_trips(cin, kh, kw):
    w = torch.randn(12, cin, kh, kw)
    p = N.pack_conv_weight(w)
    cp = -(-cin // 8) * 8
    assert p.shape == (12, kh * kw * cp)
    q = p.reshape(12, kh, kw, cp)
    assert torch.equal(q[3, kh - 1, 0, :cin], w[3, :, kh - 1, 0])          # [cout][ky][kx][cin]
    assert bool((q[..., cin:] == 0).all())                                 # the stem's padded channels
    assert torch.equal(N.unpack_conv_weight(p, cin, kh, kw), w)


@pytest.mark.parametrize("name", sorted(R.NETWORK_CASES))
def test_the_seeded_network_is_alive(name):
    """Precondition of tests/test_inception_gpu.py: a dead network would pass any error bound."""
    net, x = R.network_case(name)
    with torch.no_grad():
        outs = net(x.double())
    assert [o.shape[1] for o in outs] == [64, 192, 768, 2048]
    for o in outs:
        assert torch.isfinite(o).all() and float(o.std()) > 1e-3, "a feature map is constant"
    pooled = outs[3].flatten(1)
    assert int((pooled != 0).sum(dim=1).min()) >= 1024, (pooled != 0).sum(dim=1)


def test_load_state_dict_takes_the_pytorch_fid_keys():
    sd = R.seeded_state_dict(0)
    assert "Conv2d_1a_3x3.conv.weight" in sd and "Mixed_5b.branch1x1.bn.running_var" in sd
    assert "Mixed_7c.branch_pool.bn.num_batches_tracked" in sd
    full = dict(sd)
    full["fc.weight"], full["fc.bias"] = torch.zeros(1008, 2048), torch.zeros(1008)
    net = N.InceptionV3()
    assert set(net.state_dict()) == set(sd)
    net.load_state_dict(full)
    assert torch.equal(net.Mixed_6e.branch7x7dbl_5.conv.weight, sd["Mixed_6e.branch7x7dbl_5.conv.weight"])
    del full["Mixed_6a.branch3x3.bn.running_mean"]
    with pytest.raises(RuntimeError, match="Mixed_6a.branch3x3.bn.running_mean"):
        N.InceptionV3().load_state_dict(full)
    assert N.BLOCK_INDEX_BY_DIM == {64: 0, 192: 1, 768: 2, 2048: 3}


def test_conv_count_is_94():
    assert sum(isinstance(m, N.BasicConv2d) for m in N.InceptionV3().modules()) == 94


# ---- frechet_distance ------------------------------------------------------------------------------------------------------

def _floor(d, s1, s2):
    """A symmetric eigensolver's backward error on matrices of this size and scale, with a 2^9 margin."""
    return d * 2.0 ** -44 * (np.trace(s1) + np.trace(s2))


@pytest.mark.parametrize("d", [8, 64])
def test_frechet_distance_against_the_reference(d):
    g = np.load(GOLDEN)
    mu1, mu2, s1, s2 = (g["full_%d_%s" % (d, k)] for k in ("mu1", "mu2", "s1", "s2"))
    d12, d21 = float(g["full_%d_d12" % d]), float(g["full_%d_d21" % d])
    tol = max(8 * abs(d12 - d21), _floor(d, s1, s2))
    ours, swapped = FID.frechet_distance(mu1, s1, mu2, s2), FID.frechet_distance(mu2, s2, mu1, s1)
    print("dims %d: reference %.15g / %.15g, ours %.15g / %.15g, tol %.3g" % (d, d12, d21, ours, swapped, tol))
    assert abs(ours - d12) <= tol and abs(swapped - d12) <= tol


@pytest.mark.parametrize("d", [8, 64])
def test_frechet_distance_closed_form(d):
    g = np.load(GOLDEN)
    a, b, mu1, mu2 = (g["diag_%d_%s" % (d, k)] for k in ("a", "b", "mu1", "mu2"))
    exact = float(((mu1 - mu2) ** 2).sum() + ((np.sqrt(a) - np.sqrt(b)) ** 2).sum())
    tol = _floor(d, np.diag(a), np.diag(b))
    assert abs(FID.frechet_distance(mu1, np.diag(a), mu2, np.diag(b)) - exact) <= tol
    assert abs(float(g["diag_%d_d12" % d]) - exact) <= max(8 * abs(float(g["diag_%d_d12" % d]) - float(g["diag_%d_d21" % d])),
                                                           tol)       # the fixture itself agrees with the closed form


def test_frechet_distance_rank_deficient_is_finite_and_real():
    """N < dims: where the reference's sqrtm returns round-off noise, the symmetric form is exact zero eigenvalues."""
    rng = np.random.RandomState(1)
    x = rng.randn(5, 16)
    s = np.cov(x, rowvar=False)
    assert abs(FID.frechet_distance(x.mean(0), s, x.mean(0), s)) <= _floor(16, s, s)
    with pytest.raises(ValueError):
        FID.frechet_distance(np.zeros(3), np.eye(3), np.zeros(4), np.eye(4))


# ---- FIDPreProcess ---------------------------------------------------------------------------------------------------------

def test_fid_preprocess_from_config_matches_the_reference_geometry():
    cases = np.load(GOLDEN)["crop_cases"]
    assert len(cases) == 4
    for fh, fw, lo, hi, rh, rw, left, top, right, bottom in cases:
        cfg = {"dataset": {"image_size": [int(fh), int(fw)], "augment2d": {"resize": [[float(lo), float(hi)]]}}}
        pre = FID.FIDPreProcess.from_config(cfg)
        assert pre.resize == (int(rh), int(rw))
        assert pre.box == (int(left), int(top), int(right), int(bottom))
        assert pre.size == (int(fh), int(fw))
        assert tuple(pre.mean) == (0.0, 0.0, 0.0) and tuple(pre.std) == (1.0, 1.0, 1.0) and pre.dtype == torch.float32
    assert FID.FIDPreProcess().identity
    with pytest.raises(ValueError):
        FID.FIDPreProcess.from_config({"dataset": {}})


# ---- FIDStatistics ---------------------------------------------------------------------------------------------------------

def test_fid_statistics_host_logic(tmp_path):
    g = torch.Generator().manual_seed(4)
    a, b = torch.randn(5, 6, generator=g), torch.randn(3, 6, generator=g)
    st = FID.FIDStatistics(6)
    with pytest.raises(ValueError, match="at least 2"):
        st.finalize()
    st.update(a[:1])
    with pytest.raises(ValueError, match="at least 2"):
        st.finalize()
    st.update(a[1:])
    st.update(b)
    mu, sigma = st.finalize()
    act = torch.cat([a, b]).numpy().astype(np.float64)      # the reference collects into np.empty(...): float64
    assert mu.dtype == sigma.dtype == np.float64
    assert np.allclose(mu, np.mean(act, axis=0), rtol=0, atol=1e-14)
    assert np.allclose(sigma, np.cov(act, rowvar=False), rtol=0, atol=1e-14)
    path = str(tmp_path / "stats.npz")
    st.save(path)
    with np.load(path) as f:
        assert sorted(f.files) == ["mu", "sigma"]
    back = FID.FIDStatistics.load(path)
    assert np.array_equal(back.mu, mu) and np.array_equal(back.sigma, sigma) and back.dims == 6
    with pytest.raises(ValueError):
        st.update(torch.zeros(2, 5))
    with pytest.raises(ValueError):
        st.update(torch.zeros(2, 6, dtype=torch.float64))


def test_ops_fail_loudly_on_cpu_tensors():
    from dualdiff_amd import ops
    h = torch.float16
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.conv2d(torch.zeros(4, 8, dtype=h), torch.zeros(4, 8, dtype=h), torch.zeros(4), torch.zeros(4), 1, 2, 2, 1, 1)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.pool3x3(torch.zeros(9, 8, dtype=h), 1, 3, 3, "max_s2")
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.global_avgpool(torch.zeros(4, 8, dtype=h), 1, 4)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.inception_input(torch.zeros(1, 3, 4, 4), (5, 5))
    with pytest.raises(RuntimeError, match="GPU only"):
        N.InceptionV3().features(torch.zeros(1, 3, 8, 8))


# ---- validation without a GPU ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from dualdiff_amd import _build, _native
    if not os.path.exists(_build.lib_path()):
        pytest.skip("library not built (run __graft_entry__.build())")
    return _native.load(build_if_missing=False)


def _conv(lib, **kw):
    a = dict(x=16, w=16, scale=16, shift=16, out=16, ldc=64, c_off=0, m=1, h=8, wd=8, cin=32, cout=64, kh=3, kw=3, stride=1,
             pad_h=1, pad_w=1, relu=1, tile=0, dtype=0)
    a.update(kw)
    return lib.dd_conv2d_nhwc(a["x"], a["w"], a["scale"], a["shift"], a["out"], a["ldc"], a["c_off"], a["m"], a["h"], a["wd"],
                              a["cin"], a["cout"], a["kh"], a["kw"], a["stride"], a["pad_h"], a["pad_w"], a["relu"],
                              a["tile"], a["dtype"], None)


def test_conv2d_validates_before_any_launch(lib):
    for name in ("x", "w", "scale", "shift", "out"):
        assert _conv(lib, **{name: None}) == -1, name               # null pointers
    assert _conv(lib, kh=0) == -2 and _conv(lib, kh=8) == -2 and _conv(lib, kw=8, pad_w=0) == -2      # kernel 1..7
    assert _conv(lib, stride=3) == -2 and _conv(lib, stride=0) == -2
    assert _conv(lib, cin=3) == -2 and _conv(lib, cin=20) == -2                                       # cin % 8
    assert _conv(lib, cout=30) == -2
    assert _conv(lib, pad_h=2) == -2 and _conv(lib, pad_w=-1) == -2                                   # pad <= k / 2
    assert _conv(lib, ldc=63) == -1 and _conv(lib, c_off=4) == -1 and _conv(lib, c_off=-4) == -1      # slice must fit ldc
    assert _conv(lib, ldc=66) == -1                                                                     # ldc % 4
    assert _conv(lib, x=8) == -1 and _conv(lib, out=4) == -1                                          # alignment
    assert _conv(lib, dtype=2) == -1 and _conv(lib, tile=3) == -2
    assert _conv(lib, h=2, wd=2, kh=7, kw=7, pad_h=0, pad_w=0) == -1                                  # no output pixel
    assert _conv(lib, m=0) == -1
    assert lib.dd_conv2d_kernel_name(0, 64, 0, 0) == b"" and lib.dd_conv2d_kernel_name(10, 64, 9, 0) == b""
    assert lib.dd_conv2d_kernel_name(3200, 448, 0, 0) == b"dd_conv2d_kernel<_Float16, 64, 64>"
    assert lib.dd_conv2d_kernel_name(61250, 96, 0, 1) == b"dd_conv2d_kernel<__bf16, 128, 64>"


@pytest.mark.parametrize("dt", [3, -1, 2])
def test_new_launchers_reject_other_element_types(lib, dt):
    """What tests/test_launcher_validation_cpu.py asks of every 16-bit launcher in its tables, for the four entry points
    of csrc/conv2d.hip (their header parameter is `storage_type`; the input kernel's `in_type` also takes 2 = fp32)."""
    assert _conv(lib, dtype=dt) == -1
    assert lib.dd_pool3x3_nhwc(16, 16, 64, 0, 1, 8, 8, 64, 0, dt, None) == -1
    assert lib.dd_global_avgpool_nhwc(16, 16, 1, 4, 8, dt, None) == -1
    assert lib.dd_inception_input(16, 16, 1, 8, 8, 9, 9, 8, 1, 1, 2, dt, None) == -1
    if dt != 2:
        assert lib.dd_inception_input(16, 16, 1, 8, 8, 9, 9, 8, 1, 1, dt, 0, None) == -1
    assert lib.dd_conv2d_kernel_name(100, 64, 0, dt) == b""


def test_pools_and_input_validate_before_any_launch(lib):
    pool = lambda **kw: (lambda a: lib.dd_pool3x3_nhwc(a["x"], a["out"], a["ldc"], a["c_off"], a["m"], a["h"], a["wd"], a["c"],
                                                       a["mode"], a["dtype"], None))(
        {**dict(x=16, out=16, ldc=64, c_off=0, m=1, h=8, wd=8, c=64, mode=0, dtype=0), **kw})
    assert pool(x=None) == -1 and pool(out=None) == -1
    assert pool(mode=3) == -2 and pool(c=12) == -2
    assert pool(ldc=56) == -1 and pool(c_off=8) == -1 and pool(ldc=68) == -1
    assert pool(h=2) == -1 and pool(dtype=2) == -1 and pool(m=0) == -1
    assert lib.dd_global_avgpool_nhwc(None, 16, 1, 4, 8, 0, None) == -1
    assert lib.dd_global_avgpool_nhwc(16, None, 1, 4, 8, 0, None) == -1
    assert lib.dd_global_avgpool_nhwc(16, 16, 1, 0, 8, 0, None) == -1
    assert lib.dd_global_avgpool_nhwc(16, 16, 1, 4, 8, 2, None) == -1
    inp = lambda **kw: (lambda a: lib.dd_inception_input(a["x"], a["out"], a["m"], a["h"], a["wd"], a["oh"], a["ow"], a["c_pad"],
                                                         a["resize"], a["normalize"], a["in_dtype"], a["dtype"], None))(
        {**dict(x=16, out=16, m=1, h=8, wd=8, oh=299, ow=299, c_pad=8, resize=1, normalize=1, in_dtype=2, dtype=0), **kw})
    assert inp(x=None) == -1 and inp(out=None) == -1
    assert inp(c_pad=3) == -2 and inp(c_pad=12) == -2
    assert inp(resize=0) == -1                                      # resize = 0 needs oh == h, ow == wd
    assert inp(in_dtype=3) == -1 and inp(dtype=2) == -1 and inp(oh=0) == -1 and inp(out=8) == -1
