"""Image output without a GPU: the numpy restatement of PIL's 8-bit bicubic resize against PIL itself and against the
fixture minted from PIL, the package's coefficient tables against the restatement's, the quantisation rule on every
fp16 / bf16 value in [0, 1], and the argument handling of the Python layer and of the built library."""
import os

import numpy as np
import pytest
import torch

from tests import pil_resample_reference as R
from tests.golden import mint_pil_resample as M

FIXTURE = M.PATH
CASES = list(M.cases())


@pytest.mark.parametrize("name,size,img", CASES, ids=[c[0] for c in CASES])
def test_restatement_equals_pil(name, size, img):
    Image = pytest.importorskip("PIL.Image")
    ref = np.asarray(Image.fromarray(img).resize((size[1], size[0]), Image.BICUBIC))
    got = R.resize(img, size)
    assert got.shape == ref.shape and got.dtype == np.uint8
    assert int((got != ref).sum()) == 0


def test_restatement_equals_fixture():
    """The same cases against PIL's bytes as minted into tests/golden/pil_resample.npz (inputs re-derived from the seeds
    AND stored: a drift of the generator would show as an input mismatch, not as a resample error)."""
    z = np.load(FIXTURE)
    assert str(z["pil_version"])
    for name, size, img in CASES:
        assert np.array_equal(z["in_" + name], img), name
        got = R.resize(img, size)
        assert np.array_equal(got, z["out_" + name]), (name, int((got != z["out_" + name]).sum()))
    assert len(z.files) == 1 + 2 * len(CASES)


def test_pad_and_identity_axis():
    img = R.noise_u8((5, 7, 3), "uniform", 1)
    assert R.resize(img, (5, 7)) is img                      # both passes skipped
    p = R.pad(img, (1, 2, 3, 0), fill=7)
    assert p.shape == (7, 11, 3) and np.array_equal(p[2:, 1:8], img)
    assert (p[:2] == 7).all() and (p[:, 0] == 7).all() and (p[:, 8:] == 7).all()
    # the table of an unchanged axis is the identity, so running the pass anyway changes nothing
    kk, b = R.coeffs(7, 7)
    assert np.array_equal(R.pass1d(img, kk, b, axis=1), img)
    for xx in range(7):
        row = np.zeros(kk.shape[1], dtype=np.int64)
        row[xx - int(b[xx, 0])] = 1 << R.PB
        assert np.array_equal(kk[xx], row)


AXIS_PAIRS = sorted({p for (h, w), (oh, ow), _ in R.PRODUCTION for p in ((h, oh), (w, ow))}
                    | {p for (h, w), (oh, ow) in R.SMALL_SHAPES for p in ((h, oh), (w, ow))} | {(64, 16), (100, 25)})


@pytest.mark.parametrize("pair", AXIS_PAIRS, ids=["%d_%d" % p for p in AXIS_PAIRS])
def test_resample_tables_equal_the_restatement(pair):
    from dualdiff_amd.pipeline.image_output import resample_tables
    kk, bounds = resample_tables(*pair)
    rk, rb = R.coeffs(*pair)
    assert kk.dtype == torch.int32 and bounds.dtype == torch.int32
    assert tuple(kk.shape) == rk.shape and tuple(bounds.shape) == rb.shape == (pair[1], 2)
    assert np.array_equal(kk.numpy(), rk) and np.array_equal(bounds.numpy(), rb)
    scale = max(pair[0] / pair[1], 1.0)
    assert kk.shape[1] == 2 * int(np.ceil(2.0 * scale)) + 1
    assert resample_tables(*pair)[0] is kk                   # cached
    # what the kernel's LDS slice relies on: T consecutive outputs read at most ceil((T - 1) in / out) + ksize + 1 inputs
    lo, hi = rb[:, 0].astype(np.int64), (rb[:, 0] + rb[:, 1]).astype(np.int64)
    assert (np.diff(lo) >= 0).all() and (np.diff(hi) >= 0).all() and hi.max() <= pair[0] and rb[:, 1].max() <= kk.shape[1]
    for t in (4, 8, 16, 32, 64):
        t = min(t, pair[1])
        span = (hi[t - 1:] - lo[:pair[1] - t + 1]).max()
        assert span <= -(-(t - 1) * pair[0] // pair[1]) + kk.shape[1] + 1


def test_table_ratio_four_has_ksize_17():
    from dualdiff_amd.pipeline.image_output import resample_tables
    assert resample_tables(64, 16)[0].shape[1] == 17 and resample_tables(16, 7)[0].shape[1] == 11


def _all_values(dtype):
    """Every value of a 16-bit float type in [0, 1]: the bit patterns 0 .. bits(1.0)."""
    one = torch.ones((), dtype=dtype).view(torch.int16).item()
    return torch.arange(one + 1, dtype=torch.int32).to(torch.int16).view(dtype)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_quantize_on_every_16_bit_value(dtype):
    v = _all_values(dtype)
    assert v.numel() == (15361 if dtype == torch.float16 else 16257) and v[0] == 0 and v[-1] == 1
    x = v.float().numpy()
    ref = (x * 255).round().astype("uint8")
    assert np.array_equal(R.quantize(x), ref)
    assert ref[0] == 0 and ref[-1] == 255
    half = int((v == 0.5).nonzero()[0])
    assert x[half] * 255 == 127.5 and ref[half] == 128       # the exact tie rounds to even
    # the [-1, 1] form is decode_latents' arithmetic in front of the same rule
    x11 = np.concatenate([x, -x])
    t = (torch.from_numpy(x11) / 2 + 0.5).clamp_(0, 1).numpy()
    assert np.array_equal(R.quantize(x11, m11=True), (t * 255).round().astype("uint8"))


def test_quantize_clamps():
    x = np.array([-3.0, -0.0, 1.0, 1.5, 0.5 / 255, 1.5 / 255], dtype=np.float32)
    assert R.quantize(x).tolist()[:4] == [0, 0, 255, 255]


# ---- the Python layer ------------------------------------------------------------------------------------------------------

def test_post_process_from_config():
    from dualdiff_amd.pipeline.image_output import ImagePostProcess
    p = ImagePostProcess.from_config({"fid": {"resize": [896, 1600], "padding": [0, 4, 0, 0], "raw_output": False}})
    assert p.resize == (896, 1600) and p.padding == (0, 4, 0, 0)
    p = ImagePostProcess.from_config({"fid": {"resize": [533, 1466], "padding": [67, 367, 67, 0]}})
    assert p.resize == (533, 1466) and p.padding == (67, 367, 67, 0)
    p = ImagePostProcess.from_config({"fid": {"resize": [896, 1600], "padding": [0, 4, 0, 0], "raw_output": True}})
    assert p.resize is None

    class Node:                                              # attribute access, as an OmegaConf node gives
        def __init__(self, **kw):
            self.__dict__.update(kw)
    p = ImagePostProcess.from_config(Node(fid=Node(resize=(800, 1600), padding=(0, 100, 0, 0), raw_output=False)))
    assert p.resize == (800, 1600) and p.padding == (0, 100, 0, 0)
    with pytest.raises(ValueError, match="fid"):
        ImagePostProcess.from_config({})
    with pytest.raises(ValueError, match="resize"):
        ImagePostProcess.from_config({"fid": {"raw_output": False}})


def test_padding_forms():
    from dualdiff_amd import ops
    from dualdiff_amd.pipeline.image_output import ImagePostProcess
    assert ops.image_padding(3) == (3, 3, 3, 3)
    assert ops.image_padding([2, 5]) == (2, 5, 2, 5)         # left / right, top / bottom
    assert ops.image_padding((1, 2, 3, 4)) == (1, 2, 3, 4)
    assert ImagePostProcess(resize=(8, 8)).padding == (0, 0, 0, 0)
    assert ImagePostProcess(resize=(8, 8), padding=2).padding == (2, 2, 2, 2)
    for bad in ((1, 2, 3), (1, -2), -1, "a", 1.5, (1.0, 2.0)):
        with pytest.raises(ValueError, match="padding"):
            ops.image_padding(bad)


def test_value_errors():
    from dualdiff_amd import ops
    from dualdiff_amd.pipeline.image_output import ImagePostProcess, resample_tables, to_pil
    with pytest.raises(ValueError, match="bicubic"):
        ImagePostProcess(resize=(8, 8), interpolation="bilinear")
    with pytest.raises(ValueError, match="resize"):
        ImagePostProcess(resize=(8, 0))
    with pytest.raises(ValueError, match="resize"):
        ImagePostProcess(resize=900)
    with pytest.raises(ValueError, match="raw output"):
        ImagePostProcess(padding=(0, 4, 0, 0))
    with pytest.raises(ValueError):
        resample_tables(0, 4)
    x = torch.zeros((2, 3, 4, 5))
    with pytest.raises(ValueError, match=r"\(m, 3, h, w\)"):
        ops.image_quantize_u8(torch.zeros((2, 4, 4, 5)))
    with pytest.raises(ValueError, match=r"\(m, 3, h, w\)"):
        ops.image_resample_u8(torch.zeros((3, 4, 5)), (8, 8))
    with pytest.raises(ValueError, match="fp16 / bf16 / fp32"):
        ops.image_quantize_u8(x.double())
    with pytest.raises(ValueError, match="contiguous"):
        ops.image_quantize_u8(x.permute(0, 1, 3, 2))
    with pytest.raises(ValueError, match="size"):
        ops.image_resample_u8(x, (8, 0))
    with pytest.raises(ValueError, match="size"):
        ops.image_resample_u8(x, 8)
    with pytest.raises(ValueError, match="fill"):
        ops.image_resample_u8(x, (8, 8), fill=256)
    with pytest.raises(ValueError, match="out must be"):
        ops.image_resample_u8(x, (8, 8), padding=1, out=torch.zeros((2, 8, 8, 3), dtype=torch.uint8))
    with pytest.raises(ValueError, match="out must be"):
        ops.image_quantize_u8(x, out=torch.zeros((2, 4, 5, 3), dtype=torch.int8))
    with pytest.raises(ValueError, match=r"\(b, n, 3, h, w\)"):
        ImagePostProcess()(torch.zeros((3, 4, 5)))
    with pytest.raises(ValueError, match="uint8"):
        to_pil(torch.zeros((1, 4, 5, 3)))


def test_ops_fail_loudly_on_cpu_tensors():
    from dualdiff_amd import ops
    from dualdiff_amd.pipeline.image_output import ImagePostProcess
    x = torch.zeros((1, 3, 4, 6), dtype=torch.float16)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.image_quantize_u8(x)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.image_resample_u8(x, (8, 12), (0, 1, 0, 0))
    with pytest.raises(RuntimeError, match="GPU only"):
        ImagePostProcess(resize=(8, 12))(x[None])


def test_to_pil_levels():
    pytest.importorskip("PIL")
    from dualdiff_amd.pipeline.image_output import to_pil
    u8 = torch.from_numpy(R.noise_u8((2, 3, 4, 5, 3), "uniform", 3))
    pil = to_pil(u8)
    assert len(pil) == 2 and all(len(s) == 3 for s in pil) and pil[1][2].size == (5, 4) and pil[1][2].mode == "RGB"
    assert np.array_equal(np.asarray(pil[1][2]), u8[1, 2].numpy())
    assert len(to_pil(u8[0])) == 3


def test_package_does_not_import_pil():
    """Only to_pil needs PIL, and only when it is called."""
    import subprocess
    import sys
    code = ("import sys; import dualdiff_amd.pipeline.image_output, dualdiff_amd.ops; "
            "assert not any(m == 'PIL' or m.startswith('PIL.') for m in sys.modules), 'PIL imported'")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], cwd=root, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ---- the built library, without a GPU -------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from dualdiff_amd import _build, _native
    if not os.path.exists(_build.lib_path()):
        pytest.skip("library not built (run __graft_entry__.build())")
    return _native.load(build_if_missing=False)


def test_library_validates_before_any_launch(lib):
    """dd_image_quantize_u8 / dd_image_resample_u8 turn bad calls down before anything is launched, so this runs on a box
    without a GPU: NULL pointers, non-positive sizes, negative pads and a fill that is no byte are DD_ERR_BAD_ARG (-1);
    a filter wider than DD_IMAGE_MAX_KSIZE and more images than the grid takes are DD_ERR_UNSUPPORTED (-2)."""
    P = 1 << 20                                              # a non-NULL pointer; never dereferenced on these paths

    def resample(x=P, out=P, m=1, h=8, w=12, oh=19, ow=31, kx=P, bx=P, ksx=5, ky=P, by=P, ksy=5, pads=(0, 0, 0, 0), fill=0,
                 dtype=0):
        return lib.dd_image_resample_u8(x, out, m, h, w, oh, ow, kx, bx, ksx, ky, by, ksy, *pads, fill, 0, dtype, None)

    for name in ("x", "out", "kx", "bx", "ky", "by"):
        assert resample(**{name: None}) == -1, name
    for name in ("m", "h", "w", "oh", "ow", "ksx", "ksy"):
        assert resample(**{name: 0}) == -1, name
        assert resample(**{name: -3}) == -1, name
    assert resample(pads=(0, -1, 0, 0)) == -1 and resample(fill=256) == -1 and resample(fill=-1) == -1
    assert resample(dtype=3) == -1
    assert resample(ksx=34) == -2 and resample(ksy=35) == -2   # in / out beyond 8
    assert resample(m=65536) == -2

    def quantize(x=P, out=P, m=1, h=8, w=12, dtype=2):
        return lib.dd_image_quantize_u8(x, out, m, h, w, 0, dtype, None)
    assert quantize(x=None) == -1 and quantize(out=None) == -1
    assert quantize(m=0) == -1 and quantize(h=0) == -1 and quantize(w=-1) == -1 and quantize(dtype=7) == -1
    assert quantize(m=65536) == -2 and quantize(h=1 << 16, w=1 << 15) == -2
    assert b"unsupported" in lib.dd_error_string(-2)
