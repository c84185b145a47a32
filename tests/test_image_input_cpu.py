"""Image input without a GPU: the restatement of the dataset transform (tests/image_input_reference.py) against PIL and
torch themselves and against the fixture minted from PIL, the geometry of the reference's four configurations, the
normalisation table, the bound the kernel sizes its LDS slice by, and the argument handling of the Python layer and of
the built library."""
import math
import os
import zlib

import numpy as np
import pytest
import torch

from tests import image_input_reference as RI
from tests import pil_resample_reference as R
from tests.golden import mint_image_input as M

CASES = list(M.cases())
ORI = (900, 1600)


# ---- the restatement ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,size,box,img", CASES, ids=[c[0] for c in CASES])
def test_restatement_equals_pil_and_torch(name, size, box, img):
    """resize + crop against PIL's bytes; ToTensor / Normalize against torch's ops as torchvision calls them."""
    Image = pytest.importorskip("PIL.Image")
    pil = Image.fromarray(img).resize((size[1], size[0])).crop(box)          # the default filter, as ImageAug3D calls it
    ref_u8 = np.asarray(pil)
    got_u8 = RI.crop_u8(img, size, box)
    assert got_u8.shape == ref_u8.shape == (box[3] - box[1], box[2] - box[0], 3)
    assert int((got_u8 != ref_u8).sum()) == 0
    assert np.array_equal(ref_u8, np.asarray(Image.fromarray(img).resize((size[1], size[0]), Image.BICUBIC).crop(box)))
    for mean, std in (RI.HALF, RI.IMAGENET):
        # torchvision.transforms.functional.to_tensor / normalize, written out
        x = torch.from_numpy(np.array(pil, copy=True)).permute((2, 0, 1)).contiguous().to(dtype=torch.float32).div(255)
        mt = torch.as_tensor(mean, dtype=x.dtype)
        st = torch.as_tensor(std, dtype=x.dtype)
        x = x.clone().sub_(mt.view(-1, 1, 1)).div_(st.view(-1, 1, 1))
        got = RI.pixel_values(img[None], size, box, mean, std)
        assert got.dtype == torch.float32 and int((got[0] != x).sum()) == 0
        for dtype in (torch.float16, torch.bfloat16):
            assert torch.equal(RI.pixel_values(img[None], size, box, mean, std, dtype)[0], x.to(dtype))


def test_restatement_equals_fixture():
    z = np.load(M.PATH)
    assert str(z["pil_version"])
    for name, size, box, img in CASES:
        assert int(z["crc_" + name]) == zlib.crc32(img.tobytes()), name
        got = RI.crop_u8(img, size, box)
        assert np.array_equal(got, z["out_" + name]), (name, int((got != z["out_" + name]).sum()))
    assert len(z.files) == 1 + 2 * len(CASES)
    assert os.path.getsize(M.PATH) < 128 * 1024


def test_cases_cover_the_shapes():
    """Down in both axes, up in both, each axis alone kept, a tiny source whose windows are all clipped, ratio 4 and ratio
    1 / 0.24 — each with an off-origin box."""
    by = {c[0]: c for c in RI.CASES}
    for name, (h, w), (oh, ow), box in RI.CASES:
        assert box[0] < box[2] <= ow and box[1] < box[3] <= oh and (box[0] or box[1])
    assert by["down4"][1][0] / by["down4"][2][0] == 4 and by["down4"][1][1] / by["down4"][2][1] == 4
    assert R.coeffs(180, 45)[0].shape[1] == 17 and R.coeffs(150, 36)[0].shape[1] == 19 and R.coeffs(200, 48)[0].shape[1] == 19
    assert R.coeffs(50, 24)[0].shape[1] == 11 and R.coeffs(150, 72)[0].shape[1] == 11
    assert by["up_both"][2][0] > by["up_both"][1][0] and by["up_both"][2][1] > by["up_both"][1][1]
    assert by["keep_h"][1][0] == by["keep_h"][2][0] and by["keep_w"][1][1] == by["keep_w"][2][1]
    kk, b = R.coeffs(3, 11)
    assert (b[:, 1] < kk.shape[1]).all()                     # every window of the tiny source is clipped by the border


# ---- geometry -----------------------------------------------------------------------------------------------------------------

class Node:                                                  # attribute access, as an OmegaConf node gives
    def __init__(self, **kw):
        self.__dict__.update(kw)


@pytest.mark.parametrize("image_size,lim,resized,box", RI.CONFIGS, ids=["%dx%d" % c[0] for c in RI.CONFIGS])
def test_from_config_reproduces_the_reference_configurations(image_size, lim, resized, box):
    from dualdiff_amd.pipeline.image_input import ImagePreProcess
    assert RI.geometry(ORI, image_size, lim) == (resized, box)
    cfg = {"dataset": {"image_size": list(image_size), "augment2d": {"resize": [list(lim)], "rotate": None}}}
    for c in (cfg, Node(dataset=Node(image_size=image_size, augment2d=Node(resize=[lim])))):
        p = ImagePreProcess.from_config(c, ORI)
        assert p.resize == resized and p.box == box and p.size == tuple(image_size)
        assert p.mean == (0.5, 0.5, 0.5) and p.std == (0.5, 0.5, 0.5) and p.dtype == torch.float32
    ks = [R.coeffs(ORI[0], resized[0])[0].shape[1], R.coeffs(ORI[1], resized[1])[0].shape[1]]
    assert ks == {224: [17, 17], 256: [11, 11], 432: [11, 11], 192: [19, 19]}[image_size[0]]
    p = ImagePreProcess.from_config(cfg, ORI, mean=RI.IMAGENET[0], std=RI.IMAGENET[1], dtype=torch.bfloat16)
    assert p.mean == RI.IMAGENET[0] and p.std == RI.IMAGENET[1] and p.dtype == torch.bfloat16


def test_from_config_errors():
    from dualdiff_amd.pipeline.image_input import ImagePreProcess
    with pytest.raises(ValueError, match="dataset"):
        ImagePreProcess.from_config({}, ORI)
    with pytest.raises(ValueError, match="image_size"):
        ImagePreProcess.from_config({"dataset": {"augment2d": {"resize": [[0.25, 0.25]]}}}, ORI)
    with pytest.raises(ValueError, match="augment2d"):
        ImagePreProcess.from_config({"dataset": {"image_size": [224, 400]}}, ORI)
    # 224 rows out of a 200-row resize: PIL would pad with black; not built
    with pytest.raises(ValueError, match="leaves"):
        ImagePreProcess.from_config({"dataset": {"image_size": [224, 400], "augment2d": {"resize": [[0.25, 0.25]]}}}, (800, 1600))
    with pytest.raises(ValueError, match="leaves"):
        ImagePreProcess.from_config({"dataset": {"image_size": [224, 416], "augment2d": {"resize": [[0.25, 0.25]]}}}, ORI)


# ---- the normalisation table ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mean,std", [RI.HALF, RI.IMAGENET], ids=["half", "imagenet"])
def test_lut_equals_torch(mean, std):
    from dualdiff_amd import ops
    lut = ops.image_norm_lut(mean, std)
    assert lut.shape == (3, 256) and lut.dtype == torch.float32 and lut.is_contiguous()
    u8 = np.arange(256, dtype=np.uint8).reshape(1, 256, 1).repeat(3, axis=2)             # one row of every byte value
    ref = RI.normalize(u8, mean, std)[:, 0, :]
    assert int((lut != ref).sum()) == 0
    for c in range(3):                                       # and the scalar form of the same arithmetic
        assert torch.equal(lut[c], torch.arange(256).float().div(255).sub(torch.tensor(mean[c])).div(torch.tensor(std[c])))
    if (mean, std) == RI.HALF:
        assert lut[0, 0] == -1 and lut[1, 255] == 1 and torch.equal(lut[0], lut[2])


# ---- the bound the kernel sizes its LDS slice by -----------------------------------------------------------------------------

AXES = sorted({p for _, (h, w), (oh, ow), _ in RI.CASES for p in ((h, oh), (w, ow))}
              | {p for _, _, (nh, nw), _ in RI.CONFIGS for p in ((ORI[0], nh), (ORI[1], nw))} | {(64, 8), (7, 7)})


@pytest.mark.parametrize("pair", AXES, ids=["%d_%d" % p for p in AXES])
def test_window_span_is_bounded_by_ksize_alone(pair):
    """dd_image_load_u8 gets a slice of the tables and not the resized size, so it sizes a tile's input window from
    ksize: T consecutive outputs read at most ceil((T - 1) * max(ksize - 1, 4) / 4) + ksize + 1 inputs."""
    from dualdiff_amd.pipeline.image_output import resample_tables
    n_in, n_out = pair
    if n_in == n_out:                                        # the one-tap table device_tables gives an axis that keeps its size
        kk, b = torch.ones((n_in, 1)), torch.stack([torch.arange(n_in), torch.ones(n_in, dtype=torch.long)], dim=1)
    else:
        kk, b = resample_tables(n_in, n_out)
    ks = kk.shape[1]
    assert n_in / n_out <= max(ks - 1, 4) / 4
    lo, hi = b[:, 0].long().numpy(), (b[:, 0] + b[:, 1]).long().numpy()
    for t in (4, 8, 16, 32, 64):
        t = min(t, n_out)
        span = (hi[t - 1:] - lo[:n_out - t + 1]).max()
        assert span <= math.ceil((t - 1) * max(ks - 1, 4) / 4) + ks + 1


# ---- the Python layer ---------------------------------------------------------------------------------------------------------

def test_value_errors():
    from dualdiff_amd import ops
    from dualdiff_amd.pipeline.image_input import ImagePreProcess, encode_images
    f = torch.zeros((2, 8, 12, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match=r"\(m, h, w, 3\)"):
        ops.image_load_u8(torch.zeros((2, 3, 8, 12), dtype=torch.uint8), (4, 6))
    with pytest.raises(ValueError, match=r"\(m, h, w, 3\)"):
        ops.image_load_u8(f[0], (4, 6))
    with pytest.raises(ValueError, match="uint8"):
        ops.image_load_u8(f.float(), (4, 6))
    with pytest.raises(ValueError, match="contiguous"):
        ops.image_load_u8(torch.zeros((2, 12, 8, 3), dtype=torch.uint8).permute(0, 2, 1, 3), (4, 6))
    with pytest.raises(ValueError, match="size"):
        ops.image_load_u8(f, (4, 0))
    with pytest.raises(ValueError, match="size"):
        ops.image_load_u8(f, 4)
    for box in ((0, 0, 7, 4), (0, 0, 6, 5), (-1, 0, 6, 4), (0, -1, 6, 4), (3, 0, 3, 4), (0, 2, 6, 2), (4, 0, 2, 4)):
        with pytest.raises(ValueError, match="box"):         # outside the 6 x 4 resized image, or empty
            ops.image_load_u8(f, (4, 6), box)
    with pytest.raises(ValueError, match="box"):
        ops.image_load_u8(f, (4, 6), (0, 0, 6))
    with pytest.raises(ValueError, match="std"):
        ops.image_load_u8(f, (4, 6), std=(0.5, 0.0, 0.5))
    with pytest.raises(ValueError, match="mean and std"):
        ops.image_load_u8(f, (4, 6), mean=(0.5, 0.5))
    with pytest.raises(ValueError, match="layout"):
        ops.image_load_u8(f, (4, 6), layout="nhwc")
    with pytest.raises(ValueError, match="fp16 / bf16 / fp32"):
        ops.image_load_u8(f, (4, 6), dtype=torch.float64)
    with pytest.raises(ValueError, match="out must be"):
        ops.image_load_u8(f, (4, 6), out=torch.zeros((2, 3, 4, 5)))
    with pytest.raises(ValueError, match="out must be"):
        ops.image_load_u8(f, (4, 6), dtype=torch.float16, out=torch.zeros((2, 3, 4, 6)))
    with pytest.raises(ValueError, match="out must be"):
        ops.image_load_u8(f, (4, 6), layout="nhwc8", out=torch.zeros((2, 3, 4, 6)))
    with pytest.raises(ValueError, match="resize"):
        ImagePreProcess(resize=(8, 0))
    with pytest.raises(ValueError, match="resize"):
        ImagePreProcess(resize=225)
    with pytest.raises(ValueError, match="leaves"):
        ImagePreProcess(resize=(225, 400), box=(0, 2, 400, 226))
    with pytest.raises(ValueError, match="std"):
        ImagePreProcess(resize=(4, 6), std=(0, 1, 1))
    pre = ImagePreProcess(resize=(4, 6))
    assert pre.box == (0, 0, 6, 4) and pre.size == (4, 6)
    with pytest.raises(ValueError, match=r"\(b, n, H, W, 3\)"):
        pre(torch.zeros((8, 12, 3), dtype=torch.uint8))
    with pytest.raises(ValueError, match="uint8"):
        pre(f.float())
    with pytest.raises(ValueError, match=r"\(b, n, H, W, 3\)"):
        encode_images(None, f, pre)
    with pytest.raises(ValueError, match="multiples of 8"):
        encode_images(None, f[None], pre)
    with pytest.raises(ValueError, match="given"):
        encode_images(None, f[None], ImagePreProcess(resize=(8, 8)), given=torch.ones((1, 3), dtype=torch.bool))


def test_ops_fail_loudly_on_cpu_tensors():
    from dualdiff_amd import ops
    from dualdiff_amd.pipeline.image_input import ImagePreProcess, encode_images
    f = torch.zeros((2, 8, 12, 3), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.image_load_u8(f, (4, 6))
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.image_load_u8(f, (4, 6), (1, 1, 5, 3), layout="nhwc8", dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.image_load_u8(f, (4, 6), out=torch.zeros((2, 3, 4, 6)))
    with pytest.raises(RuntimeError, match="GPU only"):
        ImagePreProcess(resize=(4, 6))(f[None])
    with pytest.raises(RuntimeError, match="GPU only"):
        encode_images(None, f[None], ImagePreProcess(resize=(8, 8)))


def test_module_does_not_import_pil():
    import subprocess
    import sys
    code = ("import sys; import dualdiff_amd.pipeline.image_input, dualdiff_amd.ops; "
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
    """dd_image_load_u8 turns bad calls down before anything is launched, so this runs on a box without a GPU: NULL
    pointers, non-positive sizes, an unknown dtype or layout and a misaligned channels-last `out` are DD_ERR_BAD_ARG
    (-1); a filter wider than DD_IMAGE_MAX_KSIZE, more images than the grid takes and a side of 2^24 are
    DD_ERR_UNSUPPORTED (-2)."""
    P = 1 << 20                                              # a non-NULL pointer; never dereferenced on these paths

    def load(x=P, out=P, m=1, h=80, w=120, oh=19, ow=31, kx=P, bx=P, ksx=17, ky=P, by=P, ksy=17, lut=P, dtype=0, layout=0):
        return lib.dd_image_load_u8(x, out, m, h, w, oh, ow, kx, bx, ksx, ky, by, ksy, lut, dtype, layout, None)

    for name in ("x", "out", "kx", "bx", "ky", "by", "lut"):
        assert load(**{name: None}) == -1, name
    for name in ("m", "h", "w", "oh", "ow", "ksx", "ksy"):
        assert load(**{name: 0}) == -1, name
        assert load(**{name: -3}) == -1, name
    assert load(dtype=3) == -1 and load(dtype=-1) == -1
    assert load(layout=2) == -1 and load(layout=-1) == -1
    assert load(layout=1, out=P + 8) == -1                   # channels-last rows go out as 16-byte stores
    assert load(ksx=34) == -2 and load(ksy=35) == -2         # in / out beyond 8
    assert load(m=65536) == -2
    assert load(h=1 << 24) == -2 and load(ow=1 << 24) == -2
    assert b"unsupported" in lib.dd_error_string(-2)
