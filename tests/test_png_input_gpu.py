"""PNG input on the GPU against pixels known by construction (tests/png_input_cases.py) and against PIL's pixels for the
files PIL wrote (tests/golden/png_input.npz).  Inflate, the filters and the conversion are integer arithmetic, and the
condition's values come from a table, so every comparison is equality, with no tolerance.  The broken streams fed here are
the ones that tests/test_png_input_cpu.py::test_decode_core_on_the_host_under_sanitizers ran through the decode core on the
host first."""
import functools

import numpy as np
import pytest
import torch

from dualdiff_amd import ops
from dualdiff_amd.pipeline import png_input as PI
from tests import png_cases
from tests import png_input_cases as C
from tests.golden import mint_png_input as MI

pytestmark = pytest.mark.gpu

NAMES = [c.name for c in C.cases()]
OWN = [c.name for c in png_cases.cases()]


@functools.lru_cache(maxsize=None)
def _golden():
    return {name: (data, pix) for name, data, pix in MI.files()}


@functools.lru_cache(maxsize=None)
def _own():
    return {name: (f, img) for name, f, img in C.own_files()}


def _decode(files, chunked=None):
    streams, table, tab, types, h, w = PI.upload_png(files, "cuda")
    return ops.png_decode_u8(streams, table, tab, types, h, w, chunked=chunked)


def _same(frames, want):
    return torch.equal(frames.cpu(), torch.from_numpy(np.array(want)))


@pytest.mark.parametrize("name", NAMES)
def test_constructed_pixels(name):
    c = next(c for c in C.cases() if c.name == name)
    frames = PI.decode_png([c.data])
    assert frames.dtype == torch.uint8 and frames.is_cuda and tuple(frames.shape) == (1,) + c.pixels.shape
    assert _same(frames[0], c.pixels)
    frames, status, paths = _decode([c.data], chunked=False)
    assert status.tolist() == [0] and paths.tolist() == [0] and _same(frames[0], c.pixels)


def test_files_pil_wrote(tmp_path):
    for name, (data, pix) in _golden().items():
        assert _same(PI.decode_png([data])[0], pix), name
    data, pix = _golden()["crop_road"]
    path = tmp_path / "road.png"
    path.write_bytes(data)
    frames = PI.load_png([[str(path), str(path)]])
    assert tuple(frames.shape) == (1, 2, 64, 96, 3) and _same(frames[0, 1], pix)


@pytest.mark.parametrize("name", OWN)
def test_our_own_files_on_both_paths(name):
    f, img = _own()[name]
    a, status_a, paths_a = _decode([f, f], chunked=None)
    assert status_a.tolist() == [0, 0] and paths_a.tolist() == [1, 1]            # the chunk-parallel result was used
    assert _same(a[0], img) and _same(a[1], img)
    b, status_b, paths_b = _decode([f, f], chunked=False)
    assert status_b.tolist() == [0, 0] and paths_b.tolist() == [0, 0]            # ... and here it was not
    assert torch.equal(a, b)


def test_foreign_file_of_our_shape_falls_back():
    f, img = C.foreign_chunk_shaped()
    assert PI.parse_png(f).chunked                                               # the host precondition holds
    own, own_img = _own()["128x85_two_chunks"]
    frames, status, paths = _decode([own, f, own])
    assert status.tolist() == [0, 0, 0] and paths.tolist() == [1, 0, 1]
    assert _same(frames[1], img) and _same(frames[0], own_img) and _same(frames[2], own_img)


def test_nested_batch_with_one_colour_type_per_file():
    rs = np.random.RandomState(11)
    files, want = [], []
    for i, colour in enumerate((2, 6, 0, 6, 0, 2)):
        pix = rs.randint(0, 256, (9, 11, C.CHANNELS[colour])).astype(np.uint8)
        types = tuple(rs.randint(0, 5, 9).tolist())
        files.append(C.png_file(9, 11, colour, C.deflate(C.filter_rows(pix, types), level=(0, 6, 9)[i % 3])))
        want.append(C.rgb(pix))
    frames, status = PI.decode_png([files[:3], files[3:]], check=False)
    assert tuple(frames.shape) == (2, 3, 9, 11, 3) and tuple(status.shape) == (2, 3) and int(status.abs().sum()) == 0
    assert _same(frames.reshape(6, 9, 11, 3), np.stack(want))


@pytest.mark.parametrize("name", [b.name for b in C.broken()])
def test_broken_stream_sets_its_status_bit(name):
    b = next(b for b in C.broken() if b.name == name)
    good = next(c for c in C.cases() if c.name == "7x5_rgba")
    frames, status = PI.decode_png([good.data, b.data, good.data], check=False)
    assert status.tolist() == [0, b.status, 0]
    assert _same(frames[0], good.pixels) and _same(frames[2], good.pixels)
    text = dict(ops.PNG_DECODE_STATUS)[b.status]
    with pytest.raises(ValueError, match="^frame 1: the stream does not decode: " + text):
        PI.decode_png([good.data, b.data, good.data])


def test_round_trip_on_the_device():
    from dualdiff_amd.pipeline import image_output as IO
    frames = torch.from_numpy(png_cases.batch()).cuda()
    files = IO.encode_png(frames)
    back = PI.decode_png(files)
    assert torch.equal(back, frames)
    streams, table, tab, types, h, w = PI.upload_png(files, "cuda")
    assert ops.png_decode_u8(streams, table, tab, types, h, w)[2].tolist() == [1] * len(files)


def _want_condition(pixels, occ):
    """torch.stack([crop(ToTensor()(pil_rgb)) ...]) with the crop as slicing"""
    x = torch.stack([torch.from_numpy(np.array(p)).permute(2, 0, 1).float().div(255) for p in pixels])
    top, left, oh, ow = occ.crop(x.shape[2], x.shape[3])
    pw = x.shape[3] // occ.views
    return torch.cat([x[:, :, top:top + oh, v * pw + left:v * pw + left + ow] for v in range(occ.views)], dim=3)


def test_occ_condition_equals_totensor_and_crop():
    data, pix = _golden()["panorama"]
    occ = PI.OccCondition()
    got = occ([data, data])
    assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == (2, 3, 12, 60) and got.is_contiguous()
    assert torch.equal(got.cpu(), _want_condition([pix, pix], occ))
    rs = np.random.RandomState(972)
    rgba = [rs.randint(0, 256, (9, 72, 4)).astype(np.uint8) for _ in range(3)]
    files = [C.png_file(9, 72, 6, C.deflate(C.filter_rows(p, tuple(rs.randint(0, 5, 9).tolist())))) for p in rgba]
    occ = PI.OccCondition(views=6, in_hw=(9, 12), out_hw=(5, 8))
    got = occ(files)
    assert tuple(got.shape) == (3, 3, 5, 48)
    assert torch.equal(got.cpu(), _want_condition([C.rgb(p) for p in rgba], occ))
    assert torch.equal(occ(PI.decode_png(files)), got)                           # frames already on the device
    # every byte value through the table: float32(b) / 255, correctly rounded
    ramp = torch.arange(256, dtype=torch.uint8).reshape(1, 1, 256, 1).expand(1, 2, 256, 3).contiguous().cuda()
    assert torch.equal(ops.png_condition(ramp, views=1)[0, 1, 0].cpu(), torch.arange(256).float().div(255))


@torch.no_grad()
def test_condition_feeds_the_embedder():
    from dualdiff_amd.networks.layers import device_init_
    from dualdiff_amd.networks.map_embedder import ControlNetConditioningEmbedding
    rs =np.random.RandomState(1696)
    pix = rs.randint(0, 256, (16, 96, 4)).astype(np.uint8)
    cond = PI.OccCondition()([C.png_file(16, 96, 6, C.deflate(C.filter_rows(pix, (1,) * 16)))] * 2)
    assert tuple(cond.shape) == (2, 3, 16, 96)
    net = ControlNetConditioningEmbedding(320).to("cuda", torch.float16).eval()
    device_init_(net, 1)
    rows, m, h, w = net.run(cond)
    assert (m, h, w) == (12, 2, 2) and tuple(rows.shape) == (12 * 2 * 2, 320) and bool(torch.isfinite(rows.float()).all())
