"""The resized ORS condition on the GPU (`ops.png_condition_resized`, `ResizedOccCondition`) against the numpy restatement
that defines its arithmetic (tests/occ_condition_reference.py), bit for bit: the kernel reads the host's float32 tables and
combines with explicit fused multiply-adds and rounded products, so there is nothing to tolerate.  The restatement's own
distance from the reference's torch calls is held by tests/test_occ_condition_resize_cpu.py."""
import functools

import numpy as np
import pytest
import torch

from dualdiff_amd import ops
from dualdiff_amd.pipeline import png_input as PI
from tests import occ_condition_reference as R
from tests import png_input_cases as C

pytestmark = pytest.mark.gpu

# beside the issue's six: a row of 3 * 7 = 21 floats and 2 * 3 * 5 * 21 = 630 in all — runs of four that cross rows and
# planes, and a last run of two; and one view whose row of 13 floats is odd as well
TAIL = (3, 6, 10, 1, (5, 7), 0, 0, (5, 7))
ONE_VIEW = (1, 11, 17, 1, (9, 13), 1, 0, (8, 13))
GEOMETRIES = R.GEOMETRIES + (TAIL, ONE_VIEW)
IDS = [R.geometry_id(g) for g in GEOMETRIES]


def _args(g):
    return dict(views=g[0], pad_top=g[3], resize=g[4], top=g[5], left=g[6], size=g[7])


@functools.lru_cache(maxsize=None)
def _case(g):
    """(frames, restatement) at b = 2, computed once and not written to afterwards"""
    frames = R.random_frames(g, 2, seed=384 + GEOMETRIES.index(g))
    want = R.restatement(frames, **_args(g))
    frames.setflags(write=False)
    want.setflags(write=False)
    return frames, want


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _device(frames):
    return torch.tensor(frames).cuda()


@pytest.mark.parametrize("g", GEOMETRIES, ids=IDS)
def test_equals_the_restatement_bit_for_bit(g):
    frames, want = _case(g)
    assert (g[0] * g[7][1]) % 4 != 0 or g not in (TAIL, ONE_VIEW)
    assert want.size % 4 != 0 or g != TAIL
    got = ops.png_condition_resized(_device(frames), **_args(g))
    assert got.dtype == torch.float32 and got.is_cuda and got.is_contiguous() and tuple(got.shape) == want.shape
    assert want.shape == (2, 3, g[7][0], g[0] * g[7][1])
    same = _bits(got) == torch.tensor(want.view(np.int32))
    assert bool(same.all()), "%d of %d elements differ" % (int((~same).sum()), want.size)


def test_identity_resize_equals_the_plain_condition():
    frames = _device(R.random_frames((6, 9, 12), 3, seed=7))                     # (3, 9, 72, 3)
    plain = ops.png_condition(frames, views=6, top=4, left=2, size=(5, 8))
    for resize in (None, (9, 12)):
        got = ops.png_condition_resized(frames, views=6, pad_top=0, resize=resize, top=4, left=2, size=(5, 8))
        assert torch.equal(_bits(got), _bits(plain))
    assert torch.equal(_bits(ops.png_condition_resized(frames, views=6)), _bits(ops.png_condition(frames, views=6)))
    # a pad without a resize: zero rows on top of the plain condition
    got = ops.png_condition_resized(frames, views=6, pad_top=2)
    assert tuple(got.shape) == (3, 3, 11, 72) and int(_bits(got[:, :, :2]).abs().max()) == 0
    assert torch.equal(_bits(got[:, :, 2:]), _bits(ops.png_condition(frames, views=6)))
    # every byte value through the table
    ramp = torch.arange(256, dtype=torch.uint8).reshape(1, 1, 256, 1).expand(1, 2, 256, 3).contiguous().cuda()
    assert torch.equal(ops.png_condition_resized(ramp, views=1)[0, 1, 0].cpu(), torch.arange(256).float().div(255))


def test_out_is_honoured_and_two_calls_agree():
    g = R.GEOMETRIES[2]
    frames, want = _case(g)
    dev = _device(frames)
    out = torch.full(want.shape, -7.0, dtype=torch.float32, device="cuda")
    guard = out.clone()
    got = ops.png_condition_resized(dev, out=out, **_args(g))
    assert got is out and torch.equal(_bits(out), torch.tensor(want.view(np.int32)))
    again = ops.png_condition_resized(dev, **_args(g))
    assert again.data_ptr() != out.data_ptr() and torch.equal(_bits(again), _bits(out))
    assert bool((guard == -7.0).all())
    with pytest.raises(ValueError, match="out must be"):
        ops.png_condition_resized(dev, out=torch.empty(want.shape, dtype=torch.float16, device="cuda"), **_args(g))
    with pytest.raises(ValueError, match="16-byte"):
        ops.png_condition_resized(dev, out=torch.empty(want.size + 1, device="cuda")[1:].view(want.shape), **_args(g))


def test_true_geometry_twice_gives_the_same_bits():
    frames, _ = _case(R.TRUE)
    dev = _device(frames)
    a = ops.png_condition_resized(dev, **_args(R.TRUE))
    b = ops.png_condition_resized(dev, **_args(R.TRUE))
    assert a.numel() == 2 * 3 * 192 * 2304 and torch.equal(_bits(a), _bits(b))


def test_drivewm_on_files_equals_the_call_on_frames():
    # noise in bands of eight equal rows, every row behind a band's first filtered "up" to zeros: two files of the
    # reference's size whose streams one wave each inflates in milliseconds
    rs = np.random.RandomState(1923)
    rgba = [np.repeat(rs.randint(0, 256, (28, 2400, 4)).astype(np.uint8), 8, axis=0) for _ in range(2)]
    types = tuple(2 if y % 8 else (0, 1, 3)[y // 8 % 3] for y in range(224))
    files = [C.png_file(224, 2400, 6, C.deflate(C.filter_rows(p, types))) for p in rgba]
    occ = PI.occ_condition_from_config({"dataset": {"image_size": [192, 384]}})
    got = occ(files)
    assert got.dtype == torch.float32 and got.is_cuda and got.is_contiguous() and tuple(got.shape) == (2, 3, 192, 2304)
    frames = PI.decode_png(files)
    assert torch.equal(frames.cpu(), torch.from_numpy(np.stack([C.rgb(p) for p in rgba])))
    assert torch.equal(_bits(occ(frames)), _bits(got))
    assert torch.equal(_bits(PI.ResizedOccCondition.drivewm()(frames)), _bits(got))
    want = R.restatement(frames[:1].cpu().numpy(), **_args(R.TRUE))               # ... and is the restatement of those frames
    assert torch.equal(_bits(got[:1]), torch.tensor(want.view(np.int32)))
    with pytest.raises(ValueError, match="defined for 224 x 6 x 400"):
        occ(frames[:, :200].contiguous())
