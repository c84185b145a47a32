"""Map output on the GPU against the numpy restatement (tests/map_output_reference.py, pinned to the reference's own
pictures by tests/test_map_output_cpu.py) on the cases of tests/golden/map_output.npz.  The whole path is table look-ups
and PIL's integer resize, so every comparison is equality of bytes.  The legend function here is a look-up into the
fixture's legends: nothing needs matplotlib."""
import functools

import numpy as np
import pytest
import torch

from dualdiff_amd import ops
from dualdiff_amd.pipeline import map_output as MO
from tests import map_output_reference as R
from tests.golden import mint_map_output as M

pytestmark = pytest.mark.gpu

DTYPES = {"bool": torch.bool, "uint8": torch.uint8, "fp16": torch.float16, "fp32": torch.float32}
LAUNCHES = ("map_render_u8", "image_resample_u8", "map_compose_u8")


@functools.lru_cache(maxsize=None)
def fixture():
    z = M.load()
    legends = {}
    for name, (_, target, _, _, _) in M.CASES.items():
        legends[(frozenset(M.used(z, name)), target)] = z["legend_" + name]
    return z, M.colors(z), M.priority(z), legends


def fixture_legend(names, long_edge_size):
    return fixture()[3][(frozenset(names), long_edge_size)]


@functools.lru_cache(maxsize=None)
def restated(name):
    """(frame, used word, whole picture) of a case by the restatement: computed once, shared, never written to."""
    z, colors, priority, _ = fixture()
    _, target, _, mc, oc = M.CASES[name]
    frame, used = R.render(M.inputs(name), mc, oc, colors, priority, target)
    whole = R.compose(frame, z["legend_" + name])
    frame.setflags(write=False)
    whole.setflags(write=False)
    return frame, R.used_word(used, mc, oc), whole


def same(t, want):
    return tuple(t.shape) == want.shape and t.dtype == torch.uint8 and np.array_equal(t.cpu().numpy(), want)


def on_gpu(m, dtype, gpu):
    return torch.from_numpy(np.ascontiguousarray(m)).to(gpu).to(dtype)


def padded(name, channels=18):
    """A 12 x 12 case as an 18-layer map: further layers empty, or the layers past 18 dropped (nothing reads them)."""
    m = M.inputs(name)
    out = np.zeros((channels,) + m.shape[1:], dtype=np.uint8)
    out[:min(channels, m.shape[0])] = m[:channels]
    return out


class Launches:
    """Counts the library launches that go through ops._timer.launch, by name."""

    def __init__(self, monkeypatch):
        self.names = []
        real = ops._timer.launch

        def launch(what, fn, *a, **kw):
            self.names.append(what)
            return real(what, fn, *a, **kw)
        monkeypatch.setattr(ops._timer, "launch", launch)


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("name", sorted(M.CASES))
def test_render_and_call_equal_the_restatement(gpu, name, dtype):
    _, target, _, mc, oc = M.CASES[name]
    r = MO.MapRender(mc, oc, target_size=target)
    maps = on_gpu(M.inputs(name)[None], DTYPES[dtype], gpu)
    frame, word, whole = restated(name)
    frames, used = r.render(maps)
    assert used.dtype == torch.int32 and used.tolist() == [word]
    assert same(frames, frame[None])
    pics = r(maps, legend=fixture_legend)
    assert len(pics) == 1 and same(pics[0], whole)


def test_three_class_sets_give_three_shapes(gpu, monkeypatch):
    names = ("few_dynamic", "empty", "aux", "few_dynamic")
    r = MO.MapRender(M.MAP_CLASSES, M.OBJECT_CLASSES, target_size=40)
    maps = on_gpu(np.stack([padded(n) for n in names]), torch.float32, gpu)
    spy = Launches(monkeypatch)
    frames, used = r.render(maps)
    assert spy.names == list(LAUNCHES)
    assert used.tolist() == [restated(n)[1] for n in names]
    assert same(frames, np.stack([restated(n)[0] for n in names]))
    del spy.names[:]
    pics = r(maps, legend=fixture_legend)
    assert spy.names == list(LAUNCHES[:2]) + ["map_compose_u8"] * 3        # one compose per distinct legend
    assert len({tuple(p.shape) for p in pics}) == 3
    for p, n in zip(pics, names):
        assert same(p, restated(n)[2]), n
    assert [r.names(w) for w in used.tolist()] == [M.used(fixture()[0], n) for n in names]


def test_identical_maps_identical_frames_and_bits(gpu, monkeypatch):
    r = MO.MapRender(M.MAP_CLASSES, M.OBJECT_CLASSES, target_size=50)
    maps = on_gpu(np.repeat(M.inputs("mixed")[None], 8, axis=0), torch.uint8, gpu)
    frame, word, whole = restated("mixed")
    frames, used = r.render(maps)
    assert used.tolist() == [word] * 8
    assert same(frames, np.repeat(frame[None], 8, axis=0))
    again, used2 = r.render(maps)
    assert torch.equal(again, frames) and torch.equal(used2, used)          # the launcher clears `used` every time
    spy = Launches(monkeypatch)
    pics = r(maps, legend=fixture_legend)
    assert spy.names == list(LAUNCHES)                                      # one legend: one compose
    assert all(same(p, whole) for p in pics)


def test_a_tall_legend_goes_to_the_right(gpu):
    tall = np.random.RandomState(7).randint(0, 256, (40, 7, 3)).astype(np.uint8)
    square = np.random.RandomState(8).randint(0, 256, (40, 40, 3)).astype(np.uint8)
    r = MO.MapRender(M.MAP_CLASSES, M.OBJECT_CLASSES, target_size=40)
    maps = on_gpu(padded("aux")[None], torch.bool, gpu)
    frame = restated("aux")[0]
    for leg in (tall, square):                                              # lh == lw goes below, as in the reference
        def fn(names, long_edge_size, leg=leg):
            return leg
        pic, = r(maps, legend=fn)
        assert same(pic, R.compose(frame, leg))
    assert tuple(r(maps, legend=lambda n, s: tall)[0].shape) == (40, 47, 3)
    with pytest.raises(ValueError, match="does not fit"):
        r(maps, legend=lambda n, s: tall[:39])


def test_bit_31_reports_a_value_other_than_0_and_1(gpu):
    r = MO.MapRender(M.MAP_CLASSES, M.OBJECT_CLASSES, target_size=40)
    m = np.stack([padded("few_dynamic"), padded("few_dynamic")])
    m[1, 13, 11, 0] = 2                                                     # barrier, at a pixel free of objects
    maps = on_gpu(m, torch.uint8, gpu)
    _, used = r.render(maps)
    word = restated("few_dynamic")[1]
    got = used.tolist()
    assert got[0] == word and got[1] < 0 and got[1] & 0x7fffffff == word | 1 << 13
    with pytest.raises(ValueError, match="map 1 holds a value other than 0 / 1"):
        r(maps, legend=fixture_legend)
    _, used = r.render(maps.float())                                        # a float map is `!= 0`: inside the contract
    assert used.tolist() == [word, word | 1 << 13]


def test_quantiser_returns_every_colour_byte(gpu):
    """The float route to the resize: dd_image_resample_u8's quantiser gives c for float32(c) / 255, all 256 bytes, on its
    own and through a same-size resample (one-tap tables)."""
    c = (np.arange(256, dtype=np.float32) / np.float32(255)).reshape(16, 16)
    x = torch.from_numpy(np.stack([c, c[::-1].copy(), c.T.copy()])[None]).to(gpu)
    want = np.arange(256, dtype=np.uint8).reshape(16, 16)
    want = np.stack([want, want[::-1], want.T], axis=-1)[None]
    assert same(ops.image_quantize_u8(x), want)
    assert same(ops.image_resample_u8(x, (16, 16)), want)
