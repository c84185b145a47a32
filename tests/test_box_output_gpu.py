"""Box output on the GPU against the oracle (tests/box_output_reference.py: numpy float64 geometry, PIL's thin line), whose
cases keep every decision a margin away from the rounding of the four-term sums.  Integers and bytes: every comparison
is equality."""
import functools

import numpy as np
import pytest
import torch

from dualdiff_amd import ops
from dualdiff_amd.pipeline import box_output as BO
from tests import box_output_reference as R

pytestmark = pytest.mark.gpu

PALETTE = np.asarray(R.PALETTE, np.uint8)


def same(t, want):
    return tuple(t.shape) == want.shape and str(t.dtype).split(".")[1] == str(want.dtype) and np.array_equal(t.cpu().numpy(), want)


@functools.lru_cache(maxsize=None)
def pictures(name, transparent):
    out = R.overlay(R.cases()[name], transparent)
    out.setflags(write=False)
    return out


def on_device(case, gpu):
    """(corners, labels, offsets, transforms) of a case as ops.box_edges takes them."""
    sizes = [len(x) for x in case.labels]
    corners = np.concatenate([np.asarray(c, np.float32).reshape(-1, 8, 3) for c in case.corners])
    labels = np.concatenate([np.asarray(x, np.int64).reshape(-1) for x in case.labels])
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    return tuple(torch.from_numpy(np.array(a)).to(gpu) for a in (corners, labels, offs, case.transforms))


class Launches:
    """Counts the library launches that go through ops._timer.launch, by name."""

    def __init__(self, monkeypatch):
        self.names = []
        real = ops._timer.launch

        def launch(what, fn, *a, **kw):
            self.names.append(what)
            return real(what, fn, *a, **kw)
        monkeypatch.setattr(ops._timer, "launch", launch)


# ---- dd_box_edges -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,cap", [("two_scenes", 7),              # 2 scenes x 3 views, 0 and 7 boxes; cap = the count's bound
                                      ("seventy", 70),                 # 70 boxes ranked by more than one wave, cap = count
                                      ("seventy", 90),                 # cap above the count: zero slots behind it
                                      ("seventy", 8),                  # cap below the count: bit 2, the nearest eight, the true count
                                      ("around", 23), ("bad_label", 5),   # bit 0
                                      ("saturating", 2)])              # bit 1
def test_edges_equal_the_oracle(gpu, name, cap):
    case = R.cases()[name]
    pts, cls, counts, flags = ops.box_edges(*on_device(case, gpu), cap, len(R.OBJECT_CLASSES))
    want = R.edge_arrays(case, cap)
    print(name, cap, "counts", counts.cpu().tolist(), "flags", flags.item(), "want", want[2].tolist(), want[3])
    assert same(counts, want[2]) and flags.tolist() == [want[3]]
    assert same(cls, want[1])
    assert same(pts, want[0])


def test_edges_flags_are_cleared_by_every_launch(gpu):
    bad = ops.box_edges(*on_device(R.cases()["bad_label"], gpu), 5, 10)[3]
    good = ops.box_edges(*on_device(R.cases()["two_scenes"], gpu), 7, 10)[3]
    assert bad.tolist() == [R.FLAG_LABEL] and good.tolist() == [0]


# ---- dd_box_draw_u8, from hand-made integer end points ------------------------------------------------------------------

def flat_box(x0, y0, x1, y1):
    return np.array([[x0, y0], [x0, y0], [x1, y0], [x1, y0], [x0, y1], [x0, y1], [x1, y1], [x1, y1]], np.int32)


def draw_both_ways(gpu, frames, pts, cls, counts, h, w):
    """ops.box_draw_u8 against R.draw_arrays, over the frames and on the transparent canvas."""
    dev = [torch.from_numpy(np.ascontiguousarray(a)).to(gpu) for a in (frames, pts, cls, counts, PALETTE)]
    opaque = ops.box_draw_u8(*dev)
    assert same(opaque, R.draw_arrays(frames, pts, cls, counts, R.PALETTE, h, w, False))
    assert same(dev[0], frames)                                        # the input is not written
    rgba = ops.box_draw_u8(None, *dev[1:], transparent=True, size=(h, w))
    assert same(rgba, R.draw_arrays(None, pts, cls, counts, R.PALETTE, h, w, True))
    assert same(ops.box_draw_u8(dev[0], *dev[1:], transparent=True), rgba.cpu().numpy())      # frames are ignored then


def test_draw_odd_canvas_and_degenerate_edges(gpu):
    """37 x 53, a multiple of no tile; a one-pixel box, horizontal and vertical edges, end points at +-2^20, the canvas'
    own corners, and two views with different counts in one launch (slots past a count are not drawn)."""
    h, w, far = 37, 53, 1 << 20
    rs = np.random.RandomState(3)
    frames = rs.randint(0, 256, (2, h, w, 3)).astype(np.uint8)
    pts = np.zeros((2, 5, 8, 2), np.int32)
    pts[0, 0] = flat_box(7, 5, 7, 5)                                   # one pixel
    pts[0, 1] = flat_box(0, 0, w - 1, h - 1)                           # the canvas' border: horizontal and vertical edges
    pts[0, 2] = flat_box(-far, 11, far, 30)                            # two horizontal lines through the whole canvas, verticals far outside
    pts[0, 3] = np.array([[-far, -far + 7], [far, far - 3], [far - 5, -far], [-far + 9, far], [-far, 20], [far, 13],
                          [33, -far], [21, far]], np.int32)           # long slanted lines through the canvas
    pts[0, 4] = flat_box(60, 40, 90, 70)                               # wholly outside
    pts[1, 0] = np.array([[3, 30], [40, 2], [50, 35], [10, 20], [-4, 8], [25, 36], [52, 0], [30, 18]], np.int32)
    pts[1, 1:] = pts[0, 1]                                             # behind the count of view 1: must not be drawn
    cls = np.array([[0, 1, 2, 3, 4], [5, 6, 7, 8, 9]], np.int32)
    counts = np.array([5, 1], np.int32)
    draw_both_ways(gpu, frames, pts, cls, counts, h, w)


def test_draw_tells_every_edges_direction(gpu):
    """Twelve views of one box each: box e shows which way edge e is drawn (tests/test_box_output_cpu.py)."""
    pts = R.direction_boxes()[:, None]
    frames = np.random.RandomState(4).randint(0, 256, (12, 16, 24, 3)).astype(np.uint8)
    cls = (np.arange(12, dtype=np.int32) % 10)[:, None]
    draw_both_ways(gpu, frames, pts, cls, np.ones(12, np.int32), 16, 24)
    back = pts[:, :, [1, 0, 3, 2, 5, 4, 7, 6]]                         # another box: the pictures differ from the first ones
    got = ops.box_draw_u8(None, *(torch.from_numpy(np.ascontiguousarray(a)).to(gpu) for a in (back, cls, np.ones(12, np.int32), PALETTE)),
                          transparent=True, size=(16, 24))
    assert same(got, R.draw_arrays(None, back, cls, np.ones(12, np.int32), R.PALETTE, 16, 24, True))


def test_draw_three_hundred_boxes_in_two_chunks(gpu):
    """300 small boxes on 48 x 80 in view 0 (more than one LDS chunk of 256), 37 in view 1."""
    h, w = 48, 80
    rs = np.random.RandomState(5)
    centre = np.stack([rs.randint(-6, w + 6, (2, 300)), rs.randint(-6, h + 6, (2, 300))], axis=-1)
    pts = (centre[:, :, None, :] + rs.randint(-9, 10, (2, 300, 8, 2))).astype(np.int32)
    cls = rs.randint(0, 10, (2, 300)).astype(np.int32)
    frames = rs.randint(0, 256, (2, h, w, 3)).astype(np.uint8)
    draw_both_ways(gpu, frames, pts, cls, np.array([300, 37], np.int32), h, w)


# ---- the whole call --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("transparent", (False, True))
def test_overlay_equals_the_oracle(gpu, monkeypatch, transparent):
    case = R.cases()["two_scenes"]
    o = BO.BoxOverlay(R.OBJECT_CLASSES, transparent_bg=transparent)
    frames = torch.from_numpy(case.frames.copy()).to(gpu)
    want = pictures("two_scenes", transparent)
    spy = Launches(monkeypatch)
    got = o(frames, case.corners, case.labels, case.transforms)
    assert spy.names == ["box_edges", "box_draw_u8"]
    assert same(got, want) and got.shape == (2, 3, 64, 96, 4 if transparent else 3)
    assert same(frames, case.frames)                                   # the input is never written
    assert torch.equal(o(frames, case.corners, case.labels, case.transforms), got)        # the same bits twice
    if transparent:
        assert same(o(None, case.corners, case.labels, case.transforms, size=(64, 96)), want)


def test_check_false_reads_nothing_back(gpu, monkeypatch):
    case = R.cases()["around"]
    o = BO.BoxOverlay(R.OBJECT_CLASSES)
    frames = torch.from_numpy(case.frames.copy()).to(gpu)
    corners, labels, offs, trans = on_device(case, gpu)
    offsets = offs.cpu().tolist()
    o(frames, corners, labels, trans, offsets=offsets)                 # the palette becomes a device constant here
    reads = []
    for name in ("cpu", "item", "tolist", "numpy"):
        real = getattr(torch.Tensor, name)

        def spy(self, *a, _real=real, _name=name, **kw):
            reads.append(_name)
            return _real(self, *a, **kw)
        monkeypatch.setattr(torch.Tensor, name, spy)
    got = o(frames, corners, labels, trans, offsets=offsets, check=False)
    assert reads == []
    checked = o(frames, corners, labels, trans, offsets=offsets)
    assert reads == ["item"]                                           # check=True: the 4-byte flags word
    monkeypatch.undo()
    assert same(got, pictures("around", False)) and torch.equal(checked, got)


def test_check_names_the_flag_bits(gpu):
    case = R.cases()["bad_label"]
    o = BO.BoxOverlay(R.OBJECT_CLASSES, transparent_bg=True)
    with pytest.raises(ValueError, match="bit 0: a label outside"):
        o(None, case.corners, case.labels, case.transforms, size=(case.h, case.w))
    got = o(None, case.corners, case.labels, case.transforms, size=(case.h, case.w), check=False)
    assert same(got, pictures("bad_label", True))                      # the other boxes are drawn
    sat = R.cases()["saturating"]
    with pytest.raises(ValueError, match="bit 1: a projected coordinate"):
        o(None, sat.corners, sat.labels, sat.transforms, size=(sat.h, sat.w))


# ---- RGBA files ----------------------------------------------------------------------------------------------------------

def rgba_bound(h, w):
    """The issue's size bound: 51 + 17 ceil(n / 16384) + n bytes, n = h (1 + 4 w)."""
    n = h * (1 + 4 * w)
    return 51 + 17 * (-(-n // 16384)) + n


def test_rgba_files_decode_to_the_frames(gpu, tmp_path):
    import io

    from PIL import Image

    from dualdiff_amd.pipeline import image_output as IO
    from tests import png_reference as PNG
    case = R.cases()["two_scenes"]
    o = BO.BoxOverlay(R.OBJECT_CLASSES, transparent_bg=True)
    overlay = o(None, case.corners, case.labels, case.transforms, size=(64, 96))
    rs = np.random.RandomState(6)
    batches = [overlay, IO.concat_views(overlay, oneline=True), torch.from_numpy(rs.randint(0, 256, (1, 1, 1, 4)).astype(np.uint8)).to(gpu),
               torch.from_numpy(rs.randint(0, 256, (3, 5, 7, 4)).astype(np.uint8)).to(gpu)]
    assert batches[1].shape == (2, 64, 288, 4)
    for frames in batches:
        files = IO.encode_png_rgba(frames)
        flat = frames.flatten(0, 1) if frames.dim() == 5 else frames
        files = [f for row in files for f in row] if frames.dim() == 5 else files
        assert len(files) == flat.shape[0]
        for data, want in zip(files, flat.cpu().numpy()):
            im = Image.open(io.BytesIO(data))
            im.load()
            assert im.mode == "RGBA" and im.size == (want.shape[1], want.shape[0])
            assert np.array_equal(np.asarray(im), want)
            assert len(data) <= rgba_bound(*want.shape[:2])
    sizes = IO.save_png_rgba(overlay[0], [str(tmp_path / ("v%d_box.png" % i)) for i in range(3)])
    assert [np.array_equal(np.asarray(Image.open(tmp_path / ("v%d_box.png" % i))), overlay[0, i].cpu().numpy()) for i in range(3)] == [True] * 3
    assert len(sizes) == 3
    # RGB: the bytes of before, through both entry points
    rgb = np.array(pictures("two_scenes", False)[1, :2])
    want = [PNG.encode(f) for f in rgb]
    dev = torch.from_numpy(rgb).to(gpu)
    assert IO.encode_png(dev) == want
    buf, lengths = ops.png_encode_u8c(dev)
    assert [buf[i, :n].cpu().numpy().tobytes() for i, n in enumerate(lengths.tolist())] == want
