"""Box input on the GPU against the restatement of the reference's `_preprocess_bbox` (tests/box_input_reference.py, pinned
to the reference's own results by tests/test_box_input_cpu.py).  Selection, order and padding are exact, and the payload is
copied, so every comparison is torch.equal, with no tolerance.

Input condition, not a tolerance: the kernel's float64 sums may differ from numpy's in summation order, so every case
asserts ON THE HOST that its inputs keep each decisive quantity (corner z; for the canvas filter x, x - w, y, y - h) at
least 1e-6 from its threshold (`_batch`); the seeds are fixed so that all do."""
import numpy as np
import pytest
import torch

from dualdiff_amd import ops
from dualdiff_amd.networks.layers import box_capacity
from dualdiff_amd.pipeline.box_input import BoxPreProcess, BoxViews
from tests import box_input_reference as RB

pytestmark = pytest.mark.gpu

SENTINEL = 77
GUARD = 64
FILTERS = {"positive_z": True, "canvas": False}              # ops filter name -> use_3d_filter
EDGE_BATCHES = [(0, 1, 63), (64, 65, 255), (256, 257, 300)]   # lane, wave and 256-box chunk edges


_BATCHES = {}


def _batch(seed, counts, f3d, shared=False, make=None):
    """(data, transforms, per-scene keep masks) of a seeded batch, computed once; asserts the input condition."""
    key = (seed, tuple(counts), f3d, shared, make)
    if key not in _BATCHES:
        data = RB.batch(seed, counts) if make is None else make(seed, counts)
        keeps, margin = RB.keeps_of(data, shared, f3d)
        assert margin >= RB.MARGIN, (key, margin)
        trans = None if shared else RB.transforms_of(data, f3d)
        _BATCHES[key] = (data, trans, keeps)
    return _BATCHES[key]


def _frontal(seed, counts):
    """Every box in front of camera 0 (x >= 12, |y| <= 3): the rear cameras see none of them, camera 0 all of them."""
    data = RB.batch(seed, counts)
    for s, b in enumerate(data["boxes"]):
        b[:, 0] = np.abs(b[:, 0]) + 12.0
        b[:, 1] = b[:, 1] * 0.06
        data["corners"][s] = RB.corners_of(b, RB.BOTTOM)
        data["filter_corners"][s] = RB.corners_of(b, RB.CENTRE)
    return data


def _guarded(shape, dtype, front):
    n = int(np.prod(shape))
    buf = torch.full((front + n + GUARD,), SENTINEL, dtype=dtype, device="cuda")
    return buf, buf[front:front + n].view(shape)


def _intact(buf, n, front):
    return bool((buf[:front] == SENTINEL).all()) and bool((buf[front + n:] == SENTINEL).all())


def _misaligned(x, front):
    """x copied `front` elements into a larger device buffer (torch's own allocations are 256-byte aligned)."""
    buf = torch.zeros((front + x.numel() + GUARD,), dtype=x.dtype, device="cuda")
    view = buf[front:front + x.numel()].view(x.shape)
    view.copy_(x)
    return view


def _launch(data, trans, keeps, mode, filt, cap, front=4, in_front=0, canvas=RB.CANVAS):
    """ops.box_views into sentinel-guarded outputs `front` elements into their buffers, against the restatement at `cap`
    slots: every slot below cap, the true counts, their maximum, and the guards."""
    cat = lambda parts, tail, dt: np.concatenate([np.asarray(p, dt).reshape((-1,) + tail) for p in parts])
    corners = torch.from_numpy(cat(data["corners"], (8, 3), np.float32))
    fcorners = torch.from_numpy(cat(data["filter_corners"], (8, 3), np.float32))
    labels = torch.from_numpy(cat(data["labels"], (), np.int64))
    offsets = torch.tensor(np.concatenate([[0], np.cumsum([len(c) for c in data["corners"]])]), dtype=torch.int32)
    scenes, views = len(keeps), keeps[0].shape[0]
    pts = 8 if mode == "all-xyz" else 4
    shapes = ((scenes, views, cap, pts, 3), (scenes, views, cap), (scenes, views, cap), (scenes, views), (1,))
    dtypes = (torch.float32, torch.int64, torch.bool, torch.int32, torch.int32)
    fronts = (front, 1, 3, 1, 1)
    pairs = [_guarded(s, torch.uint8 if d == torch.bool else d, f) for s, d, f in zip(shapes, dtypes, fronts)]
    outs = tuple(v.view(torch.bool) if d == torch.bool else v for (_, v), d in zip(pairs, dtypes))
    assert outs[0].data_ptr() % 16 == (4 * front) % 16
    dev = lambda x: _misaligned(x, in_front) if in_front else x.cuda()
    got = ops.box_views(dev(corners), labels.cuda(), offsets.cuda(), None if trans is None else torch.from_numpy(trans).cuda(),
                        views, cap, points_mode=mode, filter_mode=filt, canvas_size=canvas if filt == "canvas" else None,
                        filter_corners=None if trans is None else dev(fcorners), out=outs)
    assert all(g is o for g, o in zip(got, outs))
    want = RB.select(data["corners"], data["labels"], keeps, mode, cap)
    for name, g, w in zip(("bboxes", "classes", "masks", "counts"), got, want):
        g = g.cpu()
        assert torch.equal(g, torch.from_numpy(w)), (name, mode, filt, cap, int((g != torch.from_numpy(w)).sum()))
    assert int(got[4].item()) == int(want[3].max())
    for (buf, view), f in zip(pairs, fronts):
        assert _intact(buf, view.numel(), f)
    return want[3]


def _equal(got, want):
    assert (got is None) == (want is None)
    if want is not None:
        for key, dtype in (("bboxes", torch.float32), ("classes", torch.int64), ("masks", torch.bool)):
            assert got[key].is_cuda and got[key].dtype == dtype and got[key].is_contiguous()
            assert torch.equal(got[key].cpu(), want[key]), key


def _pre(data, trans, mode, f3d, shared=False, **kw):
    pre = BoxPreProcess(bbox_mode=mode, view_shared=shared, use_3d_filter=f3d, canvas_size=RB.CANVAS)
    return pre(data["corners"], data["labels"], trans, filter_corners=data["filter_corners"], **kw)


@pytest.mark.parametrize("mode", ["all-xyz", "cxyz"])
@pytest.mark.parametrize("filt", sorted(FILTERS))
def test_chunk_edges(gpu, filt, mode):
    """Per-scene N in {0, 1, 63, 64, 65, 255, 256, 257, 300}, three scenes x six views a batch: the public call against the
    reference's dict, and the launch at the capacity against the padded rows, counts and guards."""
    f3d = FILTERS[filt]
    for i, counts in enumerate(EDGE_BATCHES):
        data, trans, keeps = _batch(11 + i, counts, f3d)
        _equal(_pre(data, trans, mode, f3d), RB.preprocess(data, mode, False, f3d))
        _launch(data, trans, keeps, mode, filt, box_capacity(max(counts)))


@pytest.mark.parametrize("mode", ["all-xyz", "cxyz"])
def test_view_shared(gpu, mode):
    """views = 1, filter 0: every box kept, so the slots run over every lane, wave and chunk edge without a gap."""
    for i, counts in enumerate(EDGE_BATCHES):
        data, _, keeps = _batch(21 + i, counts, True, shared=True)
        got = _pre(data, None, mode, True, shared=True)
        _equal(got, RB.preprocess(data, mode, True, True))
        assert got["bboxes"].shape[1:3] == (1, max(counts))
        _launch(data, None, keeps, mode, "all", box_capacity(max(counts)))


@pytest.mark.parametrize("filt", sorted(FILTERS))
def test_nothing_visible(gpu, filt):
    """A batch with nothing visible gives None (max_len == 0) and rows that are padding throughout; a batch whose rear views
    see nothing, and whose view 0 sees every box of the largest scene (no padding in that row)."""
    f3d = FILTERS[filt]
    inv = lambda seed, counts: RB.batch(seed, counts, invisible=True)
    data, trans, keeps = _batch(31, (4, 0, 9), f3d, make=inv)
    assert all(not k.any() for k in keeps)
    assert _pre(data, trans, "all-xyz", f3d) is None
    assert _pre(data, trans, "all-xyz", f3d, uncond_first=True) is None
    assert int(_launch(data, trans, keeps, "all-xyz", filt, 32).max()) == 0
    data, trans, keeps = _batch(32, (2, 3), f3d, make=_frontal)
    per_view = np.stack([k.sum(axis=1) for k in keeps])
    assert (per_view[:, 3] == 0).all() and per_view[1, 0] == 3 == per_view.max()
    got = _pre(data, trans, "cxyz", f3d)
    _equal(got, RB.preprocess(data, "cxyz", False, f3d))
    assert got["masks"][1, 0].all() and not got["masks"][:, 3].any()
    _launch(data, trans, keeps, "cxyz", filt, 32)


@pytest.mark.parametrize("cap", [8, 32, 320])
def test_capacities(gpu, cap):
    """cap below the visible count (8, and 32 for the larger scenes): counts report the true number, the slots below cap hold
    the first cap kept boxes, nothing is written beyond; 320 holds everything."""
    data, trans, keeps = _batch(12, EDGE_BATCHES[1], True)
    counts = _launch(data, trans, keeps, "all-xyz", "positive_z", cap)
    assert (counts.max() > cap) == (cap < 320) and counts.min() < 32 < counts.max()
    data, trans, keeps = _batch(12, EDGE_BATCHES[1], False)
    _launch(data, trans, keeps, "cxyz", "canvas", cap)


@pytest.mark.parametrize("counts", [(0, 7, 40), (40, 7, 0), (0, 0, 5), (0,)])
def test_empty_scenes(gpu, counts):
    data, trans, keeps = _batch(41, counts, True)
    _equal(_pre(data, trans, "all-xyz", True), RB.preprocess(data, "all-xyz", False, True))
    _launch(data, trans, keeps, "all-xyz", "positive_z", 64)


@pytest.mark.parametrize("front", [1, 2, 3])
def test_alignment(gpu, front):
    """corners, filter_corners and the rows written 4, 8 and 12 bytes off a 16-byte boundary: the 16-byte accesses are taken
    only where the base allows them."""
    for mode in ("all-xyz", "cxyz"):
        data, trans, keeps = _batch(13, EDGE_BATCHES[2], True)
        _launch(data, trans, keeps, mode, "positive_z", 320, front=front, in_front=front)
        data, trans, keeps = _batch(23, EDGE_BATCHES[2], True, shared=True)
        _launch(data, None, keeps, mode, "all", 320, front=front, in_front=front)


def test_uncond_first_and_unsynced(gpu):
    data, trans, keeps = _batch(11, EDGE_BATCHES[0], True)
    want = RB.preprocess(data, "all-xyz", False, True)
    _equal(_pre(data, trans, "all-xyz", True, uncond_first=True), RB.add_uncond(want))
    ml = want["masks"].shape[2]
    for uncond in (False, True):
        bv = _pre(data, trans, "all-xyz", True, sync=False, uncond_first=uncond)
        assert isinstance(bv, BoxViews) and bv.masks.dtype == torch.bool and bv.classes.dtype == torch.int64
        cap = box_capacity(63)
        assert bv.bboxes.shape == ((6 if uncond else 3), 6, cap, 8, 3) and int(bv.max_len_dev.item()) == ml
        assert torch.equal(bv.counts.cpu(), torch.from_numpy(np.stack([k.sum(axis=1) for k in keeps]).astype(np.int32)))
        full = RB.add_uncond(want) if uncond else want
        for key, t, pad in (("bboxes", bv.bboxes, 0), ("classes", bv.classes, -1), ("masks", bv.masks, 0)):
            assert torch.equal(t[:, :, :ml].cpu(), full[key]), key
            tail = t[-3:, :, ml:].cpu()
            assert bool((tail == pad).all()), key
            if uncond:
                assert not t[:3].any()


def test_concatenated_device_inputs(gpu):
    """The concatenated form with offsets, corners and labels already on the device."""
    data, trans, _ = _batch(11, EDGE_BATCHES[0], False)
    want = RB.preprocess(data, "cxyz", False, False)
    pre = BoxPreProcess(bbox_mode="cxyz", use_3d_filter=False, canvas_size=RB.CANVAS)
    cat = lambda parts: torch.from_numpy(np.concatenate(parts)).cuda()
    offsets = np.concatenate([[0], np.cumsum(EDGE_BATCHES[0])])
    got = pre(cat(data["corners"]), cat(data["labels"]), trans, filter_corners=cat(data["filter_corners"]), offsets=offsets)
    _equal(got, want)


def test_prepare_tokens_end_to_end(gpu, monkeypatch):
    """The dict goes through BEVControlNetModel.prepare_tokens of a small seeded ControlNet and gives bit-identical tokens to
    the same dict built by the restatement and copied to the device."""
    from dualdiff_amd import tuning
    from dualdiff_amd.networks.layers import device_init_
    from tests.test_host_logic import small_cnet
    monkeypatch.setattr(tuning, "_AUTOTUNE", False)          # the library's own tile plan: no run-time sweep of new shapes
    with torch.device("cuda"):
        net = small_cnet().to(torch.float16).eval()
    device_init_(net, 3)
    data, trans, _ = _batch(42, (5, 40), True)
    got = _pre(data, trans, "all-xyz", True)
    want = {k: v.cuda() for k, v in RB.preprocess(data, "all-xyz", False, True).items()}
    g = torch.Generator().manual_seed(5)
    cam = torch.randn((2, 6, 3, 7), generator=g).cuda()
    text = torch.randn((2, 77, 768), generator=g).cuda().half()
    with torch.no_grad():
        a = net.prepare_tokens(cam, got, text)
        b = net.prepare_tokens(cam, want, text)
    assert a["lc"] == b["lc"] == 78 + want["masks"].shape[2] and a["m"] == 12
    for k in ("ctx", "ctx2d", "txt"):
        assert torch.isfinite(a[k].float()).all() and torch.equal(a[k], b[k]), k
    # uncond_first is the model's own add_uncond_to_kwargs applied to the synchronised result
    cfg = net.add_uncond_to_kwargs(camera_param=cam, bboxes_3d_data=got, image=None)["bboxes_3d_data"]
    first = _pre(data, trans, "all-xyz", True, uncond_first=True)
    for k in ("bboxes", "classes", "masks"):
        assert first[k].dtype == cfg[k].dtype and torch.equal(first[k], cfg[k]), k
