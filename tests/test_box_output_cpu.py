"""Box output without a GPU: the closed form of PIL's thin line against PIL, the oracle's own properties
(tests/box_output_reference.py), the planted faults its case list has to catch, the arithmetic core of the kernels
(csrc/box_overlay_core.h) run on the host under the sanitizers against the oracle, the validation codes of the two
launchers and the host side of `BoxOverlay`.  Everything is integers and bytes: every comparison is equality."""
import functools
import os
import shutil
import struct
import subprocess
import types

import numpy as np
import pytest
import torch

from dualdiff_amd import _build, _native
from dualdiff_amd import pipeline as P
from dualdiff_amd.pipeline import box_output as BO
from dualdiff_amd.pipeline import map_output as MO
from tests import box_output_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG, UNSUPPORTED = -1, -2
PTR = 16                                                 # non-null, 16-byte aligned, never dereferenced


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


@functools.lru_cache(maxsize=None)
def pictures(name, transparent, fault=None):
    """The oracle's overlay of a case: computed once, shared, never written to."""
    out = R.overlay(R.cases()[name], transparent, fault=fault)
    out.setflags(write=False)
    return out


DRAWN = tuple(n for n, c in R.cases().items() if not c.saturating)       # PIL's own integers end below 2^29


# ---- the line ---------------------------------------------------------------------------------------------------------

def mask_of(h, w, pixels):
    m = np.zeros((h, w), dtype=bool)
    for x, y in pixels:
        if 0 <= x < w and 0 <= y < h:
            m[y, x] = True
    return m


def test_closed_form_is_pils_line_on_every_small_pair():
    """All end point pairs in [-3, 10]^2 on an 8 x 8 canvas: 14^4 = 38 416 lines, the pixel list and the per-pixel test."""
    r = range(-3, 11)
    n = 0
    for x0 in r:
        for y0 in r:
            for x1 in r:
                for y1 in r:
                    want = R.pil_line_mask(8, 8, x0, y0, x1, y1)
                    assert np.array_equal(mask_of(8, 8, R.line_pixels(x0, y0, x1, y1)), want), (x0, y0, x1, y1)
                    if (x0 + 3 * y0 + 5 * x1 + 7 * y1) % 16 == 0:      # the membership form on a sixteenth of them
                        got = np.array([[R.on_line(int(x), int(y), x0, y0, x1, y1) for x in range(8)] for y in range(8)])
                        assert np.array_equal(got, want), (x0, y0, x1, y1)
                    n += 1
    assert n == 38416


def test_membership_form_is_pils_line_far_outside_the_canvas():
    """2 000 seeded lines with end points up to +-2^20 on a 40 x 24 canvas, half of them steered through the canvas."""
    rs = np.random.RandomState(20)
    h, w, hit = 24, 40, 0
    for k in range(2000):
        x0, y0, x1, y1 = (int(v) for v in rs.randint(-(1 << 20), (1 << 20) + 1, 4))
        if k % 2:                                                       # through a point of the canvas: the end is its mirror
            cx, cy = int(rs.randint(0, w)), int(rs.randint(0, h))
            x1, y1 = 2 * cx - x0 + int(rs.randint(-3, 4)), 2 * cy - y0 + int(rs.randint(-3, 4))
        want = R.pil_line_mask(h, w, x0, y0, x1, y1)
        got = np.array([[R.on_line(x, y, x0, y0, x1, y1) for x in range(w)] for y in range(h)])
        assert np.array_equal(got, want), (x0, y0, x1, y1)
        hit += bool(want.any())
    assert hit >= 900


# ---- the oracle's own properties ----------------------------------------------------------------------------------------

def test_a_line_depends_on_its_direction():
    assert R.line_pixels(0, 0, 2, 1) == [(0, 0), (1, 1), (2, 1)]
    assert sorted(R.line_pixels(2, 1, 0, 0)) == [(0, 0), (1, 0), (2, 1)]
    assert not np.array_equal(R.pil_line_mask(4, 4, 0, 0, 2, 1), R.pil_line_mask(4, 4, 2, 1, 0, 0))


def test_direction_boxes_tell_every_edges_direction():
    """The hand-made boxes the GPU test draws: reversing edge e changes box e's picture, for all twelve."""
    pts = R.direction_boxes()
    for e in range(12):
        good = R.draw_view(None, pts[e:e + 1], [e % 10], R.PALETTE, 16, 24, True)
        bad = R.draw_view(None, pts[e:e + 1], [e % 10], R.PALETTE, 16, 24, True, fault="reversed_edge:%d" % e)
        assert good[11, 11, 3] == 255 and good[10, 11, 3] == 0 and bad[10, 11, 3] == 255, e


def flat_box(x0, y0, x1, y1):
    """Integer points of a "box" whose twelve edges all lie on the rectangle (x0, y0) - (x1, y1)."""
    return np.array([[x0, y0], [x0, y0], [x1, y0], [x1, y0], [x0, y1], [x0, y1], [x1, y1], [x1, y1]])


def test_a_later_box_covers_an_earlier_one():
    pts = np.stack([flat_box(1, 1, 8, 6), flat_box(4, 1, 11, 6)])
    pic = R.draw_view(None, pts, [0, 8], R.PALETTE, 9, 14, True)
    assert tuple(pic[1, 2]) == R.PALETTE[0] + (255,)
    assert tuple(pic[1, 6]) == R.PALETTE[8] + (255,) and tuple(pic[1, 8]) == R.PALETTE[8] + (255,)      # shared pixels: the later
    assert tuple(pic[3, 3]) == (0, 0, 0, 0)
    swapped = R.draw_view(None, pts[::-1], [8, 0], R.PALETTE, 9, 14, True)
    assert tuple(swapped[1, 6]) == R.PALETTE[0] + (255,)


def test_a_corner_behind_the_camera_drops_the_box():
    rs = np.random.RandomState(0)
    t = R.camera(0.0, 32, 48, 40.0)
    inside = R.cuboid(rs, np.array([10.0, 0.5, 0.0]), np.array([2.0, 2.0, 2.0]), 0.3)
    through = R.cuboid(rs, np.array([0.5, 0.2, 0.0]), np.array([3.0, 1.0, 1.0]), 0.0)         # x from -1 to 2: z_cam < 0 at four corners
    _, _, z = R.project(np.stack([inside, through]), t)
    assert (z[0] > 0).all() and (z[1] > 0).sum() == 4
    pts, cls, count, flags = R.view_edges(np.stack([inside, through]), [1, 2], t, 10)
    assert count == 1 and cls.tolist() == [1] and flags == 0
    assert R.view_edges(np.stack([inside, through]), [1, 2], t, 10, fault="any_z")[2] == 2


def test_labels_index_as_python_does():
    rs = np.random.RandomState(0)
    t = R.camera(0.0, 32, 48, 40.0)
    boxes = np.stack([R.cuboid(rs, np.array([10.0 + 3 * k, 0.5, 0.0]), np.array([1.0, 1.0, 1.0]), 0.0) for k in range(5)])
    pts, cls, count, flags = R.view_edges(boxes, [-1, -10, 10, 9, -11], t, 10)
    assert count == 3 and flags == R.FLAG_LABEL
    assert cls.tolist() == [9, 0, 9]                                  # farthest first: boxes 3, 1, 0
    assert R.edge_arrays(R.cases()["bad_label"], 5)[3] & R.FLAG_LABEL


def test_alpha_is_any_channel_above_zero():
    palette = ((0, 0, 0), (0, 0, 1), (9, 0, 0))
    pts = np.stack([flat_box(0, 0, 3, 0), flat_box(0, 2, 3, 2), flat_box(0, 4, 3, 4), flat_box(2, 0, 2, 4)])
    pic = R.draw_view(None, pts, [2, 1, 2, 0], palette, 6, 5, True)
    assert pic[0].tolist() == [[9, 0, 0, 255], [9, 0, 0, 255], [0, 0, 0, 0], [9, 0, 0, 255], [0, 0, 0, 0]]       # black on top: alpha 0
    assert pic[2, 0].tolist() == [0, 0, 1, 255] and pic[1, 0].tolist() == [0, 0, 0, 0]
    frame = np.full((6, 5, 3), 77, np.uint8)
    assert R.draw_view(frame, pts, [2, 1, 2, 0], palette, 6, 5, False)[0, 2].tolist() == [0, 0, 0]                # opaque lines


def test_case_list_covers_what_the_issue_lists():
    c = R.cases()
    assert c["two_scenes"].transforms.shape[:2] == (2, 3) and [len(x) for x in c["two_scenes"].labels] == [0, 7]
    assert (c["two_scenes"].h, c["two_scenes"].w) == (64, 96)
    pts, cls, counts, flags = R.edge_arrays(c["seventy"], 70)
    assert counts.shape == (1, 1) and 64 < counts[0, 0] <= 70 and flags == 0
    assert R.edge_arrays(c["seventy"], 8)[3] == R.FLAG_CAP and R.edge_arrays(c["seventy"], 8)[2][0, 0] == counts[0, 0]
    assert same(R.edge_arrays(c["seventy"], 8)[0][0, 0], pts[0, 0, counts[0, 0] - 8:counts[0, 0]])                # the nearest eight
    assert R.edge_arrays(c["saturating"], 2)[3] == R.FLAG_SATURATED
    assert np.abs(R.edge_arrays(c["saturating"], 2)[0]).max() == R.SAT
    for name in DRAWN:                                                 # every drawn case draws something
        assert (pictures(name, True)[..., 3] == 255).any(), name
    assert R.edge_arrays(c["two_scenes"], 7)[2][1].sum() > 0 and R.edge_arrays(c["two_scenes"], 7)[2][0].sum() == 0


@pytest.mark.parametrize("fault", R.FAULTS)
def test_case_list_catches_planted_fault(fault):
    order = sorted(DRAWN, key=lambda n: n != "around")                # the case with the most ground first: stop at the first hit
    assert any(not same(pictures(n, t, fault), pictures(n, t)) for n in order for t in (False, True)), fault


# ---- the kernels' arithmetic on the host, under the sanitizers ---------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def hostcheck(tmp):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        return None, "no C++ compiler"
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    probe = os.path.join(tmp, "probe.cpp")
    with open(probe, "w") as f:
        f.write("int main() { return 0; }\n")
    for static in (["-static-libasan", "-static-libubsan"], []):
        if subprocess.run([cxx] + flags + static + [probe, "-o", os.path.join(tmp, "probe")], capture_output=True).returncode == 0:
            break
    else:
        return None, "the compiler links no sanitizer runtime"
    exe = os.path.join(tmp, "box_overlay_hostcheck")
    build = subprocess.run([cxx] + flags + static + ["-I", os.path.join(ROOT, "include"),
                            os.path.join(ROOT, "tools", "box_overlay_hostcheck.cpp"), "-o", exe, "-lm"],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    return exe, None


def run_hostcheck(exe, tmp, case, cap, transparent):
    offs = np.concatenate([[0], np.cumsum([len(x) for x in case.labels])]).astype(np.int32)
    corners = np.concatenate([np.asarray(c, np.float32).reshape(-1, 8, 3) for c in case.corners])
    labels = np.concatenate([np.asarray(x, np.int64).reshape(-1) for x in case.labels])
    s, v = case.transforms.shape[:2]
    palette = np.asarray(R.PALETTE, np.uint8)
    src, dst = os.path.join(tmp, "case.bin"), os.path.join(tmp, "out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<9i", s, v, len(labels), cap, len(palette), case.h, case.w, int(transparent), len(palette)))
        for a in (offs, corners, labels, case.transforms.astype(np.float32), palette):
            f.write(np.ascontiguousarray(a).tobytes())
        if not transparent:
            f.write(np.ascontiguousarray(case.frames).tobytes())
    run = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.returncode, run.stdout[-2000:], run.stderr[-3000:])
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
    raw = open(dst, "rb").read()
    m, ch = s * v, 4 if transparent else 3
    sizes = (m * cap * 16 * 4, m * cap * 4, m * 4, 4, m * case.h * case.w * ch)
    assert len(raw) == sum(sizes)
    at = np.cumsum((0,) + sizes)
    pts = np.frombuffer(raw[at[0]:at[1]], np.int32).reshape(s, v, cap, 8, 2)
    cls = np.frombuffer(raw[at[1]:at[2]], np.int32).reshape(s, v, cap)
    counts = np.frombuffer(raw[at[2]:at[3]], np.int32).reshape(s, v)
    flags = int(np.frombuffer(raw[at[3]:at[4]], np.int32)[0])
    out = np.frombuffer(raw[at[4]:at[5]], np.uint8).reshape(s, v, case.h, case.w, ch)
    return pts, cls, counts, flags, out


@pytest.mark.parametrize("transparent", (False, True))
@pytest.mark.parametrize("name,cap", [("two_scenes", 7), ("seventy", 70), ("seventy", 90), ("seventy", 8), ("around", 23),
                                      ("bad_label", 5), ("saturating", 2)])
def test_core_on_the_host_under_sanitizers(name, cap, transparent, tmp_path_factory):
    """tools/box_overlay_hostcheck.cpp, built with -fsanitize=address,undefined: the header's functions in the kernels'
    sequence give the oracle's pts, cls, counts, flags and pictures, and run clean."""
    exe, why = hostcheck(str(tmp_path_factory.getbasetemp()))
    if exe is None:
        pytest.skip(why)
    case = R.cases()[name]
    pts, cls, counts, flags, out = run_hostcheck(exe, str(tmp_path_factory.mktemp("hc")), case, cap, transparent)
    want = R.edge_arrays(case, cap)
    assert same(pts, want[0]) and same(cls, want[1]) and same(counts, want[2]) and flags == want[3]
    if case.saturating:
        return                                                         # PIL's own integers end below 2^29: the run being clean is the check
    s, v = counts.shape
    frames = None if transparent else case.frames.reshape(s * v, case.h, case.w, 3)
    pic = R.draw_arrays(frames, want[0].reshape(s * v, cap, 8, 2), want[1].reshape(s * v, cap), want[2].reshape(-1),
                        R.PALETTE, case.h, case.w, transparent)
    assert same(out.reshape(pic.shape), pic)
    if cap >= counts.max():
        assert same(out, pictures(name, transparent))


# ---- the launchers' validation, without a GPU ------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_build.lib_path()):
        pytest.skip("library not built (run __graft_entry__.build())")
    return _native.load(build_if_missing=False)


EDGE_KEYS = ("corners", "labels", "offsets", "transforms", "total", "scenes", "views", "cap", "n_classes", "pts", "cls",
             "counts", "flags")
DRAW_KEYS = ("frames", "pts", "cls", "counts", "palette", "out", "m", "cap", "h", "w", "n_palette", "transparent")


def edge_args(**kw):
    a = dict(corners=PTR, labels=PTR, offsets=PTR, transforms=PTR, total=7, scenes=2, views=3, cap=7, n_classes=10, pts=PTR,
             cls=PTR, counts=PTR, flags=PTR)
    a.update(kw)
    return tuple(a[k] for k in EDGE_KEYS) + (None,)


def draw_args(**kw):
    a = dict(frames=PTR, pts=PTR, cls=PTR, counts=PTR, palette=PTR, out=PTR, m=6, cap=7, h=64, w=96, n_palette=10, transparent=0)
    a.update(kw)
    return tuple(a[k] for k in DRAW_KEYS) + (None,)


EDGES_BAD = [dict(corners=None), dict(labels=None), dict(offsets=None), dict(transforms=None), dict(pts=None), dict(cls=None),
             dict(counts=None), dict(flags=None), dict(total=-1), dict(scenes=0), dict(views=0), dict(views=-3), dict(cap=0),
             dict(cap=-1), dict(n_classes=0), dict(corners=18), dict(labels=20), dict(offsets=17), dict(transforms=18),
             dict(pts=24), dict(pts=20), dict(cls=18), dict(counts=17), dict(flags=22)]
EDGES_UNSUPPORTED = [dict(cap=1025), dict(cap=0x7fffffff), dict(scenes=0x7fffffff, views=0x7fffffff),
                     dict(scenes=1 << 16, views=1 << 15)]
DRAW_BAD = [dict(pts=None), dict(cls=None), dict(counts=None), dict(palette=None), dict(out=None), dict(frames=None),
            dict(transparent=2), dict(transparent=-1), dict(m=0), dict(cap=0), dict(h=0), dict(w=-96), dict(n_palette=0),
            dict(pts=24), dict(cls=18), dict(counts=17), dict(transparent=1, out=18)]
DRAW_UNSUPPORTED = [dict(h=1 << 15), dict(w=1 << 15), dict(m=65536), dict(m=65535, cap=0x7fffffff),
                    dict(h=0x7fffffff, w=0x7fffffff)]


def test_launchers_validate_before_any_launch(lib):
    """DD_ERR_LAUNCH (-3) on a machine without a GPU would mean that a check came after a runtime call."""
    for kw in EDGES_BAD:
        assert lib.dd_box_edges(*edge_args(**kw)) == BAD_ARG, kw
    for kw in EDGES_UNSUPPORTED:
        assert lib.dd_box_edges(*edge_args(**kw)) == UNSUPPORTED, kw
    for kw in DRAW_BAD:
        assert lib.dd_box_draw_u8(*draw_args(**kw)) == BAD_ARG, kw
    for kw in DRAW_UNSUPPORTED:
        assert lib.dd_box_draw_u8(*draw_args(**kw)) == UNSUPPORTED, kw
    assert lib.dd_box_edges(*edge_args(total=0, corners=None, labels=None, cap=0)) == BAD_ARG       # NULL corners are legal with no boxes: cap decides


# ---- the Python layer ---------------------------------------------------------------------------------------------------

def test_default_palette_is_the_map_colours():
    assert tuple(BO.OBJECT_COLORS) == R.OBJECT_CLASSES
    assert tuple(BO.OBJECT_COLORS.values()) == R.PALETTE == tuple(MO.COLORS[n] for n in R.OBJECT_CLASSES)
    o = BO.BoxOverlay(R.OBJECT_CLASSES[::-1])
    assert same(o.palette_table(), np.asarray(R.PALETTE[::-1], np.uint8))
    o = BO.BoxOverlay(["a", "b"], palette={"a": (1, 2, 3), "b": [4, 5, 6], "c": (7, 8, 9)})
    assert o.palette_table().tolist() == [[1, 2, 3], [4, 5, 6]]


def test_exported_and_from_config():
    assert P.BoxOverlay is BO.BoxOverlay and P.box_output is BO and P.MapRender is MO.MapRender
    with pytest.raises(AttributeError):
        P.NoSuchName
    ds = {"object_classes": list(R.OBJECT_CLASSES)}
    for cfg in ({"dataset": ds}, types.SimpleNamespace(dataset=types.SimpleNamespace(**ds))):
        o = BO.BoxOverlay.from_config(cfg, transparent_bg=True)
        assert o.object_classes == R.OBJECT_CLASSES and o.transparent_bg is True and o.colors == R.PALETTE
    assert BO.BoxOverlay.from_config({"dataset": ds}).transparent_bg is False
    with pytest.raises(ValueError, match="object_classes"):
        BO.BoxOverlay.from_config({})
    with pytest.raises(ValueError, match="object_classes"):
        BO.BoxOverlay.from_config({"dataset": {"map_classes": []}})


def test_refusals():
    with pytest.raises(ValueError, match="non-empty"):
        BO.BoxOverlay([])
    with pytest.raises(ValueError, match="non-empty"):
        BO.BoxOverlay(None)
    with pytest.raises(ValueError, match="'tram' has no colour"):
        BO.BoxOverlay(["car", "tram"])
    with pytest.raises(ValueError, match="three bytes"):
        BO.BoxOverlay(["car"], palette={"car": (1, 2, 256)})
    with pytest.raises(ValueError, match="three bytes"):
        BO.BoxOverlay(["car"], palette={"car": (1, 2)})
    case = R.cases()["two_scenes"]
    o = BO.BoxOverlay(R.OBJECT_CLASSES)
    args = (case.corners, case.labels, case.transforms)
    with pytest.raises(RuntimeError, match="GPU only"):
        o(torch.from_numpy(case.frames.copy()), *args)
    with pytest.raises(ValueError, match=r"\(b, n, H, W, 3\)"):
        o(torch.from_numpy(case.frames[0].copy()), *args)
    with pytest.raises(ValueError, match=r"\(b, n, H, W, 3\)"):
        o(torch.from_numpy(case.frames.copy()).float(), *args)
    with pytest.raises(ValueError, match="transparent_bg only"):
        o(None, *args)
    x = torch.zeros(1, 8, 2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="GPU only"):
        BO.O.box_draw_u8(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), x[None], x[:, :1, 0], x[0, :1, 0], torch.zeros(2, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match=r"pts \(m, cap, 8, 2\)"):
        BO.O.box_draw_u8(None, x, x, x, x)
    with pytest.raises(ValueError, match="size="):
        BO.O.box_draw_u8(None, x[None], x[:, :1, 0], x[0, :1, 0], torch.zeros(2, 3, dtype=torch.uint8), transparent=True)
    with pytest.raises(RuntimeError, match="GPU only"):
        BO.O.box_edges(torch.zeros(2, 8, 3), torch.zeros(2, dtype=torch.int64), torch.tensor([0, 2], dtype=torch.int32),
                       torch.zeros(1, 3, 4, 4), 2, 10)
    with pytest.raises(_native.Unsupported, match="at most 1024"):
        BO.O.box_edges(torch.zeros(2, 8, 3), torch.zeros(2, dtype=torch.int64), torch.tensor([0, 2], dtype=torch.int32),
                       torch.zeros(1, 3, 4, 4), 1025, 10)
    with pytest.raises(ValueError, match="fp32 corners"):
        BO.O.box_edges(torch.zeros(2, 8, 3).double(), torch.zeros(2, dtype=torch.int64), torch.tensor([0, 2], dtype=torch.int32),
                       torch.zeros(1, 3, 4, 4), 2, 10)


# ---- RGBA files ----------------------------------------------------------------------------------------------------------

def test_rgba_entry_points_without_a_gpu(lib):
    import ctypes

    from dualdiff_amd import ops
    from dualdiff_amd.image_tables import png_capacity
    from dualdiff_amd.pipeline import image_output as IO
    assert lib.dd_png_workspace_bytes_c(2, 20, 32, 3) == lib.dd_png_workspace_bytes(2, 20, 32)
    need = lib.dd_png_workspace_bytes_c(2, 20, 32, 4)
    assert need >= 2 * (20 * 129 + 16389 + 16 + 4 + 8) and need % 16 == 0
    for ch in (0, 1, 2, 5, -4):
        assert lib.dd_png_workspace_bytes_c(2, 20, 32, ch) == -1
    assert lib.dd_png_workspace_bytes_c(1, 25000, 25000, 3) > 0 and lib.dd_png_workspace_bytes_c(1, 25000, 25000, 4) == -1
    P = ctypes.c_void_p(4096)

    def call(frames=P, m=2, h=20, w=32, ch=4, ws=P, ws_bytes=need, out=P, capacity=4096, lengths=P):
        return lib.dd_png_encode_u8c(frames, m, h, w, ch, ws, ws_bytes, out, capacity, lengths, None)
    for kw in ({"frames": None}, {"ws": None}, {"out": None}, {"lengths": None}, {"m": 0}, {"h": 0}, {"w": -8}, {"ch": 2},
               {"ch": 5}, {"ch": 0}, {"ws_bytes": need - 1}, {"capacity": 50}, {"ws": ctypes.c_void_p(4100)},
               {"lengths": ctypes.c_void_p(4098)}):
        assert call(**kw) == BAD_ARG, kw
    assert call(h=25000, w=25000, ws_bytes=1 << 62) == UNSUPPORTED and call(m=65536, ws_bytes=1 << 62) == UNSUPPORTED
    assert png_capacity(5, 7, 4) == 51 + 17 + 5 * 29 and png_capacity(5, 7) == png_capacity(5, 7, 3) == 51 + 17 + 5 * 22
    rgba = torch.zeros((2, 16, 24, 4), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="GPU only"):
        IO.encode_png_rgba(rgba)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.png_encode_u8c(rgba)
    for bad in (rgba[..., :3], rgba.float(), rgba[0, 0], rgba[:0]):
        with pytest.raises(ValueError, match="encode_png_rgba takes"):
            IO.encode_png_rgba(bad)
    with pytest.raises(ValueError, match="3 or 4"):
        ops.png_encode_u8c(rgba[..., :2])
    with pytest.raises(ValueError, match=r"\(m, H, W, 3\) frame batch"):
        ops.png_encode_u8(rgba)                                        # the RGB wrapper keeps refusing four channels
    with pytest.raises(ValueError, match="colour type 2"):
        IO.encode_png(rgba)
    x = torch.from_numpy(np.random.RandomState(3).randint(0, 256, (2, 6, 5, 7, 4)).astype(np.uint8))
    grid = IO.concat_views(x)
    assert grid.shape == (2, 10, 21, 4) and torch.equal(grid[1, 5:, 7:14], x[1, 4])
    assert IO.concat_views(x, oneline=True).shape == (2, 5, 42, 4)
    with pytest.raises(ValueError, match="concat_views takes"):
        IO.concat_views(x[..., :2])
