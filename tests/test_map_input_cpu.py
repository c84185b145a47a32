"""Map input without a GPU: the numpy restatement (tests/map_input_reference.py) against the fixture minted from the
reference's own lines, its polygon fill against Pillow itself (where importable) and against the pinned Pillow pictures,
the kernels' arithmetic core on the host under the sanitizers, the bit fields, the launcher's argument validation and the
interface errors of `BevMapInput`."""
import functools
import itertools
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from dualdiff_amd import _build, _native
from tests import map_input_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "map_input.npz")
BAD_ARG, UNSUPPORTED = -1, -2
P = 16                                                   # non-null, 16-byte aligned, never dereferenced
AUX = ("visibility", "center_offset", "center_ohw", "height")
PIL_SIDE = 12


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_build.lib_path()):
        pytest.skip("library not built (run __graft_entry__.build())")
    return _native.load(build_if_missing=False)


def scene_of(gold, s):
    return {k: gold["%s_%d" % (k, s)] for k in ("corners", "labels", "bottom_center", "height", "visibility")}


def ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


# ---- the restatement against the reference's own lines ----------------------------------------------------------------------

@pytest.mark.parametrize("s", (0, 1, 2))
def test_restatement_equals_the_reference_lines(gold, s):
    """Masks exact.  Aux: visibility, center_offset and height exact; center_ohw within 1 float32 ulp (numpy's norm goes
    through a BLAS dot whose contraction is not defined).  OBSERVED on the fixture: 0 ulp, every element equal."""
    bound = tuple(gold["bound"].tolist())
    sc = scene_of(gold, s)
    assert len(sc["labels"]) == int(gold["counts"][s])
    static = R.one_hot_decode(gold["static_bits_%d" % s], 8)
    masks, aux = R.scene(static, sc["corners"], sc["labels"], sc["bottom_center"], sc["height"], sc["visibility"], 10, AUX,
                         bound, bound)
    want_m, want_a = gold["gt_masks_bev_%d" % s], gold["gt_aux_bev_%d" % s]
    assert masks.dtype == np.uint8 and masks.shape == want_m.shape == (18, 200, 200)
    assert np.array_equal(masks, want_m)
    assert aux.dtype == np.float32 and aux.shape == want_a.shape == (8, 200, 200)
    for ch in (0, 1, 2, 7):
        assert np.array_equal(aux[ch], want_a[ch]), ch
    worst = int(ulps(aux[3:7], want_a[3:7]).max())
    print("scene %d: center_ohw differs by at most %d ulp" % (s, worst))
    assert worst <= 1
    assert R.flagged(sc["corners"], gold["lidar2canvas"]) == 0


def test_fixture_keeps_its_conditions(gold):
    """the scenes hold what the tests are about: boxes beyond the canvas, labels outside the classes, thin boxes whose
    quads have repeated vertices, overlapping boxes, and every aux channel set somewhere"""
    l2c = gold["lidar2canvas"]
    assert np.array_equal(l2c, R.canvas_of((-50.0, 50.0, 0.5), (-50.0, 50.0, 0.5))[1])
    assert gold["counts"].tolist() == [0, 5, 70]
    sc = scene_of(gold, 2)
    quads = np.stack([R.quad_of(c, l2c) for c in sc["corners"]])
    assert (quads < 0).any() and (quads > 199).any()
    assert (sc["labels"] == -1).any() and (sc["labels"] == 10).any()
    repeated = sum(len({tuple(p) for p in q}) < 4 for q in quads)
    assert repeated >= 5, repeated
    masks, aux = gold["gt_masks_bev_2"], gold["gt_aux_bev_2"]
    assert masks[8:].any(axis=(1, 2)).sum() >= 8 and (masks[8:].sum(axis=0) > 1).any()
    assert all(np.any(aux[ch] != 0) for ch in range(8))
    assert not gold["gt_masks_bev_0"][8:].any() and not gold["gt_aux_bev_0"].any()
    # the reference's bounds: the canvas coordinates are exact, so the rounded vertex is defined everywhere
    c = R.to_canvas(sc["corners"][:, list(R.BOTTOM), :2], l2c)
    assert np.array_equal(c, sc["corners"][:, list(R.BOTTOM), :2].astype(np.float64) * 2 + 100)


def test_aux_order_is_fixed_and_subsets_keep_it(gold):
    sc = scene_of(gold, 1)
    l2c = gold["lidar2canvas"]
    full = gold["gt_aux_bev_1"]
    rows = {"visibility": [0], "center_offset": [1, 2], "center_ohw": [3, 4, 5, 6], "height": [7]}
    for k in range(1, 5):
        for names in itertools.combinations(AUX, k):
            got = R.aux_layers(sc["corners"], sc["bottom_center"], sc["height"], sc["visibility"], names[::-1], 200, l2c)
            want = full[[r for n in AUX if n in names for r in rows[n]]]
            assert got.shape == want.shape and np.array_equal(got, want), names
    assert R.aux_layers(sc["corners"], sc["bottom_center"], sc["height"], sc["visibility"], None, 200, l2c) is None
    assert R.aux_layers(sc["corners"], sc["bottom_center"], sc["height"], sc["visibility"], (), 200, l2c) is None
    with pytest.raises(ValueError, match="unknown aux_data"):
        R.aux_channels_of(("visibility", "yaw"))


def test_bit_fields_against_one_hot_decode(gold):
    for s in range(3):
        assert np.array_equal(R.one_hot_decode(gold["static_bits_%d" % s], 8), gold["gt_masks_bev_%d" % s][:8])
        assert np.array_equal(R.one_hot_encode(gold["gt_masks_bev_%d" % s][:8]), gold["static_bits_%d" % s])
    assert np.array_equal(R.one_hot_decode(gold["masks_bits_2"], 18), gold["gt_masks_bev_2"])
    assert np.array_equal(R.one_hot_encode(gold["gt_masks_bev_2"]), gold["masks_bits_2"])
    assert np.array_equal(R.one_hot_decode(gold["bits30"], 30), gold["layers30"])
    assert gold["bits30"].dtype == np.int32 and gold["bits30"][1, 2] == 1 << 29 and gold["bits30"][3, 3] == (1 << 29) + 1


def test_collate_against_the_reference(gold):
    want = np.unpackbits(gold["bev_map_with_aux_bits"])[:3 * 8 * 200 * 200].reshape(3, 8, 200, 200).astype(np.float32)
    got = R.collate([gold["gt_masks_bev_%d" % s] for s in range(3)], 8)
    assert got.dtype == np.float32 and np.array_equal(got, want)


# ---- the polygon fill against Pillow ------------------------------------------------------------------------------------------

def pil_fill(q, size):
    from PIL import Image, ImageDraw
    im = Image.fromarray(np.zeros((size, size), np.uint8))
    ImageDraw.Draw(im).polygon([int(v) for p in q for v in p], fill=1)
    return np.array(im)


def repeated_vertex_quads(points):
    """every ring of four out of `points` with a repeated vertex: the point, the segment-like, the triangle-like and the
    opposite-vertices families, in every rotation"""
    seen = set()
    for a in points:
        for b in points:
            for c in points:
                for q in ((a, a, b, c), (a, b, b, c), (a, b, c, c), (a, b, c, a), (a, b, a, c), (b, a, c, a)):
                    if q not in seen:
                        seen.add(q)
                        yield q


def rotated_rectangles(rng, n, size):
    for it in range(n):
        cx, cy = rng.uniform(-4, size + 4, 2)
        l, w, yaw = rng.uniform(0.3, 1.2 * size), rng.uniform(0.3, 0.5 * size), rng.uniform(-math.pi, math.pi)
        kind = it % 10
        if kind < 3:
            yaw = round(yaw / (math.pi / 4)) * math.pi / 4                        # axis-aligned and 45 degrees
        elif kind < 5:                                                            # edges of slope 1/2 and 2: the rounding ties
            yaw = math.atan2(*((1, 2), (2, 1), (-1, 2), (1, -2))[(it // 10) % 4])
            cx, cy, l, w = round(cx), round(cy), max(1, round(l / 3)) * math.sqrt(5), max(1, round(w / 3)) * math.sqrt(5)
        elif kind == 5:
            l, w = rng.uniform(0.2, 1.4), rng.uniform(0.2, 1.4)                   # a pedestrian, a cone: repeated vertices
        c, s = math.cos(yaw), math.sin(yaw)
        yield tuple(tuple(int(v) for v in np.round((cx + c * a * l / 2 - s * b * w / 2, cy + s * a * l / 2 + c * b * w / 2)))
                    for a, b in ((-1, -1), (-1, 1), (1, 1), (1, -1)))


def test_polygon_equals_pillow_on_every_repeated_vertex_quad():
    """Exhaustive on a 4 x 4 grid that straddles the canvas's first corner and on one that straddles its last: every quad
    with a repeated vertex that is not of the undrawn family equals Pillow with 0 differing pixels; the undrawn family is
    exactly what `quad_unsupported` names.  (The same enumeration on a 7 x 7 grid, -2 .. 4, gave 0 differing pixels for
    the point, segment-like and triangle-like families when the rule was established; it takes minutes.)"""
    pytest.importorskip("PIL")
    size, checked, undrawn = 6, 0, 0
    for lo in (-1, size - 3):
        pts = [(x, y) for x in range(lo, lo + 4) for y in range(lo, lo + 4)]
        for q in repeated_vertex_quads(pts):
            if R.quad_unsupported(q):
                undrawn += 1
                assert q[0] == q[2] or q[1] == q[3]
                continue
            checked += 1
            got = R.polygon_fill(np.zeros((size, size), np.uint8), q)
            assert np.array_equal(got, pil_fill(q, size)), q
    assert checked > 20000 and undrawn > 0


def test_polygon_equals_pillow_on_rounded_rectangles():
    """10 000 random rotated rectangles, rounded: multiples of 45 degrees, slopes of 1/2 and 2, quads off the canvas, negative
    coordinates, boxes of a pixel or less.  No rounded rectangle is of the undrawn family."""
    pytest.importorskip("PIL")
    rng = np.random.default_rng(401)
    size, repeated, off = 24, 0, 0
    for q in rotated_rectangles(rng, 10000, size):
        assert not R.quad_unsupported(q), q
        repeated += len(set(q)) < 4
        off += min(min(p) for p in q) < 0 or max(max(p) for p in q) >= size
        assert np.array_equal(R.polygon_fill(np.zeros((size, size), np.uint8), q), pil_fill(q, size)), q
    assert repeated > 300 and off > 2000, (repeated, off)


def test_polygon_equals_the_pinned_pillow_pictures(gold):
    quads = gold["pil_quads"].astype(np.int64)
    n = len(quads)
    pics = np.unpackbits(gold["pil_masks"])[:n * PIL_SIDE * PIL_SIDE].reshape(n, PIL_SIDE, PIL_SIDE)
    assert n > 3000 and str(gold["pil_version"]).split(".")[0].isdigit()
    for q, want in zip(quads, pics):
        assert not R.quad_unsupported(q)
        assert np.array_equal(R.polygon_fill(np.zeros((PIL_SIDE, PIL_SIDE), np.uint8), q), want), q.tolist()


def test_undrawn_family_is_what_the_documents_say():
    assert R.quad_unsupported(((0, 0), (2, 1), (0, 0), (1, 3)))
    assert R.quad_unsupported(((5, 5), (3, 3), (9, 9), (3, 3)))
    assert not R.quad_unsupported(((0, 0), (1, 1), (0, 0), (-1, 0)))            # within a pixel of the repeated vertex
    assert not R.quad_unsupported(((0, 0), (5, 5), (0, 0), (5, 5)))             # segment-like
    assert not R.quad_unsupported(((0, 0), (0, 0), (5, 5), (2, 7)))             # triangle-like
    assert not R.quad_unsupported(((0, 0), (5, 0), (5, 3), (0, 3)))


# ---- the kernels' arithmetic on the host, under the sanitizers ---------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def hostcheck(tmp):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        return None, "no C++ compiler"
    flags = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    probe = os.path.join(tmp, "probe.cpp")
    with open(probe, "w") as f:
        f.write("int main() { return 0; }\n")
    for static in (["-static-libasan", "-static-libubsan"], []):
        if subprocess.run([cxx] + flags + static + [probe, "-o", os.path.join(tmp, "probe")], capture_output=True).returncode == 0:
            break
    else:
        return None, "the compiler links no sanitizer runtime"
    exe = os.path.join(tmp, "bev_map_hostcheck")
    build = subprocess.run([cxx] + flags + static + ["-I", os.path.join(ROOT, "dualdiff_amd", "csrc"),
                            os.path.join(ROOT, "tools", "bev_map_hostcheck.cpp"), "-o", exe, "-lm"],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    return exe, None


def test_core_on_the_host_under_sanitizers(gold, tmp_path_factory):
    """tools/bev_map_hostcheck.cpp, built with -fsanitize=address,undefined: the functions of csrc/bev_map_core.h that the
    kernels call give the restatement's pixels for the pinned quads, for rounded rectangles, for arbitrary quads and for
    saturated vertices, name the same quads as undrawn, and run clean."""
    exe, why = hostcheck(str(tmp_path_factory.mktemp("bev_map_hc")))
    if exe is None:
        pytest.skip(why)
    rng = np.random.default_rng(77)
    quads = [tuple(map(tuple, q)) for q in gold["pil_quads"].astype(int).tolist()][::3]
    quads += list(rotated_rectangles(rng, 1500, PIL_SIDE))
    quads += [tuple(tuple(int(v) for v in rng.integers(-3, PIL_SIDE + 3, 2)) for _ in range(4)) for _ in range(1500)]
    pts = [(x, y) for x in (-1, 1, 3) for y in (0, 2, 11)]
    quads += [q for q in repeated_vertex_quads(pts)]
    quads += [((-(1 << 20), 3), (5, -(1 << 20)), (1 << 20, 7), (4, 1 << 20)), ((0, 0), (1 << 20, 1 << 20), (3, 9), (0, 5))]
    text = "".join("%d %s\n" % (PIL_SIDE, " ".join("%d %d" % p for p in q)) for q in quads)
    run = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    lines = run.stdout.split("\n")[:-1]
    assert len(lines) == len(quads)
    undrawn = 0
    for q, line in zip(quads, lines):
        if R.quad_unsupported(q):
            undrawn += 1
            assert line == "F", q
            continue
        want = R.polygon_fill(np.zeros((PIL_SIDE, PIL_SIDE), np.uint8), q)
        assert line == "".join(map(str, want.reshape(-1).tolist())), q
    assert undrawn > 100


# ---- the launcher and the interface -------------------------------------------------------------------------------------------

ARGS = ("stat", "bits", "corners", "bc", "height", "vis", "labels", "offsets", "total", "b", "size", "ns", "nd", "aux_sel",
        "sx", "ox", "sy", "oy", "ws", "ws_bytes", "masks", "aux", "flags")


def layer_args(**kw):
    a = dict(stat=P, bits=0, corners=P, bc=P, height=P, vis=P, labels=P, offsets=P, total=3, b=1, size=40, ns=8, nd=10,
             aux_sel=15, sx=2.0, ox=20.0, sy=2.0, oy=20.0, ws=P, ws_bytes=3 * 208, masks=P, aux=P, flags=P)
    a.update(kw)
    return tuple(a[k] for k in ARGS) + (None,)


@pytest.mark.parametrize("bad", [dict(stat=None), dict(corners=None), dict(bc=None), dict(height=None), dict(vis=None),
                                 dict(labels=None), dict(offsets=None), dict(ws=None), dict(masks=None), dict(flags=None),
                                 dict(aux=None), dict(aux_sel=0), dict(aux_sel=16), dict(aux_sel=-1), dict(bits=2),
                                 dict(total=-1), dict(b=0), dict(size=0), dict(ns=-1), dict(nd=-1), dict(ns=0, nd=0),
                                 dict(ns=21, nd=10), dict(sx=float("nan")), dict(oy=float("inf")), dict(ws_bytes=3 * 208 - 1),
                                 dict(ws=24), dict(labels=20), dict(corners=18), dict(aux=18), dict(flags=18),
                                 dict(stat=18, bits=1), dict(offsets=18)],
                         ids=lambda d: ",".join("%s=%s" % kv for kv in d.items()))
def test_launcher_rejects_bad_arguments(lib, bad):
    """the bad-argument code, not the launch-failure code: validation comes before any HIP runtime call"""
    assert lib.dd_bev_map_layers(*layer_args(**bad)) == BAD_ARG


def test_launcher_limits_and_workspace(lib):
    assert lib.dd_bev_map_layers(*layer_args(size=4097)) == UNSUPPORTED
    assert lib.dd_bev_map_layers(*layer_args(b=65536)) == UNSUPPORTED
    assert lib.dd_bev_map_layers(*layer_args(total=(1 << 20) + 1, ws_bytes=1 << 40)) == UNSUPPORTED
    assert lib.dd_bev_map_workspace_bytes(0) == 208 and lib.dd_bev_map_workspace_bytes(3) == 3 * 208
    assert lib.dd_bev_map_workspace_bytes(-1) == -1 and lib.dd_bev_map_workspace_bytes((1 << 20) + 1) == -1


def test_abi_has_the_entry_points(lib):
    import re
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dualdiff_hip.h")).read(), flags=re.S)
    for name in ("dd_bev_map_layers", "dd_bev_map_workspace_bytes"):
        assert name in _native.SIGNATURES and hasattr(lib, name)
        assert re.search(r"\b%s\s*\(" % name, hdr) is not None
    assert "bev_map.hip" in _build.SOURCES and "bev_map.hip" not in _build.EXTRA_FLAGS        # built as boxes.hip is: no fast-math
    assert lib.dd_abi_version() == 4


def test_interface_errors():
    from dualdiff_amd.pipeline import BevMapInput
    from dualdiff_amd.pipeline import map_input as M
    with pytest.raises(ValueError, match="non-square canvas"):
        BevMapInput((-50, 50, 0.5), (-25, 25, 0.5))
    with pytest.raises(ValueError, match="more than 30 layers"):
        BevMapInput(n_static=21, n_object=10)
    BevMapInput(n_static=20, n_object=10, device="cpu")
    with pytest.raises(ValueError, match=r"unknown aux_data \['yaw'\]"):
        BevMapInput(aux_data=("visibility", "yaw"))
    with pytest.raises(ValueError, match="no layer"):
        BevMapInput(n_static=0, n_object=0)
    with pytest.raises(ValueError, match="xbound"):
        BevMapInput(xbound=(50, -50, 0.5))
    mi = BevMapInput(aux_data=("height", "visibility"), device="cpu")
    assert (mi.size, mi.ns, mi.nd, mi.aux_sel, mi.aux_channels) == (200, 8, 10, 9, 2) and mi.l2c == (2.0, 100.0, 2.0, 100.0)
    assert BevMapInput(aux_data=None, device="cpu").aux_channels == 0 and BevMapInput(aux_data=(), device="cpu").aux_sel == 0
    cfg = {"dataset": {"map_bound": {"x": [-50.0, 50.0, 0.5], "y": [-50.0, 50.0, 0.5]}, "map_classes": ["a"] * 8,
                       "object_classes": ["b"] * 10, "aux_data": ["visibility", "center_offset", "center_ohw", "height"]}}
    mi = BevMapInput.from_config(cfg, device="cpu")
    assert (mi.size, mi.ns, mi.nd, mi.aux_channels) == (200, 8, 10, 8)
    with pytest.raises(ValueError, match="map_bound"):
        BevMapInput.from_config({"dataset": {"map_classes": []}})
    src = open(M.__file__).read()
    assert "import PIL" not in src and "from PIL" not in src
    # CPU tensors where device tensors are required
    static = torch.zeros((1, 8, 200, 200), dtype=torch.uint8)
    empty = dict(bottom_center=[torch.zeros((0, 3))], height=[torch.zeros(0)], visibility=[torch.zeros(0)])
    with pytest.raises(RuntimeError, match="static must be on the device"):
        mi(static, [torch.zeros((0, 8, 3))], [torch.zeros(0, dtype=torch.int64)], **empty)


def test_ops_refuse_cpu_tensors():
    from dualdiff_amd import ops as O
    if not os.path.exists(_build.lib_path()):
        pytest.skip("library not built")
    z = torch.zeros
    with pytest.raises(RuntimeError, match="GPU only"):
        O.bev_map_layers(z((1, 8, 16, 16), dtype=torch.uint8), z((2, 8, 3)), z((2, 3)), z(2), z(2), z(2, dtype=torch.int64),
                         torch.tensor([0, 2], dtype=torch.int32), 16, 8, 10, 15, (2.0, 8.0, 2.0, 8.0))
    with pytest.raises(ValueError, match="at most 30 layers"):
        O.bev_map_layers(None, z((0, 8, 3)), z((0, 3)), z(0), z(0), z(0, dtype=torch.int64),
                         torch.tensor([0, 0], dtype=torch.int32), 16, 21, 10, 0, (2.0, 8.0, 2.0, 8.0))
