"""FGM loss mask without a GPU: the numpy restatement (tests/fgm_reference.py) against the fixture minted from the
reference's own `create_heatmap_gt` and `hd_crop`, its hull and crossing rule against scipy and matplotlib themselves (where
importable), the kernels' arithmetic core on the host under the sanitizers, the launchers' argument validation and the
interface of `FgmMask` / `fgm_loss`."""
import functools
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

from dualdiff_amd import _build, _native
from tests import fgm_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "fgm_mask.npz")
BAD_ARG, UNSUPPORTED = -1, -2
P = 16                                                   # non-null, 16-byte aligned, never dereferenced
SETS = (("seeded", "grid", None), ("hand", "hand_grid", None), ("crop", "crop_grid", "crop"))


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_build.lib_path()):
        pytest.skip("library not built (run __graft_entry__.build())")
    return _native.load(build_if_missing=False)


def case(gold, name, grid_key, crop_key):
    grid = tuple(int(v) for v in gold[grid_key])
    crop = None if crop_key is None else tuple(int(v) for v in gold[crop_key])
    return gold[name + "_bboxes"], gold[name + "_masks"], gold[name + "_l2i"], grid, crop


@functools.lru_cache(maxsize=None)
def restated(name):
    g = dict(np.load(GOLD))
    grid_key, crop_key = {s[0]: s[1:] for s in SETS}[name]
    bboxes, masks, l2i, grid, crop = case(g, name, grid_key, crop_key)
    return R.heatmap(bboxes, masks, l2i, grid, crop)


# ---- the restatement against the reference's own run -------------------------------------------------------------------

def test_fixture_holds_the_cases(gold):
    assert tuple(gold["grid"]) == (12, 9) and gold["seeded_masks"].shape == (2, 2, 72)
    assert sorted(gold["seeded_masks"].sum(-1).reshape(-1).tolist()) == [0, 5, 33, 70]
    names = set(gold["hand_names"].tolist())
    assert {"triangle", "triangle_reversed", "collinear_on_hull_edge", "line_horizontal", "line_vertical", "line_diagonal",
            "line_not_monotone", "one_point", "two_points", "all_behind", "duplicates", "whole_grid", "negative_truncation",
            "overlap_max", "past_the_bound"} <= names
    assert tuple(gold["crop_grid"]) == (96, 54) and tuple(gold["crop"]) == (32, 88) and gold["crop_heat"].shape == (1, 2, 32, 88)
    assert int(gold["hand_flagged"]) == 1
    for name in ("seeded", "hand", "crop"):                # no view of a fixture is trivially empty by accident
        assert (gold[name + "_heat"] != 0).mean() > 0.1


@pytest.mark.parametrize("name", [s[0] for s in SETS])
def test_restatement_equals_the_reference(gold, name):
    """every element of the map, the flagged count, and per box what the reference's own per-instance call painted"""
    res = restated(name)
    want = gold[name + "_heat"]
    assert res["heat"].dtype == np.float32 and res["heat"].shape == want.shape
    assert np.array_equal(res["heat"], want)
    assert res["flagged"] == (int(gold["hand_flagged"]) if name == "hand" else 0)
    ran = gold[name + "_npts"] >= 0                        # the boxes that went through the reference
    painted = np.where(res["area"] > 0, res["weight"], np.float32(0))
    assert np.array_equal(painted[ran], gold[name + "_peak"][ran])
    assert np.array_equal(np.where(res["weight"] != 0, res["area"], 0)[ran], gold[name + "_count"][ran])
    if name == "crop":
        full = R.heatmap(*case(gold, "crop", "crop_grid", None)[:4])["heat"]
        assert np.array_equal(full, gold["crop_heat_full"])
    if name == "hand":
        j = gold["hand_names"].tolist().index("whole_grid")
        assert res["area"][0, j, 0] == 16 * 9 and res["weight"][0, j, 0] == 0
        j = gold["hand_names"].tolist().index("negative_truncation")
        assert (0, 0) in res["rings"][(0, j, 0)]           # (-0.7, -0.7) truncates toward zero


@pytest.mark.parametrize("name", [s[0] for s in SETS])
def test_explicit_projection_equals_the_reference_matmul(gold, name):
    """the k = 0..3 single-operation projection gives the integers the reference's `@` gave, on every fixture box"""
    bboxes, masks, l2i, grid, _ = case(gold, name, *{s[0]: s[1:] for s in SETS}[name])
    b, n, m = masks.shape
    seen = 0
    for i in range(b):
        for j in range(n):
            for k in range(m):
                cnt = int(gold[name + "_npts"][i, j, k])
                if cnt < 0:
                    continue
                pts, bad = R.project(bboxes[i, j, k], l2i[i, j], grid)
                assert not bad
                assert pts == [tuple(p) for p in gold[name + "_pts"][i, j, k, :cnt].tolist()], (i, j, k)
                seen += 1
    assert seen == int((gold[name + "_npts"] >= 0).sum()) > 0


# ---- the hull and the rule against the libraries -----------------------------------------------------------------------

def library_mask(pts, width, height):
    """the reference's lines with the libraries themselves: ConvexHull's vertices or, where it raises, the points; then
    contains_point per pixel -> (mask, whether the hull was taken)"""
    from matplotlib.patches import Polygon
    from scipy.spatial import ConvexHull
    coords = np.array(pts, dtype=int).reshape(-1, 2)
    hulled = False
    try:
        coords = coords[ConvexHull(coords).vertices]
        hulled = True
    except Exception:
        pass
    poly = Polygon(coords, closed=True)
    mask = np.zeros((height, width), bool)
    for x in range(width):
        for y in range(height):
            mask[y, x] = poly.contains_point((x, y), radius=0)
    return mask, hulled


def point_sets(rng, count):
    """1..8 integer points around a 12 x 9 grid: spread, clustered (repeats), collinear in every direction, off the grid"""
    for it in range(count):
        n = int(rng.integers(1, 9))
        kind = it % 5
        if kind == 0:
            pts = rng.integers(-3, 15, (n, 2))
        elif kind == 1:
            pts = rng.integers(3, 6, (n, 2))
        elif kind == 2:
            o, d = rng.integers(0, 9, 2), rng.integers(-2, 3, 2)
            pts = o + np.outer(rng.integers(-3, 5, n), d)
        elif kind == 3:
            pts = rng.integers(0, 12, (n, 2))
            pts[:, int(rng.integers(0, 2))] = int(rng.integers(0, 9))
        else:
            pts = rng.integers(-20, 30, (n, 2))
        yield [tuple(int(v) for v in p) for p in pts]


def test_hull_and_rule_equal_scipy_and_matplotlib():
    """>= 2000 seeded point sets: the restated polygon paints what the libraries paint, and ConvexHull raises exactly
    where the exact hull has fewer than three vertices — the sweep that licenses computing the hull ourselves"""
    pytest.importorskip("scipy.spatial")
    pytest.importorskip("matplotlib.patches")
    rng = np.random.default_rng(20277)
    total = degenerate = painted_degenerate = 0
    for pts in point_sets(rng, 2200):
        want, hulled = library_mask(pts, 12, 9)
        h = R.hull(pts)
        assert hulled == (len(h) >= 3), pts
        got = R.paint(R.ring(pts), 12, 9)
        assert np.array_equal(got, want), pts
        assert got[0, 0] == R.inside(R.ring(pts), 0, 0) and got[4, 6] == R.inside(R.ring(pts), 6, 4)
        total += 1
        degenerate += not hulled
        painted_degenerate += (not hulled) and bool(want.any())
    assert total >= 2000 and degenerate > 300 and painted_degenerate > 50
    assert not R.paint([], 12, 9).any() and not library_mask([], 12, 9)[0].any()           # the empty polygon


def test_thin_triangles_at_the_bound_equal_the_libraries():
    """coordinates up to 2^25 in magnitude, triangles a pixel or less wide across the grid: qhull still returns the
    hull, and the int64 rule equals matplotlib's float64 rule"""
    pytest.importorskip("scipy.spatial")
    pytest.importorskip("matplotlib.patches")
    rng = np.random.default_rng(9)
    far = R.BOUND
    for it in range(300):
        y0, y1 = (int(v) for v in rng.integers(-4, 13, 2))
        a = (-far + int(rng.integers(0, 3)), y0)
        b = (far - int(rng.integers(0, 3)), y1)
        c = (far - int(rng.integers(0, 3)), y1 + int(rng.integers(1, 3))) if it % 2 else (int(rng.integers(0, 12)), far)
        pts = [a, b, c][::1 if it % 3 else -1]
        want, hulled = library_mask(pts, 12, 9)
        assert hulled and len(R.hull(pts)) == 3, pts
        assert np.array_equal(R.paint(R.ring(pts), 12, 9), want), pts


# ---- the kernels' arithmetic on the host, under the sanitizers ---------------------------------------------------------

@pytest.fixture(scope="module")
def hostcheck(tmp_path_factory):
    """(the program built under the sanitizers, None) or (None, why not): built once for the module"""
    tmp = str(tmp_path_factory.mktemp("fgm_mask_hc"))
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
    exe = os.path.join(tmp, "fgm_mask_hostcheck")
    build = subprocess.run([cxx] + flags + static + ["-I", os.path.join(ROOT, "dualdiff_amd", "csrc"),
                            os.path.join(ROOT, "tools", "fgm_mask_hostcheck.cpp"), "-o", exe, "-lm"],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    return exe, None


def hostcheck_input(bboxes, masks, l2i, grid, crop):
    b, n, m = masks.shape
    ho, wo = crop if crop is not None else (grid[1], grid[0])
    bits64 = lambda v: struct.unpack("<Q", struct.pack("<d", v))[0]                          # noqa: E731
    words = [grid[0], grid[1], wo, ho, b * n, m, bboxes.shape[3], bits64(grid[0] / 1600), bits64(grid[1] / 900)]
    cb = np.ascontiguousarray(bboxes, np.float32).view(np.uint32).reshape(b * n, m, -1)
    tb = np.ascontiguousarray(l2i, np.float32).view(np.uint32).reshape(b * n, 16)
    for v in range(b * n):
        words += tb[v].tolist()
        for k in range(m):
            words.append(int(masks.reshape(b * n, m)[v, k]))
            words += cb[v, k].tolist()
    return " ".join(str(w) for w in words) + "\n"


@pytest.mark.parametrize("name", [s[0] for s in SETS])
def test_core_on_the_host_under_sanitizers(gold, name, hostcheck):
    """tools/fgm_mask_hostcheck.cpp, built with -fsanitize=address,undefined as its own program: the functions of
    csrc/fgm_mask_core.h that the kernels call, in the kernels' sequence, give the restatement's map bit for bit, its
    areas and its flagged count on the fixture, and run clean"""
    exe, why = hostcheck
    if exe is None:
        pytest.skip(why)
    bboxes, masks, l2i, grid, crop = case(gold, name, *{s[0]: s[1:] for s in SETS}[name])
    run = subprocess.run([exe], input=hostcheck_input(bboxes, masks, l2i, grid, crop), capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    lines = run.stdout.split("\n")[:-1]
    b, n, m = masks.shape
    assert len(lines) == 2 * b * n + 1
    res = restated(name)
    assert lines[-1] == "flags %d" % res["flagged"]
    want = res["heat"].reshape(b * n, -1)
    for v in range(b * n):
        assert lines[2 * v].split()[1:] == [str(a) for a in res["area"].reshape(b * n, m)[v].tolist()], v
        got = np.array([int(w, 16) for w in lines[2 * v + 1].split()], np.uint32).view(np.float32)
        assert np.array_equal(got, want[v]), v


# ---- the launchers and the interface -----------------------------------------------------------------------------------

MASK_ARGS = ("corners", "masks", "l2i", "views", "m", "points", "w", "h", "wo", "ho", "sx", "sy", "ws", "ws_bytes", "out",
             "flags")


def mask_args(**kw):
    a = dict(corners=P, masks=P, l2i=P, views=12, m=40, points=8, w=50, h=28, wo=50, ho=28, sx=50 / 1600, sy=28 / 900, ws=P,
             ws_bytes=12 * 40 * 96, out=P, flags=P)
    a.update(kw)
    return tuple(a[k] for k in MASK_ARGS) + (None,)


@pytest.mark.parametrize("bad", [dict(corners=None), dict(masks=None), dict(l2i=None), dict(ws=None), dict(out=None),
                                 dict(flags=None), dict(points=0), dict(points=9), dict(w=0), dict(h=0), dict(w=1025, h=1024),
                                 dict(wo=51), dict(ho=29), dict(wo=0), dict(ho=0), dict(wo=49), dict(views=0), dict(m=-1),
                                 dict(sx=float("nan")), dict(sy=float("inf")), dict(ws_bytes=12 * 40 * 96 - 1), dict(ws=24),
                                 dict(corners=18), dict(l2i=18), dict(out=18), dict(flags=18)],
                         ids=lambda d: ",".join("%s=%s" % kv for kv in d.items()))
def test_mask_launcher_rejects_bad_arguments(lib, bad):
    """the bad-argument code, not the launch-failure code: validation comes before any HIP runtime call"""
    assert lib.dd_fgm_mask(*mask_args(**bad)) == BAD_ARG


def test_mask_launcher_limits_and_workspace(lib):
    assert lib.dd_fgm_mask(*mask_args(views=65536, m=1, ws_bytes=1 << 40)) == UNSUPPORTED
    assert lib.dd_fgm_mask(*mask_args(views=1025, m=1024, ws_bytes=1 << 40)) == UNSUPPORTED
    assert lib.dd_fgm_mask(*mask_args(w=1024, h=1025)) == BAD_ARG and lib.dd_fgm_mask(*mask_args(w=0, wo=0)) == BAD_ARG
    assert lib.dd_fgm_workspace_bytes(0) == 96 and lib.dd_fgm_workspace_bytes(3) == 3 * 96
    assert lib.dd_fgm_workspace_bytes(-1) == -1 and lib.dd_fgm_workspace_bytes((1 << 20) + 1) == -1


LOSS_ARGS = ("pred", "target", "heat", "grad", "loss", "ws", "ws_bytes", "views", "c", "hw", "dtype")


def loss_args(**kw):
    a = dict(pred=P, target=P, heat=P, grad=P, loss=P, ws=P, ws_bytes=4 * 33, views=6, c=4, hw=1400, dtype=0)
    a.update(kw)
    return tuple(a[k] for k in LOSS_ARGS) + (None,)


@pytest.mark.parametrize("bad", [dict(pred=None), dict(target=None), dict(loss=None), dict(ws=None), dict(views=0), dict(c=0),
                                 dict(hw=0), dict(dtype=3), dict(dtype=-1), dict(ws_bytes=4 * 33 - 1), dict(pred=17),
                                 dict(target=17), dict(grad=17), dict(pred=18, dtype=2), dict(heat=18), dict(loss=18),
                                 dict(ws=18)],
                         ids=lambda d: ",".join("%s=%s" % kv for kv in d.items()))
def test_loss_launcher_rejects_bad_arguments(lib, bad):
    assert lib.dd_fgm_loss(*loss_args(**bad)) == BAD_ARG


def test_loss_launcher_limits_and_workspace(lib):
    assert lib.dd_fgm_loss(*loss_args(views=1 << 31, c=1, hw=1, ws_bytes=1 << 20)) == UNSUPPORTED
    assert lib.dd_fgm_loss(*loss_args(views=1 << 16, c=1 << 8, hw=1 << 8, ws_bytes=1 << 20)) == UNSUPPORTED
    assert lib.dd_fgm_loss_workspace_bytes(0) == -1 and lib.dd_fgm_loss_workspace_bytes(1 << 31) == -1
    for count in (1, 1024, 1025, 33600, 1 << 20, (1 << 20) + 1, (1 << 31) - 1):
        assert lib.dd_fgm_loss_workspace_bytes(count) == 4 * R.loss_groups(count), count
    assert R.loss_groups(33600) == 33 and R.loss_groups(1 << 30) == 1024
    from dualdiff_amd import ops as O
    assert all(O.fgm_loss_groups(c) == R.loss_groups(c) for c in (1, 1024, 1025, 33600, 1 << 30))


def test_abi_has_the_entry_points(lib):
    import re
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dualdiff_hip.h")).read(), flags=re.S)
    for name in ("dd_fgm_mask", "dd_fgm_workspace_bytes", "dd_fgm_loss", "dd_fgm_loss_workspace_bytes"):
        assert name in _native.SIGNATURES and hasattr(lib, name)
        assert re.search(r"\b%s\s*\(" % name, hdr) is not None
    assert "fgm_mask.hip" in _build.SOURCES and "fgm_mask.hip" not in _build.EXTRA_FLAGS          # no fast-math
    assert lib.dd_abi_version() == 4


def test_from_config_covers_the_reference_sizes():
    from dualdiff_amd.pipeline import FgmMask
    want = {(224, 400): ((50, 28), None, (28, 50)), (192, 384): ((48, 27), (24, 48), (24, 48)),
            (432, 768): ((96, 54), None, (54, 96)), (256, 704): ((96, 54), (32, 88), (32, 88))}
    for size, (resolution, crop, out_shape) in want.items():
        fm = FgmMask.from_config({"dataset": {"image_size": list(size)}})
        assert (fm.resolution, fm.crop, fm.out_shape) == (resolution, crop, out_shape)
        assert fm.scale == (resolution[0] / 1600, resolution[1] / 900)
    with pytest.raises(ValueError, match=r"image_size \[272, 736\] has no FGM mask"):
        FgmMask.from_config({"dataset": {"image_size": [272, 736]}})
    with pytest.raises(ValueError, match="no dataset.image_size"):
        FgmMask.from_config({"dataset": {}})


def test_interface_errors():
    from dualdiff_amd.pipeline import FgmMask
    from dualdiff_amd.pipeline import fgm_mask as M
    with pytest.raises(ValueError, match="larger than the grid"):
        FgmMask((48, 27), crop=(28, 48))
    with pytest.raises(ValueError, match="odd number of columns"):
        FgmMask((48, 27), crop=(24, 47))
    with pytest.raises(ValueError, match="more than"):
        FgmMask((2048, 1024))
    with pytest.raises(ValueError, match="resolution must be"):
        FgmMask((50,))
    with pytest.raises(ValueError, match="positive"):
        FgmMask((50, 0))
    fm = FgmMask()
    assert (fm.resolution, fm.crop, fm.source_size, fm.out_shape) == ((50, 28), None, (1600, 900), (28, 50))
    l2i = torch.zeros((1, 2, 4, 4))
    with pytest.raises(RuntimeError, match="lidar2image must be on the device"):
        fm(torch.zeros((1, 2, 3, 8, 3)), torch.zeros((1, 2, 3), dtype=torch.bool), l2i)
    with pytest.raises(ValueError, match=r"lidar2image must be a \(b, n, 4, 4\) tensor"):
        fm(None, None, torch.zeros((2, 4, 4)))
    with pytest.raises(ValueError, match="masks .* go with bboxes"):
        fm(torch.zeros((1, 2, 3, 8, 3)), None, l2i)
    src = open(M.__file__).read()
    for lib_name in ("scipy", "matplotlib"):
        assert "import " + lib_name not in src and "from " + lib_name not in src
    with pytest.raises(ValueError, match="pred only"):
        M.fgm_loss(torch.zeros((1, 1, 1, 2, 2)), torch.zeros((1, 1, 1, 2, 2), requires_grad=True))


def test_ops_refuse_cpu_tensors_and_bad_shapes():
    from dualdiff_amd import ops as O
    if not os.path.exists(_build.lib_path()):
        pytest.skip("library not built")
    z = torch.zeros
    good = (z((1, 2, 3, 8, 3)), z((1, 2, 3), dtype=torch.bool), z((1, 2, 4, 4)))
    with pytest.raises(RuntimeError, match="GPU only"):
        O.fgm_mask(*good, (12, 9))
    with pytest.raises(ValueError, match="bboxes"):
        O.fgm_mask(z((1, 2, 3, 9, 3)), good[1], good[2], (12, 9))
    with pytest.raises(ValueError, match="masks"):
        O.fgm_mask(good[0], z((1, 2, 4), dtype=torch.bool), good[2], (12, 9))
    with pytest.raises(ValueError, match="lidar2image"):
        O.fgm_mask(good[0], good[1], z((1, 3, 4, 4)), (12, 9))
    with pytest.raises(ValueError, match="crop"):
        O.fgm_mask(*good, (12, 9), crop=(10, 12))
    with pytest.raises(ValueError, match="crop"):
        O.fgm_mask(*good, (12, 9), crop=(9, 11))
    with pytest.raises(RuntimeError, match="GPU only"):
        O.fgm_loss(z((1, 2, 4, 9, 12)), z((1, 2, 4, 9, 12)), z((1, 2, 9, 12)))
    with pytest.raises(TypeError, match="fp16 / bf16 / fp32"):
        O.fgm_loss(z((1, 2, 4, 9, 12), dtype=torch.float64), z((1, 2, 4, 9, 12), dtype=torch.float64))
    with pytest.raises(ValueError, match="one shape"):
        O.fgm_loss(z((1, 2, 4, 9, 12)), z((1, 2, 4, 9, 11)))
    with pytest.raises(ValueError, match="heat"):
        O.fgm_loss(z((1, 2, 4, 9, 12)), z((1, 2, 4, 9, 12)), z((1, 2, 9, 11)))


def test_loss_restatement_is_the_two_reference_lines():
    """tests/fgm_reference.loss against torch's own mse_loss / mean lines in float64"""
    g = torch.Generator().manual_seed(3)
    p, t = (torch.randn((2, 2, 4, 9, 12), generator=g, dtype=torch.float64) for _ in range(2))
    heat = torch.rand((2, 2, 9, 12), generator=g, dtype=torch.float64)
    p.requires_grad_(True)
    loss = torch.nn.functional.mse_loss(p, t, reduction="none")
    loss = loss.mean() + (loss * heat.unsqueeze(2)).mean()
    loss.backward()
    value, grad = R.loss(p.detach().numpy(), t.numpy(), heat.numpy())
    assert abs(value - float(loss.detach())) <= 1e-14 * abs(value)
    assert np.allclose(grad, p.grad.numpy(), rtol=1e-13, atol=0)
    plain, _ = R.loss(p.detach().numpy(), t.numpy(), None)
    assert abs(plain - float(torch.nn.functional.mse_loss(p.detach(), t))) <= 1e-14 * plain
