"""Map output without a GPU: the numpy restatement (tests/map_output_reference.py) against the reference's own pictures
(tests/golden/map_output.npz, minted from `visualize_map`), our tables against the reference's, the planted faults the
fixture has to catch, the host side of `MapRender` and the validation codes of the two launchers.  Everything is bytes:
every comparison is equality."""
import functools
import os
import types

import numpy as np
import pytest

from dualdiff_amd import _build, _native
from dualdiff_amd import pipeline as P
from dualdiff_amd.pipeline import map_output as MO
from tests import map_output_reference as R
from tests import pil_resample_reference as PR
from tests.golden import mint_map_output as M

BAD_ARG, UNSUPPORTED = -1, -2
PTR = 16                                                 # non-null, 16-byte aligned, never dereferenced


@functools.lru_cache(maxsize=None)
def fixture():
    z = M.load()
    return z, M.colors(z), M.priority(z)


@functools.lru_cache(maxsize=None)
def restated(name, fault=None, swap=None):
    """(frame, used, whole picture with the fixture's legend) of a case: computed once, shared, never written to."""
    z, colors, priority = fixture()
    _, target, _, mc, oc = M.CASES[name]
    frame, used = R.render(M.inputs(name), mc, oc, colors, priority, target, fault=fault, swap=swap)
    whole = R.compose(frame, z["legend_" + name], fault=fault)
    frame.setflags(write=False)
    whole.setflags(write=False)
    return frame, frozenset(used), whole


def same(a, b):
    return a.shape == b.shape and np.array_equal(a, b)


@pytest.mark.parametrize("name", sorted(M.CASES))
def test_restatement_equals_the_reference(name):
    z, _, _ = fixture()
    s, target, c, _, _ = M.CASES[name]
    m = M.inputs(name)
    assert np.array_equal(np.unpackbits(z["in_" + name])[:m.size].reshape(m.shape), m)
    frame, used, whole = restated(name)
    t = R.target_side(s, target)
    assert frame.shape == (t, t, 3)
    assert same(whole, z["out_" + name])
    assert used == M.used(z, name)


def test_fixture_covers_what_the_issue_lists():
    z, _, _ = fixture()
    assert {(v[0], v[1]) for v in M.CASES.values()} == {(12, 40), (20, 50), (200, 400)}
    assert {v[2] for v in M.CASES.values()} >= {8, 12, 18, 26}
    assert M.used(z, "empty") == {"car"}                               # argmax of an empty map is the first object class
    assert "car" in M.used(z, "few_dynamic") and not M.inputs("few_dynamic")[8].any()
    assert M.used(z, "pairs") == set(M.MAP_CLASSES)                    # C <= ns: no dynamic part at all
    assert os.path.getsize(M.PATH) < 300 * 1000


def test_our_tables_are_the_references():
    _, colors, priority = fixture()
    assert list(MO.COLORS.items()) == list(colors.items())             # the order too: the legend's patches follow it
    assert list(MO.STATIC_PRIORITY) == priority
    assert [priority.index(n) for n in M.BY_PRIORITY] == sorted(priority.index(n) for n in M.MAP_CLASSES)
    r = MO.MapRender(M.MAP_CLASSES, M.OBJECT_CLASSES)
    st, dt = r.static_table(), r.dynamic_table()
    assert st.shape == (9, 4) and dt.shape == (10, 4) and st.dtype == dt.dtype == np.float32
    assert np.array_equal(PR.quantize(st[:, :3]), np.array([colors[n] for n in M.MAP_CLASSES + ("nothing",)], dtype=np.uint8))
    assert np.array_equal(PR.quantize(dt[:, :3]), np.array([colors[n] for n in M.OBJECT_CLASSES], dtype=np.uint8))
    assert st[:8, 3].tolist() == [priority.index(n) for n in M.MAP_CLASSES]
    assert r.static_table(3).shape == (4, 4) and r.dynamic_table(4).shape == (4, 4)


def test_quantiser_identity_on_the_host():
    """float32(c) / 255 goes back to c through `(x * 255).round()` for every byte: the float route to the resize."""
    c = np.arange(256, dtype=np.float32)
    assert np.array_equal(PR.quantize(c / np.float32(255)), np.arange(256, dtype=np.uint8))


@pytest.mark.parametrize("name", sorted(M.CASES))
def test_used_words_name_the_references_class_sets(name):
    z, _, _ = fixture()
    _, target, _, mc, oc = M.CASES[name]
    r = MO.MapRender(mc, oc, target_size=target)
    word = R.used_word(restated(name)[1], mc, oc)
    assert r.names(word) == M.used(z, name)
    assert r.names(word | 1 << 31) == M.used(z, name)
    assert r.names(0) == set()


def test_default_legend_reproduces_the_references():
    z, _, _ = fixture()
    matplotlib = pytest.importorskip("matplotlib")
    pytest.importorskip("PIL")
    if matplotlib.__version__ != str(z["matplotlib_version"]):
        pytest.skip("matplotlib %s installed, fixture minted with %s: the legend's pixels belong to matplotlib"
                    % (matplotlib.__version__, z["matplotlib_version"]))
    matplotlib.use("Agg")
    for name in ("empty", "aux", "mixed", "full"):
        got = MO.matplotlib_legend(M.used(z, name), M.CASES[name][1])
        assert same(got, z["legend_" + name]), name


def test_exported_and_from_config():
    assert P.MapRender is MO.MapRender and P.map_output is MO
    ds = {"map_classes": list(M.MAP_CLASSES), "object_classes": list(M.OBJECT_CLASSES)}
    for cfg in ({"dataset": ds}, types.SimpleNamespace(dataset=types.SimpleNamespace(**ds))):
        r = MO.MapRender.from_config(cfg, target_size=50)
        assert (r.map_classes, r.object_classes, r.target_size) == (M.MAP_CLASSES, M.OBJECT_CLASSES, 50)
        assert (r.ns, r.nd) == (8, 10)
    r = MO.MapRender.from_config({"dataset": {"map_classes": None, "object_classes": ["car"]}})
    assert (r.ns, r.nd, r.target_size) == (0, 1, 400)
    with pytest.raises(ValueError, match="dataset"):
        MO.MapRender.from_config({})
    assert [MO.MapRender(M.MAP_CLASSES, M.OBJECT_CLASSES).layers(c) for c in (3, 8, 12, 18, 26)] == \
        [(3, 0), (8, 0), (8, 4), (8, 10), (8, 10)]


def test_target_side_is_the_references_expression():
    for s, target in ((12, 40), (20, 50), (200, 400), (7, 400), (49, 100), (3, 400), (200, 399), (13, 41), (400, 400), (97, 50), (77, 40)):
        ratio = max(target / s, target / s)
        assert MO.target_side(s, target) == R.target_side(s, target) == int(s * ratio)
    assert MO.target_side(97, 50) == 49 and MO.target_side(77, 40) == 39          # s * (target / s) < target in float


def test_refusals_by_name():
    with pytest.raises(ValueError, match="'lane'.*STATIC_PRIORITY"):
        MO.MapRender(["drivable_area", "lane"], None)
    with pytest.raises(ValueError, match="'road_segment'.*STATIC_PRIORITY"):
        MO.MapRender(["road_segment"], ["car"])
    with pytest.raises(ValueError, match="'divider'.*COLORS"):
        MO.MapRender(["divider"], None)
    with pytest.raises(ValueError, match="'tram'.*COLORS"):
        MO.MapRender(None, ["car", "tram"])
    with pytest.raises(ValueError, match="map_classes holds a None"):
        MO.MapRender(["drivable_area", None], ["car"])
    with pytest.raises(ValueError, match="object_classes holds a None"):
        MO.MapRender(["drivable_area"], [None])
    with pytest.raises(ValueError, match="both None"):
        MO.MapRender(None, None)
    with pytest.raises(ValueError, match="both None"):
        MO.MapRender([], None)
    with pytest.raises(ValueError, match="at most 31 layers"):
        MO.MapRender(M.MAP_CLASSES, M.OBJECT_CLASSES * 3)
    with pytest.raises(ValueError, match="target_size"):
        MO.MapRender(M.MAP_CLASSES, None, target_size=0)
    import torch
    r = MO.MapRender(M.MAP_CLASSES, M.OBJECT_CLASSES)
    with pytest.raises(ValueError, match="non-square"):
        r.render(torch.zeros(1, 18, 12, 20, dtype=torch.uint8))
    with pytest.raises(ValueError, match="non-square"):
        r(torch.zeros(1, 18, 12, 20))
    with pytest.raises(ValueError, match=r"\(b, C, S, S\)"):
        r.render(torch.zeros(18, 12, 12))
    with pytest.raises(ValueError, match="bool, uint8"):
        r.render(torch.zeros(1, 18, 12, 12, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="GPU only"):
        r.render(torch.zeros(1, 18, 12, 12, dtype=torch.uint8))


def test_default_legend_names_matplotlib_when_it_is_missing(monkeypatch):
    import builtins
    real = builtins.__import__

    def no_matplotlib(name, *a, **kw):
        if name.split(".")[0] == "matplotlib":
            raise ImportError("No module named 'matplotlib'")
        return real(name, *a, **kw)
    monkeypatch.setattr(builtins, "__import__", no_matplotlib)
    with pytest.raises(ImportError, match="needs matplotlib"):
        MO.matplotlib_legend({"car"}, 40)


# ---- planted faults: each must change at least one fixture case ---------------------------------------------------

def changed(fault, swap=None):
    """The cases whose whole picture or class set the fault changes."""
    hit = []
    for n in sorted(M.CASES):
        bad, good = restated(n, fault, swap), restated(n)
        if not same(bad[2], good[2]) or bad[1] != good[1]:
            hit.append(n)
    return hit


@pytest.mark.parametrize("pair", list(zip(M.BY_PRIORITY[:-1], M.BY_PRIORITY[1:])))
def test_fixture_catches_swapped_neighbouring_priorities(pair):
    assert "pairs" in changed("swap_priorities", pair)


@pytest.mark.parametrize("fault", [f for f in R.FAULTS if f != "swap_priorities"])
def test_fixture_catches_planted_fault(fault):
    hit = changed(fault)
    assert hit, fault
    if fault == "dynamic_used_from_set_pixels":
        assert {"empty", "few_dynamic", "mixed"} <= set(hit)
    if fault in ("last_dynamic", "static_over_dynamic"):
        assert {"few_dynamic", "mixed"} <= set(hit)


def test_turn_before_resize_differs_at_full_size():
    """The order matters at 200 -> 400 too: PIL's horizontal pass rounds to a byte before the vertical one."""
    assert not same(restated("full", "turn_before_resize")[0], restated("full")[0])


# ---- the launchers' validation, without a GPU ------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_build.lib_path()):
        pytest.skip("library not built (run __graft_entry__.build())")
    return _native.load(build_if_missing=False)


def render_args(**kw):
    a = dict(maps=PTR, stab=PTR, dtab=PTR, img=PTR, used=PTR, b=2, c=18, s=12, ns=8, nd=10)
    a.update(kw)
    return tuple(a[k] for k in ("maps", "stab", "dtab", "img", "used", "b", "c", "s", "ns", "nd")) + (None,)


def compose_args(**kw):
    a = dict(src=PTR, index=PTR, legend=PTR, out=PTR, m=4, g=2, t=40, lh=4, lw=40, side=1)
    a.update(kw)
    return tuple(a[k] for k in ("src", "index", "legend", "out", "m", "g", "t", "lh", "lw", "side")) + (None,)


RENDER_BAD = [dict(maps=None), dict(stab=None), dict(img=None), dict(used=None), dict(dtab=None), dict(b=0), dict(c=0),
              dict(s=0), dict(s=-12), dict(ns=-1), dict(nd=-1), dict(ns=0, nd=0), dict(c=17), dict(ns=9), dict(stab=18),
              dict(dtab=17), dict(img=2), dict(used=20 + 1)]
RENDER_UNSUPPORTED = [dict(c=40, ns=16, nd=16), dict(c=32, ns=0, nd=32), dict(s=1 << 14), dict(b=65536)]
COMPOSE_BAD = [dict(src=None), dict(out=None), dict(m=0), dict(g=0), dict(t=0), dict(lh=-1), dict(lw=-1), dict(side=2),
               dict(side=-1), dict(legend=None), dict(lh=0), dict(lw=0), dict(lh=0, lw=0), dict(index=None),
               dict(index=18), dict(lw=41), dict(side=0, lh=41, lw=4)]
COMPOSE_UNSUPPORTED = [dict(t=1 << 14), dict(t=1 << 14, lw=1 << 14), dict(m=65536), dict(g=65536),
                       dict(side=0, lh=40, lw=1 << 14)]


def test_launchers_validate_before_any_launch(lib):
    """DD_ERR_LAUNCH (-3) on a machine without a GPU would mean that a check came after a runtime call."""
    for kw in RENDER_BAD:
        assert lib.dd_map_render_u8(*render_args(**kw)) == BAD_ARG, kw
    for kw in RENDER_UNSUPPORTED:
        assert lib.dd_map_render_u8(*render_args(**kw)) == UNSUPPORTED, kw
    for kw in COMPOSE_BAD:
        assert lib.dd_map_compose_u8(*compose_args(**kw)) == BAD_ARG, kw
    for kw in COMPOSE_UNSUPPORTED:
        assert lib.dd_map_compose_u8(*compose_args(**kw)) == UNSUPPORTED, kw
