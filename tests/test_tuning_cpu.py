"""dualdiff_amd.tuning without a library or a GPU: the table's file format, the key builders, and the path on which
`ops.CHALLENGE_TILES` reaches the tuner.

The keys are the contract between the code and the 1,376 tracked entries: a builder that spells a key differently
orphans every entry of that kind without any error (each shape then goes to the run-time tuner), so the tuples are pinned
here as literals."""
import ast
import json

import pytest
import torch

from dualdiff_amd import _native, ops, tuning
from dualdiff_amd._native import DD_BF16, DD_EPI_GEGLU, DD_F16


@pytest.fixture
def table():
    """An empty table that reads no tracked file; the process's own state comes back afterwards."""
    saved = (dict(tuning._TUNED), tuning._TABLE_LOADED, set(tuning._CHALLENGED))
    tuning.forget_tuned()
    tuning._CHALLENGED.clear()
    yield tuning._TUNED
    tuning._TUNED.clear()
    tuning._TUNED.update(saved[0])
    tuning._TABLE_LOADED = saved[1]
    tuning._CHALLENGED.clear()
    tuning._CHALLENGED.update(saved[2])


def write_table(path, rows, arch="gfx950"):
    path.write_text(json.dumps({"arch": arch, "entries": [[repr(k), list(v)] for k, v in rows]}))
    return str(path)


def test_tracked_table_round_trips_byte_for_byte(table, tmp_path):
    assert ops.load_tuned(ops.TUNE_TABLE_PATH) == 1376
    out = tmp_path / "sub" / "gfx950.json"
    ops.save_tuned(str(out))
    assert out.read_bytes() == open(ops.TUNE_TABLE_PATH, "rb").read()
    assert all(len(v) == 3 and v[2] == 0 for v in ops.tuned_table().values())


def test_two_value_legacy_rows_load_with_a_zero(table, tmp_path):
    k2, k3 = tuning.gemm_key(7, 64, 64, 0, DD_F16), tuning.conv_key(1, 4, 4, 64, 64, 1, 4, 4, DD_F16)
    assert ops.load_tuned(write_table(tmp_path / "t.json", [(k2, (30, 2)), (k3, (52, 1, 0))])) == 2
    assert ops.tuned_table() == {k2: (30, 2, 0), k3: (52, 1, 0)}


def test_merge_keeps_untouched_entries_of_the_file(table, tmp_path):
    theirs, ours = tuning.gemm_key(7, 64, 64, 0, DD_F16), tuning.gemm_key(9, 64, 64, 0, DD_BF16)
    path = write_table(tmp_path / "t.json", [(theirs, (30, 2)), (ours, (30, 1, 0))])
    table[ours] = (52, 4, 0)
    ops.save_tuned(path)                                  # merge=True is the default
    rows = {ast.literal_eval(k): tuple(v) for k, v in json.load(open(path))["entries"]}
    assert rows == {theirs: (30, 2, 0), ours: (52, 4, 0)}
    ops.save_tuned(path, merge=False)
    rows = {ast.literal_eval(k): tuple(v) for k, v in json.load(open(path))["entries"]}
    assert rows == {ours: (52, 4, 0)}


def test_load_keeps_entries_already_tuned_here(table, tmp_path):
    key = tuning.gemm_key(7, 64, 64, 0, DD_F16)
    table[key] = (52, 4, 0)
    assert ops.load_tuned(write_table(tmp_path / "t.json", [(key, (30, 2, 0))])) == 0
    assert ops.tuned_table()[key] == (52, 4, 0)


def test_table_of_another_arch_raises(table, tmp_path):
    with pytest.raises(RuntimeError, match="gfx950"):
        ops.load_tuned(write_table(tmp_path / "t.json", [], arch="gfx942"))
    assert ops.tuned_table() == {}


def test_forget_tuned_empties_and_stops_the_lazy_load(table):
    tuning._TABLE_LOADED = False
    tuning._load_default_table()
    assert len(ops.tuned_table()) == 1376                 # the lazy load reads the tracked file ...
    ops.forget_tuned()
    assert ops.tuned_table() == {}
    tuning._load_default_table()
    assert ops.tuned_table() == {}                        # ... and not again after forget_tuned()


def test_lazy_load_honours_dd_tune_table(table, tmp_path, monkeypatch):
    key = tuning.gemm_key(7, 64, 64, 0, DD_F16)
    monkeypatch.setenv("DD_TUNE_TABLE", write_table(tmp_path / "t.json", [(key, (30, 2, 0))]))
    tuning._TABLE_LOADED = False
    tuning._load_default_table()
    assert ops.tuned_table() == {key: (30, 2, 0)}
    tuning.forget_tuned()
    monkeypatch.setenv("DD_TUNE_TABLE", "0")
    tuning._TABLE_LOADED = False
    tuning._load_default_table()
    assert ops.tuned_table() == {}


def test_key_builders_spell_the_tracked_tuples():
    g = tuning.gemm_key
    assert g(2800, 320, 320, 0, DD_F16) == ("g", 2800, 320, 320, 0, 0, False, False)
    assert g(2800, 1280, 320, DD_EPI_GEGLU, DD_BF16, True, False) == ("g", 2800, 1280, 320, 1, 1, True, False)
    base = ("g", 96, 64, 512, 0, 1, False, False)
    assert g(96, 64, 512, 0, DD_BF16, out_f32=True) == base + ("f32",)
    assert g(96, 64, 512, 0, DD_BF16, stats_out=True) == base + ("so",)
    assert g(96, 64, 512, 0, DD_BF16, stats_in=True) == base + ("si",)
    assert g(96, 64, 512, 0, DD_BF16, head_major=40) == base + ("hm", 40)
    assert g(96, 64, 512, 0, DD_BF16, res=True) == base + ("res",)
    assert g(96, 64, 512, 0, DD_BF16, acc=True) == base + ("acc",)
    # every flag at once: the order is f32, so, si, hm, res, acc whatever the order of the arguments
    assert g(96, 64, 512, 0, DD_BF16, acc=True, res=True, head_major=80, stats_in=True, stats_out=True, out_f32=True) \
        == base + ("f32", "so", "si", "hm", 80, "res", "acc")
    # tests/test_tuned_table_gpu.py::test_rejected_call_is_not_cached
    assert g(64, 64, 512, 0, DD_BF16, False, True) == ("g", 64, 64, 512, 0, _native.DD_BF16, False, True)
    conv = (6, 28, 50, 320, 640, 2, 28, 50, DD_F16)
    assert tuning.conv_key(*conv) == ("c", 6, 28, 50, 320, 640, 2, 28, 50, 0)
    assert tuning.conv_pad0_key(*conv) == ("c", 6, 28, 50, 320, 640, 2, 28, 50, 0, "p0")


def gemm_fields(key):
    """The arguments of gemm_key a tracked "g" key was built from."""
    kw, flags, i = {}, key[8:], 0
    names = {"f32": "out_f32", "so": "stats_out", "si": "stats_in", "res": "res", "acc": "acc"}
    while i < len(flags):
        if flags[i] == "hm":
            i += 1
            kw["head_major"] = flags[i]
        else:
            kw[names[flags[i]]] = True
        i += 1
    return key[1:8], kw


def test_builders_reproduce_every_tracked_key():
    with open(ops.TUNE_TABLE_PATH) as f:
        keys = [ast.literal_eval(k) for k, _ in json.load(f)["entries"]]
    kinds = {"g": 0, "c": 0}
    for key in keys:
        kinds[key[0]] += 1
        if key[0] == "g":
            args, kw = gemm_fields(key)
            assert tuning.gemm_key(*args, **kw) == key
        elif key[-1] == "p0":
            assert tuning.conv_pad0_key(*key[1:-1]) == key
        else:
            assert tuning.conv_key(*key[1:]) == key
    assert kinds["g"] > 0 and kinds["c"] > 0 and sum(kinds.values()) == 1376


class FakeTimes:
    """Stands in for tuning._time_launch: ms per (tile, split) from a dict (None: the library turns the pair down)."""

    def __init__(self, ms):
        self.ms, self.calls = ms, []

    def __call__(self, L, d, device, warm, tile, split, iters):
        self.calls.append((tile, split, iters))
        d.tile, d.split_k = tile, split
        return self.ms.get((tile, split))


@pytest.fixture
def cpu_tuner(table, monkeypatch):
    """tune() on the host: no capture to ask about, the scratch output on the CPU, the timing faked."""
    monkeypatch.setattr(tuning, "_capturing", lambda: False)
    monkeypatch.setattr(tuning, "_AUTOTUNE", True)

    def install(ms):
        fake = FakeTimes(ms)
        monkeypatch.setattr(tuning, "_time_launch", fake)
        return fake
    return install


def desc(rows, n, k):
    d = _native.GemmDesc()
    d.rows, d.n, d.k, d.out, d.ldc, d.accumulate, d.tile, d.split_k, d.ws, d.ws_bytes = rows, n, k, 4096, n, 1, 7, 9, 8192, 16
    return d


def state(d):
    return (d.out, d.ldc, d.accumulate, d.tile, d.split_k, d.ws, d.ws_bytes)


def test_challenge_tiles_assigned_on_ops_reach_the_tuner(cpu_tuner, table, monkeypatch):
    """bench.py --challenge-tiles assigns ops.CHALLENGE_TILES after import; the tuner must time exactly those tiles
    against the incumbent, once per key."""
    key = tuning.gemm_key(96, 64, 512, 0, DD_BF16)
    table[key] = (30, 2, 0)
    L = tuning.launcher(None)
    d = desc(96, 64, 512)
    fake = cpu_tuner({(30, 2): 1.0, (52, 1): 0.99, (52, 2): 0.5, (61, 1): None, (61, 2): 2.0})
    assert ops.CHALLENGE_TILES == ()                       # (DD_TUNE_CHALLENGE is not set in a test session)
    ops._tune(L, d, key, (96, 64), torch.bfloat16, torch.device("cpu"), ())
    assert fake.calls == [] and (d.tile, d.split_k) == (30, 2)
    monkeypatch.setattr(ops, "CHALLENGE_TILES", (52, 61))
    d = desc(96, 64, 512)
    before = state(d)
    ops._tune(L, d, key, (96, 64), torch.bfloat16, torch.device("cpu"), ())
    # incumbent 21 samples; a challenger gets 5, and 21 more only within 10 % of the best; (61, 1) does not launch
    assert fake.calls == [(30, 2, 21), (52, 1, 5), (52, 1, 21), (52, 2, 5), (52, 2, 21), (61, 1, 5), (61, 2, 5)]
    assert (d.tile, d.split_k) == (52, 2) and ops.tuned_table()[key] == (52, 2, 0)      # 0.99 is no 3 % win, 0.5 is
    assert state(d)[:3] == before[:3] and state(d)[5:] == before[5:]
    del fake.calls[:]
    ops._tune(L, d, key, (96, 64), torch.bfloat16, torch.device("cpu"), ())
    assert fake.calls == []                                # challenged once


def test_sweep_caches_the_fastest_and_restores_the_descriptor(cpu_tuner, table, monkeypatch):
    key = tuning.gemm_key(96, 64, 512, 0, DD_BF16)
    monkeypatch.setattr(tuning, "_TILES", (30, 52))
    d = desc(96, 64, 512)
    before = state(d)
    cands = tuning.tune_candidates(None, d)
    assert cands == [(30, 1), (30, 2), (52, 1), (52, 2)]   # k / 64 = 8 K-steps: split 2 keeps 4 per slab, 3 does not
    fake = cpu_tuner({(30, 1): 3.0, (30, 2): 2.0, (52, 1): None, (52, 2): 2.5})
    assert tuning.tune(tuning.launcher(None), d, key, (96, 64), torch.bfloat16, torch.device("cpu")) == (30, 2, 0)
    assert state(d) == before and ops.tuned_table() == {key: (30, 2, 0)}
    assert [c[:2] for c in fake.calls[:4]] == cands and len(fake.calls) == 4 + 3
    del fake.calls[:]
    assert tuning.tune(tuning.launcher(None), d, key, (96, 64), torch.bfloat16, torch.device("cpu")) == (30, 2, 0)
    assert fake.calls == []


def test_a_call_no_candidate_launches_is_not_cached(cpu_tuner, table, monkeypatch):
    monkeypatch.setattr(tuning, "_TILES", (30,))
    cpu_tuner({})
    key = tuning.gemm_key(64, 64, 512, 0, DD_BF16, False, True)
    d = desc(64, 64, 512)
    assert tuning.tune(tuning.launcher(None), d, key, (64, 64), torch.bfloat16, torch.device("cpu")) == (0, 0, 0)
    assert ops.tuned_table() == {}


def test_autotune_off_takes_the_library_plan(cpu_tuner, table, monkeypatch):
    fake = cpu_tuner({(30, 1): 1.0})
    monkeypatch.setattr(tuning, "_AUTOTUNE", False)
    d = desc(96, 64, 512)
    assert tuning.tune(tuning.launcher(None), d, ("g", 1), (96, 64), torch.bfloat16, torch.device("cpu")) == (0, 0, 0)
    assert fake.calls == [] and ops.tuned_table() == {}
