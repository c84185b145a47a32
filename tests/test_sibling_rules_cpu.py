"""What the sibling-overlap tests (tests/test_sibling_overlap_gpu.py) rest on and that needs no GPU:
the committed seed of the interleaving test really exercises the overlap, and the table of raw-pointer writers
(tests/sibling_cases.py: RAW_WRITERS) names every public wrapper of dualdiff_amd/ops.py that writes a tensor of its
caller's — a wrapper added later without a row fails here, and its row is held to a version count on the GPU."""
import ast
import collections
import os

from tests import sibling_cases as C

OPS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dualdiff_amd", "ops.py")


def test_the_committed_sequences_exercise_the_overlap():
    seqs = C.sequences()
    assert len(seqs) == C.SEQS == 40 and all(len(s) == C.LENGTH == 8 for s in seqs)
    assert seqs == C.sequences() and seqs != C.sequences(C.SEED + 1)          # seeded
    seen = collections.Counter(a for s in seqs for a in s)
    assert set(seen) == set(C.ACTIONS) and min(seen.values()) >= C.MIN_PER_ACTION == 10, seen
    calls = [r for row in C.predict(seqs) for r in row if r is not None]
    b = [overlapped for model, overlapped in calls if model == "B"]
    assert len(b) == seen["call_B"] + seen["call_B_other_stream"]
    assert sum(b) >= C.MIN_OVERLAPPED_SHARE * len(b) and C.MIN_OVERLAPPED_SHARE == 0.25, (sum(b), len(b))
    # the refusals are exercised too: a sharing pair, a call on another stream, and calls of every model on both sides
    assert {(m, o) for m, o in calls} == {(m, o) for m in "ABS" for o in (False, True)}


def test_the_rule_refuses_what_it_must():
    r = C.Rule()
    three = lambda m: [r.call(m) for _ in range(3)]
    assert three("A") == [False] * 3                     # the same model twice in a row
    assert [r.call("B"), r.call("A"), r.call("B"), r.call("A"), r.call("B")] == [False, True, False, True, True]
    assert r.call("S") is False and r.call("A") is False # S's first sight; A shares a sub-module with S
    assert r.call("B") is True
    r.write_x()
    assert r.call("A") is False and r.call("B") is True  # written since B's entry; A's entry has the new version
    r.new_x()
    assert r.call("A") is False
    r.invalidate("B")
    assert r.call("A") is False and [r.call("B"), r.call("A"), r.call("B"), r.call("A"), r.call("B")] == \
        [False, True, False, True, True]
    assert r.call("A", "other") is False and r.call("B") is False and r.call("A") is True


def _public_functions():
    tree = ast.parse(open(OPS).read())
    return {f.name: [a.arg for a in f.args.posonlyargs + f.args.args + f.args.kwonlyargs]
            for f in tree.body if isinstance(f, ast.FunctionDef) and not f.name.startswith("_")}


def test_every_raw_writer_of_ops_has_a_row():
    funcs = _public_functions()
    assert len(funcs) > 60                               # the walk found the module
    assert set(C.IN_PLACE) <= set(funcs)
    for name, args in C.IN_PLACE.items():
        assert set(args) <= set(funcs[name]), name
    want = {}
    for name, params in funcs.items():
        written = tuple(p for p in params if p in C.WRITER_PARAMS) + tuple(C.IN_PLACE.get(name, ()))
        if written:
            want[name] = written
    missing = sorted(set(want) - set(C.RAW_WRITERS))
    assert not missing, "wrappers of ops.py that write a caller's tensor and have no row in RAW_WRITERS: %s" % missing
    assert not sorted(set(C.RAW_WRITERS) - set(want)), "rows that name no writer of ops.py"
    for name, written in want.items():
        row = C.RAW_WRITERS[name]
        assert sorted(row["writes"]) == sorted(written), (name, row["writes"], written)
        assert callable(row["make"])
