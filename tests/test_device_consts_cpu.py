"""The one rule for process-lifetime device constants built on the host (dualdiff_amd/_consts.py), on device "cpu": one
build per key, one key spelling, tuples stay tuples, nothing half-built is published — and the sites that use it (the
neighbour-view maps, the view-shard maps, the resample tables) return what they returned before."""
import os
import subprocess
import sys
import threading

import pytest
import torch

from dualdiff_amd._consts import _CONSTS, device_const

PAIR = {0: [5, 1], 1: [0, 2], 2: [1, 3], 3: [2, 4], 4: [3, 5], 5: [4, 0]}


def _counted(make):
    calls = []

    def build():
        calls.append(1)
        return make()
    return build, calls


def test_one_build_per_key_and_the_same_tensors():
    build, calls = _counted(lambda: torch.arange(5, dtype=torch.int32))
    a = device_const(("test_consts", "once"), "cpu", build)
    b = device_const(("test_consts", "once"), "cpu", build)
    assert a is b and len(calls) == 1 and a.tolist() == [0, 1, 2, 3, 4]


def test_string_and_device_are_one_entry():
    build, calls = _counted(lambda: torch.ones(3))
    a = device_const(("test_consts", "spelling"), "cpu", build)
    b = device_const(("test_consts", "spelling"), torch.device("cpu"), build)
    assert a is b and len(calls) == 1
    assert (("test_consts", "spelling"), "cpu", None) in _CONSTS


def test_tuple_stays_a_tuple():
    got = device_const(("test_consts", "tuple"), "cpu", lambda: (torch.zeros(2), torch.ones(3, dtype=torch.uint8)))
    assert isinstance(got, tuple) and len(got) == 2
    assert all(t.device.type == "cpu" for t in got) and got[0].tolist() == [0, 0] and got[1].tolist() == [1, 1, 1]
    assert device_const(("test_consts", "tuple"), "cpu", lambda: None) is got


BAD = {"list": lambda: [1, 2, 3], "none": lambda: None, "tuple-with-int": lambda: (torch.zeros(1), 7),
       "list-of-tensors": lambda: [torch.zeros(1)], "empty-tuple": lambda: ()}


@pytest.mark.parametrize("name", sorted(BAD))
def test_non_tensor_is_a_type_error_and_leaves_no_entry(name):
    key = ("test_consts", "bad", name)
    with pytest.raises(TypeError):
        device_const(key, "cpu", BAD[name])
    assert not any(k[0] == key for k in _CONSTS)
    assert device_const(key, "cpu", lambda: torch.zeros(1)).tolist() == [0]        # the key is still free


def test_eight_threads_one_build():
    build, calls = _counted(lambda: torch.full((4,), 7, dtype=torch.int32))
    barrier, got = threading.Barrier(8), [None] * 8

    def ask(i):
        barrier.wait()
        got[i] = device_const(("test_consts", "threads"), "cpu", build)
    threads = [threading.Thread(target=ask, args=(i,)) for i in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert len(calls) == 1 and all(g is got[0] for g in got) and got[0].tolist() == [7] * 4


def _block(pair):
    from dualdiff_amd.networks.blocks import BasicMultiviewTransformerBlock
    return BasicMultiviewTransformerBlock(64, 2, 32, cross_attention_dim=24, neighboring_view_pair=pair)


def test_blocks_with_the_same_pairs_share_their_maps():
    a, b = _block(PAIR), _block({str(k): list(v) for k, v in PAIR.items()})     # JSON spelling of the same pairs
    ma, mb = a.neighbour_maps(12, "cpu"), b.neighbour_maps(12, torch.device("cpu"))
    assert len(ma) == len(mb) == 2 and all(x is y for x, y in zip(ma, mb))
    left, right = ma
    assert left.dtype == right.dtype == torch.int32
    assert left.tolist() == [5, 0, 1, 2, 3, 4, 11, 6, 7, 8, 9, 10]             # test_neighbour_maps_follow_view_pairs
    assert right.tolist() == [1, 2, 3, 4, 5, 0, 7, 8, 9, 10, 11, 6]
    other = _block({0: [1, 5], 1: [2, 0], 2: [3, 1], 3: [4, 2], 4: [5, 3], 5: [0, 4]})
    mo = other.neighbour_maps(12, "cpu")
    assert mo[0] is not left and mo[0].tolist() == right.tolist() and mo[1].tolist() == left.tolist()
    assert a.neighbour_maps(6, "cpu")[0] is not left and a.neighbour_maps(6, "cpu")[0].tolist() == [5, 0, 1, 2, 3, 4]


def test_view_shard_maps_are_kept():
    from dualdiff_amd.parallel import ViewShard, ViewSplitPlan
    plan = ViewSplitPlan(3, 1, PAIR, cfg_split=False)
    shard = ViewShard(plan, exchange=lambda kv: kv)
    first, again = shard.maps(2, "cpu"), shard.maps(2, "cpu")
    assert all(x is y for x, y in zip(first, again))
    assert [m.tolist() for m in first] == plan.kv_maps(2) and all(m.dtype == torch.int32 for m in first)
    # keyed by what kv_maps depends on: an equal plan shares, another rank's plan does not
    assert ViewShard(ViewSplitPlan(3, 1, PAIR, cfg_split=False), exchange=lambda kv: kv).maps(2, "cpu")[0] is first[0]
    rank2 = ViewSplitPlan(3, 2, PAIR, cfg_split=False)
    assert [m.tolist() for m in ViewShard(rank2, exchange=lambda kv: kv).maps(2, "cpu")] == rank2.kv_maps(2)


def test_device_tables_on_cpu():
    from dualdiff_amd.pipeline.image_output import PRECISION_BITS, device_tables, resample_tables
    kk, bounds = device_tables(8, 5, "cpu")
    want_kk, want_bounds = resample_tables(8, 5)
    assert torch.equal(kk, want_kk) and torch.equal(bounds, want_bounds)
    assert kk.dtype == bounds.dtype == torch.int32 and kk.is_contiguous() and bounds.is_contiguous()
    kk, bounds = device_tables(5, 5, "cpu")                                    # the one-tap identity table
    assert kk.dtype == bounds.dtype == torch.int32
    assert kk.tolist() == [[1 << PRECISION_BITS]] * 5 and bounds.tolist() == [[i, 1] for i in range(5)]


def test_ops_does_not_import_the_pipeline():
    """The launch layer stands below the pipeline: the table builders it needs live in dualdiff_amd.image_tables."""
    code = ("import sys; import dualdiff_amd.ops; "
            "up = sorted(m for m in sys.modules if m.startswith('dualdiff_amd.pipeline')); assert not up, up")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], cwd=root, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
