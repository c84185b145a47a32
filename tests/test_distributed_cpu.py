"""world_size-2 gloo test of the scene sharding used by bench.py --gpus N (no data-path collective;
only bookkeeping collectives: max-over-ranks time, result gather)."""
import os
import socket

import pytest

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from dualdiff_amd.parallel import gather_scenes, max_over_ranks, shard_scenes


def test_shard_scenes_partition():
    for n in (1, 2, 5, 8, 13):
        for world in (1, 2, 4, 8):
            cover = []
            for r in range(world):
                lo, hi = shard_scenes(n, r, world)
                assert 0 <= lo <= hi <= n and hi - lo in (n // world, n // world + 1)
                cover += list(range(lo, hi))
            assert cover == list(range(n))


def _worker(rank, world, port, n_scenes, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    lo, hi = shard_scenes(n_scenes, rank, world)
    # stand-in for "denoise my scenes": every scene's latents are a function of its global index only
    local = torch.stack([torch.full((6, 4, 2, 3), float(i)) for i in range(lo, hi)]) if hi > lo \
        else torch.zeros((0, 6, 4, 2, 3))
    full = gather_scenes(local, n_scenes)
    t = max_over_ranks(1.0 + rank)
    if rank == 0:
        out.put((full[:, 0, 0, 0, 0].tolist(), t))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_gloo_gather_and_timing():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    n_scenes = 5                                         # ragged: ranks get 3 and 2 scenes
    procs = [ctx.Process(target=_worker, args=(r, 2, port, n_scenes, q)) for r in range(2)]
    for p in procs:
        p.start()
    vals, t = q.get(timeout=120)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert vals == [0.0, 1.0, 2.0, 3.0, 4.0]
    assert t == 2.0                                      # slowest rank


def _cfg_worker(rank, world, port, out):
    from dualdiff_amd.parallel import cfg_all_gather, cfg_pair_groups
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    groups = cfg_pair_groups(world)
    mine = groups[rank // 2]
    # stand-in for "noise prediction of my CFG half": value = 10 * scene + half
    eps_half = torch.full((6, 4, 2, 3), 10.0 * (rank // 2) + (rank % 2))
    eps2 = cfg_all_gather(eps_half, mine)
    # classifier-free guidance on the gathered halves (pipeline_bev_controlnet.py:487-490)
    guided = eps2[0] + 2.0 * (eps2[1] - eps2[0])
    out.put((rank, tuple(eps2.shape), eps2[0, 0, 0, 0, 0].item(), eps2[1, 0, 0, 0, 0].item(), guided[0, 0, 0, 0].item()))
    dist.barrier()
    dist.destroy_process_group()


def test_cfg_split_exchange_gloo():
    """CFG split over rank pairs: 4 ranks = 2 scenes x {uncond, cond}; every rank of a pair
    must see [uncond, cond] in that order and compute the same guided prediction."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    world = 4
    procs = [ctx.Process(target=_cfg_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = sorted(q.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, shape, u, c, g in got:
        scene = rank // 2
        assert shape == (2, 6, 4, 2, 3)
        assert (u, c) == (10.0 * scene, 10.0 * scene + 1.0)
        assert g == u + 2.0 * (c - u)


# ------------------------------------------------------------------------- view split ----
PAIR = {0: [5, 1], 1: [0, 2], 2: [1, 3], 3: [2, 4], 4: [3, 5], 5: [4, 0]}


def _attn_ref(q, k, v):
    """(heads, l, d) x (heads, lk, d): plain softmax attention, one instance at a time (so that sharded and
    unsharded runs execute identical arithmetic per instance -> bit-for-bit comparable)."""
    s = (q @ k.transpose(-1, -2)) * (q.shape[-1] ** -0.5)
    return s.softmax(dim=-1) @ v


def _full_case(nb, heads=2, l=5, d=8, n_cam=6):
    g = torch.Generator().manual_seed(123)
    q = torch.randn((nb, n_cam, heads, l, d), generator=g)
    kv = torch.randn((n_cam, nb, 2 * heads, l, d), generator=g)       # slot-major like the block's buffer
    out = torch.zeros((nb, n_cam, heads, l, d))
    for bi in range(nb):
        for v in range(n_cam):
            for u in PAIR[v]:                                          # blocks.py:203-217: sum over the neighbours
                out[bi, v] += _attn_ref(q[bi, v], kv[u, bi, :heads], kv[u, bi, heads:])
    return q, kv, out


def _view_worker(rank, world, port, cfg_split, out):
    import os
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    from dualdiff_amd.parallel import HaloExchange, ViewShard, ViewSplitPlan, view_split_groups
    dist.init_process_group("gloo", rank=rank, world_size=world)
    halves, pairs = view_split_groups(world, cfg_split)
    plan = ViewSplitPlan(world, rank, PAIR, cfg_split=cfg_split)
    group = halves[plan.half or 0]
    shard = ViewShard(plan, HaloExchange(plan, group))
    heads = 2
    nb_full = 2                                   # two CFG halves of one scene
    q, kv_full, ref = _full_case(nb_full, heads=heads)
    # this rank's CFG halves: one (cfg_split) or both
    bis = [plan.half] if cfg_split else list(range(nb_full))
    nb, nloc = len(bis), len(plan.local)
    kv = torch.full((plan.n_slots, nb) + tuple(kv_full.shape[2:]), float("nan"))
    for si, v in enumerate(plan.local):
        kv[si] = kv_full[v][bis]
    shard.exchange(kv)
    ok_kv = all(torch.equal(kv[plan.slot(v)], kv_full[v][bis]) for v in plan.remote) and not torch.isnan(kv).any()
    maps = shard.maps(nb, "cpu")
    flat = kv.reshape(plan.n_slots * nb, *kv.shape[2:])
    ok_out = True
    for i in range(nb * nloc):                    # instance (bi, vi) = i // nloc, i % nloc
        bi, vi = i // nloc, i % nloc
        acc = torch.zeros_like(ref[0, 0])
        for mp in maps:
            src = flat[int(mp[i])]
            acc += _attn_ref(q[bis[bi], plan.local[vi]], src[:heads], src[heads:])
        ok_out = ok_out and torch.equal(acc, ref[bis[bi], plan.local[vi]])
    out.put((rank, plan.half, plan.local, bool(ok_kv), bool(ok_out)))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,cfg_split", [(2, False), (3, False), (4, True), (6, False)])
def test_view_split_halo_exchange_gloo(world, cfg_split):
    """Views of a scene sharded over `world` ranks: after the point-to-point K/V halo exchange every rank's
    buffer holds exactly the neighbour views' K/V (bit for bit), and the neighbour-view attention computed
    from it equals the single-process result bit for bit — world 2 / 3 / 6 (both CFG halves per rank) and
    4 (CFG halves x 2 view shards, exchange inside the half groups)."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_view_worker, args=(r, world, port, cfg_split, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = sorted(q.get(timeout=180) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    covered = {}
    for rank, half, local, ok_kv, ok_out in got:
        assert ok_kv and ok_out, (rank, half, local, ok_kv, ok_out)
        covered.setdefault(half, []).extend(local)
    for half, views in covered.items():
        assert sorted(views) == list(range(6)), (half, views)


def test_view_split_plan_properties():
    """Every layout: each view owned once per half group, send / recv lists mirror each other, the 8-GPU
    layout is the SURVEY's 4 x 2 + 4 x 1 instances."""
    from dualdiff_amd.parallel import ViewSplitPlan
    for world in (1, 2, 3, 4, 5, 6, 8, 12):
        plans = [ViewSplitPlan(world, r, PAIR) for r in range(world)]
        for p in plans:
            for s, views in p.send.items():
                peer = plans[p.rank_of(s)]
                assert peer.recv[p.shard] == views and (peer.half == p.half)
            for v in p.remote:
                assert v not in p.local and any(v in PAIR[u] for u in p.local)
            for j, mp_ in enumerate(p.kv_maps(1)):
                for vi, slot in enumerate(mp_):
                    want = PAIR[p.local[vi]][j]
                    assert (p.local + p.remote)[slot] == want
    p8 = [ViewSplitPlan(8, r, PAIR) for r in range(8)]
    assert sorted(len(p.local) for p in p8) == [1, 1, 1, 1, 2, 2, 2, 2]
    assert p8[0].message_bytes(1400, 320) == (2 * 2 * 1400 * 320 * 2, 2 * 2 * 1400 * 320 * 2)


def _bench_line(argv, env=None, timeout=600):
    """Runs bench.py as the driver does (`python bench.py --gpus N ...`, NO torchrun environment) and returns the
    one JSON line rank 0 printed."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    e = {k: v for k, v in os.environ.items()
         if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    e.update(env or {})
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py")] + argv, capture_output=True, text=True,
                       timeout=timeout, env=e, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.parametrize("n", [1, 2, 3])
def test_bench_gpus_flag_self_launches_n_ranks(n):
    """VERDICT r2 missing #1: `python bench.py --gpus N` without a torchrun environment must start N ranks itself
    (reference tools/downstream_v3_batched.py:287 self-spawns) and report n_gpus == N.  `--plumbing-check` swaps the
    measured path for the rendezvous + barrier + max-over-ranks bookkeeping only (gloo, no GPU)."""
    out = _bench_line(["--gpus", str(n), "--plumbing-check"])
    assert out["n_gpus"] == n and out["requested_gpus"] == n
    assert out["plumbing_check"] is True and out["value"] is None
    assert out["slowest_rank_seconds"] == float(n)          # max over ranks of (1 + rank)
    # for N > 1 the line shows that the collective backend saw N ranks (all-reduce of the rank ids);
    # item 6: it lists the DD_* switches of the process
    if n > 1:
        assert out["collective"] == {"backend": "gloo", "world_size": n, "rank_sum": n * (n - 1) // 2, "rank_sum_check": True}
    else:
        assert "collective" not in out
    assert out["env"] == []


def test_bench_lists_dd_switches_and_refuses_an_alternative_library():
    """DD_* environment switches change what a run measures, so the line lists them; DD_HIP_LIB (another
    build of the C-ABI library) is refused outright unless --allow-alt-lib says the A/B is intended."""
    import subprocess
    import sys
    out = _bench_line(["--gpus", "1", "--plumbing-check"], env={"DD_PERSIST": "0", "DD_FUSED_TOKENS": "1"})
    assert out["env"] == ["DD_FUSED_TOKENS=1", "DD_PERSIST=0"]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    e = dict(os.environ, DD_HIP_LIB="/tmp/some_other_lib.so")
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--plumbing-check"],
                       capture_output=True, text=True, timeout=300, env=e, cwd=root)
    assert r.returncode != 0 and "--allow-alt-lib" in r.stderr and not any(ln.startswith("{") for ln in r.stdout.splitlines())
    ok = _bench_line(["--gpus", "1", "--plumbing-check", "--allow-alt-lib"], env={"DD_HIP_LIB": "/tmp/some_other_lib.so"})
    assert ok["env"] == ["DD_HIP_LIB=/tmp/some_other_lib.so"]


def test_bench_strong_scaling_leg_is_a_child_job_in_the_same_line():
    """with N > 1 the line also says what ONE scene over all N GPUs does (`strong_scaling`, the
    view-split mode north_star's ">= 6x at 8 GPUs" is about) — measured by a fresh CHILD job after the weak-scaling
    ranks have left their group, so that a crash or hang there cannot touch `value`.  Plumbing form: gloo, no GPU."""
    out = _bench_line(["--gpus", "2", "--plumbing-check", "--full"], timeout=600)
    ss = out["strong_scaling"]
    assert out["n_gpus"] == 2 and ss["mode"] == "view-split" and ss["plumbing_check"] is True and ss["n_gpus"] == 2
    assert "error" not in ss
    off = _bench_line(["--gpus", "2", "--plumbing-check", "--full", "--strong-leg", "off"])
    assert "strong_scaling" not in off
    plain = _bench_line(["--gpus", "2", "--plumbing-check"])          # the leg is not part of a plain run
    assert plain["n_gpus"] == 2 and "strong_scaling" not in plain


def test_bench_strong_scaling_leg_timeout_is_reported_not_hung():
    """A strong-scaling child that overruns its budget is killed (its own process group only) and reported as an error
    object; the parent's line — the weak-scaling result — is still printed, once."""
    import time
    t0 = time.time()
    out = _bench_line(["--gpus", "2", "--plumbing-check", "--full", "--strong-timeout", "20"],
                      env={"DD_PLUMBING_SLEEP": "12"}, timeout=600)
    # the parent's own ranks sleep 12 s (inside the budget of the test), the child would need 12 s more plus start-up
    assert out["n_gpus"] == 2 and out["plumbing_check"] is True
    assert "strong_scaling" in out
    ss = out["strong_scaling"]
    assert ss["mode"] == "view-split" and ("error" in ss or ss.get("plumbing_check") is True)
    assert time.time() - t0 < 300


def test_bench_gpus_flag_mismatch_is_an_error():
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    e = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "3", "--plumbing-check"],
                       capture_output=True, text=True, env=e, timeout=300)
    assert r.returncode != 0 and "--gpus 3" in (r.stderr + r.stdout)


# ---------------------------------------------------------------- frame split (extension) ----
def _frame_worker(rank, world, port, n_frames, out):
    import os
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    from dualdiff_amd.parallel import FrameExchange, FrameShard, FrameSplitPlan
    dist.init_process_group("gloo", rank=rank, world_size=world)
    plan = FrameSplitPlan(world, rank, n_frames)
    shard = FrameShard(plan, FrameExchange(plan))
    g = torch.Generator().manual_seed(3)
    full = torch.randn((n_frames, 2, 5, 4), generator=g)              # per-frame K/V stand-in, same on every rank
    local = full[plan.lo:plan.hi].contiguous()
    first, prev = shard.exchange.st_sources(local[0].contiguous(), local[-1].contiguous())
    ok_st = torch.equal(first, full[0]) and torch.equal(prev, full[max(plan.lo - 1, 0)])
    ok_all = torch.equal(shard.exchange.gather_frames(local), full)
    inst = torch.arange(3 * n_frames * 6).reshape(3 * n_frames * 6, 1)      # 3 scenes x T frames x 6 views
    took = shard.take_frames(inst, 3, 6).reshape(3, plan.n_local, 6)
    ok_take = torch.equal(took, inst.reshape(3, n_frames, 6)[:, plan.lo:plan.hi])
    out.put((rank, plan.local, bool(ok_st), bool(ok_all), bool(ok_take), plan.message_bytes(1400, 320)))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,n_frames", [(2, 8), (3, 8), (4, 4), (2, 3)])
def test_frame_split_exchange_gloo(world, n_frames):
    """Frames of a scene sharded over `world` ranks (balanced and ragged): the ST-Attn sources (frame 0 from rank 0,
    the previous frame from the rank before) and the temporal all-gather arrive bit for bit; the ranges tile [0, T)."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_frame_worker, args=(r, world, port, n_frames, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = sorted(q.get(timeout=180) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert sum((g[1] for g in got), []) == list(range(n_frames))
    assert all(g[2] and g[3] and g[4] for g in got), got
    frame_kv = 2 * 6 * 1400 * 320 * 2
    assert got[0][5][0] == world * frame_kv if world > 1 else 0           # rank 0: frame 0 to everyone + its last frame
    assert got[-1][5] == (0, (n_frames - len(got[-1][1])) * frame_kv)      # last rank sends nothing


def test_frame_split_plan_rejects_more_ranks_than_frames():
    from dualdiff_amd.parallel import FrameSplitPlan
    with pytest.raises(ValueError):
        FrameSplitPlan(4, 0, 3)
