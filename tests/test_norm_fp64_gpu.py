"""Every GroupNorm and LayerNorm kernel path against the fp64 reference and per-element bound of norm_reference.py.

GroupNorm.  `gn_fused_plan` / `gn_plan` (csrc/norm.hip) pick the form from (hw, c, groups): dd_gn_fused_kernel with 256 or
1024 threads (the slab in registers, `nv` 16-byte vectors per thread on `plc` pixel lanes), else dd_gn_stats_kernel +
dd_gn_apply_kernel over splits of `pps` pixels.  GN_CASES names the smallest shape found for each path; `fused_plan` and
`two_launch_plan` below mirror the planner so that the table can say what each shape exercises, and
test_case_table_takes_every_path (no GPU) holds the mirror and the tags against dd_groupnorm_is_fused.  The GPU tests
launch through ops.groupnorm / ops.layernorm into the first rows of a NaN-filled buffer with 8 guard rows, compare EVERY
element, and want the guard rows back as NaN.  Each prints one `[norm fp64]` line.

The plans that only DD_GN_BIG_CAP reaches (vectors 5..8 of the NVMAX = 8 instantiations) run once each in a child
process of their own: the variable is read once per process."""
import collections
import itertools
import os
import subprocess
import sys

import pytest
import torch

from dualdiff_amd import _native
from tests import norm_reference as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [torch.float16, torch.bfloat16]
IDS = ["f16", "bf16"]
_TN = {torch.float16: "f16", torch.bfloat16: "bf16"}
GUARD = 8
GN_THREADS, GN_MAX_SPLIT, GN_UNROLL = 256, 64, 4


# ---- the planner, mirrored (csrc/norm.hip: gn_fused_plan, gn_plan) ------------------------------------------------------

def fused_plan(hw, c, groups, big_cap=4):
    """-> dict(threads, cpb, vpp, plc, nv) or None (two launches)."""
    cpg = c // groups
    for gpb in range(1, min(groups, 64) + 1):
        if groups % gpb:
            continue
        cb = cpg * gpb
        if cb % 8 or cb < 40:
            continue
        v = cb // 8
        for th, cap in ((256, 4), (1024, min(big_cap, 8)), (256, 8)):
            if v > th:
                continue
            pl = min(th // v, hw)
            n = -(-hw // pl)
            if n <= cap:
                return dict(threads=th, cpb=cb, vpp=v, plc=pl, nv=n)
        return None
    return None


def two_launch_plan(hw, c):
    """-> dict(pps, nsplit, last, lanes): pixels per split, splits, pixels of the last split, pixel lanes per block."""
    cv = c // 8
    lanes = 1 if cv >= GN_THREADS else GN_THREADS // cv
    pps = min(max(-(-hw // GN_MAX_SPLIT), lanes * GN_UNROLL), hw)
    nsplit = -(-hw // pps)
    return dict(pps=pps, nsplit=nsplit, last=hw - (nsplit - 1) * pps, lanes=lanes)


# threads (0 = two launches), hw, c1, c2, groups, what the planner must give, what it exercises
GnCase = collections.namedtuple("GnCase", "threads hw c1 c2 groups plan what")
GN_CASES = [
    GnCase(0, 817, 320, 0, 32, dict(pps=24, nsplit=35, last=1, lanes=6), "last split of 1 pixel (tail loop only), 16 idle threads"),
    GnCase(0, 409, 1280, 1280, 32, dict(pps=7, nsplit=59, last=3, lanes=1), "c >= 2048: one pixel lane, second channel pass"),
    GnCase(0, 513, 128, 0, 32, dict(pps=64, nsplit=9, last=1, lanes=16), "4 channels per group: two whole groups per vector"),
    GnCase(0, 350, 320, 640, 32, dict(pps=8, nsplit=44, last=6, lanes=2), "a group straddles the x1 / x2 seam"),
    GnCase(0, 9, 4096, 0, 1, dict(pps=4, nsplit=3, last=1, lanes=1), "the largest c, one group, two full channel passes"),
    GnCase(0, 513, 512, 0, 64, dict(pps=16, nsplit=33, last=1, lanes=4), "64 groups"),
    GnCase(0, 6400, 640, 0, 32, dict(pps=100, nsplit=64, last=100, lanes=3), "64 splits: unrolled iterations and a tail"),
    GnCase(0, 817, 192, 0, 32, dict(pps=40, nsplit=21, last=17, lanes=10), "6 channels per group"),
    GnCase(0, 817, 224, 0, 32, dict(pps=36, nsplit=23, last=25, lanes=9), "7 channels per group"),
    GnCase(256, 28, 320, 0, 32, dict(vpp=5, plc=28, nv=1), "hw < 51 pixel lanes: 140 of 256 threads active"),
    GnCase(256, 204, 320, 0, 32, dict(vpp=5, plc=51, nv=4), "4 vectors per thread, the last exactly full"),
    GnCase(256, 203, 320, 0, 32, dict(vpp=5, plc=51, nv=4), "4 vectors per thread, the last partial"),
    GnCase(256, 91, 1280, 1280, 32, dict(cpb=80, vpp=10, plc=25, nv=4), "one group of 10 vectors per block"),
    GnCase(256, 91, 128, 0, 32, dict(cpb=64, vpp=8, plc=32, nv=3), "16 groups per block, 4 channels per group"),
    GnCase(256, 28, 640, 320, 32, dict(cpb=120, vpp=15, plc=17, nv=2), "x1 / x2 seam inside a group"),
    GnCase(256, 1, 320, 0, 32, dict(vpp=5, plc=1, nv=1), "one pixel"),
    GnCase(256, 60, 512, 0, 64, dict(cpb=64, vpp=8, plc=32, nv=2), "64 groups"),
    GnCase(256, 28, 192, 0, 32, dict(cpb=48, vpp=6, plc=28, nv=1), "6 channels per group"),
    GnCase(256, 28, 224, 0, 32, dict(cpb=56, vpp=7, plc=28, nv=1), "7 channels per group"),
    GnCase(1024, 350, 320, 0, 32, dict(vpp=5, plc=204, nv=2), "second vector partial"),
    GnCase(1024, 816, 320, 0, 32, dict(vpp=5, plc=204, nv=4), "4 vectors per thread, the last exactly full"),
    GnCase(1024, 815, 320, 0, 32, dict(vpp=5, plc=204, nv=4), "4 vectors per thread, the last partial"),
    GnCase(1024, 350, 1280, 1280, 32, dict(cpb=80, vpp=10, plc=102, nv=4), "one group of 10 vectors per block"),
    GnCase(1024, 91, 640, 320, 32, dict(cpb=120, vpp=15, plc=68, nv=2), "x1 / x2 seam inside a group"),
    GnCase(1024, 350, 128, 0, 32, dict(cpb=64, vpp=8, plc=128, nv=3), "4 channels per group"),
    GnCase(1024, 350, 256, 0, 32, dict(cpb=64, vpp=8, plc=128, nv=3), "8 channels per group: a vector is a group"),
    GnCase(1024, 350, 224, 0, 32, dict(cpb=56, vpp=7, plc=146, nv=3), "7 channels per group"),
]
# (DD_GN_BIG_CAP, hw, c, threads, nv): vectors 5..8 of both instantiations
EXPERIMENTAL = [(8, 1400, 320, 1024, 7), (0, 350, 320, 256, 7)]


def case_id(c):
    return "%s_hw%d_c%d%s_g%d" % ("two" if c.threads == 0 else "fused%d" % c.threads, c.hw, c.c1,
                                  "+%d" % c.c2 if c.c2 else "", c.groups)


def test_case_table_takes_every_path():
    lib = _native.load()
    cover = set()
    for c in GN_CASES:
        ch = c.c1 + c.c2
        assert lib.dd_groupnorm_is_fused(c.hw, ch, c.groups) == c.threads, case_id(c)
        fp = fused_plan(c.hw, ch, c.groups)
        assert (fp["threads"] if fp else 0) == c.threads, (case_id(c), fp)
        got = fp if fp else two_launch_plan(c.hw, ch)
        assert {k: got[k] for k in c.plan} == c.plan, (case_id(c), got)
        cover.add((c.threads, ch // c.groups))
    for th in (0, 256, 1024):
        for cpg in (4, 6, 7, 8, 10):              # 10: vectors straddle two groups; 6 and 7: the limit of the two-group logic
            if (th, cpg) != (1024, 6):            # (6 at 1024 threads is 7's twin: one of the two is enough there)
                assert (th, cpg) in cover, (th, cpg)
    two_pass = [c for c in GN_CASES if c.threads == 0 and c.c1 + c.c2 >= 8 * GN_THREADS]
    assert two_pass and any(c.groups == 32 for c in two_pass), "no two-launch case with c >= 2048 (second channel pass)"
    assert any(c.plan.get("last") == 1 for c in GN_CASES), "no last split of one pixel"
    assert any(c.threads == 0 and c.c2 for c in GN_CASES) and any(c.threads and c.c2 for c in GN_CASES)
    # the experimental plans, as the planner would give them with the variable set
    for cap, hw, ch, th, nv in EXPERIMENTAL:
        fp = fused_plan(hw, ch, 32, big_cap=cap)
        assert (fp["threads"], fp["nv"]) == (th, nv), (cap, hw, ch, fp)
        assert fp["nv"] > 4 and fused_plan(hw, ch, 32) != fp
    # five channels per group: a vector would touch three groups; no form takes it (2 and 3: likewise)
    for hw in (1, 28, 91, 350, 817):
        for ch, groups in ((160, 32), (80, 16), (320, 64), (64, 32), (96, 32)):
            assert lib.dd_groupnorm_is_fused(hw, ch, groups) == 0, (hw, ch, groups)


# ---- the check, shared by the tests and the child process ---------------------------------------------------------------

def out_buffer(rows, c, dtype, dev):
    buf = N.nan_like((rows + GUARD, c), dtype, dev)
    return buf, buf[:rows]


def guard_untouched(buf, rows):
    return bool(torch.isnan(buf[rows:]).all())


def compare(y, ref, e, kind, what, stats):
    stats[0].append(N.check(y, ref, e, what))
    stats[1].append(N.mean_ratio(y, ref, e))
    if kind == "const":                                 # var = 0: act(beta), bit for bit wherever E cannot cross a rounding
        ok, val = N.settled(ref, e, y.dtype)
        share = float(ok.float().mean())
        assert share > 0.9, "%s: only %.3f of the elements have one right answer" % (what, share)
        bad = ok & (y != val)
        assert not bool(bad.any()), "%s: %d elements differ from round(act(beta))" % (what, int(bad.sum()))


def run_groupnorm(ops, dev, hw, c1, c2, groups, dtype, kind, silu, eps, m, seed, stats, what):
    c = c1 + c2
    x = N.groupnorm_data(kind, m, hw, c, groups, dtype, seed, dev)
    x1 = x[:, :c1].contiguous() if c2 else x
    x2 = x[:, c1:].contiguous() if c2 else None
    gamma, beta = N.affine(c, dtype, seed + 1, dev)
    buf, out = out_buffer(m * hw, c, dtype, dev)
    y = ops.groupnorm(x1, gamma, beta, m, hw, groups, eps, silu, x2=x2, out=out)
    assert y.data_ptr() == out.data_ptr()
    ref, e = N.groupnorm_reference(x1, gamma, beta, m, hw, groups, eps, silu, x2=x2)
    what = "%s %s %s silu=%d eps=%g m=%d" % (what, _TN[dtype], kind, silu, eps, m)
    compare(out, ref, e, kind, what, stats)
    assert guard_untouched(buf, m * hw), what + ": wrote past the last row"


def variants(index, elems):
    """(kind, silu, eps, m) of a case: every kind with SiLU on and off; eps and m alternate so that each value meets each
    kind and each SiLU setting somewhere in the table (m = 2 only where three instances would pass 4 M elements)."""
    for k, (kind, silu) in enumerate(itertools.product(N.KINDS, (False, True))):
        eps = (1e-5, 1e-6)[(k // 2 + k + index) % 2]
        m = 2 + (k // 2 + index // 2) % 2
        yield kind, silu, eps, (2 if 3 * elems > (1 << 22) else m)


@pytest.fixture(scope="module")
def ops(gpu):
    from dualdiff_amd import ops as O
    return O


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", GN_CASES, ids=case_id)
def test_groupnorm_matches_fp64(ops, gpu, case, dtype):
    index = GN_CASES.index(case)
    stats = ([], [])
    for v, (kind, silu, eps, m) in enumerate(variants(index, case.hw * (case.c1 + case.c2))):
        run_groupnorm(ops, gpu, case.hw, case.c1, case.c2, case.groups, dtype, kind, silu, eps, m, 1000 + 16 * index + 2 * v,
                      stats, case_id(case))
    torch.cuda.synchronize()
    print("\n[norm fp64] " + N.report_line("gn %s %s" % (case_id(case), _TN[dtype]), *stats))


@pytest.mark.gpu
@pytest.mark.parametrize("cap,hw,c,threads,nv", EXPERIMENTAL, ids=["big_cap8_1024x7", "big_cap0_256x7"])
def test_experimental_plans_match_fp64(gpu, cap, hw, c, threads, nv):
    env = dict(os.environ, DD_GN_BIG_CAP=str(cap))
    cmd = [sys.executable, "-m", "tests.test_norm_fp64_gpu", str(hw), str(c), str(threads)]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("[norm fp64]")]
    print("\n" + "\n".join(lines))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert len(lines) == 1


def child_main(argv):
    """One experimental plan in a process of its own: spike and offset data in both types through run_groupnorm; the
    first failure raises (exit status 1) and nothing is launched after it."""
    hw, c, threads = int(argv[0]), int(argv[1]), int(argv[2])
    from dualdiff_amd import ops as O
    lib = _native.load()
    got = lib.dd_groupnorm_is_fused(hw, c, 32)
    if got != threads:
        raise SystemExit("DD_GN_BIG_CAP=%s: hw %d c %d takes form %d, expected %d"
                         % (os.environ.get("DD_GN_BIG_CAP"), hw, c, got, threads))
    dev = torch.device("cuda:0")
    stats = ([], [])
    for i, (dtype, (kind, silu, eps, m)) in enumerate(itertools.product(
            DTYPES, (("spike", True, 1e-5, 3), ("offset", False, 1e-6, 2)))):
        run_groupnorm(O, dev, hw, c, 0, 32, dtype, kind, silu, eps, m, 4000 + 2 * i, stats,
                      "DD_GN_BIG_CAP=%s hw%d c%d" % (os.environ.get("DD_GN_BIG_CAP"), hw, c))
    torch.cuda.synchronize()
    print("[norm fp64] " + N.report_line("gn fused%d nv>4 hw%d c%d" % (threads, hw, c), *stats))


# ---- LayerNorm ---------------------------------------------------------------------------------------------------------

# c -> rows.  320 / 640 / 1280: dd_layernorm_sub_kernel with 32 / 16 / 8 rows per block (8 / 4 / 2 per wave); every other c:
# dd_layernorm_kernel, 4 rows per block, lanes >= c / 8 idle, up to 4 vectors per lane
LN_CASES = collections.OrderedDict([
    (320, (1, 31, 33, 701)), (640, (1, 17)), (1280, (9, 91)),
    (8, (1, 5, 403)), (512, (1, 5, 403)), (520, (1, 5, 403)), (768, (1, 5, 403)), (1024, (1, 5, 403)), (2048, (1, 5, 403)),
])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("c", list(LN_CASES), ids=lambda c: "c%d" % c)
def test_layernorm_matches_fp64(ops, gpu, c, dtype):
    stats = ([], [])
    gamma, beta = N.affine(c, dtype, 77 + c, gpu)
    for i, (rows, kind) in enumerate(itertools.product(LN_CASES[c], N.KINDS)):
        eps = (1e-5, 1e-6)[(i + i // 4) % 2]
        x = N.layernorm_data(kind, rows, c, dtype, 2000 + c + i, gpu)
        buf, out = out_buffer(rows, c, dtype, gpu)
        ops.layernorm(x, gamma, beta, eps, out=out)
        ref, e = N.layernorm_reference(x, gamma, beta, eps)
        what = "layernorm %dx%d %s %s eps=%g" % (rows, c, _TN[dtype], kind, eps)
        compare(out, ref, e, kind, what, stats)
        assert guard_untouched(buf, rows), what + ": wrote past the last row"
    torch.cuda.synchronize()
    kern = "sub<%d>" % (c // 40) if c in (320, 640, 1280) else "generic"
    print("\n[norm fp64] " + N.report_line("ln %s c%d %s" % (kern, c, _TN[dtype]), *stats))


# ---- rejections: an error, and nothing written ---------------------------------------------------------------------------

def _rejected(exc, call, out):
    with pytest.raises(exc):
        call()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()), "a rejected call wrote to its output"


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("c,groups", [(160, 32), (80, 16)], ids=["c160_g32", "c80_g16"])
@pytest.mark.parametrize("hw", [28, 350, 817], ids=["fused256", "fused1024", "two_launch"])
def test_five_channels_per_group_are_rejected(ops, gpu, hw, c, groups, dtype):
    """c / groups = 5: the 16-byte vector at channel 8 holds channels of groups 1, 2 AND 3, and both GroupNorm forms split
    a vector between two groups only.  The sizes are the ones at which c = 320 takes each of the three forms."""
    m = 2
    x = N.groupnorm_data("randn", m, hw, c, groups, dtype, 1, gpu)
    gamma, beta = N.affine(c, dtype, 2, gpu)
    buf, out = out_buffer(m * hw, c, dtype, gpu)
    _rejected(_native.Unsupported, lambda: ops.groupnorm(x, gamma, beta, m, hw, groups, 1e-5, True, out=out), buf)
    lib = _native.load()
    assert lib.dd_groupnorm_is_fused(hw, c, groups) == 0
    # the split-K form (real slabs behind the pointer: were the call accepted, it would read and write valid memory)
    part = torch.zeros((2, m * hw, c), dtype=torch.float32, device=gpu)
    rc = lib.dd_groupnorm_splitk(ops._ptr(part), 2, None, None, 0, None, 0, None, ops._ptr(gamma), ops._ptr(beta),
                                 ops._ptr(out), m, hw, c, groups, 1e-5, 1, ops._dt(x), ops._stream())
    torch.cuda.synchronize()
    assert rc == -2 and bool(torch.isnan(buf).all())


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_groupnorm_rejections_leave_the_output_untouched(ops, gpu, dtype):
    m, hw = 2, 28
    lib = _native.load()

    def call(c, groups, exc, x=None):
        x = N.groupnorm_data("randn", m, hw, c, groups, dtype, 3, gpu) if x is None else x
        gamma, beta = N.affine(c, dtype, 4, gpu)
        buf, out = out_buffer(m * hw, c, dtype, gpu)
        _rejected(exc, lambda: ops.groupnorm(x, gamma, beta, m, hw, groups, 1e-5, False, out=out), buf)

    call(64, 32, _native.Unsupported)                  # 2 channels per group
    call(4104, 8, RuntimeError)                        # c > 4096
    call(520, 65, RuntimeError)                        # more than 64 groups
    flat = N.groupnorm_data("randn", m, hw, 328, 1, dtype, 5, gpu).reshape(-1)
    call(320, 32, RuntimeError, x=flat[4:4 + m * hw * 320].view(m * hw, 320))      # contiguous, 8 bytes off 16-byte alignment
    # a workspace one float short of dd_groupnorm_workspace_bytes
    c, groups = 320, 32
    x = N.groupnorm_data("randn", m, hw, c, groups, dtype, 6, gpu)
    gamma, beta = N.affine(c, dtype, 7, gpu)
    buf, out = out_buffer(m * hw, c, dtype, gpu)
    need = lib.dd_groupnorm_workspace_bytes(m, groups)
    ws = torch.zeros(need // 4, dtype=torch.float32, device=gpu)
    launch = lambda nbytes: lib.dd_groupnorm_nhwc(ops._ptr(x), c, None, 0, ops._ptr(gamma), ops._ptr(beta), ops._ptr(out), m,
                                                  hw, groups, 1e-5, 0, ops._dt(x), ops._ptr(ws), nbytes, ops._stream())
    _rejected(RuntimeError, lambda: _native.check(launch(need - 4), "groupnorm"), buf)
    assert launch(need - 4) == -4
    assert launch(need) == 0                           # the same call with the full workspace goes through
    torch.cuda.synchronize()
    assert not bool(torch.isnan(out).any()) and guard_untouched(buf, m * hw)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("c", [2056, 12])
def test_layernorm_rejections_leave_the_output_untouched(ops, gpu, c, dtype):
    rows = 5
    x = N.layernorm_data("randn", rows, c, dtype, 8, gpu)
    gamma, beta = N.affine(c, dtype, 9, gpu)
    buf, out = out_buffer(rows, c, dtype, gpu)
    _rejected(_native.Unsupported, lambda: ops.layernorm(x, gamma, beta, 1e-5, out=out), buf)


if __name__ == "__main__":
    child_main(sys.argv[1:])
