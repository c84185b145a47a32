"""Per-launch HIP-event timing (bench.py's roofline leg): the timer, the one bracket every timed launch site goes
through, and the FLOP / byte bookkeeping of the GEMM / conv launches.  With no timer installed a launch costs the call."""
import ctypes
import re

import torch

from . import _native


class KernelTimer:
    """Optional per-launch HIP-event timing of the MFMA kernels (bench.py roofline leg).

    When installed (`ops.set_timer(KernelTimer())`) every gemm / conv3x3 / attention launch is
    bracketed by events recorded on the stream the kernel is launched on; `summary()` groups the
    launches by kernel symbol and returns count, total time and algorithmic FLOPs."""

    def __init__(self, shapes=False):
        self.records = []
        self.shapes = shapes
        self.overhead_ms = 0.0
        self.empty_bracket_ms = 0.0
        self.probe_ms = 0.0

    def calibrate(self, n=48, probe_us=15.0):
        """Event overhead per bracket, MEASURED at run time (not a fitted constant) and subtracted in
        summary() so that the per-kernel averages are comparable with rocprofv3's kernel durations.

        Probe: dd_probe_spin — one wave that busy-waits `probe_us` on the constant 100 MHz s_memrealtime counter and
        stores its own first and last reading, i.e. a kernel whose DEVICE-SIDE duration is known without events or a
        profiler.  n such launches are bracketed like the kernels of the instrumented step (queue kept busy);
        overhead = median(bracket - in-kernel duration): what an event pair adds around a ~15 us kernel (the
        dominant classes are 15-45 us).  A first attempt subtracted a probe's back-to-back time instead; that time
        contains the launch-to-launch gap a profiler does not count and gave 0.  The empty-bracket figure
        (4.6-4.8 us on MI355X) is kept in `empty_bracket_ms` for the JSON line; kernels of ~5 us stay the least
        certain rows of the table."""
        lib = _native.load()
        st = torch.cuda.current_stream()
        dev = torch.device("cuda", torch.cuda.current_device())
        pairs = []
        for _ in range(n):
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record(st)
            e1.record(st)
            pairs.append((e0, e1))
        torch.cuda.synchronize()
        d = sorted(a.elapsed_time(b) for a, b in pairs)
        self.empty_bracket_ms = d[len(d) // 2]
        stamps = torch.zeros((n, 2), dtype=torch.int64, device=dev)
        ticks = int(probe_us * 100)
        backlog = torch.empty(64 << 20, dtype=torch.uint8, device=dev)
        for _ in range(40):                       # keep the GPU behind the host while the brackets are enqueued
            backlog.zero_()
        pairs = []
        for i in range(n):
            a0, a1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a0.record(st)
            _native.check(lib.dd_probe_spin(ctypes.c_void_p(stamps[i].data_ptr()), ticks, _stream()), "probe_spin")
            a1.record(st)
            pairs.append((a0, a1))
        torch.cuda.synchronize()
        inside = (stamps[:, 1] - stamps[:, 0]).double().cpu() * 1e-5          # 100 MHz ticks -> ms
        over = sorted(p.elapsed_time(q) - float(inside[i]) for i, (p, q) in enumerate(pairs))
        self.probe_ms = float(inside.median())
        self.overhead_ms = min(max(over[len(over) // 2], 0.0), self.empty_bracket_ms)
        return self.overhead_ms

    def start(self):
        e = torch.cuda.Event(enable_timing=True)
        e.record(torch.cuda.current_stream())
        return e

    def stop(self, e0, name, flops, nbytes, staged=0.0):
        """staged: bytes the launch moves from L2 into LDS (tiled GEMM / conv families: every tile re-stages its operand
        slabs) — the quantity that actually bounds those kernels, reported beside the contract's roofs."""
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record(torch.cuda.current_stream())
        self.records.append((name, flops, nbytes, e0, e1, staged))

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for name, flops, nbytes, e0, e1, staged in self.records:
            d = out.setdefault(name, {"count": 0, "ms": 0.0, "flops": 0.0, "bytes": 0.0, "staged": 0.0})
            d["count"] += 1
            d["ms"] += max(e0.elapsed_time(e1) - self.overhead_ms, 0.0)
            d["flops"] += flops
            d["bytes"] += nbytes
            d["staged"] += staged
        return out


_TIMER = None


def set_timer(t):
    global _TIMER
    _TIMER = t


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def launch(what, fn, *args, book=None):
    """_native.check(fn(*args), what).  Under a timer the call is bracketed by events and booked as
    book() = (name, flops, nbytes[, staged]); book is not called otherwise."""
    t = _TIMER
    if t is None or book is None:
        return _native.check(fn(*args), what)
    e0 = t.start()
    _native.check(fn(*args), what)
    t.stop(e0, *book())


def mm_cost(kind, rows, n_w, k, a_elems, n_out, passes=1):
    """(shape suffix of the name, FLOPs, HBM bytes) of a GEMM / implicit-GEMM conv over two-byte elements: `a_elems`
    activation elements and the n_w x k weight read once, the rows x n_out result touched `passes` times (written; +1
    for a residual read, +1 for an accumulate read).  Call under an installed timer only."""
    return (" %s %dx%dx%d" % (kind, rows, n_w, k) if _TIMER.shapes else "", 2.0 * rows * n_w * k,
            2.0 * (a_elems + n_w * k + rows * n_out * passes))


def _staged_bytes(plan, d):
    """L2 -> LDS bytes of one dd_gemm launch, from its plan (`grid=MxN tile=BMxBN...`): every tile stages a
    (BM + BN) x 64-element slab pair per K-step; the direct small-image conv stages its (BM + 64)-row activation slab
    once per 64-channel chunk and a BN x 64 weight slab per (chunk, tap)."""
    m = re.search(r"grid=(\d+)x(\d+) tile=(.*)$", plan)
    if m is None:
        return 0.0
    tiles = int(m.group(1)) * int(m.group(2))
    t = re.search(r"(\d+)x(\d+)", m.group(3))
    if t is None:
        return 0.0
    bm, bn = int(t.group(1)), int(t.group(2))
    if "conv3s" in m.group(3):
        chunks = d.cin // 64
        return float(tiles) * chunks * ((bm + (88 if "band" in m.group(3) else 64)) * 128.0 + 9 * bn * 128.0)
    ksteps = (d.k + 63) // 64
    return float(tiles) * ksteps * (bm + bn) * 128.0


def plan_of(L, d):
    """(kernel symbol, split-K, whole plan string) of the launch L makes for `d`."""
    plan = L.kernel_name(d)
    name, _, rest = plan.partition(" split=")
    return name, int(rest.split(" ")[0]) if rest else 1, plan


def gemm_launch(L, d, what, kind, n_w, a_elems, reduce=True):
    """The GEMM / conv launch of descriptor `d` through the tuning.Launcher `L`.  kind ("gemm" / "conv"), n_w (weight
    rows: 2 n under GEGLU) and a_elems (activation elements read) feed the timer's books only.

    Under a timer a split-K launch of dd_gemm is bracketed as its two phases (dd_gemm_desc.phase) and booked under their
    own kernel symbols, so that every class of the roofline table is one kernel symbol whose average duration can be
    checked against rocprofv3's; the pad-0 conv keeps one bracket and books no staged bytes.
    reduce=False: the partial-slab phase alone — the caller's own kernel consumes the slabs (dd_groupnorm_splitk)."""
    t = _TIMER
    if not reduce:
        d.phase = 1
    if t is None:
        return _native.check(L.launch(d, _stream()), what)
    suffix, flops, nbytes = mm_cost(kind, d.rows, n_w, d.k, a_elems, d.n, 1 + (1 if d.res else 0) + (1 if d.accumulate else 0))
    name, split, plan = plan_of(L, d)
    if L.pad_lo != 1:
        return launch(what, L.launch, d, _stream(), book=lambda: (name + suffix, flops, nbytes))
    staged = _staged_bytes(plan, d)
    if split <= 1:
        return launch(what, L.launch, d, _stream(), book=lambda: (name + suffix, flops, nbytes, staged))
    slab = 4.0 * split * d.rows * d.n
    if not reduce:
        return launch(what, L.launch, d, _stream(),
                      book=lambda: (name + suffix, flops, 2.0 * (a_elems + n_w * d.k) + slab, staged))
    d.phase = 1
    launch(what, L.launch, d, _stream(), book=lambda: (name + suffix, flops, nbytes + slab, staged))   # operands once + the fp32 slabs written
    d.phase = 2
    launch(what, L.launch, d, _stream(), book=lambda: ("dd_splitk_reduce_kernel", 0.0, slab + 2.0 * d.rows * d.n))
    d.phase = 0
