"""The helpers every launch wrapper goes through, without a GPU: the event bracket and the GEMM / conv books of _timer
(with a recording stand-in for the timer and for the library), the scratch attachment of _workspace, and the output /
dtype helpers of ops."""
import pytest
import torch

from dualdiff_amd import _native, _timer, _workspace, ops, tuning


class Recorder:
    """KernelTimer's start / stop, recording instead of timing."""

    def __init__(self, shapes=True):
        self.shapes, self.records, self.log = shapes, [], []

    def start(self):
        self.log.append("start")
        return len(self.log)

    def stop(self, e0, name, flops, nbytes, staged=0.0):
        self.log.append("stop")
        self.records.append((name, flops, nbytes, staged))


@pytest.fixture
def host(monkeypatch):
    monkeypatch.setattr(_timer, "_stream", lambda: "stream")
    yield
    _timer.set_timer(None)


def fake_launcher(plan, pad_lo=1, phases=None):
    def launch(d, st):
        if phases is not None:
            phases.append(d.phase)
        return 0
    return tuning.Launcher(None, pad_lo, launch, lambda d: 0, lambda d: plan)


def gemm_desc(rows, n, k, res=False, acc=False):
    d = _native.GemmDesc()
    d.rows, d.n, d.k, d.accumulate = rows, n, k, int(acc)
    d.res = 4096 if res else None
    return d


def test_bracket_costs_nothing_without_a_timer(host):
    calls = []

    def book():
        raise AssertionError("the books were asked for with no timer installed")
    _timer.launch("x", lambda a, b: calls.append((a, b)) or 0, 1, 2, book=book)
    assert calls == [(1, 2)]
    with pytest.raises(RuntimeError):                    # the return code is still checked
        _timer.launch("x", lambda: -1, book=book)


def test_bracket_books_after_the_launch(host):
    t = Recorder()
    _timer.set_timer(t)
    _timer.launch("x", lambda: t.log.append("launch") or 0, book=lambda: ("k", 1.0, 2.0))
    _timer.launch("x", lambda: 0)                        # a site without books is not bracketed
    assert t.log == ["start", "launch", "stop"] and t.records == [("k", 1.0, 2.0, 0.0)]


def test_gemm_books_one_launch(host):
    t = Recorder()
    _timer.set_timer(t)
    d = gemm_desc(96, 64, 512, res=True)
    _timer.gemm_launch(fake_launcher("dd_gemm2_kernel<f> split=1 grid=2x3 tile=64x32 w4"), d, "gemm", "gemm", 128, 96 * 512)
    # GEGLU-style call: 128 weight rows, 64 output columns; output written + residual read
    assert t.records == [("dd_gemm2_kernel<f> gemm 96x128x512", 2.0 * 96 * 128 * 512,
                          2.0 * (96 * 512 + 128 * 512 + 96 * 64 * 2), 6.0 * 8 * (64 + 32) * 128.0)]
    t.shapes, t.records = False, []
    _timer.gemm_launch(fake_launcher("dd_gemm2_kernel<f> split=1 grid=2x3 tile=64x32 w4"), gemm_desc(96, 64, 512), "gemm", "gemm", 64, 1)
    assert t.records[0][0] == "dd_gemm2_kernel<f>"


def test_split_k_is_booked_as_its_two_phases(host):
    t, phases = Recorder(), []
    _timer.set_timer(t)
    d = gemm_desc(100, 64, 576, acc=True)
    _timer.gemm_launch(fake_launcher("dd_gemm3_kernel<f> split=3 grid=1x1 tile=128x64", phases=phases), d, "conv3x3", "conv", 64, 777)
    slab = 4.0 * 3 * 100 * 64
    nbytes = 2.0 * (777 + 64 * 576 + 100 * 64 * 2)
    assert phases == [1, 2] and d.phase == 0
    assert t.records == [("dd_gemm3_kernel<f> conv 100x64x576", 2.0 * 100 * 64 * 576, nbytes + slab, 9.0 * (128 + 64) * 128.0),
                         ("dd_splitk_reduce_kernel", 0.0, slab + 2.0 * 100 * 64, 0.0)]
    # reduce=False: the slabs alone, whatever consumes them is the caller's launch
    t.records, d = [], gemm_desc(100, 64, 576)
    del phases[:]
    _timer.gemm_launch(fake_launcher("dd_gemm3_kernel<f> split=3 grid=1x1 tile=128x64", phases=phases), d, "conv3x3", "conv", 64, 777,
                       reduce=False)
    assert phases == [1] and t.records == [("dd_gemm3_kernel<f> conv 100x64x576", 2.0 * 100 * 64 * 576,
                                            2.0 * (777 + 64 * 576) + slab, 9.0 * (128 + 64) * 128.0)]
    # without a timer the phases are the library's business (phase 0), except for reduce=False
    _timer.set_timer(None)
    del phases[:]
    _timer.gemm_launch(fake_launcher("", phases=phases), gemm_desc(100, 64, 576), "conv3x3", "conv", 64, 777)
    _timer.gemm_launch(fake_launcher("", phases=phases), gemm_desc(100, 64, 576), "conv3x3", "conv", 64, 777, reduce=False)
    assert phases == [0, 1]


def test_pad0_conv_is_one_bracket_without_staged_bytes(host):
    t, phases = Recorder(), []
    _timer.set_timer(t)
    L = fake_launcher("dd_gemm_pad0_kernel<f> split=2 grid=1x1 tile=128x64", pad_lo=0, phases=phases)
    _timer.gemm_launch(L, gemm_desc(4, 64, 576), "conv3x3(pad=0)", "conv", 64, 1024)
    assert phases == [0]
    assert t.records == [("dd_gemm_pad0_kernel<f> conv 4x64x576", 2.0 * 4 * 64 * 576, 2.0 * (1024 + 64 * 576 + 4 * 64), 0.0)]


def test_scratch_is_attached_only_when_the_launch_needs_it(monkeypatch):
    asked = []

    def workspace(nbytes, device):
        asked.append((nbytes, device))
        return torch.zeros(32, dtype=torch.float32)
    monkeypatch.setattr(_workspace, "workspace", workspace)
    d = _native.GemmDesc()
    assert _workspace.attach(d, "dev", lambda: 0) == 0 and asked == [] and not d.ws
    assert _workspace.attach(d, "dev", lambda: 100) == 100 and asked == [(100, "dev")]
    assert d.ws and d.ws_bytes == 128
    monkeypatch.setattr(_workspace, "_DBG_STAMP_WS", True)          # DD_DBG_STAMP_WS=1: always, for the stamps
    assert _workspace.attach(_native.GemmDesc(), "dev", lambda: 0) == 0 and len(asked) == 2


def test_out_helper_allocates_or_validates_and_forgets():
    cpu = torch.device("cpu")
    new = ops._out_or_new(None, (3, 4), torch.float16, cpu, "op")
    assert new.shape == (3, 4) and new.dtype == torch.float16
    like = torch.empty(4, 3, dtype=torch.bfloat16).t()
    assert ops._out_or_new(None, like, like.dtype, cpu, "op").stride() == like.stride()
    out = torch.empty(3, 4, dtype=torch.float16)
    out._ln_cache, out._ln_out, out._ln_stats, out._gn_cache, out._unwritten, out.other = 1, 2, 3, 4, True, 5
    assert ops._out_or_new(out, (3, 4), torch.float16, cpu, "op") is out
    assert not any(hasattr(out, a) for a in ("_ln_cache", "_ln_out", "_ln_stats", "_gn_cache", "_unwritten")) and out.other == 5
    with pytest.raises(TypeError, match="op: out must be torch.bfloat16"):
        ops._out_or_new(out, (3, 4), torch.bfloat16, cpu, "op")


def test_dtype_codes_go_through_one_check():
    assert ops._dt(torch.empty(1, dtype=torch.float16)) == _native.DD_F16
    assert ops._dt(torch.empty(1, dtype=torch.bfloat16)) == _native.DD_BF16
    with pytest.raises(TypeError):
        ops._dt(torch.empty(1))
    with pytest.raises(TypeError):
        ops.gemm_kernel_name(64, 64, 64, dtype=torch.float32)
    assert "split=" in ops.gemm_kernel_name(2800, 320, 320, dtype=torch.float16)
    with pytest.raises(TypeError):
        ops._check_lk_dev(torch.zeros(1, dtype=torch.int64))
    ops._check_lk_dev(None)
    ops._check_lk_dev(torch.zeros(1, dtype=torch.int32))
