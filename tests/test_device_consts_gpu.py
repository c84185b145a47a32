"""The one rule for process-lifetime device constants (dualdiff_amd/_consts.py) on the GPU: an entry is complete for every
stream the moment it can be seen, a hit inside a stream capture is served and a miss raises before any HIP call, the zero
bias built on the host is the zero bias, one device has one key spelling, and blocks share their neighbour maps."""
import pytest
import torch

from dualdiff_amd import ops
from dualdiff_amd.networks import layers as L
from dualdiff_amd.pipeline.image_output import device_tables, resample_tables

pytestmark = pytest.mark.gpu

PAIR = {0: [5, 1], 1: [0, 2], 2: [1, 3], 3: [2, 4], 4: [3, 5], 5: [4, 0]}
SLEEP = 5_000_000              # torch.cuda._sleep: ticks of the device clock, 50 ms at the 100 MHz of the constant counter


def _rand(shape, dtype, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).cuda().to(dtype)


def _xattn_case(dtype):
    """1 instance x 80 rows, 77 keys: x, one (320, 320) weight for both projections, K | V side by side."""
    return _rand((80, 320), dtype, 1), _rand((320, 320), dtype, 2, 320 ** -0.5), _rand((77, 640), dtype, 3)


def _xattn(x, w, kv, bo=None):
    return ops.xattn320(x, w, w, bo, kv[:, :320], kv[:, 320:], 1, 80, 77, 40 ** -0.5)


def test_constants_are_complete_for_every_stream(gpu):
    """Requested on stream A behind a sleeping kernel, read on stream B, which never waited for A."""
    x, w, kv = _xattn_case(torch.bfloat16)
    a, b = torch.cuda.Stream(gpu), torch.cuda.Stream(gpu)
    a.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(a):
        torch.cuda._sleep(SLEEP)
        lk = L.lk_const(12345, gpu)
        torch.cuda._sleep(SLEEP)
        kk, bounds = device_tables(37, 23, gpu)
        torch.cuda._sleep(SLEEP)
        _xattn(x, w, kv)                                      # bo=None: asks for the bf16 zero bias
    with torch.cuda.stream(b):
        zero = ops._zero_bias(torch.bfloat16, gpu)
        got = [t.cpu() for t in (lk, kk, bounds, zero)]
    torch.cuda.synchronize()
    want_kk, want_bounds = resample_tables(37, 23)
    assert lk.dtype == torch.int32 and got[0].tolist() == [12345]
    assert torch.equal(got[1], want_kk) and torch.equal(got[2], want_bounds)
    assert zero.dtype == torch.bfloat16 and zero.is_cuda and torch.equal(got[3], torch.zeros(320, dtype=torch.bfloat16))


def test_hit_inside_a_capture_replays_to_the_eager_result(gpu):
    x, w, kv = _xattn_case(torch.float16)
    eager = _xattn(x, w, kv).clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        y = _xattn(x, w, kv)
    g.replay()
    torch.cuda.synchronize()
    assert torch.isfinite(eager.float()).all() and torch.equal(y, eager)


def test_miss_inside_a_capture_raises_before_any_hip_call(gpu):
    x, w, kv = _xattn_case(torch.float16)
    eager = _xattn(x, w, kv).clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="inside a stream capture"):
        with torch.cuda.graph(g):
            L.lk_const(54321, gpu)
    again = _xattn(x, w, kv)                                  # nothing on the device was disturbed
    torch.cuda.synchronize()
    assert torch.equal(again, eager)
    assert L.lk_const(54321, gpu).tolist() == [54321]          # and the key is still free for an eager request


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_no_bias_is_the_zero_bias(gpu, dtype):
    x, w, kv = _xattn_case(dtype)
    none = _xattn(x, w, kv)
    explicit = _xattn(x, w, kv, bo=torch.zeros(320, dtype=dtype, device=gpu))
    torch.cuda.synchronize()
    assert torch.isfinite(none.float()).all() and none.float().abs().max() > 0 and torch.equal(none, explicit)


def test_one_spelling_per_device(gpu):
    assert L.lk_const(78, "cuda") is L.lk_const(78, torch.device("cuda", torch.cuda.current_device()))


def test_blocks_share_their_maps_on_the_gpu(gpu):
    from dualdiff_amd.networks.blocks import BasicMultiviewTransformerBlock
    a, b = (BasicMultiviewTransformerBlock(64, 2, 32, cross_attention_dim=24, neighboring_view_pair=PAIR) for _ in range(2))
    ma, mb = a.neighbour_maps(12, gpu), b.neighbour_maps(12, gpu)
    assert len(ma) == 2 and all(x is y for x, y in zip(ma, mb)) and all(m.is_cuda and m.dtype == torch.int32 for m in ma)
    assert [m.tolist() for m in ma] == [m.tolist() for m in a.neighbour_maps(12, "cpu")]
