"""dd_attn_probs / ops.attention_probs without a GPU: the fp64 reference against torch, the launcher's return codes (decided
before anything is launched: DD_ERR_LAUNCH on a machine without a GPU would mean the validation came after a launch), the
header, the ABI version and the binding table."""
import ctypes
import os
import re

import pytest
import torch

from dualdiff_amd import _build, _native
from tests import attn_probs_reference as AR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG, UNSUPPORTED = -1, -2
P = 16                                                   # non-null, 16-byte aligned, never dereferenced
F16, BF16 = _native.DD_F16, _native.DD_BF16


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_build.lib_path()):
        pytest.skip("library not built (run __graft_entry__.build())")
    return _native.load(build_if_missing=False)


# ---- the reference -------------------------------------------------------------------------------------------------------

def _operands(dtype, b=2, h=3, lq=5, lk=11, d=40, seed=0):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn((b, h, lq, d), generator=g).to(dtype)
    k = torch.randn((b, h, lk, d), generator=g).to(dtype)
    return q, k


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_reference_is_the_float64_softmax(dtype):
    q, k = _operands(dtype)
    scale = 40 ** -0.5
    want = torch.softmax(scale * (q.double() @ k.double().transpose(2, 3)), dim=-1)
    ref, e = AR.reference(q, k, scale, per_head=True)
    assert ref.dtype == torch.float64 and ref.shape == (2, 3, 5, 11)
    assert torch.allclose(ref, want, rtol=1e-12, atol=1e-15)
    assert torch.allclose(ref.sum(-1), torch.ones(2, 3, 5, dtype=torch.float64), rtol=0, atol=1e-13)
    assert bool((e > 0).all()) and float(e.max()) < 1e-3
    mean, _ = AR.reference(q, k, scale)
    assert torch.allclose(mean, want.mean(1), rtol=1e-12, atol=1e-15)
    assert torch.allclose(mean.sum(-1), torch.ones(2, 5, dtype=torch.float64), rtol=0, atol=1e-13)


def test_reference_key_count_weight_prescaled_and_accumulate():
    q, k = _operands(torch.float16)
    scale = 40 ** -0.5
    want = torch.softmax(scale * (q.double() @ k[:, :, :7].double().transpose(2, 3)), dim=-1)
    ref, _ = AR.reference(q, k, scale, n_keys=7, per_head=True, weight=0.5)
    assert ref.shape[-1] == 7 and torch.allclose(ref, 0.5 * want, rtol=1e-12, atol=1e-15)
    # prescaled: the operand carries scale * log2 e, the reference multiplies by 1
    qp = (q.double() * scale * AR.LOG2E)
    pre, _ = AR.reference(qp, k, None, n_keys=7, prescaled=True, per_head=True)
    assert torch.allclose(pre, want, rtol=1e-10, atol=1e-14)
    old = torch.full_like(ref, 0.25)
    acc, e = AR.reference(q, k, scale, n_keys=7, per_head=True, weight=0.5, old=old)
    assert torch.allclose(acc, 0.5 * want + 0.25, rtol=1e-12)
    two, e2 = AR.accumulated([AR.reference(q, k, scale, n_keys=7, weight=0.5)] * 2)
    assert torch.allclose(two, want.mean(1), rtol=1e-12, atol=1e-15) and bool((e2 > 0).all())


# ---- the launcher ----------------------------------------------------------------------------------------------------------

def _args(**kw):
    a = dict(q=P, k=P, p=P, ldq=320, ldk=640, qbs=4 * 320, kbs=4 * 640, qhs=0, khs=0, ldp=4, pbs=16, phs=0, batch=2, lq=4,
             lk=4, heads=8, head_dim=40, scale=0.158, prescaled=0, per_head=0, accumulate=0, weight=1.0, lk_dev=None,
             dtype=F16)
    a.update(kw)
    return tuple(a[n] for n in ("q", "k", "p", "ldq", "ldk", "qbs", "kbs", "qhs", "khs", "ldp", "pbs", "phs", "batch", "lq",
                                "lk", "heads", "head_dim", "scale", "prescaled", "per_head", "accumulate", "weight",
                                "lk_dev", "dtype")) + (None,)


BAD = [dict(q=None), dict(k=None), dict(p=None), dict(q=24), dict(k=8), dict(p=18), dict(lk_dev=18),
       dict(lk=0), dict(lq=0), dict(heads=0), dict(batch=0), dict(head_dim=0), dict(ldq=324), dict(ldk=0), dict(qbs=-8),
       dict(khs=4), dict(ldp=3), dict(pbs=-1), dict(scale=0.0), dict(dtype=2), dict(dtype=3), dict(dtype=-1)]
UNSUP = [dict(head_dim=64), dict(head_dim=32), dict(lk=257, ldp=260), dict(lk=4096, ldp=4096)]


@pytest.mark.parametrize("kw", BAD, ids=lambda kw: "-".join("%s=%s" % i for i in kw.items()))
def test_launcher_rejects_bad_arguments_before_any_launch(lib, kw):
    assert lib.dd_attn_probs(*_args(**kw)) == BAD_ARG


@pytest.mark.parametrize("kw", UNSUP, ids=lambda kw: "-".join("%s=%s" % i for i in kw.items()))
def test_launcher_reports_unsupported_shapes_before_any_launch(lib, kw):
    assert lib.dd_attn_probs(*_args(**kw)) == UNSUPPORTED


def test_launcher_orders_its_checks(lib):
    """A wrong dtype is a bad argument whatever the shape; a prescaled q needs no scale."""
    assert lib.dd_attn_probs(*_args(head_dim=64, dtype=3)) == BAD_ARG
    assert lib.dd_attn_probs(*_args(lk=257, ldp=260, p=None)) == BAD_ARG
    assert lib.dd_attn_probs(*_args(scale=0.0, prescaled=1, head_dim=64)) == UNSUPPORTED


# ---- header, ABI, binding -------------------------------------------------------------------------------------------------

def test_header_declares_and_cites():
    src = open(os.path.join(ROOT, "include", "dualdiff_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+dd_attn_probs\s*\(", code)
    assert "#define DD_ATTN_PROBS_MAX_LK 256" in code
    assert "#define DD_ABI_VERSION 4" in code
    comment = src[:src.index("int dd_attn_probs(")].rsplit("/*", 1)[1]
    assert "tools/unet_modify.py:31,47" in comment
    assert "explore_pipeline_bev_controlnet.py:352-354" in comment


def test_abi_version_and_binding(lib):
    assert lib.dd_abi_version() == _native.ABI_VERSION == 4
    assert lib.dd_desc_size(5) == -1                                    # no new descriptor
    res, args = _native.SIGNATURES["dd_attn_probs"]
    assert res is ctypes.c_int32 and len(args) == 25 and args[-1] is ctypes.c_void_p
    from dualdiff_amd import ops
    assert ops.ATTN_PROBS_MAX_LK == 256


# ---- ops.attention_probs -----------------------------------------------------------------------------------------------------

def test_ops_validates_shapes_without_a_gpu():
    from dualdiff_amd import ops
    q = torch.zeros((2 * 4, 320), dtype=torch.float16)
    k = torch.zeros((2 * 6, 640), dtype=torch.float16)
    with pytest.raises(ValueError, match="q must be"):
        ops.attention_probs(q, k[:, :320], 2, 5, 6, 8, 40)                       # rows do not match batch * lq
    with pytest.raises(ValueError, match="k must be"):
        ops.attention_probs(q, k[:, :160], 2, 4, 6, 8, 40)                       # too narrow for 8 heads of 40
    with pytest.raises(ValueError, match="head-major q"):
        ops.attention_probs(torch.zeros((8, 8, 80), dtype=torch.float16), k[:, :320], 2, 4, 6, 8, 40, q_prescaled=True)
    with pytest.raises(ValueError, match="q is"):
        ops.attention_probs(q, k[:, :320].bfloat16(), 2, 4, 6, 8, 40)
    with pytest.raises(ValueError, match="out must be"):
        ops.attention_probs(q, k[:, :320], 2, 4, 6, 8, 40, out=torch.zeros((2, 4, 7)))
    with pytest.raises(ValueError, match="out must be"):
        ops.attention_probs(q, k[:, :320], 2, 4, 6, 8, 40, per_head=True, out=torch.zeros((2, 4, 6)))
    with pytest.raises(ValueError, match="accumulate needs out"):
        ops.attention_probs(q, k[:, :320], 2, 4, 6, 8, 40, accumulate=True)
    with pytest.raises(ValueError, match="positive"):
        ops.attention_probs(q, k[:, :320], 2, 4, 0, 8, 40)
    with pytest.raises(RuntimeError, match="GPU only"):                          # valid shapes: there is no CPU fallback
        ops.attention_probs(q, k[:, :320], 2, 4, 6, 8, 40)
