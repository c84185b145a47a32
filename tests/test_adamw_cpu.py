"""The fused optimizer step without a GPU: the numpy restatement (tests/adamw_reference.py) against torch.optim.AdamW +
clip_grad_norm_ in float64, its fp32 form and torch's own fp32 path against the derived bounds, planted faults, the
arithmetic core built for the host under the sanitizers (tools/adamw_hostcheck.cpp), and the host side of the interface:
validation, the schedule lambdas, the state dict."""
import ctypes
import math
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

from tests import adamw_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 8192


def lr32(hyper):
    return [np.float32(hyper["lr"])]


@pytest.fixture(scope="module")
def fix():
    return R.fixture(CHUNK)


def test_chunk_is_the_headers():
    from dualdiff_amd import ops
    hdr = open(os.path.join(ROOT, "include", "dualdiff_hip.h")).read()
    assert int(re.search(r"#define DD_ADAMW_CHUNK (\d+)", hdr).group(1)) == ops.adamw_chunk() == CHUNK
    assert CHUNK % (4 * R.THREADS) == 0
    assert R.numels(CHUNK) == [1, 3, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5, 0, 37]


# ---- (a) the float64 form is torch's ------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(R.HYPERS))
def test_float64_form_is_torch_adamw_with_clip(fix, name):
    """Four steps of torch.optim.AdamW(foreach=False) + clip_grad_norm_ on float64 CPU parameters against four steps of
    the float64 form, each from its own state.  Allowed per step: float64 re-association (the running beta products
    against beta ** step, (w2 g) g against w2 (g g), a dozen roundings: 16 x 2^-53), plus three times the relative error of
    torch's own norm — it sums 50 000 squares naively in two levels, and its coefficient enters g once, v twice — which is
    measured against math.fsum.  Both are relative to the magnitudes that ENTER each element (|m| + sum |gc|, v + sum gc^2,
    |p| + sum step_size (|m| + sum |gc|) / den): m cancels, so its own size is no scale."""
    hyper = R.HYPERS[name]
    state, grads = fix
    lr = float(np.float32(hyper["lr"]))
    params = [torch.tensor(p.astype(np.float64), requires_grad=True) for p in state["p"]]
    opt = torch.optim.AdamW(params, lr=lr, betas=hyper["betas"], eps=hyper["eps"], weight_decay=hyper["weight_decay"],
                            foreach=False)
    ours = R.copy_state(state)
    ours["p"] = [p.astype(np.float64) for p in ours["p"]]
    ours["m"] = [np.zeros_like(p) for p in ours["p"]]
    ours["v"] = [np.zeros_like(p) for p in ours["p"]]
    worst, largest, tol = 0.0, 0.0, 0.0
    sm = [np.zeros_like(p) for p in ours["p"]]
    sv = [np.zeros_like(p) for p in ours["p"]]
    sp = [np.zeros_like(p) for p in ours["p"]]
    for k, gs in enumerate(grads):
        for p, g in zip(params, gs):
            p.grad = None if g is None else torch.tensor(g.astype(np.float64))
        total = float(torch.nn.utils.clip_grad_norm_(params, hyper["max_grad_norm"]))
        opt.step()
        ours, s = R.step(ours, gs, hyper, lr32(hyper), form="float64")
        tol += 16 * 2.0 ** -53 + 3 * abs(total - s["grad_norm"]) / s["grad_norm"]
        for i, (p, g) in enumerate(zip(params, gs)):
            if g is None:
                assert np.array_equal(p.detach().numpy(), ours["p"][i]) and len(opt.state[p]) == 0
                continue
            gc = np.abs(g.astype(np.float64)) * s["clip_coef"]
            sm[i] += gc
            sv[i] += gc * gc
            sp[i] += s["step_size"] * (np.abs(ours["m"][i]) + sm[i]) / (np.sqrt(ours["v"][i]) / s["bc2_sqrt"] + s["eps"])
            for got, want, scale in ((opt.state[p]["exp_avg"].numpy(), ours["m"][i], sm[i]),
                                     (opt.state[p]["exp_avg_sq"].numpy(), ours["v"][i], sv[i]),
                                     (p.detach().numpy(), ours["p"][i], sp[i])):
                if got.size:
                    worst = max(worst, float((np.abs(got - want) / (tol * (np.abs(want) + scale))).max()))
                    largest = max(largest, float(np.abs(got - want).max()))
            assert float(opt.state[p]["step"]) == ours["step"] == k + 1
    print("float64 form against torch, %s: worst difference / allowed = %.3g (allowed %.3g relative), largest difference %.3g"
          % (name, worst, tol, largest))
    assert tol < 1e-13 and worst < 1.0


# ---- (b), (c) the fp32 forms stay inside the bounds ------------------------------------------------------------------------

def ratios(before, after32, after64, gs, s64, clip_rel=R.U, inv_scale=1.0):
    worst = 0.0
    for i, g in enumerate(gs):
        if g is None:
            for a in "pmv":
                assert np.array_equal(after32[a][i], before[a][i])
            continue
        row = {a: before[a][i] for a in "pmv"}
        for a, bound in zip("mvp", R.bounds(row, g, s64, inv_scale=inv_scale, clip_rel=clip_rel)):
            worst = max(worst, R.worst_ratio(after32[a][i], after64[a][i], bound))
    return worst


@pytest.mark.parametrize("name", sorted(R.HYPERS))
def test_fp32_form_within_bounds(fix, name):
    hyper = R.HYPERS[name]
    state, grads = fix
    s32, worst = R.copy_state(state), 0.0
    for gs in grads:
        n32, sc = R.step(s32, gs, hyper, lr32(hyper))
        n64, s64 = R.step(s32, gs, hyper, lr32(hyper), form="float64")
        n = sum(g.size for g in gs if g is not None)
        en, ec, rel = R.scalar_bounds(n, s64["grad_norm"], s64["clip_coef"], hyper["max_grad_norm"])
        assert abs(float(sc["grad_norm"]) - s64["grad_norm"]) <= en and abs(float(sc["clip_coef"]) - s64["clip_coef"]) <= ec
        worst = max(worst, ratios(s32, n32, n64, gs, s64, clip_rel=rel))
        s32 = n32
    print("fp32 form against the float64 form, %s: worst error / bound = %.3f" % (name, worst))
    assert 0.0 < worst < 1.0


@pytest.mark.parametrize("name", sorted(R.HYPERS))
def test_torch_fp32_path_within_bounds(fix, name):
    """torch's own fp32 CPU path (vectorised lerp and addcmul: not our bits) against the float64 form from torch's state,
    with the coefficient torch applied (its fp32 norm is not under test)."""
    hyper = R.HYPERS[name]
    state, grads = fix
    lr = float(np.float32(hyper["lr"]))
    params = [torch.tensor(p, requires_grad=True) for p in state["p"]]
    opt = torch.optim.AdamW(params, lr=lr, betas=hyper["betas"], eps=hyper["eps"], weight_decay=hyper["weight_decay"],
                            foreach=False)
    ours, worst = R.copy_state(state), 0.0
    for k, gs in enumerate(grads):
        for p, g in zip(params, gs):
            p.grad = None if g is None else torch.tensor(g)
        total = torch.nn.utils.clip_grad_norm_(params, hyper["max_grad_norm"])
        coef = float(torch.clamp(hyper["max_grad_norm"] / (total + 1e-6), max=1.0))
        opt.step()
        ours["step"], ours["b1p"], ours["b2p"] = k + 1, ours["b1p"] * hyper["betas"][0], ours["b2p"] * hyper["betas"][1]
        s64 = R.scalars64(0.0, ours["b1p"], ours["b2p"], lr, hyper)
        s64["clip_coef"] = coef
        after32, after64 = R.copy_state(ours), R.copy_state(ours)
        for i, (p, g) in enumerate(zip(params, gs)):
            if g is None:
                continue
            after32["p"][i], after32["m"][i], after32["v"][i] = (p.detach().numpy().copy(), opt.state[p]["exp_avg"].numpy().copy(),
                                                                 opt.state[p]["exp_avg_sq"].numpy().copy())
            after64["p"][i], after64["m"][i], after64["v"][i] = R.update64(ours["p"][i], g, ours["m"][i], ours["v"][i], s64, 1.0)
        worst = max(worst, ratios(ours, after32, after64, gs, s64, clip_rel=0.0))
        ours = after32
    print("torch's fp32 path against the float64 form, %s: worst error / bound = %.3f" % (name, worst))
    assert 0.0 < worst < 1.0


# ---- (d) planted faults --------------------------------------------------------------------------------------------------

def conditions(state, grads, hyper, fault):
    """The conditions the kernels are held to on the GPU, applied to the fp32 form with a fault planted -> the failures"""
    failed = []
    s32 = R.copy_state(state)
    for k, gs in enumerate(grads):
        n32, _ = R.step(s32, gs, hyper, lr32(hyper), fault=fault)
        n64, s64 = R.step(s32, gs, hyper, lr32(hyper), form="float64")
        n = sum(g.size for g in gs if g is not None)
        w = ratios(s32, n32, n64, gs, s64, clip_rel=R.scalar_bounds(n, s64["grad_norm"], s64["clip_coef"], 1.0)[2])
        if not w < 1.0:
            failed.append("step %d outside the bounds (%.3g)" % (k + 1, w))
        s32 = n32
    # a skipped step leaves everything but found_inf and skipped alone, and the next one is as if it had not happened
    bad = [None if g is None else g.copy() for g in grads[0]]
    bad[-3][-1] = np.inf
    s1, _ = R.step(state, bad, hyper, lr32(hyper), fault=fault)
    if (s1["step"], s1["skipped"], s1["found_inf"]) != (state["step"], state["skipped"] + 1, 1):
        failed.append("the skipped step counts")
    if any(not np.array_equal(s1[a][i], state[a][i]) for a in "pmv" for i in range(len(state["p"]))):
        failed.append("the skipped step wrote")
    s2, _ = R.step(s1, grads[0], hyper, lr32(hyper), fault=fault)
    ref, s64 = R.step(state, grads[0], hyper, lr32(hyper), form="float64")
    if not ratios(state, s2, ref, grads[0], s64) < 1.0:
        failed.append("the step after a skipped one differs")
    return failed


@pytest.mark.parametrize("name", sorted(R.HYPERS))
def test_planted_faults_are_seen(fix, name):
    state, grads = fix
    assert conditions(state, grads, R.HYPERS[name], None) == []
    for fault in R.FAULTS:
        failed = conditions(state, grads, R.HYPERS[name], fault)
        print("%s, %s: %s" % (name, fault, "; ".join(failed)))
        assert failed, fault


# ---- (e) the core on the host, under the sanitizers ------------------------------------------------------------------------

@pytest.fixture(scope="module")
def hostcheck(tmp_path_factory):
    """(the program built under the sanitizers, None) or (None, why not): built once for the module"""
    tmp = str(tmp_path_factory.mktemp("adamw_hc"))
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        return None, "no C++ compiler"
    flags = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    probe = os.path.join(tmp, "probe.cpp")
    with open(probe, "w") as f:
        f.write("int main() { return 0; }\n")
    for static in (["-static-libasan", "-static-libubsan"], []):
        if subprocess.run([cxx] + flags + static + [probe, "-o", os.path.join(tmp, "probe")], capture_output=True).returncode == 0:
            break
    else:
        return None, "the compiler links no sanitizer runtime"
    exe = os.path.join(tmp, "adamw_hostcheck")
    build = subprocess.run([cxx] + flags + static + ["-I", os.path.join(ROOT, "dualdiff_amd", "csrc"),
                            os.path.join(ROOT, "tools", "adamw_hostcheck.cpp"), "-o", exe, "-lm"],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    return exe, None


def bits64(v):
    return struct.unpack("<Q", struct.pack("<d", v))[0]


def hostcheck_input(state, gs, hyper, lr_table, bf16, grad_scale, found_inf_in):
    words = [CHUNK, len(state["p"]), int(bf16), len(lr_table), int(grad_scale is not None), int(found_inf_in)]
    words += [bits64(v) for v in (hyper["betas"][0], hyper["betas"][1], hyper["eps"], hyper["weight_decay"],
                                  -1.0 if hyper["max_grad_norm"] is None else hyper["max_grad_norm"], state["b1p"], state["b2p"])]
    words += [state["step"], state["skipped"]]
    words += np.asarray(lr_table, np.float32).view(np.uint32).tolist()
    words.append(int(np.float32(1.0 if grad_scale is None else grad_scale).view(np.uint32)))
    out = [" ".join(str(w) for w in words)]
    for i, g in enumerate(gs):
        cols = [state["p"][i]] + ([] if g is None else [g]) + [state["m"][i], state["v"][i]]
        out.append("%d %d" % (state["p"][i].size, g is not None))
        out.append(" ".join(map(str, np.stack(cols, 1).view(np.uint32).reshape(-1).tolist())))
    return "\n".join(out) + "\n"


def run_hostcheck(exe, state, gs, hyper, lr_table, bf16=False, grad_scale=None, found_inf_in=False):
    run = subprocess.run([exe], input=hostcheck_input(state, gs, hyper, lr_table, bf16, grad_scale, found_inf_in),
                         capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    lines = run.stdout.split("\n")[:-1]
    assert len(lines) == 1 + 4 * len(gs)
    head = lines[0].split()
    got = dict(step=int(head[1]), skipped=int(head[2]), found_inf=int(head[3]),
               b1p=struct.unpack("<d", struct.pack("<Q", int(head[4], 16)))[0],
               b2p=struct.unpack("<d", struct.pack("<Q", int(head[5], 16)))[0], p=[], m=[], v=[], s=[])
    scal = np.array([int(w, 16) for w in head[6:]], np.uint32).view(np.float32)
    for i in range(len(gs)):
        for k, a in enumerate("pmv"):
            got[a].append(np.array([int(w, 16) for w in lines[1 + 4 * i + k].split()[1:]], np.uint32).view(np.float32))
        got["s"].append(np.array([int(w, 16) for w in lines[4 + 4 * i].split()[1:]], np.uint16))
    return got, dict(zip(("grad_norm",) + R.SCALAR_NAMES, scal))


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("name", sorted(R.HYPERS))
def test_core_on_the_host_under_sanitizers(fix, name, hostcheck):
    """tools/adamw_hostcheck.cpp, built with -fsanitize=address,undefined as its own program: csrc/adamw_core.h in the
    kernels' chunk order gives the fp32 form's bits — state, scalars, p, m, v and both shadows — over four steps, a scaled
    step, a step with an infinity and one the scaler marks, and runs clean"""
    exe, why = hostcheck
    if exe is None:
        pytest.skip(why)
    hyper = R.HYPERS[name]
    state, grads = fix
    table = [np.float32(0.0), np.float32(hyper["lr"]), np.float32(hyper["lr"] / 2)]       # step 1 at lr 0, steps 3+ past the end
    bad = [None if g is None else g.copy() for g in grads[0]]
    bad[-3][-1] = np.inf
    scaled = [None if g is None else g * np.float32(65536.0) for g in grads[1]]
    runs = [(gs, {}) for gs in grads] + [(scaled, dict(grad_scale=65536.0)), (bad, {}), (grads[0], dict(found_inf_in=True))]
    s32 = R.copy_state(state)
    for k, (gs, kw) in enumerate(runs):
        want, sc = R.step(s32, gs, hyper, table, **kw)
        got, scal = run_hostcheck(exe, s32, gs, hyper, table, bf16=k % 2 == 1, **kw)
        assert (got["step"], got["skipped"], got["found_inf"]) == (want["step"], want["skipped"], want["found_inf"]), k
        assert (got["b1p"], got["b2p"]) == (want["b1p"], want["b2p"]), k
        if sc is not None:
            for key in ("grad_norm",) + R.SCALAR_NAMES:
                assert np.float32(scal[key]).view(np.uint32) == np.float32(sc[key]).view(np.uint32), (k, key)
        for i in range(len(gs)):
            for a in "pmv":
                assert same_bits(got[a][i], want[a][i]), (k, a, i)
            assert np.array_equal(got["s"][i], R.shadow_bits(want["p"][i], "bf16" if k % 2 == 1 else "fp16")), (k, i)
        s32 = want
    assert s32["step"] == 5 and s32["skipped"] == 2


def test_host_shadow_rounding_at_the_edges(hostcheck):
    """the host's fp16 / bf16 rounding (the device uses the hardware conversion for fp16) at ties, subnormals, overflow"""
    exe, why = hostcheck
    if exe is None:
        pytest.skip(why)
    f16 = np.arange(0, 0x7C00, 7, dtype=np.uint16).view(np.float16).astype(np.float32)
    ties = (f16[:-1].astype(np.float64) + f16[1:].astype(np.float64)) / 2                # exact midpoints are fp32 values
    vals = np.concatenate([f16, ties.astype(np.float32), np.float32([65504, 65519.99, 65520, 1e30, 2.0 ** -25, 2.0 ** -25 * 1.0001,
                                                                     2.0 ** -24, 5.9e-8, 0.0, 1e-40, np.inf])])
    vals = np.concatenate([vals, -vals]).astype(np.float32)
    hyper = dict(R.DEFAULTS, weight_decay=0.0)
    for bf16 in (False, True):
        state = R.new_state([vals])
        state["m"][0][:] = 0.0
        # lr 0 and no decay: p keeps its bits, the shadow is the rounding of p
        got, _ = run_hostcheck(exe, state, [np.zeros_like(vals)], hyper, [np.float32(0.0)], bf16=bf16)
        assert same_bits(got["p"][0], vals)
        assert np.array_equal(got["s"][0], R.shadow_bits(vals, "bf16" if bf16 else "fp16"))
    want = torch.tensor(vals).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(R.shadow_bits(vals, "bf16"), want)


# ---- (f) the host side of the interface ---------------------------------------------------------------------------------

P = ctypes.c_void_p(4096)


def test_entry_point_validates_before_any_launch():
    from dualdiff_amd import _build, _native
    if not os.path.exists(_build.lib_path()):
        pytest.skip("library not built")
    lib = _native.load(build_if_missing=False)
    assert lib.dd_adamw_workspace_bytes(0) == 12 and lib.dd_adamw_workspace_bytes(10) == 120
    assert lib.dd_adamw_workspace_bytes(-1) == -1 and lib.dd_adamw_workspace_bytes(2 ** 31) == -1

    def call(**kw):
        a = dict(rows=P, n_rows=3, chunks=P, n_chunks=5, state=P, lr=P, lr_len=1, scale=None, inf=None, b1=0.9, b2=0.999,
                 eps=1e-8, wd=1e-2, max_norm=1.0, sdt=0, ws=P, ws_bytes=60, launches=7)
        a.update(kw)
        return lib.dd_adamw_step(*(list(a.values()) + [None]))
    for kw in (dict(state=None), dict(lr=None), dict(ws=None), dict(rows=None), dict(chunks=None), dict(n_rows=-1),
               dict(n_chunks=-1), dict(lr_len=0), dict(b1=1.0), dict(b2=-0.1), dict(eps=-1.0), dict(eps=float("inf")),
               dict(wd=float("nan")), dict(max_norm=float("nan")), dict(sdt=2), dict(launches=0), dict(launches=8),
               dict(ws_bytes=59), dict(state=ctypes.c_void_p(4100)), dict(scale=ctypes.c_void_p(4098)),
               dict(rows=ctypes.c_void_p(4100)), dict(ws=ctypes.c_void_p(4100))):
        assert call(**kw) == -1, kw


def rows_ok(n=3):
    ps = [torch.zeros(4, 5) for _ in range(n)]
    return [(p, torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p), torch.zeros(4, 5, dtype=torch.float16)) for p in ps]


def test_table_validation_names_the_row():
    from dualdiff_amd import ops

    def broken(at, which, value):
        rows = rows_ok()
        row = list(rows[at])
        row[which] = value
        rows[at] = tuple(row)
        return rows
    with pytest.raises(TypeError, match="row 1: g must be an fp32 tensor"):
        ops.adamw_table(broken(1, 1, torch.zeros(4, 5, dtype=torch.float16)))
    with pytest.raises(TypeError, match="row 2: p must be an fp32 tensor"):
        ops.adamw_table(broken(2, 0, torch.zeros(4, 5, dtype=torch.float64)))
    with pytest.raises(TypeError, match="row 0: the shadow must be an fp16 or bf16"):
        ops.adamw_table(broken(0, 4, torch.zeros(4, 5)))
    with pytest.raises(TypeError, match="row 2: the shadow is torch.bfloat16"):
        ops.adamw_table(broken(2, 4, torch.zeros(4, 5, dtype=torch.bfloat16)))
    with pytest.raises(ValueError, match=r"row 1: v has shape \(5, 4\)"):
        ops.adamw_table(broken(1, 3, torch.zeros(5, 4)))
    with pytest.raises(ValueError, match="row 2: m is not contiguous"):
        ops.adamw_table(broken(2, 2, torch.zeros(5, 4).t()))
    with pytest.raises(ValueError, match="row 0 is not"):
        ops.adamw_table([(torch.zeros(1),)])
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.adamw_table(rows_ok())
    rows = rows_ok()
    rows[1] = (rows[1][0], None, rows[1][2], rows[1][3], None)                           # no gradient, no shadow: legal
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.adamw_table(rows)
    assert ops.adamw_chunks([1, 0, CHUNK, CHUNK + 1]).tolist() == [[0, 0], [2, 0], [3, 0], [3, 1]]
    assert ops.adamw_chunks([]).shape == (0, 2) and ops.adamw_chunks([0, 0]).shape == (0, 2)
    blk = ops.adamw_state(3, (0.9, 0.999), skipped=2)
    assert blk.numel() == 96 and int(ops.adamw_state_field(blk, "step")) == 3 and int(ops.adamw_state_field(blk, "skipped")) == 2
    assert float(ops.adamw_state_field(blk, "beta1_pow")) == 0.9 ** 3 and float(ops.adamw_state_field(blk, "beta2_pow")) == 0.999 ** 3


def test_optimizer_refuses_by_name():
    from dualdiff_amd.pipeline import FusedAdamW
    p = [torch.zeros(3, requires_grad=True), torch.zeros(2, requires_grad=True)]
    for name in ("amsgrad", "maximize", "use_8bit_adam"):
        with pytest.raises(ValueError, match=name):
            FusedAdamW(p, **{name: True})
        FusedAdamW(p, **{name: False})
    with pytest.raises(TypeError, match="unknown argument 'nesterov'"):
        FusedAdamW(p, nesterov=True)
    with pytest.raises(ValueError, match="different hyper-parameters.*weight_decay"):
        FusedAdamW([dict(params=p[:1]), dict(params=p[1:], weight_decay=0.0)])
    FusedAdamW([dict(params=p[:1]), dict(params=p[1:])])                                  # equal groups are one table
    with pytest.raises(ValueError, match="not a parameter"):
        FusedAdamW(p, shadows={torch.zeros(3): torch.zeros(3, dtype=torch.float16)})
    opt = FusedAdamW(p)
    assert opt._step_supports_amp_scaling and opt.defaults["lr"] == 8e-5 and opt.defaults["weight_decay"] == 1e-2
    with pytest.raises(RuntimeError, match="GPU only"):
        opt.step()
    opt.found_inf = torch.ones(())                                                       # what GradScaler.step does
    del opt.found_inf
    assert int(opt.found_inf) == 0 and opt.steps_taken.dtype == torch.int64 and opt.grad_norm.dtype == torch.float32


def test_lr_lambdas_at_hand_computed_points():
    from dualdiff_amd.pipeline import optim
    assert [optim.constant()(k) for k in (0, 7, 10 ** 6)] == [1.0, 1.0, 1.0]
    w = optim.constant_with_warmup(4)
    assert [w(k) for k in (0, 1, 3, 4, 9)] == [0.0, 0.25, 0.75, 1.0, 1.0]
    assert optim.constant_with_warmup(0)(0) == 1.0
    c = optim.cosine(2, 10)                                 # half a cosine over the 8 steps after the warm-up
    assert [c(0), c(1), c(2)] == [0.0, 0.5, 1.0]
    assert c(6) == pytest.approx(0.5, abs=1e-15) and c(4) == pytest.approx(0.5 * (1 + math.sqrt(0.5)), abs=1e-15)
    assert c(10) == pytest.approx(0.0, abs=1e-15) and c(8) == pytest.approx(0.5 * (1 - math.sqrt(0.5)), abs=1e-15)
    full = optim.cosine(0, 8, lr_num_cycles=1)              # a whole period: back at 1 at the end
    assert full(0) == 1.0 and full(4) == pytest.approx(0.0, abs=1e-15) and full(8) == pytest.approx(1.0, abs=1e-15)
    t = optim.lr_table(8e-5, c, 4)
    assert t.dtype == torch.float32 and t.tolist() == [0.0, float(np.float32(4e-5)), float(np.float32(8e-5)), float(np.float32(8e-5 * c(3)))]
    with pytest.raises(ValueError):
        optim.lr_table(8e-5, c, 0)


def test_state_dict_round_trip_with_torch_adamw():
    from dualdiff_amd import ops
    from dualdiff_amd.pipeline import FusedAdamW
    torch.manual_seed(0)
    ps = [torch.randn(5, requires_grad=True), torch.randn(3, 4, requires_grad=True)]
    ref = torch.optim.AdamW(ps, lr=1e-3, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.05)
    for _ in range(2):
        for p in ps:
            p.grad = torch.randn_like(p)
        ref.step()
    sd = ref.state_dict()
    ours = FusedAdamW([p.detach().clone() for p in ps])
    ours.load_state_dict(sd)
    g = ours.param_groups[0]
    assert (g["lr"], tuple(g["betas"]), g["eps"], g["weight_decay"]) == (1e-3, (0.8, 0.99), 1e-6, 0.05)
    assert int(ours.steps_taken) == 2 and int(ours.skipped) == 0
    assert float(ops.adamw_state_field(ours._state_block, "beta1_pow")) == 0.8 ** 2
    assert float(ops.adamw_state_field(ours._state_block, "beta2_pow")) == 0.99 ** 2
    back = ours.state_dict()
    assert back["param_groups"][0].keys() == sd["param_groups"][0].keys()
    for k, st in sd["state"].items():
        assert float(back["state"][k]["step"]) == 2.0
        for key in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(back["state"][k][key], st[key]) and back["state"][k][key].dtype == torch.float32
    again = torch.optim.AdamW(ps, lr=1.0)
    again.load_state_dict(back)                              # ours loads into torch's
    for p in ps:
        assert float(again.state[p]["step"]) == 2.0 and torch.equal(again.state[p]["exp_avg"], ref.state[p]["exp_avg"])
    assert again.param_groups[0]["lr"] == 1e-3
    # steps that disagree have no place in one count
    sd["state"][1]["step"] = torch.tensor(5.0)
    with pytest.raises(ValueError, match="different numbers of steps"):
        FusedAdamW([p.detach().clone() for p in ps]).load_state_dict(sd)
    sd["param_groups"][0]["amsgrad"] = True
    with pytest.raises(ValueError, match="amsgrad"):
        FusedAdamW([p.detach().clone() for p in ps]).load_state_dict(sd)
