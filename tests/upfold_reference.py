"""fp64 references for the folded nearest-upsample conv (dualdiff_amd/upfold.py, dd_gemm2u_kernel), shared by
test_upfold_cpu.py and test_upfold_gpu.py.

`brute_acc` is the definition: F.interpolate(mode="nearest") to the output size, zero border, nine tap matmuls with the
ORIGINAL weights — it knows nothing of classes or slots.  `folded_acc` is what the kernel computes from ITS operands:
per output pixel the 2 x 2 source pixels of its class (zeros outside the source image) times that class's folded matrix.

Fold term: the folded weights are rounded once to the storage type, |w'_r - w'| <= u |w'| (round to nearest, u the unit
roundoff: 2^-11 fp16, 2^-8 bf16), so the two accumulators differ per element by at most u * sum |x| |w'| with w' the exact
fold — `fold_abs` is that sum.
"""
import torch
import torch.nn.functional as F

from dualdiff_amd import upfold

UNIT_ROUNDOFF = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
TAU = 2.0 ** -16                                  # tests/gemm_reference.py: accumulator bound TAU ||a_i|| ||w_j||


def brute_acc(x, w, m, hin, win, hv, wv):
    """(m*hv*wv, cout) fp64: nearest upsample then 3x3 / pad 1 conv; x (m*hin*win, cin), w packed (cout, 9*cin)."""
    cin, cout = x.shape[1], w.shape[0]
    X = x.to(torch.float64).reshape(m, hin, win, cin).permute(0, 3, 1, 2)
    X = F.interpolate(X, size=(hv, wv), mode="nearest").permute(0, 2, 3, 1)
    X = F.pad(X, (0, 0, 1, 1, 1, 1))
    W = w.to(torch.float64).reshape(cout, 3, 3, cin)
    acc = torch.zeros((m, hv, wv, cout), dtype=torch.float64, device=x.device)
    for ky in range(3):
        for kx in range(3):
            acc += X[:, ky:ky + hv, kx:kx + wv, :] @ W[:, ky, kx, :].t()
    return acc.reshape(m * hv * wv, cout)


def folded_acc(x, wf, m, hin, win, hv, wv):
    """What the folded form computes from x and the folded weights wf (ncls * cout, 4 * cin), in fp64.
    Returns (acc (m*hv*wv, cout), TAU * ||2x2 patch_i|| * ||wf_j of the pixel's class||)."""
    ycls, xcls, cls = upfold.classes(hin, win, hv, wv)
    cin = x.shape[1]
    cout = wf.shape[0] // len(cls)
    X = F.pad(x.to(torch.float64).reshape(m, hin, win, cin), (0, 0, 1, 1, 1, 1))       # source s at index s + 1
    WF = wf.to(torch.float64).reshape(len(cls), cout, 4 * cin)
    acc = torch.zeros((m, hv, wv, cout), dtype=torch.float64, device=x.device)
    ea = torch.zeros_like(acc)
    for ci, (rc, cc) in enumerate(cls):
        ys = [o for o in range(hv) if ycls[o] == rc]
        xs = [o for o in range(wv) if xcls[o] == cc]
        # slot 0 of an axis reads s - 1 (classes 0, 2) or s (class 1), slot 1 the next pixel; + 1 for the zero border
        y0 = torch.tensor([upfold.src(o, hin, hv) - (rc != 1) + 1 for o in ys], device=x.device)
        x0 = torch.tensor([upfold.src(o, win, wv) - (cc != 1) + 1 for o in xs], device=x.device)
        patch = torch.cat([X[:, y0 + sy][:, :, x0 + sx] for sy in range(2) for sx in range(2)], dim=-1)   # (m, ny, nx, 4 cin)
        yi = torch.tensor(ys, device=x.device)[:, None]
        xi = torch.tensor(xs, device=x.device)[None, :]
        acc[:, yi, xi] = patch @ WF[ci].t()
        ea[:, yi, xi] = TAU * patch.norm(dim=-1)[..., None] * WF[ci].norm(dim=1)
    return acc.reshape(m * hv * wv, cout), ea.reshape(m * hv * wv, cout)


def fold_abs(x, w, m, hin, win, hv, wv):
    """sum |x| |w'| per output element, w' the exact (fp64) fold of w."""
    wf = upfold.fold_weight(w.to(torch.float64), hin, win, hv, wv, sum_dtype=torch.float64, out_dtype=torch.float64)
    return folded_acc(x.abs(), wf.abs(), m, hin, win, hv, wv)[0]
