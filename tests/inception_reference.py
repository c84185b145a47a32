"""Restatement of the FID InceptionV3 (pytorch-fid's network, the reference's magicdrive/misc/inception.py) in plain
torch.nn, and the float64 references of the four kernels of csrc/conv2d.hip.

PARITY IS UNPINNED: torchvision and the pt_inception-2015-12-05 weights are not available here, so this file cannot be
run against the network it restates.  It is written from the architecture table of the issue that introduced it (every
BasicConv2d is conv without bias -> BatchNorm2d(eps=1e-3) in eval -> ReLU; blocks A / B / C / D / E with the FID
patches: exclusive average pools, max pool in Mixed_7c) and keeps pytorch-fid's parameter names, so that a real
checkpoint loads into it unchanged.  What the tests hold the HIP path to is THIS restatement in float64.

Seeded weights: conv ~ N(0, 2 / fan_in) (rounded to bf16, which fp16 holds exactly at that size, so that both storage
types and the float64 run read the same numbers); BatchNorm gamma in [0.8, 1.2], beta and running mean in [-0.1, 0.1],
running variance in [0.5, 1.5].  With these the signal neither dies nor explodes through the 94 ReLU layers
(tests/test_fid_cpu.py checks that).

Kernel references: computed in float64 from the SAME 16-bit operands the kernel reads.  The conv is tap-by-tap float64
matmuls over a zero-padded NHWC tensor (no F.conv2d), returning (acc, E_acc) in tests/gemm_reference.py's form.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import gemm_reference as G

BLOCK_INDEX_BY_DIM = {64: 0, 192: 1, 768: 2, 2048: 3}


def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


class BasicConv2d(nn.Module):
    def __init__(self, cin, cout, kernel_size, stride=1, padding=0):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, kernel_size, stride=stride, padding=padding, bias=False)
        self.bn = nn.BatchNorm2d(cout, eps=1e-3)

    def forward(self, x):
        return F.relu(self.bn(self.conv(x)))


def _avg(x):
    return F.avg_pool2d(x, 3, stride=1, padding=1, count_include_pad=False)


class InceptionA(nn.Module):
    def __init__(self, cin, pf):
        super().__init__()
        self.branch1x1 = BasicConv2d(cin, 64, 1)
        self.branch5x5_1 = BasicConv2d(cin, 48, 1)
        self.branch5x5_2 = BasicConv2d(48, 64, 5, padding=2)
        self.branch3x3dbl_1 = BasicConv2d(cin, 64, 1)
        self.branch3x3dbl_2 = BasicConv2d(64, 96, 3, padding=1)
        self.branch3x3dbl_3 = BasicConv2d(96, 96, 3, padding=1)
        self.branch_pool = BasicConv2d(cin, pf, 1)

    def forward(self, x):
        return torch.cat([self.branch1x1(x), self.branch5x5_2(self.branch5x5_1(x)),
                          self.branch3x3dbl_3(self.branch3x3dbl_2(self.branch3x3dbl_1(x))),
                          self.branch_pool(_avg(x))], 1)


class InceptionB(nn.Module):
    def __init__(self, cin):
        super().__init__()
        self.branch3x3 = BasicConv2d(cin, 384, 3, stride=2)
        self.branch3x3dbl_1 = BasicConv2d(cin, 64, 1)
        self.branch3x3dbl_2 = BasicConv2d(64, 96, 3, padding=1)
        self.branch3x3dbl_3 = BasicConv2d(96, 96, 3, stride=2)

    def forward(self, x):
        return torch.cat([self.branch3x3(x), self.branch3x3dbl_3(self.branch3x3dbl_2(self.branch3x3dbl_1(x))),
                          F.max_pool2d(x, 3, stride=2)], 1)


class InceptionC(nn.Module):
    def __init__(self, cin, c):
        super().__init__()
        self.branch1x1 = BasicConv2d(cin, 192, 1)
        self.branch7x7_1 = BasicConv2d(cin, c, 1)
        self.branch7x7_2 = BasicConv2d(c, c, (1, 7), padding=(0, 3))
        self.branch7x7_3 = BasicConv2d(c, 192, (7, 1), padding=(3, 0))
        self.branch7x7dbl_1 = BasicConv2d(cin, c, 1)
        self.branch7x7dbl_2 = BasicConv2d(c, c, (7, 1), padding=(3, 0))
        self.branch7x7dbl_3 = BasicConv2d(c, c, (1, 7), padding=(0, 3))
        self.branch7x7dbl_4 = BasicConv2d(c, c, (7, 1), padding=(3, 0))
        self.branch7x7dbl_5 = BasicConv2d(c, 192, (1, 7), padding=(0, 3))
        self.branch_pool = BasicConv2d(cin, 192, 1)

    def forward(self, x):
        b7 = self.branch7x7_3(self.branch7x7_2(self.branch7x7_1(x)))
        bd = self.branch7x7dbl_1(x)
        for name in ("branch7x7dbl_2", "branch7x7dbl_3", "branch7x7dbl_4", "branch7x7dbl_5"):
            bd = getattr(self, name)(bd)
        return torch.cat([self.branch1x1(x), b7, bd, self.branch_pool(_avg(x))], 1)


class InceptionD(nn.Module):
    def __init__(self, cin):
        super().__init__()
        self.branch3x3_1 = BasicConv2d(cin, 192, 1)
        self.branch3x3_2 = BasicConv2d(192, 320, 3, stride=2)
        self.branch7x7x3_1 = BasicConv2d(cin, 192, 1)
        self.branch7x7x3_2 = BasicConv2d(192, 192, (1, 7), padding=(0, 3))
        self.branch7x7x3_3 = BasicConv2d(192, 192, (7, 1), padding=(3, 0))
        self.branch7x7x3_4 = BasicConv2d(192, 192, 3, stride=2)

    def forward(self, x):
        b7 = self.branch7x7x3_1(x)
        for name in ("branch7x7x3_2", "branch7x7x3_3", "branch7x7x3_4"):
            b7 = getattr(self, name)(b7)
        return torch.cat([self.branch3x3_2(self.branch3x3_1(x)), b7, F.max_pool2d(x, 3, stride=2)], 1)


class InceptionE(nn.Module):
    def __init__(self, cin, pool):
        super().__init__()
        self.pool = pool                        # "avg": exclusive average (Mixed_7b); "max" (Mixed_7c)
        self.branch1x1 = BasicConv2d(cin, 320, 1)
        self.branch3x3_1 = BasicConv2d(cin, 384, 1)
        self.branch3x3_2a = BasicConv2d(384, 384, (1, 3), padding=(0, 1))
        self.branch3x3_2b = BasicConv2d(384, 384, (3, 1), padding=(1, 0))
        self.branch3x3dbl_1 = BasicConv2d(cin, 448, 1)
        self.branch3x3dbl_2 = BasicConv2d(448, 384, 3, padding=1)
        self.branch3x3dbl_3a = BasicConv2d(384, 384, (1, 3), padding=(0, 1))
        self.branch3x3dbl_3b = BasicConv2d(384, 384, (3, 1), padding=(1, 0))
        self.branch_pool = BasicConv2d(cin, 192, 1)

    def forward(self, x):
        b3 = self.branch3x3_1(x)
        bd = self.branch3x3dbl_2(self.branch3x3dbl_1(x))
        p = _avg(x) if self.pool == "avg" else F.max_pool2d(x, 3, stride=1, padding=1)
        return torch.cat([self.branch1x1(x), self.branch3x3_2a(b3), self.branch3x3_2b(b3), self.branch3x3dbl_3a(bd),
                          self.branch3x3dbl_3b(bd), self.branch_pool(p)], 1)


class InceptionV3(nn.Module):
    """forward(inp): inp (m, 3, h, w) in [0, 1] -> the feature maps of `output_blocks`, as pytorch-fid returns them."""

    def __init__(self, output_blocks=(3,), resize_input=True, normalize_input=True):
        super().__init__()
        self.output_blocks = sorted(output_blocks)
        self.resize_input, self.normalize_input = resize_input, normalize_input
        self.Conv2d_1a_3x3 = BasicConv2d(3, 32, 3, stride=2)
        self.Conv2d_2a_3x3 = BasicConv2d(32, 32, 3)
        self.Conv2d_2b_3x3 = BasicConv2d(32, 64, 3, padding=1)
        self.Conv2d_3b_1x1 = BasicConv2d(64, 80, 1)
        self.Conv2d_4a_3x3 = BasicConv2d(80, 192, 3)
        self.Mixed_5b = InceptionA(192, 32)
        self.Mixed_5c = InceptionA(256, 64)
        self.Mixed_5d = InceptionA(288, 64)
        self.Mixed_6a = InceptionB(288)
        self.Mixed_6b = InceptionC(768, 128)
        self.Mixed_6c = InceptionC(768, 160)
        self.Mixed_6d = InceptionC(768, 160)
        self.Mixed_6e = InceptionC(768, 192)
        self.Mixed_7a = InceptionD(768)
        self.Mixed_7b = InceptionE(1280, "avg")
        self.Mixed_7c = InceptionE(2048, "max")

    def forward(self, x):
        outs = []
        last = max(self.output_blocks)
        if self.resize_input:
            x = F.interpolate(x, size=(299, 299), mode="bilinear", align_corners=False)
        if self.normalize_input:
            x = 2 * x - 1
        x = self.Conv2d_2b_3x3(self.Conv2d_2a_3x3(self.Conv2d_1a_3x3(x)))
        x = F.max_pool2d(x, 3, stride=2)
        if 0 in self.output_blocks:
            outs.append(x)
        if last >= 1:
            x = F.max_pool2d(self.Conv2d_4a_3x3(self.Conv2d_3b_1x1(x)), 3, stride=2)
            if 1 in self.output_blocks:
                outs.append(x)
        if last >= 2:
            for name in ("Mixed_5b", "Mixed_5c", "Mixed_5d", "Mixed_6a", "Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"):
                x = getattr(self, name)(x)
            if 2 in self.output_blocks:
                outs.append(x)
        if last >= 3:
            x = self.Mixed_7c(self.Mixed_7b(self.Mixed_7a(x)))
            outs.append(F.adaptive_avg_pool2d(x, 1))
        return outs

    def features(self, x, dims=2048):
        saved, self.output_blocks = self.output_blocks, [BLOCK_INDEX_BY_DIM[dims]]
        try:
            return F.adaptive_avg_pool2d(self.forward(x)[0], 1).flatten(1)
        finally:
            self.output_blocks = saved


def seeded_state_dict(seed=0):
    """The state dict of InceptionV3 under the module docstring's initialiser (fp32 tensors, pytorch-fid key names)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}

    def uni(n, lo, hi):
        return lo + (hi - lo) * torch.rand(n, generator=g)

    for name, mod in InceptionV3().named_modules():
        if isinstance(mod, BasicConv2d):
            w = mod.conv.weight
            fan_in = w.shape[1] * w.shape[2] * w.shape[3]
            wv = torch.randn(w.shape, generator=g) * (2.0 / fan_in) ** 0.5
            sd[name + ".conv.weight"] = wv.to(torch.bfloat16).to(torch.float32)
            n = w.shape[0]
            sd[name + ".bn.weight"] = uni(n, 0.8, 1.2)
            sd[name + ".bn.bias"] = uni(n, -0.1, 0.1)
            sd[name + ".bn.running_mean"] = uni(n, -0.1, 0.1)
            sd[name + ".bn.running_var"] = uni(n, 0.5, 1.5)
            sd[name + ".bn.num_batches_tracked"] = torch.tensor(0)
    return sd


def seeded_images(shape, seed):
    """(m, 3, h, w) in [0, 1], multiples of 1 / 255 (what ToTensor yields), smooth enough to have structure."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, shape, generator=g).to(torch.float32) / 255.0


# The two whole-network cases of tests/test_inception_gpu.py (their liveness is checked in tests/test_fid_cpu.py):
# resize_input, image shape, image seed.  75 x 91 is the smallest input that survives to Mixed_7c without the resize
# (75 -> 37 -> 35 -> 35 -> 17 -> 17 -> 15 -> 7 -> 3 -> 1); 37 x 52 -> 299 x 299 is the real 35 / 17 / 8 geometry.
NETWORK_CASES = {"noresize_3x75x91": (False, (3, 3, 75, 91), 1), "resize_1x37x52": (True, (1, 3, 37, 52), 2)}
WEIGHT_SEED = 0


def network_case(name, dtype=torch.float64):
    """-> (restatement in `dtype` with the seeded weights, all four output blocks; images fp32)."""
    resize, shape, seed = NETWORK_CASES[name]
    net = InceptionV3(output_blocks=(0, 1, 2, 3), resize_input=resize).eval()
    net.load_state_dict(seeded_state_dict(WEIGHT_SEED))
    return net.to(dtype), seeded_images(shape, seed)


# ---- float64 references of the kernels ----------------------------------------------------------------------------------

def conv_acc(x, w, m, h, wd, kh, kw, stride=1, pad=(0, 0)):
    """x (m*h*wd, cin) NHWC rows, w (cout, kh*kw*cin) packed [cout][ky][kx][cin], both in the storage type -> (acc, E_acc):
    acc (m*hout*wout, cout) in float64 by kh*kw tap matmuls over the zero-padded image, E_acc = TAU ||patch_i|| ||w_j||
    (tests/gemm_reference.py: exact products, fp32 sums of depth < 256 for every K here — K / 32 MFMA steps of 8 chained
    adds each is the kernel's depth: 126 steps at K = 4032)."""
    cin, cout = x.shape[1], w.shape[0]
    ph, pw = pad
    hout, wout = (h + 2 * ph - kh) // stride + 1, (wd + 2 * pw - kw) // stride + 1
    X = F.pad(x.to(torch.float64).reshape(m, h, wd, cin), (0, 0, pw, pw, ph, ph))
    W = w.to(torch.float64).reshape(cout, kh, kw, cin)
    acc = torch.zeros((m * hout * wout, cout), dtype=torch.float64, device=x.device)
    n2 = torch.zeros((m * hout * wout,), dtype=torch.float64, device=x.device)
    for ky in range(kh):
        for kx in range(kw):
            tap = X[:, ky:ky + stride * (hout - 1) + 1:stride, kx:kx + stride * (wout - 1) + 1:stride, :].reshape(-1, cin)
            acc += tap @ W[:, ky, kx, :].t()
            n2 += (tap * tap).sum(dim=1)
    return acc, G.TAU * torch.outer(n2.sqrt(), W.reshape(cout, -1).norm(dim=1))


def bn_relu(acc, e_acc, scale, shift, relu=True):
    """The epilogue relu(acc * scale[n] + shift[n]) in float64 and its bound before the output rounding, by the rules of
    gemm_reference.epilogue: the accumulator's error is scaled by |scale| (as `alpha` there), the fma's own fp32
    rounding is within EPI_REL of the magnitudes it combines, and ReLU is 1-Lipschitz, so it widens nothing."""
    s, b = scale.to(torch.float64)[None, :], shift.to(torch.float64)[None, :]
    v = acc * s + b
    e = s.abs() * e_acc + G.EPI_REL * ((acc * s).abs() + b.abs())
    return (v.clamp(min=0) if relu else v), e


def _nchw(x, m, h, wd):
    return x.to(torch.float64).reshape(m, h, wd, -1).permute(0, 3, 1, 2)


def _rows(y):
    return y.permute(0, 2, 3, 1).reshape(-1, y.shape[1])


def pool3x3(x, m, h, wd, mode):
    """float64 3 x 3 pool of NHWC rows, by torch's own pools: "max_s2", "max_s1", "avg_s1" (count_include_pad=False)."""
    X = _nchw(x, m, h, wd)
    if mode == "max_s2":
        return _rows(F.max_pool2d(X, 3, stride=2))
    if mode == "max_s1":
        return _rows(F.max_pool2d(X, 3, stride=1, padding=1))
    return _rows(_avg(X))


def global_avgpool(x, m, hw):
    return x.to(torch.float64).reshape(m, hw, -1).mean(dim=1)


def inception_input(x, size, resize=True, normalize=True):
    """float64 evaluation of F.interpolate(mode="bilinear", align_corners=False)'s formula and 2 x - 1 -> (ref (m*oh*ow, 3),
    bound term): src = max(in / out * (dst + 0.5) - 0.5, 0), i0 = floor(src), i1 = min(i0 + 1, in - 1), weights 1 - l, l.
    The second value is the bound on the fp32 evaluation's error before the store (see the test that uses it)."""
    X = x.to(torch.float64)
    m, _, h, w = X.shape
    if resize:
        oh, ow = size

        def axis(n_in, n_out):
            src = (n_in / n_out * (torch.arange(n_out, dtype=torch.float64) + 0.5) - 0.5).clamp(min=0)
            i0 = src.floor().clamp(max=n_in - 1).long()
            i1 = (i0 + 1).clamp(max=n_in - 1)
            return i0, i1, src - i0.to(torch.float64), src

        y0, y1, ly, sy = axis(h, oh)
        x0, x1, lx, sx = axis(w, ow)
        top = X[:, :, y0][:, :, :, x0] * (1 - lx) + X[:, :, y0][:, :, :, x1] * lx
        bot = X[:, :, y1][:, :, :, x0] * (1 - lx) + X[:, :, y1][:, :, :, x1] * lx
        v = top * (1 - ly)[:, None] + bot * ly[:, None]
        # fp32 coordinates: src carries ~3 roundings relative to its own size (the ratio, the product, the subtraction),
        # so the weight l is off by <= 4 * 2^-24 * (src + 1) per axis; a weight error d moves the lerp by d * |a - b| <= d
        # for values in [0, 1].  The lerp itself is 7 fp32 operations on values <= 1: 8 * 2^-24.
        u = 2.0 ** -24
        e = (4 * u * (sy + 1))[:, None] + (4 * u * (sx + 1))[None, :] + 8 * u
        e = e[None, None].expand_as(v)
    else:
        v, e = X, torch.zeros_like(X)
    if normalize:
        v, e = 2 * v - 1, 2 * e + 2.0 ** -24
    return _rows(v), _rows(e.contiguous())
