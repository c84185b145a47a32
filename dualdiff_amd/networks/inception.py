"""InceptionV3 feature extractor of the FID evaluation on the HIP path.

Replaces the reference's magicdrive/misc/inception.py (pytorch-fid's FID network: torchvision's Inception3 with the
FID patches — exclusive average pools in the A / C / E blocks, a max pool in Mixed_7c), which tools/fid_score.py:93-156
runs in fp32 on batches of 50.  Here every BasicConv2d (conv without bias -> BatchNorm2d(eps=1e-3) in eval -> ReLU) is
ONE launch of dd_conv2d_nhwc: 16-bit NHWC activations and packed weights, fp32 accumulation, BatchNorm as an fp32
scale / shift per output channel in the epilogue (never folded into the 16-bit weights), and a block's branches write
straight into their slices of the concatenated tensor.  The pooled features leave in fp32.

Parameters keep pytorch-fid's names (Conv2d_1a_3x3.conv.weight, Mixed_5b.branch1x1.bn.running_var, ...), so that
checkpoint loads unchanged; `fc.*` is ignored.  torchvision is not a dependency: the architecture is restated here.
"""
import torch
import torch.nn as nn

from .. import ops
from .layers import _Cached, derived

BLOCK_INDEX_BY_DIM = {64: 0, 192: 1, 768: 2, 2048: 3}
CIN_MULTIPLE = 8            # dd_conv2d_nhwc's cin rule: the stem's three channels are zero-padded to it
MAX_GEOMETRIES = 4          # activation-buffer sets kept: the steady batch size, the ragged last batch, two spare


def fold_bn(gamma, beta, mean, var, eps):
    """Eval-mode BatchNorm as y = x * scale + shift, in float64: scale = gamma / sqrt(var + eps), shift = beta - mean *
    scale."""
    scale = gamma.double() / torch.sqrt(var.double() + eps)
    return scale, beta.double() - mean.double() * scale


def pack_conv_weight(w, cin_multiple=CIN_MULTIPLE):
    """(cout, cin, kh, kw) -> (cout, kh * kw * cin_p) in dd_conv2d_nhwc's [cout][ky][kx][cin] order, cin zero-padded to a
    multiple of `cin_multiple`."""
    cout, cin, kh, kw = w.shape
    cp = -(-cin // cin_multiple) * cin_multiple
    p = w.new_zeros((cout, kh, kw, cp))
    p[..., :cin] = w.permute(0, 2, 3, 1)
    return p.reshape(cout, kh * kw * cp)


def unpack_conv_weight(p, cin, kh, kw):
    """Inverse of pack_conv_weight (the padded channels are dropped)."""
    cout = p.shape[0]
    return p.reshape(cout, kh, kw, -1)[..., :cin].permute(0, 3, 1, 2).contiguous()


def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


class BasicConv2d(_Cached):
    def __init__(self, cin, cout, kernel_size, stride=1, padding=0):
        super().__init__()
        self.kh, self.kw = _pair(kernel_size)
        self.stride, self.pad = stride, _pair(padding)
        self.cin, self.cout = cin, cout
        self.conv = nn.Conv2d(cin, cout, (self.kh, self.kw), stride=stride, padding=self.pad, bias=False)
        self.bn = nn.BatchNorm2d(cout, eps=1e-3)

    def packed(self, dtype):
        """(weights [cout][ky][kx][cin_p] in `dtype`, fp32 scale, fp32 shift) under the one cache rule for derived weights."""
        bn = self.bn
        params = [self.conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var]

        def build():
            scale, shift = fold_bn(bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps)
            return (pack_conv_weight(self.conv.weight.detach()).to(dtype).contiguous(), scale.float().contiguous(),
                    shift.float().contiguous())

        return derived(self, "conv", params, build, slot=dtype)

    def run(self, x, m, h, w, dtype, out, c_off=0):
        wp, scale, shift = self.packed(dtype)
        ops.conv2d(x, wp, scale, shift, m, h, w, self.kh, self.kw, stride=self.stride, pad=self.pad, out=out, c_off=c_off)

    def out_hw(self, h, w):
        return ops.conv2d_out_hw(h, w, self.kh, self.kw, self.stride, self.pad)


class _Net:
    """One forward's view of the model: storage type, batch size and the buffer set of this input geometry."""

    def __init__(self, bufs, dtype, device, m):
        self.bufs, self.dtype, self.device, self.m = bufs, dtype, device, m

    def buf(self, name, rows, cols):
        key = (name, rows, cols)
        t = self.bufs.get(key)
        if t is None:
            t = self.bufs[key] = torch.empty((rows, cols), dtype=self.dtype, device=self.device)
        return t

    def conv(self, layer, x, h, w, name, out=None, c_off=0):
        """layer(x) into `out` at c_off, or into the layer's own buffer `name`; returns (tensor, hout, wout)."""
        ho, wo = layer.out_hw(h, w)
        if out is None:
            out = self.buf(name, self.m * ho * wo, layer.cout)
        layer.run(x, self.m, h, w, self.dtype, out, c_off)
        return out, ho, wo

    def chain(self, layers, x, h, w, name, out, c_off):
        """layers[0] .. layers[-1] in sequence; the last one writes the slice of `out` at c_off."""
        for i, layer in enumerate(layers[:-1]):
            x, h, w = self.conv(layer, x, h, w, "%s.%d" % (name, i))
        self.conv(layers[-1], x, h, w, None, out, c_off)

    def pool(self, x, h, w, mode, name, out=None, c_off=0):
        ho, wo = ((h - 3) // 2 + 1, (w - 3) // 2 + 1) if mode == "max_s2" else (h, w)
        if out is None:
            out = self.buf(name, self.m * ho * wo, x.shape[1])
        ops.pool3x3(x, self.m, h, w, mode, out=out, c_off=c_off)
        return out, ho, wo


class InceptionA(nn.Module):
    def __init__(self, cin, pf):
        super().__init__()
        self.cout = 224 + pf
        self.branch1x1 = BasicConv2d(cin, 64, 1)
        self.branch5x5_1 = BasicConv2d(cin, 48, 1)
        self.branch5x5_2 = BasicConv2d(48, 64, 5, padding=2)
        self.branch3x3dbl_1 = BasicConv2d(cin, 64, 1)
        self.branch3x3dbl_2 = BasicConv2d(64, 96, 3, padding=1)
        self.branch3x3dbl_3 = BasicConv2d(96, 96, 3, padding=1)
        self.branch_pool = BasicConv2d(cin, pf, 1)

    def run(self, net, x, h, w, name):
        out = net.buf(name, net.m * h * w, self.cout)
        net.conv(self.branch1x1, x, h, w, None, out, 0)
        net.chain([self.branch5x5_1, self.branch5x5_2], x, h, w, name + ".5x5", out, 64)
        net.chain([self.branch3x3dbl_1, self.branch3x3dbl_2, self.branch3x3dbl_3], x, h, w, name + ".dbl", out, 128)
        p, _, _ = net.pool(x, h, w, "avg_s1", name + ".pool")
        net.conv(self.branch_pool, p, h, w, None, out, 224)
        return out, h, w


class InceptionB(nn.Module):
    def __init__(self, cin):
        super().__init__()
        self.cout = 384 + 96 + cin
        self.branch3x3 = BasicConv2d(cin, 384, 3, stride=2)
        self.branch3x3dbl_1 = BasicConv2d(cin, 64, 1)
        self.branch3x3dbl_2 = BasicConv2d(64, 96, 3, padding=1)
        self.branch3x3dbl_3 = BasicConv2d(96, 96, 3, stride=2)

    def run(self, net, x, h, w, name):
        ho, wo = self.branch3x3.out_hw(h, w)
        out = net.buf(name, net.m * ho * wo, self.cout)
        net.conv(self.branch3x3, x, h, w, None, out, 0)
        net.chain([self.branch3x3dbl_1, self.branch3x3dbl_2, self.branch3x3dbl_3], x, h, w, name + ".dbl", out, 384)
        net.pool(x, h, w, "max_s2", None, out, 480)
        return out, ho, wo


class InceptionC(nn.Module):
    def __init__(self, cin, c):
        super().__init__()
        self.cout = 768
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

    def run(self, net, x, h, w, name):
        out = net.buf(name, net.m * h * w, self.cout)
        net.conv(self.branch1x1, x, h, w, None, out, 0)
        net.chain([self.branch7x7_1, self.branch7x7_2, self.branch7x7_3], x, h, w, name + ".7x7", out, 192)
        net.chain([self.branch7x7dbl_1, self.branch7x7dbl_2, self.branch7x7dbl_3, self.branch7x7dbl_4,
                   self.branch7x7dbl_5], x, h, w, name + ".dbl", out, 384)
        p, _, _ = net.pool(x, h, w, "avg_s1", name + ".pool")
        net.conv(self.branch_pool, p, h, w, None, out, 576)
        return out, h, w


class InceptionD(nn.Module):
    def __init__(self, cin):
        super().__init__()
        self.cout = 320 + 192 + cin
        self.branch3x3_1 = BasicConv2d(cin, 192, 1)
        self.branch3x3_2 = BasicConv2d(192, 320, 3, stride=2)
        self.branch7x7x3_1 = BasicConv2d(cin, 192, 1)
        self.branch7x7x3_2 = BasicConv2d(192, 192, (1, 7), padding=(0, 3))
        self.branch7x7x3_3 = BasicConv2d(192, 192, (7, 1), padding=(3, 0))
        self.branch7x7x3_4 = BasicConv2d(192, 192, 3, stride=2)

    def run(self, net, x, h, w, name):
        ho, wo = self.branch3x3_2.out_hw(h, w)
        out = net.buf(name, net.m * ho * wo, self.cout)
        net.chain([self.branch3x3_1, self.branch3x3_2], x, h, w, name + ".3x3", out, 0)
        net.chain([self.branch7x7x3_1, self.branch7x7x3_2, self.branch7x7x3_3, self.branch7x7x3_4], x, h, w,
                  name + ".7x7", out, 320)
        net.pool(x, h, w, "max_s2", None, out, 512)
        return out, ho, wo


class InceptionE(nn.Module):
    def __init__(self, cin, pool):
        super().__init__()
        self.cout = 2048
        self.pool = pool                # "avg_s1": exclusive average (Mixed_7b); "max_s1" (Mixed_7c, inception.py:333-338)
        self.branch1x1 = BasicConv2d(cin, 320, 1)
        self.branch3x3_1 = BasicConv2d(cin, 384, 1)
        self.branch3x3_2a = BasicConv2d(384, 384, (1, 3), padding=(0, 1))
        self.branch3x3_2b = BasicConv2d(384, 384, (3, 1), padding=(1, 0))
        self.branch3x3dbl_1 = BasicConv2d(cin, 448, 1)
        self.branch3x3dbl_2 = BasicConv2d(448, 384, 3, padding=1)
        self.branch3x3dbl_3a = BasicConv2d(384, 384, (1, 3), padding=(0, 1))
        self.branch3x3dbl_3b = BasicConv2d(384, 384, (3, 1), padding=(1, 0))
        self.branch_pool = BasicConv2d(cin, 192, 1)

    def run(self, net, x, h, w, name):
        out = net.buf(name, net.m * h * w, self.cout)
        net.conv(self.branch1x1, x, h, w, None, out, 0)
        b3, _, _ = net.conv(self.branch3x3_1, x, h, w, name + ".3x3")
        net.conv(self.branch3x3_2a, b3, h, w, None, out, 320)
        net.conv(self.branch3x3_2b, b3, h, w, None, out, 704)
        bd, _, _ = net.conv(self.branch3x3dbl_1, x, h, w, name + ".dbl.0")
        bd, _, _ = net.conv(self.branch3x3dbl_2, bd, h, w, name + ".dbl.1")
        net.conv(self.branch3x3dbl_3a, bd, h, w, None, out, 1088)
        net.conv(self.branch3x3dbl_3b, bd, h, w, None, out, 1472)
        p, _, _ = net.pool(x, h, w, self.pool, name + ".pool")
        net.conv(self.branch_pool, p, h, w, None, out, 1856)
        return out, h, w


_MIXED_2 = ("Mixed_5b", "Mixed_5c", "Mixed_5d", "Mixed_6a", "Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e")
_MIXED_3 = ("Mixed_7a", "Mixed_7b", "Mixed_7c")


class InceptionV3(nn.Module):
    """forward(inp): inp (m, 3, h, w) in [0, 1] on the GPU (fp16 / bf16 / fp32) -> the fp32 NCHW feature maps of
    `output_blocks` (0: 64 channels after the first max pool, 1: 192 after the second, 2: 768 after Mixed_6e, 3: the
    2048 pooled features as (m, 2048, 1, 1)), like the reference's forward.  features(inp, dims) -> (m, dims) fp32.
    `dtype` is the storage type of activations and packed weights; the parameters themselves stay as loaded."""

    def __init__(self, output_blocks=(3,), resize_input=True, normalize_input=True, dtype=torch.float16):
        super().__init__()
        self.output_blocks = sorted(int(b) for b in output_blocks)
        if not self.output_blocks or min(self.output_blocks) < 0 or max(self.output_blocks) > 3:
            raise ValueError("output_blocks must be a non-empty subset of 0..3, got %r" % (output_blocks,))
        if dtype not in (torch.float16, torch.bfloat16):
            raise ValueError("InceptionV3 stores activations in fp16 or bf16, got %s" % dtype)
        self.resize_input, self.normalize_input, self.dtype = bool(resize_input), bool(normalize_input), dtype
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
        self.Mixed_7b = InceptionE(1280, "avg_s1")
        self.Mixed_7c = InceptionE(2048, "max_s1")
        self.eval()
        self._geometries = {}

    def load_state_dict(self, state_dict, strict=True, **kw):
        """pytorch-fid's key layout; the classifier head `fc.*`, which the FID network never runs, is ignored."""
        return super().load_state_dict({k: v for k, v in state_dict.items() if not k.startswith("fc.")}, strict=strict, **kw)

    def _apply(self, fn, *a, **k):
        self._geometries = {}                        # the buffers follow the parameters' device
        return super()._apply(fn, *a, **k)

    def _net(self, inp):
        m, _, h, w = inp.shape
        key = (m, h, w, inp.device)
        bufs = self._geometries.pop(key, None)
        if bufs is None:
            bufs = {}
            while len(self._geometries) >= MAX_GEOMETRIES:
                self._geometries.pop(next(iter(self._geometries)))          # least recently used
        self._geometries[key] = bufs
        return _Net(bufs, self.dtype, inp.device, m)

    def _trunk(self, inp, last, want):
        """Runs up to block `last`; returns {block: (rows tensor, h, w)} for the blocks in `want`."""
        if inp.dim() != 4 or inp.shape[1] != 3:
            raise ValueError("InceptionV3 takes (m, 3, h, w) images, got %s" % (tuple(inp.shape),))
        if not inp.is_cuda:
            raise RuntimeError("dualdiff_amd ops run on the GPU only (got a %s tensor); there is no CPU fallback" % inp.device)
        net = self._net(inp)
        m, h, w = inp.shape[0], inp.shape[2], inp.shape[3]
        oh, ow = (299, 299) if self.resize_input else (h, w)
        x = ops.inception_input(inp.contiguous(), (oh, ow), resize=self.resize_input, normalize=self.normalize_input,
                                dtype=self.dtype, c_pad=CIN_MULTIPLE, out=net.buf("input", m * oh * ow, CIN_MULTIPLE))
        h, w = oh, ow
        got = {}
        for name in ("Conv2d_1a_3x3", "Conv2d_2a_3x3", "Conv2d_2b_3x3"):
            x, h, w = net.conv(getattr(self, name), x, h, w, name)
        x, h, w = net.pool(x, h, w, "max_s2", "pool1")
        if 0 in want:
            got[0] = (x, h, w)
        if last >= 1:
            for name in ("Conv2d_3b_1x1", "Conv2d_4a_3x3"):
                x, h, w = net.conv(getattr(self, name), x, h, w, name)
            x, h, w = net.pool(x, h, w, "max_s2", "pool2")
            if 1 in want:
                got[1] = (x, h, w)
        if last >= 2:
            for name in _MIXED_2:
                x, h, w = getattr(self, name).run(net, x, h, w, name)
            if 2 in want:
                got[2] = (x, h, w)
        if last >= 3:
            for name in _MIXED_3:
                x, h, w = getattr(self, name).run(net, x, h, w, name)
            got[3] = (x, h, w)
        return m, got

    @torch.no_grad()
    def forward(self, inp):
        m, got = self._trunk(inp, max(self.output_blocks), self.output_blocks)
        outs = []
        for b in self.output_blocks:
            x, h, w = got[b]
            if b == 3:
                outs.append(ops.global_avgpool(x, m, h * w).reshape(m, -1, 1, 1))
            else:
                outs.append(x.reshape(m, h, w, -1).permute(0, 3, 1, 2).float().contiguous())
        return outs

    @torch.no_grad()
    def features(self, inp, dims=2048):
        """The pooled (m, dims) fp32 activations of get_activations (tools/fid_score.py:93-156): the global average of the
        block that has `dims` channels.  A fresh tensor: it does not alias the reused activation buffers."""
        if dims not in BLOCK_INDEX_BY_DIM:
            raise ValueError("dims must be one of %s, got %r" % (sorted(BLOCK_INDEX_BY_DIM), dims))
        b = BLOCK_INDEX_BY_DIM[dims]
        m, got = self._trunk(inp, b, (b,))
        x, h, w = got[b]
        return ops.global_avgpool(x, m, h * w)
