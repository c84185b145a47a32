"""The resnet, the down / mid / up blocks and the VAE blocks on the HIP path, per pixel and per channel against the float64
oracle (tests/spatial_cases.py: cases, metrics, measured margins), under every setting that changes the kernels they launch.

Each test sets one row of SETTINGS with monkeypatch.setattr (every switch is first pinned to its documented default, the
layer fusion switches of tests/test_block_switches_gpu.py included, so `default` means the defaults whatever the environment
of the session says), runs the module on ONE shared HIP instance and one set of device inputs per (case, dtype), and checks
  1. every output: finite, shape, dtype, conditions 1-3 of spatial_cases; a failure names the worst pixel as (instance, y,
     x) and the worst channel;
  2. that the setting reached the code: counting spies around ops.conv3x3 / groupnorm / gemm / conv3x3_small_cout and the
     dd_groupnorm_splitk launch see the calls and keyword arguments `expected()` derives from the structure of the module;
     whether an upsampler folds is the lookup in the tracked upfold table, not a constant;
  3. that none of the hand-off attributes is left on the caller's tensors or on a returned tensor, skips included, and
     (default only) that a second run on the same tensors gives the same bits.
One line per test: [spatial] <case> <dtype> <setting> e=.. floor=.. pix=<max>/<bound> ch=<max>/<bound> calls=..  (the output
with the largest share of each bound).

gn_splitk.  ops.GN_SPLITK hands a split-K conv's reduction to the GroupNorm that reads it; whether a conv runs split-K is
the tuner's choice, which would make the path optional.  The setting therefore replaces ops._tune by a function that
writes a fixed (tile, split-K) into the descriptor of every plain 3x3 conv: the pairs of
test_ops_gpu.test_conv_splitk_reduce_folded_into_groupnorm for the widths it lists, its (31, 2) otherwise (the direct
small-image conv takes any Cin that is a multiple of 64 and images of at most 384 pixels).  Every resnet conv with a
gn_next whose image takes the single-launch GroupNorm (dd_groupnorm_is_fused) must then launch dd_groupnorm_splitk.

no_thin is left out: ops.thin_conv_ok takes none of the VAE's layers (its first convs are 8 -> 512 and 8 -> 128 channels; the
thin conv serves the condition embedder's 8 / 16 / 32-channel layers), which test_no_vae_layer_takes_the_thin_conv pins.
"""
import pytest
import torch

from tests import spatial_cases as S
from tests.parity_util import rel_l2
from tests.test_block_switches_gpu import DEFAULTS as LAYER_DEFAULTS
from tests.test_block_switches_gpu import expected as transformer_expected

pytestmark = pytest.mark.gpu

# the documented defaults: DD_GN_SPLITK, DD_UPFOLD, DD_THIN_CONV unset
DEFAULTS = {"GN_SPLITK": False, "fold_upsample": True, "_THIN_CONV": True}
SETTINGS = {
    "default": {},
    "gn_splitk": {"GN_SPLITK": True},
    "no_upfold": {"fold_upsample": False},
}
APPLIES = {
    "gn_splitk": [n for n, c in S.CASES.items() if c["kind"] in ("R", "DB", "MID", "UB")],
    "no_upfold": ["UB1280", "CUB640", "VUP512_256"],
}
MATRIX = [(n, dt, s) for n in S.CASES for dt in S.DTYPES for s in SETTINGS if s == "default" or n in APPLIES[s]]
# (cin, cout) -> (tile, split-K): the case list of test_conv_splitk_reduce_folded_into_groupnorm
PINNED = {(640, 640): (31, 2), (1280, 1280): (31, 4), (2560, 1280): (31, 12), (640, 1280): (12, 3), (320, 640): (31, 2)}
PINNED_OTHER = (31, 2)
ATTRS = ("_gn_cache", "_unwritten", "_ln_cache", "_ln_out", "_ln_stats")
KEYS = ("conv3x3", "conv.stride2", "conv.pad0", "conv.up", "conv.upfold", "conv.gn_next", "conv.rowvec", "conv.res",
        "conv.gn_cache", "gn_splitk", "groupnorm", "groupnorm.x2", "gemm", "gemm.a2", "small_cout")


def upsampler_folds(m, h, w, cin, cout, size, dtype):
    """Conv3x3.folded_up's question to the tracked table: a row for this very shape that names a tile."""
    from dualdiff_amd import ops
    row = ops.tuning.upfold_tuned(ops.tuning.conv_upfold_key(m, h, w, cin, cout, size[0], size[1], ops._dtype_code(dtype)))
    return row is not None and row[0] != 0


def expected(name, dtype, s, is_fused):
    """The calls one run_hip of the case makes under the switches `s`, from the code.  is_fused(hw, c) -> bool:
    dd_groupnorm_is_fused at 32 groups.

    ResnetBlock2D.run:  norm1 (x2= on a two-source input), conv1 (rowvec=, gn_next = norm2), norm2, the 1x1 shortcut GEMM
        where the widths differ (a2= on a two-source input; extra_res rides in its res=), conv2 (res=, gn_next = the norm of
        the Transformer2DModel behind it, if any).  Under GN_SPLITK a conv with a gn_next launches dd_groupnorm_splitk where
        the image takes the single-launch GroupNorm; its result carries _gn_cache and the norm behind it launches nothing.
    VaeResnetBlock2D.run:  the same without time vector, gn_next and second source.
    Transformer2DModel.run:  its GroupNorm and the GEMMs test_block_switches_gpu.expected counts under the defaults.
    run_down_block / run_up_block:  per layer a resnet [+ transformer]; then the stride-2 conv / the conv with up_size=.
    VaeAttention.run:  GroupNorm, the Q|K GEMM, and per view logits, V^T, P V and to_out + residual.
    run_hip itself: ONE TimeEmbProjBank GEMM per call of a UNet case."""
    c = S.CASES[name]
    k, m, (h, w) = c["kind"], c["m"], c["hw"]
    n = dict.fromkeys(KEYS, 0)
    splitk = s["GN_SPLITK"]

    def handed(hw, cout):                       # a conv with a gn_next: does its consumer find the norm done?
        n["conv.gn_next"] += 1
        hit = splitk and is_fused(hw, cout)
        n["gn_splitk"] += hit
        n["conv.gn_cache"] += hit
        return hit

    def resnet(hw, cin, cout, two=False, block_norm=False):
        n["groupnorm"] += 1
        n["groupnorm.x2"] += two
        n["conv3x3"] += 2
        n["conv.rowvec"] += 1
        n["conv.res"] += 1
        n["groupnorm"] += not handed(hw, cout)
        n["gemm"] += cin != cout
        n["gemm.a2"] += cin != cout and two
        return handed(hw, cout) if block_norm else False

    def transformer(ch, norm_done):
        t = transformer_expected("T%d" % ch, LAYER_DEFAULTS)
        n["groupnorm"] += not norm_done
        n["gemm"] += t["gemm"]
        n["gemm.a2"] += t["gemm.a2"]

    def vae_resnet(cin, cout):
        n["groupnorm"] += 2
        n["conv3x3"] += 2
        n["conv.res"] += 1
        n["gemm"] += cin != cout

    def vae_attention():
        n["groupnorm"] += 1
        n["gemm"] += 1 + 4 * m

    def up_conv(hh, ww, ch, size):
        n["conv3x3"] += 1
        n["conv.up"] += 1
        n["conv.upfold"] += s["fold_upsample"] and upsampler_folds(m, hh, ww, ch, ch, size, dtype)

    if k in ("R", "DB", "MID", "UB"):
        n["gemm"] += 1                                                   # the time-embedding bank
    if k == "R":
        for _ in range(2):                                               # without and with extra_res
            resnet(h * w, sum(c["cin"]), c["cout"], two=c["cin"][1] > 0)
    elif k == "DB":
        for i in range(2):
            done = resnet(h * w, c["cin"] if i == 0 else c["cout"], c["cout"], block_norm=c["cross"])
            if c["cross"]:
                transformer(c["cout"], done)
        if c["down"]:
            n["conv3x3"] += 1
            n["conv.stride2"] += 1
    elif k == "MID":
        transformer(c["c"], resnet(h * w, c["c"], c["c"], block_norm=True))
        resnet(h * w, c["c"], c["c"])
    elif k == "UB":
        for i, skip in enumerate((c["cout"], c["cout"], c["cin"])):
            done = resnet(h * w, (c["prev"] if i == 0 else c["cout"]) + skip, c["cout"], two=True, block_norm=c["cross"])
            if c["cross"]:
                transformer(c["cout"], done)
        up_conv(h, w, c["cout"], c["up_size"] or (2 * h, 2 * w))
    elif k == "VR":
        vae_resnet(c["cin"], c["cout"])
    elif k == "VMID":
        vae_resnet(c["c"], c["c"]), vae_attention(), vae_resnet(c["c"], c["c"])
    elif k == "VUP":
        for i in range(3):
            vae_resnet(c["cin"] if i == 0 else c["cout"], c["cout"])
        up_conv(h, w, c["cout"], (2 * h, 2 * w))
    elif k == "VDOWN":
        for i in range(2):
            vae_resnet(c["cin"] if i == 0 else c["cout"], c["cout"])
        n["conv3x3"] += 1
        n["conv.stride2"] += 1
        n["conv.pad0"] += 1
    elif k == "VDEC":                     # post_quant_conv, conv_in, mid block, four up blocks, conv_norm_out, conv_out
        n["gemm"] += 1
        n["conv3x3"] += 1
        vae_resnet(512, 512), vae_attention(), vae_resnet(512, 512)
        prev = 512
        for i, ch in enumerate((512, 512, 256, 128)):
            for j in range(3):
                vae_resnet(prev if j == 0 else ch, ch)
            if i < 3:
                up_conv(h << i, w << i, ch, (h << (i + 1), w << (i + 1)))
            prev = ch
        n["groupnorm"] += 1
        n["small_cout"] += 1
    else:                                 # VENC: conv_in, four down blocks, mid block, conv_norm_out, conv_out
        n["conv3x3"] += 1
        prev = 128
        for i, ch in enumerate((128, 256, 512, 512)):
            for j in range(2):
                vae_resnet(prev if j == 0 else ch, ch)
            if i < 3:
                n["conv3x3"] += 1
                n["conv.stride2"] += 1
                n["conv.pad0"] += 1
            prev = ch
        vae_resnet(512, 512), vae_attention(), vae_resnet(512, 512)
        n["groupnorm"] += 1
        n["conv3x3"] += 1
    return {key: int(v) for key, v in n.items()}


class Spies:
    """Counting wrappers around the launch wrappers the modules call through the ops module; a call counts when it
    returns.  dd_groupnorm_splitk is counted where ops.conv3x3 launches it, through the timer's launch helper."""

    def __init__(self, monkeypatch, ops):
        self.n = dict.fromkeys(KEYS, 0)
        for fn in ("conv3x3", "groupnorm", "gemm", "conv3x3_small_cout"):
            monkeypatch.setattr(ops, fn, self._wrap(fn, getattr(ops, fn)))
        real = ops._timer.launch

        def launch(what, *a, **kw):
            out = real(what, *a, **kw)
            self.n["gn_splitk"] += what == "groupnorm_splitk"
            return out
        monkeypatch.setattr(ops._timer, "launch", launch)

    def _wrap(self, fn, real):
        def spy(*a, **kw):
            out = real(*a, **kw)
            if fn == "conv3x3":
                self.n["conv3x3"] += 1
                self.n["conv.stride2"] += kw.get("stride", 1) == 2
                self.n["conv.pad0"] += kw.get("pad", 1) == 0
                self.n["conv.up"] += kw.get("up_size") is not None
                for key in ("upfold", "gn_next", "rowvec", "res"):
                    self.n["conv." + key] += kw.get(key) is not None
                self.n["conv.gn_cache"] += getattr(out, "_gn_cache", None) is not None
            elif fn == "groupnorm":
                self.n["groupnorm"] += 1
                self.n["groupnorm.x2"] += kw.get("x2") is not None
            elif fn == "gemm":
                self.n["gemm"] += 1
                self.n["gemm.a2"] += kw.get("a2") is not None
            else:
                self.n["small_cout"] += 1
            return out
        return spy


def pin_conv_plans(monkeypatch, ops):
    """ops._tune for the gn_splitk setting: a fixed (tile, split-K) for every plain 3x3 / stride 1 / pad 1 conv."""
    real = ops._tune

    def tune(L, d, key, out_shape, dtype, device, warm):
        if d.conv and L.pad_lo == 1 and d.stride == 1 and not d.upfold and (d.hv, d.wv) == (d.hin, d.win) and d.cin % 64 == 0:
            d.tile, d.split_k = PINNED.get((d.cin, d.n), PINNED_OTHER)
        else:
            real(L, d, key, out_shape, dtype, device, warm)
    monkeypatch.setattr(ops, "_tune", tune)


def tensors_of(tree):
    if torch.is_tensor(tree):
        return [tree]
    if isinstance(tree, dict):
        tree = list(tree.values())
    return [t for v in (tree or []) for t in tensors_of(v)] if isinstance(tree, (list, tuple)) else []


@pytest.fixture(scope="module")
def shared(gpu):
    """name -> oracle outputs (CPU, once per case); (name, dtype) -> the ONE HIP module and its device inputs."""
    cache = {}

    def get(name, dtype):
        if name not in cache:
            cache[name] = S.oracle_outputs(name)
        o = cache[name]
        if (name, dtype) not in cache:
            cache[name, dtype] = (S.make_hip(name, o["sd"], dtype), S.hip_inputs(name, o["inp"], dtype))
        return (o,) + cache[name, dtype]
    return get


def test_no_vae_layer_takes_the_thin_conv(gpu):
    """Why there is no `no_thin` setting: ops._THIN_CONV cannot change what the VAE launches."""
    from dualdiff_amd import ops
    from dualdiff_amd.networks import layers, vae_decoder, vae_encoder
    for net in (vae_decoder.AutoencoderKLDecoder(), vae_encoder.AutoencoderKLEncoder()):
        convs = [mod for mod in net.modules() if isinstance(mod, layers.Conv3x3)]
        assert convs and not [cv for cv in convs if ops.thin_conv_ok(cv.cin_pad, cv.out_channels, cv.stride, 2)]


@pytest.mark.parametrize("name,dtype,setting", MATRIX, ids=["%s-%s-%s" % (n, S.tag(dt), s) for n, dt, s in MATRIX])
def test_spatial_block(shared, monkeypatch, name, dtype, setting):
    from dualdiff_amd import _native, ops
    from dualdiff_amd.networks import blocks, layers
    o, blk, dev = shared(name, dtype)
    s = dict(DEFAULTS, **SETTINGS[setting])
    for key, v in LAYER_DEFAULTS.items():
        monkeypatch.setattr(layers.Transformer2DModel if key == "fold_proj_out" else layers, key, v)
    monkeypatch.setattr(blocks, "ATTN4_PAIR", True)
    monkeypatch.setattr(ops, "GN_SPLITK", s["GN_SPLITK"])
    monkeypatch.setattr(ops, "_THIN_CONV", s["_THIN_CONV"])
    monkeypatch.setattr(layers.Conv3x3, "fold_upsample", s["fold_upsample"])
    if s["GN_SPLITK"]:
        pin_conv_plans(monkeypatch, ops)
    lib = _native.load()
    spies = Spies(monkeypatch, ops)

    ys = S.run_hip(name, blk, dev)
    torch.cuda.synchronize()
    calls = dict(spies.n)
    assert list(ys) == S.outputs_of(name)
    worst = {}
    failures = []
    for out, y in ys.items():
        ref, emul = o["ref"][out], o["emul"][dtype][out]
        assert y.shape == ref.shape and y.dtype == dtype, out
        assert torch.isfinite(y).all(), out
        cond = S.conditions(name, dtype, y, ref, emul)
        for key, (v, b) in cond.items():
            if key not in worst or v / b > worst[key][0] / worst[key][1]:
                worst[key] = (v, b, out, rel_l2(emul, ref))
        pool = S.POOL[name]
        if cond["e"][0] > cond["e"][1]:
            failures.append("%s: whole tensor %.3e > %.3e" % (out, cond["e"][0], cond["e"][1]))
        if cond["pix"][0] > cond["pix"][1]:
            failures.append("%s: worst pixel (instance, y, x) = %s: %.3e > %.3e"
                            % (out, S.where(name, out, int(S.e_pix(y, ref, pool).argmax()), pool), cond["pix"][0], cond["pix"][1]))
        if cond["ch"][0] > cond["ch"][1]:
            failures.append("%s: worst channel %d: %.3e > %.3e" % (out, int(S.e_ch(y, ref).argmax()), cond["ch"][0], cond["ch"][1]))
    print("[spatial] %s %s %s e=%.3e floor=%.3e pix=%.3e/%.3e ch=%.3e/%.3e calls=%s"
          % (name, S.tag(dtype), setting, worst["e"][0], worst["e"][3], worst["pix"][0], worst["pix"][1], worst["ch"][0],
             worst["ch"][1], " ".join("%s=%d" % kv for kv in sorted(calls.items()) if kv[1])))
    assert calls == expected(name, dtype, s, lambda hw, c: bool(lib.dd_groupnorm_is_fused(hw, c, 32)))
    assert not failures, failures
    left = [(a, tuple(t.shape)) for t in tensors_of(dev) + tensors_of(ys) for a in ATTRS if hasattr(t, a)]
    assert not left, "hand-off attributes left behind: %s" % left
    if setting == "default":
        ys2 = S.run_hip(name, blk, dev)
        for out, y in ys.items():
            assert torch.equal(y, ys2[out]), "a second run on the same input tensors changes %s" % out
        assert spies.n == {key: 2 * v for key, v in calls.items()}
