"""Cases of the sibling-overlap tests (model_base.sibling_overlap) that need no GPU to be stated.

1. The DECISION RULE as a small pure-Python model (`Rule`), and the seeded action sequences of
   test_random_interleavings_equal_serial (`sequences`).  A forward() of model M on stream s is overlapped iff ALL of:
     - the latest forward() entry of the thread (the window) exists, was made on s, by ANOTHER live model, and neither a
       packed-weight drop (layers.CACHE_EPOCH) nor a `sibling_barrier()` / `_invalidate()` happened since;
     - every tensor argument is vouched for — same bytes, view and version as an argument of the window, or of M's own
       previous entry on s (which must be as current as the window);
     - M and the window's model share no sub-module object and no parameter storage (R4);
     - M's call replays a graph it has ALREADY recorded for its key in the current epoch (R1): the first sight of a key
       (eager) and the second (capture) run on the caller's stream.
   The tests call every model with the same timestep and context objects, so "every argument" comes down to the latents.

2. `RAW_WRITERS`: every public wrapper of dualdiff_amd/ops.py that writes a tensor its CALLER handed in through a raw
   pointer, with the names of the written arguments and a tiny launch (`make(dev)` -> (call, {argument: tensor or tuple
   of tensors})).  Each written tensor must count one version more after the call (R3): the version is what the
   readiness proof reads.  tests/test_sibling_rules_cpu.py walks ops.py and fails for a writer without a row.
"""
import random

# ---- the interleaving test ----------------------------------------------------------------------------------------------------
ACTIONS = ("call_A", "call_B", "call_S", "new_x", "mul_x", "raw_x", "invalidate_B", "call_B_other_stream")
# the share of each action: calls dominate (an overlapped call needs a recorded graph, i.e. two earlier calls of that model
# since its last invalidation, and a sibling's entry right in front of it)
WEIGHTS = (5, 6, 2, 1, 1, 1, 1, 1)
SEQS, LENGTH, SEED = 40, 8, 9
MIN_OVERLAPPED_SHARE = 0.25          # of all calls of B, the model that A and S both overlap with
MIN_PER_ACTION = 10
SHARING = {frozenset("AS")}          # S holds a sub-module of A


def sequences(seed=SEED, seqs=SEQS, length=LENGTH):
    rng = random.Random(seed)
    return [rng.choices(ACTIONS, weights=WEIGHTS, k=length) for _ in range(seqs)]


class Rule:
    """Host-side state of the decision: the window, each model's own previous entry, how often each model has seen its
    (one) key since its graphs were last dropped, the identity and version of the latents."""

    def __init__(self, models="ABS", sharing=SHARING):
        self.window = None
        self.prev = {m: None for m in models}
        self.sights = {m: 0 for m in models}            # 0: unknown key, 1: seen (eager), >= 2: recorded
        self.sharing = sharing
        self.gen = 0                                    # sibling_barrier() / _invalidate() count
        self.x = (0, 0)                                 # (which tensor, its version)
        self._ids = 0

    def new_x(self):
        self._ids += 1
        self.x = (self._ids, 0)

    def write_x(self):                                  # torch's in-place ops and this package's raw writers alike
        self.x = (self.x[0], self.x[1] + 1)

    def invalidate(self, m):
        self.sights[m] = 0
        self.window = None
        self.gen += 1

    def call(self, m, stream="main"):
        """-> whether this call is overlapped"""
        entry = {"owner": m, "stream": stream, "x": self.x, "gen": self.gen}
        window, mine = self.window, self.prev[m]
        self.window = self.prev[m] = entry
        recorded = self.sights[m] >= 2
        self.sights[m] += 1
        if window is None or window["stream"] != stream or window["owner"] == m or window["gen"] != self.gen:
            return False
        mine_ok = mine is not None and mine["stream"] == stream and mine["gen"] == self.gen
        if not (window["x"] == self.x or (mine_ok and mine["x"] == self.x)):
            return False
        if frozenset((window["owner"], m)) in self.sharing:
            return False
        return recorded

    def apply(self, action):
        """-> (model, overlapped) for a call, None otherwise"""
        if action.startswith("call_"):
            m = action[5]
            return m, self.call(m, "other" if action.endswith("other_stream") else "main")
        {"new_x": self.new_x, "mul_x": self.write_x, "raw_x": self.write_x,
         "invalidate_B": lambda: self.invalidate("B")}[action]()
        return None


def predict(seqs):
    """The test's protocol on the model: every model's graphs dropped first, new latents at the start of every sequence.
    -> per sequence, per action: None or (model, overlapped)."""
    rule = Rule()
    for m in "ABS":
        rule.invalidate(m)
    out = []
    for seq in seqs:
        rule.new_x()
        out.append([rule.apply(a) for a in seq])
    return out


# ---- the raw-pointer writers of ops.py -----------------------------------------------------------------------------------------
WRITER_PARAMS = ("out", "x_out", "x_dup")            # a public wrapper with one of these parameters writes its caller's tensor
IN_PLACE = {                                         # ... and these write arguments that carry no such name
    "given_views_noise": ("x",),
    "cfg_unipc_step": ("hist",),
    "box_tokens": ("pos", "cat", "cls_out"),
}


def _rand(shape, dtype, seed, dev, scale=1.0):
    import torch
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype).to(dev)


def _again(fn, name="out"):
    """The wrapper run once for a tensor of the layout it returns, then the launch that writes a caller's tensor of that
    layout.  -> (call, {name: the tensor(s)})"""
    import torch
    first = fn(None)
    like = (lambda t: None if t is None else torch.empty_strided(t.shape, t.stride(), dtype=t.dtype, device=t.device))
    out = tuple(like(t) for t in first) if isinstance(first, (tuple, list)) else like(first)
    return (lambda: fn(out)), {name: out}


def _f16():
    import torch
    return torch.float16


def _elementwise(name):
    def make(dev):
        from dualdiff_amd import ops
        x = _rand((3, 40), _f16(), 1, dev)
        fn = {"scale": lambda o: ops.scale(x, 0.5, out=o), "add": lambda o: ops.add(x, x, out=o),
              "silu": lambda o: ops.silu(x, out=o)}[name]
        return _again(fn)
    return make


def _gemm(dev):
    from dualdiff_amd import ops
    a, w = _rand((40, 64), _f16(), 2, dev), _rand((64, 64), _f16(), 3, dev, 0.125)
    return _again(lambda o: ops.gemm(a, w, out=o))


def _steps(name):
    def make(dev):
        import torch
        from dualdiff_amd import ops
        from dualdiff_amd.pipeline.pipeline_bev_controlnet import ddim_schedule
        from dualdiff_amd.pipeline.schedulers import unipc_schedule
        n = 12 * 40
        x, eps = _rand((n,), _f16(), 4, dev), _rand((2, n), _f16(), 5, dev)
        x_out, x_dup = torch.empty_like(x), torch.empty_like(x)
        hist = torch.zeros((3, n), dtype=torch.float32, device=dev)
        mask = torch.zeros(12, dtype=torch.uint8)
        mask[::2] = 1
        given = ops.GivenViews(mask.to(dev), _rand((n,), torch.float32, 6, dev), _rand((n,), _f16(), 7, dev),
                               torch.tensor([0.9, 0.4, 0.1], device=dev), 1)
        if name == "cfg_ddim_step":
            coef = ddim_schedule(50)[1][25].to(dev)
            return (lambda: ops.cfg_ddim_step(eps, x, coef, 2.0, x_out=x_out, x_dup=x_dup)), {"x_out": x_out, "x_dup": x_dup}
        if name == "cfg_unipc_step":
            coef = unipc_schedule(8)[1][3].to(dev)
            return (lambda: ops.cfg_unipc_step(eps, x, hist, coef, 2.0, x_out=x_out, x_dup=x_dup, given=given)), \
                {"x_out": x_out, "x_dup": x_dup, "hist": hist}
        return (lambda: ops.given_views_noise(x, given, torch.tensor([0.8, 0.6]), x_dup=x_dup)), {"x": x, "x_dup": x_dup}
    return make


def _op(build, first_of_tuple=False):
    """build(ops, dev) -> fn(out): the launch with the wrapper's own output (out = None) or the caller's"""
    def make(dev):
        from dualdiff_amd import ops
        fn = build(ops, dev)
        if not first_of_tuple:
            return _again(fn)
        call, written = _again(lambda o: fn(o)[0])     # (out, lengths / status ...): only `out` is the caller's
        return call, written
    return make


def _u8(shape, seed, dev):
    import torch
    return torch.randint(0, 256, shape, generator=torch.Generator().manual_seed(seed), dtype=torch.uint8).to(dev)


def _smooth(h, w, dev):
    """one (1, h, w, 3) uint8 frame of gentle ramps: its JPEG file is far shorter than the default capacity"""
    import torch
    y, x, c = torch.meshgrid(torch.arange(h), torch.arange(w), torch.arange(3), indexing="ij")
    return (40 + 3 * y + 2 * x + 30 * c).to(torch.uint8)[None].contiguous().to(dev)


def _unit(shape, seed, dev):
    import torch
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed)).to(dev)


def _conv3x3(ops, dev):
    x, w, b = _rand((1400, 96), _f16(), 10, dev), _rand((256, 864), _f16(), 11, dev, 864 ** -0.5), _rand((256,), _f16(), 12, dev)
    return lambda o: ops.conv3x3(x, w, b, 1, 28, 50, stride=2, out=o)


def _conv_out(ops, dev):
    x, w, b = _rand((2 * 28 * 50, 320), _f16(), 13, dev), _rand((4, 2880), _f16(), 14, dev, 0.02), _rand((4,), _f16(), 15, dev)
    return lambda o: ops.conv3x3_small_cout(x, w, b, 2, 28, 50, out=o)


def _groupnorm(ops, dev):
    x, g, b = _rand((2 * 240, 128), _f16(), 16, dev), _rand((128,), _f16(), 17, dev), _rand((128,), _f16(), 18, dev)
    return lambda o: ops.groupnorm(x, g, b, 2, 240, 32, 1e-6, True, out=o)


def _layernorm(ops, dev):
    x, g, b = _rand((5, 320), _f16(), 19, dev), _rand((320,), _f16(), 20, dev), _rand((320,), _f16(), 21, dev)
    return lambda o: ops.layernorm(x, g, b, out=o)


def _attention(ops, dev):
    q, k, v = _rand((17, 320), _f16(), 22, dev), _rand((1, 320), _f16(), 23, dev), _rand((1, 320), _f16(), 24, dev)
    return lambda o: ops.attention(q, k, v, 1, 17, 1, 8, 40, out=o)


def _attention_probs(ops, dev):
    q, k = _rand((2 * 4, 320), _f16(), 25, dev), _rand((2 * 6, 320), _f16(), 26, dev)
    return lambda o: ops.attention_probs(q, k, 2, 4, 6, 8, 40, out=o)


def _causal_attention(ops, dev):
    qkv = _rand((2 * 77, 3 * 768), _f16(), 27, dev)
    return lambda o: ops.causal_attention(qkv[:, :768], qkv[:, 768:1536], qkv[:, 1536:], 2, 77, 12, 64, out=o)


def _xattn320(ops, dev):
    x, wq, wo = _rand((160, 320), _f16(), 28, dev), _rand((320, 320), _f16(), 29, dev, 320 ** -0.5), _rand((320, 320), _f16(), 30, dev, 320 ** -0.5)
    k, v = _rand((256, 320), _f16(), 31, dev), _rand((256, 320), _f16(), 32, dev)
    return lambda o: ops.xattn320(x, wq, wo, None, k, v, 2, 80, 128, 40 ** -0.5, out=o)


def _gemm8(ops, dev):
    a8, sa = ops.rowquant_fp8(_rand((77, 200), _f16(), 33, dev))
    w8, sw = ops.quantize_fp8_padded(_rand((72, 200), _f16(), 34, dev, 200 ** -0.5))
    return lambda o: ops.gemm8(a8, sa, w8, sw, None, dtype=_f16(), out=o)


def _conv2d(ops, dev):
    import torch
    x, w = _rand((25, 8), _f16(), 35, dev), _rand((8, 72), _f16(), 36, dev, 72 ** -0.5)
    scale, shift = torch.ones(8, device=dev), torch.zeros(8, device=dev)
    return lambda o: ops.conv2d(x, w, scale, shift, 1, 5, 5, 3, 3, pad=(1, 1), out=o)


def _pool3x3(ops, dev):
    x = _rand((9, 8), _f16(), 37, dev)
    return lambda o: ops.pool3x3(x, 1, 3, 3, "max_s2", out=o)


def _global_avgpool(ops, dev):
    x = _rand((4, 8), _f16(), 38, dev)
    return lambda o: ops.global_avgpool(x, 1, 4, out=o)


def _inception_input(ops, dev):
    x = _unit((1, 3, 4, 4), 39, dev)
    return lambda o: ops.inception_input(x, (5, 5), out=o)


def _timestep_embedding(ops, dev):
    import torch
    t = torch.tensor([981.0, 481.0, 1.0], device=dev)
    return lambda o: ops.timestep_embedding(t, 320, _f16(), out=o)


def _image_quantize(ops, dev):
    x = _unit((1, 3, 4, 5), 40, dev)
    return lambda o: ops.image_quantize_u8(x, out=o)


def _image_resample(ops, dev):
    x = _unit((1, 3, 4, 5), 41, dev)
    return lambda o: ops.image_resample_u8(x, (6, 7), out=o)


def _image_load(ops, dev):
    frames = _u8((1, 4, 5, 3), 42, dev)
    return lambda o: ops.image_load_u8(frames, (6, 7), out=o)


def _jpeg_encode(ops, dev):
    frames = _smooth(16, 16, dev)
    return lambda o: ops.jpeg_encode_u8(frames, out=o)


def _png_encode(name):
    def build(ops, dev):
        frames = _u8((1, 6, 7, 3), 44, dev)
        return lambda o: getattr(ops, name)(frames, out=o)
    return build


def _file(encode, frames):
    buf, lengths = encode(frames)
    return buf[0, :int(lengths[0])].cpu().numpy().tobytes()


def _jpeg_decode(ops, dev):
    from dualdiff_amd.pipeline import jpeg_input
    args = jpeg_input.upload_jpeg([_file(ops.jpeg_encode_u8, _smooth(16, 16, dev))], dev)
    return lambda o: ops.jpeg_decode_u8(*args, out=o)


def _png_decode(ops, dev):
    from dualdiff_amd.pipeline import png_input
    args = png_input.upload_png([_file(ops.png_encode_u8, _u8((1, 6, 7, 3), 46, dev))], dev)
    return lambda o: ops.png_decode_u8(*args, out=o)


def _png_condition(name):
    def build(ops, dev):
        frames = _u8((1, 4, 12, 3), 47, dev)
        return lambda o: getattr(ops, name)(frames, views=6, out=o)
    return build


def _box_views(ops, dev):
    import torch
    corners = _rand((3, 8, 3), torch.float32, 48, dev, 10.0)
    labels, offsets = torch.tensor([0, 3, 1], device=dev), torch.tensor([0, 3], dtype=torch.int32, device=dev)
    transforms = torch.eye(4, device=dev).repeat(1, 2, 1, 1).contiguous()
    return lambda o: ops.box_views(corners, labels, offsets, transforms, 2, 4, out=o)


def _bev_map_layers(ops, dev):
    from tests import test_map_input_gpu as T       # its smallest canvas, three boxes in one scene
    static, scenes = T.random_batch(40, (3,), 1140)
    args = T.device_args(40, static, scenes)
    return lambda o: ops.bev_map_layers(*args, out=o)


def _attn_heat(ops, dev):
    import torch
    from dualdiff_amd import image_tables
    maps = _unit((2, 20, 9), 49, dev)
    cols, table = torch.tensor([1, 2], dtype=torch.int32, device=dev), image_tables.device_cmap_table("coolwarm", dev)
    return lambda o: ops.attn_heat(maps, cols, table, (4, 5), out=o)


def _attn_sheet(ops, dev):
    import torch
    tiles, index = _u8((2, 4, 5, 3), 50, dev), torch.tensor([[0, 1]], dtype=torch.int32, device=dev)
    return lambda o: ops.attn_sheet_u8(tiles, index, 1, 2, 1, out=o)


def _box_tokens(dev):
    """the operands of tests/test_tokens_gpu.py::test_box_tokens_class_index_is_bounds_checked, with in-range classes"""
    import torch
    from dualdiff_amd import ops
    rows, npts, nf, ctd, ncls = 6, 8, 4, 768, 10
    pts = _unit((rows, npts, 3), 51, dev).to(_f16())
    table, null_cls = _rand((ncls, ctd), _f16(), 52, dev), _rand((ctd,), _f16(), 53, dev)
    null_pos = _rand((npts * 3 * (1 + 2 * nf),), _f16(), 54, dev)
    classes, masks = torch.tensor([3, 0, 9, 9, 1, 2], device=dev), torch.tensor([True, True, True, True, False, False], device=dev)
    pos = torch.empty((rows, npts * 3 * (1 + 2 * nf)), dtype=_f16(), device=dev)
    cat, cls_out = torch.zeros((rows, 2 * ctd), dtype=_f16(), device=dev), torch.empty((rows, ctd), dtype=_f16(), device=dev)
    freqs = [2.0 ** i for i in range(nf)]
    return (lambda: ops.box_tokens(pts, classes, masks, table, null_pos, null_cls, freqs, True, pos, cat, ctd, cls_out=cls_out)), \
        {"pos": pos, "cat": cat, "cls_out": cls_out}


def _row(make, writes=("out",)):
    return {"writes": writes, "make": make}


RAW_WRITERS = {
    "scale": _row(_elementwise("scale")),
    "add": _row(_elementwise("add")),
    "silu": _row(_elementwise("silu")),
    "gemm": _row(_gemm),
    "gemm8": _row(_op(_gemm8)),
    "conv3x3": _row(_op(_conv3x3)),
    "conv3x3_small_cout": _row(_op(_conv_out)),
    "groupnorm": _row(_op(_groupnorm)),
    "layernorm": _row(_op(_layernorm)),
    "attention": _row(_op(_attention)),
    "attention_probs": _row(_op(_attention_probs)),
    "causal_attention": _row(_op(_causal_attention)),
    "xattn320": _row(_op(_xattn320)),
    "timestep_embedding": _row(_op(_timestep_embedding)),
    "conv2d": _row(_op(_conv2d)),
    "pool3x3": _row(_op(_pool3x3)),
    "global_avgpool": _row(_op(_global_avgpool)),
    "inception_input": _row(_op(_inception_input)),
    "image_quantize_u8": _row(_op(_image_quantize)),
    "image_resample_u8": _row(_op(_image_resample)),
    "image_load_u8": _row(_op(_image_load)),
    "jpeg_encode_u8": _row(_op(_jpeg_encode, first_of_tuple=True)),
    "png_encode_u8": _row(_op(_png_encode("png_encode_u8"), first_of_tuple=True)),
    "png_encode_u8c": _row(_op(_png_encode("png_encode_u8c"), first_of_tuple=True)),
    "jpeg_decode_u8": _row(_op(_jpeg_decode, first_of_tuple=True)),
    "png_decode_u8": _row(_op(_png_decode, first_of_tuple=True)),
    "png_condition": _row(_op(_png_condition("png_condition"))),
    "png_condition_resized": _row(_op(_png_condition("png_condition_resized"))),
    "box_views": _row(_op(_box_views)),
    "bev_map_layers": _row(_op(_bev_map_layers)),
    "attn_heat": _row(_op(_attn_heat)),
    "attn_sheet_u8": _row(_op(_attn_sheet)),
    "box_tokens": _row(_box_tokens, ("pos", "cat", "cls_out")),
    "cfg_ddim_step": _row(_steps("cfg_ddim_step"), ("x_out", "x_dup")),
    "cfg_unipc_step": _row(_steps("cfg_unipc_step"), ("x_out", "x_dup", "hist")),
    "given_views_noise": _row(_steps("given_views_noise"), ("x", "x_dup")),
}
