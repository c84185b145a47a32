"""Attention-map pictures on the GPU against the host restatement (tests/attn_output_reference.py: matplotlib's own
`cmap(...)`, PIL's own `resize`, view_images' arithmetic).  Every step is exact — the fp64 normalisation, the colour-map
index, PIL's integer resize, the paste — so every comparison is equality of bytes."""
import functools

import numpy as np
import pytest
import torch

from dualdiff_amd import image_tables, ops
from dualdiff_amd.pipeline import attn_output as AO
from dualdiff_amd.pipeline.image_output import encode_png
from dualdiff_amd.pipeline.png_input import decode_png
from tests import attn_output_reference as R

pytestmark = pytest.mark.gpu

LAUNCHES = ["attn_heat", "image_resample_u8", "attn_sheet_u8"]
# name -> (views, hw, size, n, first box column): the reference's own size, and a small one whose 35 rows and 9 columns are
# no multiple of the kernel's 64-row chunks and 16-column groups
SHAPES = {"full": (2, (28, 50), (224, 400), 106, 78), "small": (1, (5, 7), (40, 56), 9, 7)}
SPECIAL = ("constant", "edges", "subnormal", "adjacent", "span")          # in columns 1 .. 5 of view 0


def special_column(kind, q, rng):
    f = np.float32
    if kind == "constant":                               # 0 / 0: NaN everywhere, the "bad" colour
        return np.full(q, 0.0094339624, dtype=f)
    if kind == "edges":                                  # exact k / 256: every bin edge, and X = 1
        x = (np.arange(q) * 37 % 257).astype(f) / f(256)
        x[0], x[1] = 0.0, 1.0
        return x
    if kind == "subnormal":                              # float32 subnormals with exact zeros and -0.0
        x = (rng.randint(1, 1 << 23, q).astype(np.uint32)).view(f).copy()
        x[::5], x[1::7] = 0.0, -0.0
        x[2], x[3] = np.uint32(1).view(f), np.uint32((1 << 23) - 1).view(f)
        return x
    if kind == "adjacent":                               # min and max are neighbouring floats: X is 0 or 1
        lo = f(0.3)
        x = np.where(rng.randint(0, 2, q) == 1, np.nextafter(lo, f(1)), lo).astype(f)
        x[0], x[1] = lo, np.nextafter(lo, f(1))
        return x
    if kind == "span":                                   # 1e-38 .. 1
        x = (f(10) ** rng.uniform(-38, 0, q)).astype(f)
        x[0], x[1] = f(1e-38), f(1)
        return x
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def host_maps(name):
    """(views, h * w, n) float32: softmax rows of logits x 4, and in view 0 the columns that can go wrong.  Built once,
    shared, never written to."""
    views, hw, _, n, first = SHAPES[name]
    q = hw[0] * hw[1]
    rng = np.random.RandomState(11 + n)
    logits = rng.randn(views, q, n) * 4
    e = np.exp(logits - logits.max(-1, keepdims=True))
    maps = (e / e.sum(-1, keepdims=True)).astype(np.float32)
    for j, kind in enumerate(SPECIAL):
        maps[0, :, 1 + j] = special_column(kind, q, rng)
    maps[0, :, n - 1] = special_column("subnormal", q, rng)                 # one among the box columns too
    assert np.abs(maps[0, :, 3]).max() < np.finfo(np.float32).tiny and (maps[0, :, 3] != 0).any()
    maps.setflags(write=False)
    return maps


def device_maps(name, gpu, pitch=None):
    """The maps on the device: contiguous, or a view of a buffer of row pitch `pitch` (what a capture holds)."""
    m = torch.from_numpy(host_maps(name).copy())
    if pitch is None:
        return m.to(gpu)
    buf = torch.full(m.shape[:2] + (pitch,), float("nan"), device=gpu)
    view = buf[..., :m.shape[2]]
    view.copy_(m)
    assert view.stride(1) == pitch and not view.is_contiguous()
    return view


def render_for(name):
    _, hw, size, _, _ = SHAPES[name]
    return AO.AttnMapRender(hw=hw, size=size)


def want_tile(name, v, col):
    _, hw, size, _, _ = SHAPES[name]
    return R.tile(host_maps(name)[v, :, col], hw, size)


def same(t, want):
    return tuple(t.shape) == want.shape and t.dtype == torch.uint8 and np.array_equal(t.cpu().numpy(), want)


class Launches:
    """Counts the library launches that go through ops._timer.launch, by name."""

    def __init__(self, monkeypatch):
        self.names = []
        real = ops._timer.launch

        def launch(what, fn, *a, **kw):
            self.names.append(what)
            return real(what, fn, *a, **kw)
        monkeypatch.setattr(ops._timer, "launch", launch)


# ---- tiles ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(SHAPES))
def test_every_column_equals_the_restatement(gpu, name):
    views, hw, size, n, _ = SHAPES[name]
    r = render_for(name)
    maps = device_maps(name, gpu, pitch=12 if name == "small" else None)     # small: a non-contiguous view at pitch 12
    got = r.tiles(maps, list(range(n)), strip=False)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (views, n) + size + (3,)
    got = got.cpu().numpy()
    for v in range(views):
        for c in range(n):
            assert np.array_equal(got[v, c], want_tile(name, v, c)), (v, c)
    assert not want_tile(name, 0, 1).any()                                   # the constant column is black
    assert len({want_tile(name, 0, 1 + j).tobytes() for j in range(len(SPECIAL))}) == len(SPECIAL)
    striped = r.tiles(maps, torch.tensor([3, 0, 3], dtype=torch.int32, device=gpu))      # any order, repeats, a tensor
    assert tuple(striped.shape) == (views, 3, size[0] + r.strip, size[1], 3)
    for i, c in enumerate((3, 0, 3)):
        assert same(striped[0, i], R.with_strip(want_tile(name, 0, c), r.label_ratio))


def test_a_custom_colour_map_is_looked_up_the_same_way(gpu):
    table = (np.arange(768).reshape(256, 3) * 7 % 256).astype(np.uint8)
    _, hw, size, n, _ = SHAPES["small"]
    r = AO.AttnMapRender(hw=hw, size=size, cmap=table)
    got = r.tiles(device_maps("small", gpu), list(range(1, 6)), strip=False)
    for j in range(5):
        rgb = R.colour_by_table(R.normalise(host_maps("small")[0, :, 1 + j], hw), table)
        assert same(got[0, j], R.resized(rgb, size)), j


# ---- sheets --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_text", [1, 3, 4, 5, 7, 8])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_text_sheets_equal_view_images(gpu, name, n_text):
    views, hw, size, _, _ = SHAPES[name]
    r = render_for(name)
    maps = device_maps(name, gpu)
    if n_text == 1:
        # 1 tile on 4 rows: (1 + 1) // 4 = 0 columns.  The reference's canvas is then offset * -1 pixels wide: numpy refuses
        # a negative width, and where the offset is 0 (tiles under 50 rows) the canvas has no pixel.  No picture either way.
        try:
            assert R.text_sheet(host_maps(name)[0], 1, hw, size).size == 0
        except ValueError:
            pass
        with pytest.raises(ValueError, match="no column"):
            r.text_sheets(maps, 1)
        num_rows = 1
    else:
        num_rows = 4
    got = r.text_sheets(maps, n_text, num_rows=num_rows)
    assert got.shape[0] == views
    for v in range(views):
        assert same(got[v], R.text_sheet(host_maps(name)[v], n_text, hw, size, num_rows=num_rows)), v


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_box_sheets_with_many_one_and_no_box_column(gpu, name):
    views, hw, size, n, first = SHAPES[name]
    r = render_for(name)
    maps = device_maps(name, gpu)
    for width in (n, first + 1):                         # every box column; one (a view of row pitch n)
        got = r.box_sheets(maps[:, :, :width], first=first)
        for v in range(views):
            assert same(got[v], R.box_sheet(host_maps(name)[v, :, :width], hw, size, first=first)), (width, v)
    assert r.box_sheets(maps[:, :, :first], first=first) is None


@pytest.mark.parametrize("per_view", [False, True])
def test_label_strips_land_in_their_cells(gpu, per_view):
    views, hw, size, _, _ = SHAPES["full"]
    r = render_for("full")
    n_text, lh, tw = 7, r.strip, size[1]
    rng = np.random.RandomState(5)
    strips = rng.randint(0, 255, ((views,) if per_view else ()) + (n_text, lh, tw, 3)).astype(np.uint8)
    strips[..., 0, 0, :] = np.arange(1, n_text + 1, dtype=np.uint8)[:, None]              # a distinct mark per tile
    got = r.text_sheets(device_maps("full", gpu), n_text, labels=torch.from_numpy(strips).to(gpu))
    for v in range(views):
        want = R.text_sheet(host_maps("full")[v], n_text, hw, size, strips=strips[v] if per_view else strips)
        assert same(got[v], want), v
    th, gap = size[0] + lh, r.gap(size[0] + lh)
    assert int(got[0, 2 * (th + gap) + size[0], tw + gap, 0]) == 6                        # cell (2, 1) is tile 5: mark 6


def test_string_labels_change_the_strips_and_nothing_else(gpu):
    views, hw, size, _, _ = SHAPES["full"]
    r = render_for("full")
    words = ["a", "car", "a", "bus"]
    maps = device_maps("full", gpu)
    plain, drawn = r.text_sheets(maps, 4).cpu().numpy(), r.text_sheets(maps, 4, labels=words).cpu().numpy()
    th = size[0] + r.strip
    gap = r.gap(th)
    differs = (plain != drawn).any(axis=(0, 2, 3))
    rows = np.arange(plain.shape[1])
    assert differs.any() and not differs[(rows % (th + gap)) < size[0]].any()             # only rows of a strip differ
    want = np.stack([AO.draw_label(w, r.strip, size[1]) for w in words])
    for i in range(4):
        assert np.array_equal(drawn[1, i * (th + gap) + size[0]: i * (th + gap) + th, :size[1]], want[i]), i


# ---- the capture hand-off ---------------------------------------------------------------------------------------------

class FakeCapture:
    """What AttnMapRender asks of a CrossAttnMapCapture: mean_map(hw)."""

    def __init__(self, maps):
        self.maps, self.asked = maps, []

    def mean_map(self, hw):
        self.asked.append(tuple(hw))
        return self.maps


def test_a_capture_buffer_with_a_padded_pitch_is_taken_as_it_is(gpu, monkeypatch):
    views, hw, size, n, first = SHAPES["full"]
    pitch = (n + 3) // 4 * 4                             # networks/attn_maps.py: rows at a pitch of whole float4 groups
    assert pitch != n
    maps = device_maps("full", gpu, pitch=pitch)
    seen = []
    real = ops.attn_heat

    def heat(m, *a, **kw):
        seen.append((m.data_ptr(), m.stride()))
        return real(m, *a, **kw)
    monkeypatch.setattr(ops, "attn_heat", heat)
    r = render_for("full")
    cap = FakeCapture(maps)
    text, box = r(cap, 5)
    assert cap.asked == [hw]
    assert seen == [(maps.data_ptr(), (hw[0] * hw[1] * pitch, pitch, 1))] * 2              # no copy was made
    for v in range(views):
        assert same(text[v], R.text_sheet(host_maps("full")[v], 5, hw, size)), v
        assert same(box[v], R.box_sheet(host_maps("full")[v], hw, size, first=first)), v


# ---- buffer discipline ---------------------------------------------------------------------------------------------------

def guarded(shape, dtype, gpu, offset):
    """A tensor of `shape` inside a larger buffer of canaries, `offset` elements in -> (tensor, check)."""
    numel = int(np.prod(shape))
    canary = -123456.0 if dtype == torch.float32 else 0xA5
    big = torch.full((offset + numel + 64,), canary, dtype=dtype, device=gpu)
    inner = big[offset:offset + numel].view(shape)

    def intact():
        return bool((big[:offset] == canary).all()) and bool((big[offset + numel:] == canary).all())
    return inner, intact


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_nothing_is_written_outside_the_outputs_and_a_rerun_gives_the_same_bytes(gpu, name):
    views, hw, size, n, _ = SHAPES[name]
    r = render_for(name)
    maps = device_maps(name, gpu, pitch=n + 3)
    cols = torch.arange(1, 8, dtype=torch.int32, device=gpu)
    table = image_tables.device_cmap_table("coolwarm", gpu)
    t, th = 7, size[0] + r.strip
    rows, ncols, cells = AO.sheet_layout(t, 4)
    index = torch.tensor([[c + v * t if c >= 0 else -1 for c in cells] for v in range(views)], dtype=torch.int32, device=gpu)
    gap = r.gap(th)
    labels = torch.randint(0, 255, (views * t, r.strip, size[1], 3), dtype=torch.uint8, device=gpu)
    img, img_ok = guarded((views * t, 3) + hw, torch.float32, gpu, 64)
    u8, u8_ok = guarded((views * t, th, size[1], 3), torch.uint8, gpu, 64)
    # the sheet at an odd address: no alignment is asked of it
    sheet, sheet_ok = guarded((views, rows * th + gap * (rows - 1), ncols * size[1] + gap * (ncols - 1), 3), torch.uint8,
                              gpu, 67)
    first = None
    for _ in range(2):
        sheet.fill_(0x5A)
        assert ops.attn_heat(maps, cols, table, hw, out=img) is img
        ops.image_resample_u8(img, size, padding=(0, 0, 0, r.strip), fill=255, out=u8)
        assert ops.attn_sheet_u8(u8, index, rows, ncols, gap, labels, out=sheet) is sheet
        assert img_ok() and u8_ok() and sheet_ok()
        if first is None:
            first = (img.clone(), sheet.clone())
    assert torch.equal(first[0].view(torch.int32), img.view(torch.int32)) and torch.equal(first[1], sheet)
    strips = labels.reshape(views, t, r.strip, size[1], 3).cpu().numpy()
    for v in range(views):
        assert same(sheet[v], R.text_sheet(host_maps(name)[v], t, hw, size, strips=strips[v])), v


def test_text_sheets_is_three_launches_and_no_readback(gpu, monkeypatch):
    views, hw, size, _, _ = SHAPES["full"]
    r = render_for("full")
    maps = device_maps("full", gpu)
    strips = torch.zeros((views, 8, r.strip, size[1], 3), dtype=torch.uint8, device=gpu)
    want = r.text_sheets(maps, 8, labels=strips)         # the constants of this shape are on the device after this call
    spy = Launches(monkeypatch)
    reads = []
    for method in ("item", "cpu", "tolist", "numpy"):
        def record(self, *a, _method=method, **kw):
            reads.append(_method)
            raise AssertionError("text_sheets read a tensor back: .%s()" % _method)
        monkeypatch.setattr(torch.Tensor, method, record)
    got = r.text_sheets(maps, 8, labels=strips)
    monkeypatch.undo()
    assert spy.names == LAUNCHES and reads == []
    assert torch.equal(got, want)
    spy = Launches(monkeypatch)
    r.box_sheets(maps)
    assert spy.names == LAUNCHES


# ---- the files -----------------------------------------------------------------------------------------------------------

def test_png_round_trip_and_save(gpu, tmp_path):
    r = render_for("small")
    maps = device_maps("small", gpu)
    text, box = r(maps, 5)
    assert box is None                                   # 9 context columns: none from 78 on
    files = encode_png(text)
    assert torch.equal(decode_png(files, device=gpu), text)
    box = r.box_sheets(maps, first=SHAPES["small"][4])
    paths = r.save(tmp_path, text, box)
    assert [p.rsplit("/", 1)[1] for p in paths] == ["view_images_0.png", "view_images_0box.png"]
    from PIL import Image
    assert np.array_equal(np.asarray(Image.open(paths[0])), text[0].cpu().numpy())
    assert np.array_equal(np.asarray(Image.open(paths[1])), box[0].cpu().numpy())
