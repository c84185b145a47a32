"""Map output on the GPU: the BEV map picture the reference's demo and validation path makes of every sample.

The reference's `run_one_batch` (misc/test_utils.py:344-348) starts with `visualize_map(cfg, bev_map_with_aux[i])`
(runner/map_visualizer.py:143-211), and tools/test.py:76 saves the result as `{n}_map.png`:

1. `render_static` (:106-118), a Python loop over the pixels: among the set static layers of a pixel the class with the
   greatest index in `STATIC_PRIORITY`, in its `COLORS` entry;
2. `render_dynamic` (:121-132): the colour of `argmax` over the dynamic layers, which replaces the static colour where any
   dynamic layer is set (:185-189); a pixel with nothing set is `COLORS["nothing"]`;
3. `Image.resize` to `target_size` (PIL's default for RGB, bicubic), then `rotate(90)` (:193-198);
4. `show_legend` (:80-103) of the classes in use, a matplotlib figure, pasted to the right or below (:200-211).

Here 1-3 are three launches per batch (`ops.map_render_u8`, the PIL-exact `ops.image_resample_u8`, `ops.map_compose_u8`)
with no host synchronisation, byte for byte; `MapRender.__call__` reads the classes in use back (4 bytes per sample),
draws each distinct legend once on the host and composes the samples that share one in one launch.

    render = MapRender.from_config(cfg)                   # cfg.dataset.map_classes / .object_classes
    frames, used = render.render(bev_map_with_aux)        # (b, T, T, 3) uint8 and (b,) int32, on the GPU
    pictures = render(bev_map_with_aux)                   # b uint8 tensors: visualize_map(cfg, maps[i]) each
    save_png(pictures[i][None], ["%d_map.png" % n])       # image_output.save_png / encode_png take them as they are

There is no writer of its own: a picture is a uint8 (H, W, 3) frame, and `encode_png` / `save_png` of
pipeline/image_output.py take a batch of those.

A quirk that is kept: `argmax` is 0 where no dynamic layer is set, so with dynamic layers present the first object class
is in the legend of every map that has a pixel free of objects (:127-128).  Only square maps are accepted: a non-square
picture goes through PIL's affine `rotate`, which is not built.  The box overlays (`show_box_on_views`) are
pipeline/box_output.py.
"""
import numpy as np
import torch

from .. import ops as O
from .._consts import device_const
from .image_output import _get

# runner/map_visualizer.py:13-44, in its order: the legend's patches follow it
COLORS = {
    "drivable_area": (166, 206, 227), "drivable_area*": (144, 196, 255), "lane": (110, 110, 110),
    "road_segment": (90, 90, 90), "ped_crossing": (251, 154, 153), "walkway": (227, 26, 28),
    "stop_line": (253, 191, 111), "carpark_area": (255, 127, 0), "road_block": (178, 223, 138),
    "road_divider": (255, 200, 0), "lane_divider": (130, 130, 130),
    "car": (255, 158, 0), "truck": (255, 99, 71), "construction_vehicle": (233, 150, 70), "bus": (255, 127, 80),
    "trailer": (255, 140, 0), "barrier": (112, 128, 144), "motorcycle": (255, 61, 99), "bicycle": (220, 20, 60),
    "pedestrian": (0, 0, 230), "traffic_cone": (47, 79, 79),
    "nothing": (200, 200, 200),
}
# :49-60: a later entry covers an earlier one
STATIC_PRIORITY = ("drivable_area", "drivable_area*", "road_block", "walkway", "stop_line", "carpark_area", "ped_crossing",
                   "divider", "road_divider", "lane_divider")
BAD_VALUE_BIT = 31                        # of a `used` word: a uint8 map held a value other than 0 / 1


def target_side(s, target_size):
    """The side of the resized picture, with the reference's own float expression (:195-196)."""
    ratio = max(target_size / s, target_size / s)
    return int(s * ratio)


def matplotlib_legend(names, long_edge_size, ncol=4):
    """`show_legend` (:80-103): a matplotlib figure legend of the classes in `names`, in the order of COLORS, saved as
    a tight PNG and resized with NEAREST so that its long edge is `long_edge_size` -> (lh, lw, 3) uint8."""
    try:
        import matplotlib.patches as mpatches
        import matplotlib.pyplot as plt
    except ImportError as e:
        raise ImportError("the default legend of MapRender needs matplotlib, which is not installed; pass legend= a "
                          "function (names, long_edge_size) -> (lh, lw, 3) uint8 array, or use MapRender.render") from e
    try:
        from PIL import Image
    except ImportError as e:
        raise ImportError("the default legend of MapRender reads matplotlib's PNG with Pillow (PIL), which is not "
                          "installed") from e
    import io
    fig = plt.figure("Legend plot")
    patches = [mpatches.Patch(color=[c / 255.0 for c in v], label=k) for k, v in COLORS.items() if k in names]
    fig.legend(handles=patches, loc="center", ncol=ncol)
    with io.BytesIO() as buf:
        fig.savefig(buf, format="png", bbox_inches="tight")
        im = Image.open(buf)
        w, h = im.size
        ratio = long_edge_size / max(w, h)
        if w > h:
            size = (long_edge_size, int(h * ratio))
        elif h > w:
            size = (int(w * ratio), long_edge_size)
        else:
            size = (long_edge_size, long_edge_size)
        out = np.array(im.resize(size, resample=Image.NEAREST))[..., :3]
    plt.close("all")
    return out


def _class_list(classes, what):
    if classes is None:
        return ()
    classes = tuple(classes)
    for name in classes:
        if name is None:
            raise ValueError("%s holds a None: the reference then skips the whole group of layers, which is not built" % what)
        if not isinstance(name, str):
            raise ValueError("%s must hold class names, got %r" % (what, name))
    return classes


class MapRender:
    """`visualize_map` on the GPU.  map_classes / object_classes: the lists of `cfg.dataset`, either may be None (or
    empty); target_size: the side the picture is resized to."""

    def __init__(self, map_classes, object_classes, target_size=400):
        self.map_classes = _class_list(map_classes, "map_classes")
        self.object_classes = _class_list(object_classes, "object_classes")
        if not self.map_classes and not self.object_classes:
            raise ValueError("map_classes and object_classes are both None or empty: there is no layer to draw")
        for name in self.map_classes:
            if name not in STATIC_PRIORITY:
                raise ValueError("map class %r is not in STATIC_PRIORITY (%s): the reference cannot rank it"
                                 % (name, ", ".join(STATIC_PRIORITY)))
            if name not in COLORS:
                raise ValueError("map class %r has no colour in COLORS" % (name,))
        for name in self.object_classes:
            if name not in COLORS:
                raise ValueError("object class %r has no colour in COLORS" % (name,))
        self.ns, self.nd = len(self.map_classes), len(self.object_classes)
        if self.ns + self.nd > O.MAP_MAX_LAYERS:
            raise ValueError("at most %d layers fit the `used` word, got %d map + %d object classes"
                             % (O.MAP_MAX_LAYERS, self.ns, self.nd))
        if isinstance(target_size, bool) or not isinstance(target_size, int) or target_size <= 0:
            raise ValueError("target_size must be a positive int, got %r" % (target_size,))
        self.target_size = target_size

    @classmethod
    def from_config(cls, cfg, target_size=400):
        """cfg: any mapping (or object) with `dataset.map_classes` and `dataset.object_classes`."""
        ds = _get(cfg, "dataset")
        if ds is None:
            raise ValueError("config has no `dataset` section")
        mc, oc = _get(ds, "map_classes"), _get(ds, "object_classes")
        return cls(None if mc is None else list(mc), None if oc is None else list(oc), target_size=target_size)

    def static_table(self, ns=None):
        """(ns + 1, 4) float32: colour / 255 and rank in STATIC_PRIORITY per static layer, then the "nothing" row."""
        names = self.map_classes[:self.ns if ns is None else ns]
        rows = [[np.float32(c) / np.float32(255) for c in COLORS[n]] + [np.float32(STATIC_PRIORITY.index(n))] for n in names]
        rows.append([np.float32(c) / np.float32(255) for c in COLORS["nothing"]] + [np.float32(-1)])
        return np.asarray(rows, dtype=np.float32)

    def dynamic_table(self, nd=None):
        """(nd, 4) float32: colour / 255 per dynamic layer (the fourth column is unused)."""
        names = self.object_classes[:self.nd if nd is None else nd]
        return np.asarray([[np.float32(c) / np.float32(255) for c in COLORS[n]] + [np.float32(0)] for n in names],
                          dtype=np.float32).reshape(len(names), 4)

    def layers(self, channels):
        """(static, dynamic) layers read of a map with `channels` channels (:168-175)."""
        ns = min(self.ns, channels)
        return ns, max(0, min(self.nd, channels - self.ns))

    def names(self, used_word):
        """The class names of one `used` word: what the reference hands to `show_legend`."""
        word = int(used_word) & 0xffffffff
        every = self.map_classes + self.object_classes
        return {name for k, name in enumerate(every) if word >> k & 1}

    def _resized(self, maps):
        if not isinstance(maps, torch.Tensor) or maps.dim() != 4 or maps.numel() == 0:
            raise ValueError("maps must be a (b, C, S, S) tensor, got %s"
                             % (tuple(maps.shape) if isinstance(maps, torch.Tensor) else type(maps).__name__,))
        if maps.shape[2] != maps.shape[3]:
            raise ValueError("non-square maps are not built (%d x %d): without `expand` PIL turns them on its affine path"
                             % (maps.shape[2], maps.shape[3]))
        if maps.dtype == torch.bool:
            u8 = maps.contiguous().view(torch.uint8)
        elif maps.dtype == torch.uint8:
            u8 = maps.contiguous()
        elif maps.dtype.is_floating_point:
            u8 = (maps != 0).view(torch.uint8)
        else:
            raise ValueError("maps must be bool, uint8 (0 / 1) or a float type, got %s" % (maps.dtype,))
        ns, nd = self.layers(maps.shape[1])
        dev = maps.device
        stab = device_const(("map_static", self.map_classes[:ns]), dev, lambda: torch.from_numpy(self.static_table(ns)))
        dtab = None
        if nd > 0:
            dtab = device_const(("map_dynamic", self.object_classes[:nd]), dev,
                                lambda: torch.from_numpy(self.dynamic_table(nd)))
        img, used = O.map_render_u8(u8, stab, dtab, ns, nd)
        t = target_side(maps.shape[2], self.target_size)
        if t <= 0:
            raise ValueError("target_size %d gives an empty picture of a %d x %d map" % (self.target_size, maps.shape[2],
                                                                                       maps.shape[2]))
        return O.image_resample_u8(img, (t, t)), used

    @torch.no_grad()
    def render(self, maps):
        """maps (b, C, S, S) on the device, bool / uint8 (0 / 1) / float (`!= 0`) -> (frames (b, T, T, 3) uint8, used (b,)
        int32), both on the device, no host synchronisation: frames[i] is the picture `visualize_map` holds before it adds
        the legend, used[i] the classes it hands to `show_legend` (`names`); bit 31: a uint8 map held another value."""
        resized, used = self._resized(maps)
        return O.map_compose_u8(resized), used

    @torch.no_grad()
    def __call__(self, maps, legend=None):
        """-> a list of b uint8 tensors (H_i, W_i, 3) on the device, `visualize_map(cfg, maps[i], target_size)` each.
        legend: (names: set of str, long_edge_size: int) -> (lh, lw, 3) uint8 ndarray; default `matplotlib_legend`.
        It goes to the right of the picture where it is taller than wide, below otherwise, and must be as long as the
        side it lies along.  One readback of `used`; every distinct legend is drawn once per process and kept on the
        device (a constant under the rule of _consts, keyed by the legend function, the class set and the size)."""
        legend = matplotlib_legend if legend is None else legend
        resized, used = self._resized(maps)
        words = used.cpu().tolist()                      # the one synchronisation: 4 bytes per sample
        t = resized.shape[1]
        groups = {}
        for i, word in enumerate(words):
            if word < 0:
                raise ValueError("map %d holds a value other than 0 / 1" % i)
            groups.setdefault(word, []).append(i)
        order = [i for idx in groups.values() for i in idx]
        index = torch.tensor(order, dtype=torch.int32).to(resized.device) if len(groups) > 1 else None
        out, start = [None] * len(words), 0
        for word, idx in groups.items():
            names = self.names(word)

            def build(names=names):
                arr = np.ascontiguousarray(legend(set(names), self.target_size))
                if arr.ndim != 3 or arr.shape[2] != 3 or arr.dtype != np.uint8 or arr.size == 0:
                    raise ValueError("legend must return a uint8 (lh, lw, 3) array, got %s %s" % (arr.dtype, arr.shape))
                return torch.from_numpy(arr)
            leg = device_const(("map_legend", legend, tuple(sorted(names)), self.target_size), resized.device, build)
            lh, lw = leg.shape[0], leg.shape[1]
            side = "right" if lh > lw else "below"
            if (lh if side == "right" else lw) != t:
                raise ValueError("a %d x %d legend does not fit %s a %d x %d picture: numpy cannot paste it either"
                                 % (lh, lw, side, t, t))
            pics = O.map_compose_u8(resized, None if index is None else index[start:start + len(idx)], leg, side)
            for j, i in enumerate(idx):
                out[i] = pics[j]
            start += len(idx)
        return out
