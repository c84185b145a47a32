"""The pipeline's modules are imported by their dotted paths; `MapRender` (map_output.py), `BoxOverlay`
(box_output.py), `OccRender` (occ_render.py), `BevMapInput` (map_input.py), `AttnMapRender` (attn_output.py), `FgmMask`
(fgm_mask.py) and `FusedAdamW` (optim.py) are also names of the package, resolved on first use so that importing one module
does not import the others."""

_LAZY = {"MapRender": "map_output", "BoxOverlay": "box_output", "OccRender": "occ_render", "BevMapInput": "map_input",
         "AttnMapRender": "attn_output", "FgmMask": "fgm_mask", "FusedAdamW": "optim"}


def __getattr__(name):
    if name in _LAZY or name in _LAZY.values():
        import importlib
        mod = importlib.import_module("." + _LAZY.get(name, name), __name__)
        return mod if name in _LAZY.values() else getattr(mod, name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
