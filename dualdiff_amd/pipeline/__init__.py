"""The pipeline's modules are imported by their dotted paths; `MapRender` (map_output.py) is also a name of the package,
resolved on first use so that importing one module does not import the others."""


def __getattr__(name):
    if name in ("MapRender", "map_output"):
        import importlib
        mod = importlib.import_module(".map_output", __name__)
        return mod if name == "map_output" else mod.MapRender
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
