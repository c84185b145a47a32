#!/usr/bin/env python3
"""What does the Python side ask the library to do?  Every dd_* call of a pytest run, argument by argument.

    DD_AUTOTUNE=0 python tools/launch_trace.py OUT.jsonl [--timer] -- tests/test_ops_gpu.py -m gpu -q

Replaces dualdiff_amd._native.load with a wrapper whose result stands in for the library, runs pytest.main on the given
arguments in this process, and appends one JSON line per dd_* call: the function's name and every argument.  Integers
and floats are written by value, a ctypes.byref(struct) is expanded into its fields, ctypes arrays into their values.
A pointer — a pointer argument or a pointer field — is written as null or as [n, address % 256]: n numbers the distinct
non-null pointers of that one call in order of first appearance (two fields on one buffer get one number); raw addresses
differ from run to run and are not written.  The stream (the last argument of every launch) is "stream0" for the null
stream, else "stream".

Launches go to OUT.jsonl.  Calls that only ask the planner (workspace sizes, kernel names, tile ids, ...) go to
OUT.jsonl.planner: a change of the host code may make fewer of those, never other launches.

--timer installs ops.KernelTimer(shapes=True) for the whole session and appends its records — (name, flops, nbytes,
staged), without the events — to OUT.jsonl when the session ends: the names and the FLOP / byte formulas of every timed
launch site.

A host-side refactor is checked by running this on both commits and comparing the files line by line.  DD_AUTOTUNE=0
keeps shapes outside the tracked table on the library's own deterministic plan instead of a timing race.
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANNER = ("_workspace_bytes", "_kernel_name")
PLANNER_NAMES = {"dd_groupnorm_is_fused", "dd_gemm_num_tiles", "dd_gemm_tile_id", "dd_abi_version", "dd_desc_size",
                 "dd_error_string", "dd_target_arch"}
_BYREF = type(ctypes.byref(ctypes.c_int()))


def is_planner(name):
    return name.endswith(PLANNER) or name in PLANNER_NAMES


class Labels:
    """Pointer labels of one call."""

    def __init__(self):
        self.seen = {}

    def __call__(self, p):
        p = p.value if isinstance(p, ctypes.c_void_p) else p
        if not p:
            return None
        return [self.seen.setdefault(p, len(self.seen)), p % 256]


def plain(v):
    if isinstance(v, ctypes.Array):
        return [plain(x) for x in v]
    if isinstance(v, ctypes._SimpleCData):
        v = v.value
    return v.decode() if isinstance(v, bytes) else v


def expand(struct, label):
    out = {}
    for name, ftype in struct._fields_:
        v = getattr(struct, name)
        out[name] = label(v) if ftype is ctypes.c_void_p else plain(v)
    return out


def record(name, args, argtypes):
    label = Labels()
    out = []
    launch = not is_planner(name)
    for i, a in enumerate(args):
        at = argtypes[i] if i < len(argtypes) else None
        if isinstance(a, _BYREF):
            out.append(expand(a._obj, label))
        elif isinstance(a, ctypes.Structure):
            out.append(expand(a, label))
        elif at is ctypes.c_void_p:
            if launch and i == len(argtypes) - 1:
                out.append("stream" if label(a) else "stream0")
            else:
                out.append(label(a))
        else:
            out.append(plain(a))
    return {"fn": name, "args": out}


class LibProxy:
    def __init__(self, lib, sink, signatures):
        self.__dict__.update(_lib=lib, _sink=sink, _sigs=signatures)

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("dd_"):
            return fn
        argtypes = self._sigs[name][1] if name in self._sigs else ()
        out = self._sink[is_planner(name)]

        def call(*args):
            out.write(json.dumps(record(name, args, argtypes)) + "\n")
            return fn(*args)
        self.__dict__[name] = call
        return call


def main():
    argv = sys.argv[1:]
    rest = []
    if "--" in argv:
        rest = argv[argv.index("--") + 1:]
        argv = argv[:argv.index("--")]
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("out")
    ap.add_argument("--timer", action="store_true", help="install KernelTimer(shapes=True) and append its records")
    args = ap.parse_args(argv)
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import pytest
    from dualdiff_amd import _native, ops

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    sink = {False: open(args.out, "w"), True: open(args.out + ".planner", "w")}
    real_load, proxies = _native.load, {}

    def load(*a, **kw):
        lib = real_load(*a, **kw)
        if id(lib) not in proxies:
            proxies[id(lib)] = LibProxy(lib, sink, _native.SIGNATURES)
        return proxies[id(lib)]
    _native.load = load
    timer = None
    if args.timer:
        timer = ops.KernelTimer(shapes=True)
        ops.set_timer(timer)
    try:
        rc = pytest.main(rest)
    finally:
        _native.load = real_load
        if timer is not None:
            ops.set_timer(None)
            for r in timer.records:
                sink[False].write(json.dumps({"timer": [r[0], r[1], r[2], r[5]]}) + "\n")
        for f in sink.values():
            f.close()
    return int(rc)


if __name__ == "__main__":
    sys.exit(main())
