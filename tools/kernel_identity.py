#!/usr/bin/env python3
"""Are the device kernels of two builds of the library the same machine code?

    python tools/kernel_identity.py OLD/libdualdiff_hip.so NEW/libdualdiff_hip.so [--match dd_gemm,dd_conv3s,dd_splitk]

Reads the gfx950 code objects out of both libraries (the offload bundles of their .hip_fatbin section) and compares, per
kernel: the set of kernels, the code bytes, and the kernel descriptor (the hardware's statement of VGPRs, SGPRs, scratch,
LDS and with them occupancy).  Kernels are keyed by their demangled name up to the closing `>` of the template arguments
(the parameter list is not part of the identity: a kernel-argument struct may move between namespaces).
Exit status 0 when nothing differs.  Needs no GPU and no tool besides Python.

A refactor that moves kernels between translation units, or a compiler flag that should not matter, is checked with
this before any timing is looked at: a kernel whose bytes differ is a different kernel.
"""
import argparse
import hashlib
import re
import struct
import sys

MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def code_objects(path):
    """Every amdgcn ELF of every offload bundle in the file."""
    data = open(path, "rb").read()
    if b"CCOB" in data and MAGIC not in data:
        sys.exit("%s: compressed offload bundles; extract them with clang-offload-bundler first" % path)
    pos = data.find(MAGIC)
    while pos >= 0:
        n, = struct.unpack_from("<Q", data, pos + len(MAGIC))
        at = pos + len(MAGIC) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", data, at)
            triple = data[at + 24:at + 24 + tlen].decode()
            at += 24 + tlen
            if "amdgcn" in triple and size:
                yield data[pos + off:pos + off + size]
        pos = data.find(MAGIC, pos + len(MAGIC))


def kernels_of(elf):
    """{mangled name: (code bytes, descriptor bytes)} of one ELF64 code object."""
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", elf, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", elf, shoff + i * shentsize) for i in range(shnum)]
    out, funcs, descs = {}, {}, {}
    for sec in secs:
        if sec[1] != 2:                                   # SHT_SYMTAB
            continue
        strtab = secs[sec[6]]
        for i in range(sec[5] // 24):
            name_off, info, _, shndx, value, size = struct.unpack_from("<IBBHQQ", elf, sec[4] + i * 24)
            if not 0 < shndx < shnum:
                continue
            end = elf.index(b"\0", strtab[4] + name_off)
            name = elf[strtab[4] + name_off:end].decode()
            home = secs[shndx]
            body = elf[home[4] + value - home[3]:home[4] + value - home[3] + size]
            if info & 15 == 2:                            # STT_FUNC
                funcs[name] = body
            elif name.endswith(".kd"):                    # without the code's offset from the descriptor: layout, not content
                descs[name[:-3]] = body[:16] + body[24:]
    for name, kd in descs.items():
        if name in funcs:
            out[name] = (funcs[name], kd)
    return out


ARG = re.compile(r"DF16_|DF16b|Li(n?\d+)E|Lb([01])E|Lj(\d+)E|[fdihjb]")
PLAIN = {"DF16_": "_Float16", "DF16b": "__bf16", "f": "float", "d": "double", "i": "int", "h": "unsigned char", "j": "unsigned", "b": "bool"}


def key_of(name):
    """`kernel<args>` of a mangled kernel name, without its parameter list: enough of the Itanium grammar for kernels
    whose template arguments are types, integers and booleans (binutils' c++filt does not know DF16_ / DF16b); any other
    name is its own key."""
    m = re.match(r"_ZN?(?:12_GLOBAL__N_1)?(\d+)", name)
    if not m:
        return name
    end = m.end() + int(m.group(1))
    base, args = name[m.end():end], []
    if name[end:end + 1] != "I":
        return base
    at = end + 1
    while name[at:at + 1] != "E":
        a = ARG.match(name, at)
        if not a:
            return name
        tok = a.group(0)
        args.append(PLAIN.get(tok) or (a.group(1) or "").replace("n", "-") or a.group(3) or ("true" if a.group(2) == "1" else "false"))
        at = a.end()
    return "%s<%s>" % (base, ", ".join(args))


def load(path, match):
    kernels = {}
    for elf in code_objects(path):
        found = kernels_of(elf)
        for name, key in ((n, key_of(n)) for n in found):
            if match and not any(m in key for m in match):
                continue
            if key in kernels and kernels[key] != found[name]:
                sys.exit("%s: kernel %s occurs twice with different code" % (path, key))
            kernels[key] = found[name]
    return kernels


def describe(kd):
    """The fields of an amdhsa kernel descriptor that a register-allocation change would move."""
    lds, scratch = struct.unpack_from("<II", kd, 0)
    rsrc3, rsrc1 = struct.unpack_from("<II", kd, 36)
    return "vgpr_blocks=%d accum_offset=%d sgpr_blocks=%d scratch=%d lds=%d" % (
        rsrc1 & 63, rsrc3 & 63, (rsrc1 >> 6) & 15, scratch, lds)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--match", default="", help="comma-separated substrings of the kernel names to compare (default: all)")
    ap.add_argument("-v", "--verbose", action="store_true", help="list every kernel with a hash of its code")
    args = ap.parse_args()
    match = [m for m in args.match.split(",") if m]
    old, new = load(args.old, match), load(args.new, match)
    lost, added = sorted(set(old) - set(new)), sorted(set(new) - set(old))
    code = sorted(k for k in set(old) & set(new) if old[k][0] != new[k][0])
    desc = sorted(k for k in set(old) & set(new) if old[k][1] != new[k][1])
    for k in lost:
        print("LOST   %s" % k)
    for k in added:
        print("ADDED  %s" % k)
    for k in code:
        print("CODE   %s: %d -> %d bytes" % (k, len(old[k][0]), len(new[k][0])))
    for k in desc:
        print("RSRC   %s: %s -> %s" % (k, describe(old[k][1]), describe(new[k][1])))
    if args.verbose:
        for k in sorted(new):
            print("%s %6d B  %s  %s" % (hashlib.sha1(new[k][0]).hexdigest()[:12], len(new[k][0]), describe(new[k][1]), k))
    print("kernels: %d old, %d new; lost %d, added %d; code differs in %d, descriptor (registers / scratch / LDS) in %d; "
          "code bytes %d old, %d new" % (len(old), len(new), len(lost), len(added), len(code), len(desc),
                                         sum(len(v[0]) for v in old.values()), sum(len(v[0]) for v in new.values())))
    return 1 if lost or added or code or desc else 0


if __name__ == "__main__":
    sys.exit(main())
