"""Mints tests/golden/jpeg_input.npz: the pixels PIL's `np.asarray(Image.open(f).convert("RGB"))` returns for small JPEG
files, so that the numpy restatement (tests/jpeg_decode_reference.py) and the GPU decoder stay pinned to PIL's pixels where
PIL is not installed.  Needs Pillow:  python -m tests.golden.mint_jpeg_input

The accepted files are the 36 `out_*` files of jpeg_output.npz (re-used from there, not copied: `pix_<name>` here) and a
few new ones written by PIL (`file_<name>` and `pix_<name>`): 4:4:4 sampling and optimised Huffman tables.  `refused_<kind>`
are files PIL writes that the decoder turns down.  The kinds PIL cannot write are made from an accepted file by rewriting
header bytes (`rewrite`), at test time.  main() asserts that the paths the cases are there for do occur."""
import io
import os

import numpy as np

from tests import jpeg_decode_reference as R
from tests.golden import mint_jpeg as M

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "jpeg_input.npz")

# name -> ((H, W), content, seed, PIL's save options)
NEW = {
    "8x8_444": ((8, 8), "uniform", 701, {"subsampling": 0}),
    "9x7_444": ((9, 7), "saturated", 702, {"subsampling": 0}),
    "33x47_444": ((33, 47), "uniform", 703, {"subsampling": 0}),
    "17x31_optimize": ((17, 31), "lone", 704, {"optimize": True}),
    "20x32_optimize": ((20, 32), "smooth", 706, {"optimize": True}),
    "37x53_optimize": ((37, 53), "uniform", 705, {"optimize": True}),
    # a 4:2:0 chroma plane of one or two columns: libjpeg replicates it instead of filtering (jdsample.c); 5 wide filters
    "3x1_narrow": ((3, 1), "uniform", 707, {}),
    "9x3_narrow": ((9, 3), "uniform", 708, {}),
    "17x4_narrow": ((17, 4), "saturated", 709, {}),
    "33x2_narrow": ((33, 2), "uniform", 710, {}),
    "7x5_narrow": ((7, 5), "uniform", 711, {}),
}
# kind -> (PIL mode, save options, a word of the ValueError that turns it down)
REFUSED = {
    "progressive": ("RGB", {"progressive": True}, "progressive"),
    "restart": ("RGB", {"restart_marker_blocks": 2}, "restart interval"),
    "422": ("RGB", {"subsampling": 1}, "sampling 2x1"),
    "grayscale": ("L", {}, "grayscale"),
    "cmyk": ("CMYK", {}, "CMYK"),
}
# kinds made by rewrite(): kind -> a word of the ValueError
REWRITTEN = {"q16": "16-bit quantisation", "scans": "several scans", "no_sos": "missing SOS", "no_eoi": "missing EOI",
             "adobe_rgb": "an RGB JPEG", "rgb_ids": "an RGB JPEG"}


def _find(data, marker):
    """offset of the first segment `marker` in the header of data"""
    pos = 2
    while data[pos + 1] != marker:
        pos += 2 + int.from_bytes(data[pos + 2:pos + 4], "big")
    return pos


def rewrite(kind, data):
    """An accepted file -> a file of a kind no encoder at hand writes, by its header bytes alone."""
    if kind == "q16":                                        # the first DQT segment with 16-bit entries
        at = _find(data, 0xDB)
        n = int.from_bytes(data[at + 2:at + 4], "big")
        assert n == 67 and data[at + 4] >> 4 == 0
        body = bytes([0x10 | data[at + 4]]) + b"".join(bytes([0, v]) for v in data[at + 5:at + 69])
        return data[:at + 2] + (len(body) + 2).to_bytes(2, "big") + body + data[at + 2 + n:]
    if kind == "scans":                                      # an SOS that names the first component only
        at = _find(data, 0xDA)
        n = int.from_bytes(data[at + 2:at + 4], "big")
        body = data[at + 4:at + 7] + data[at + 2 + n - 3:at + 2 + n]
        return data[:at + 2] + (len(body) + 2).to_bytes(2, "big") + bytes([1]) + body[1:] + data[at + 2 + n:]
    if kind == "adobe_rgb":                                  # an Adobe APP14 segment with transform 0 in place of JFIF's APP0
        at = _find(data, 0xE0)
        return (data[:at] + b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x00"
                + data[at + 2 + int.from_bytes(data[at + 2:at + 4], "big"):])
    if kind == "rgb_ids":                                    # no JFIF segment, components named R, G, B in SOF0 and SOS
        at = _find(data, 0xE0)
        data = data[:at] + data[at + 2 + int.from_bytes(data[at + 2:at + 4], "big"):]
        sof, sos = _find(data, 0xC0), _find(data, 0xDA)
        out = bytearray(data)
        for i, c in enumerate(b"RGB"):
            out[sof + 10 + 3 * i] = c
            out[sos + 5 + 2 * i] = c
        return bytes(out)
    if kind == "no_sos":
        return data[:_find(data, 0xDA)] + b"\xff\xd9"
    if kind == "no_eoi":
        assert data.endswith(b"\xff\xd9") and data.count(b"\xff\xd9") == 1
        return data[:-2]
    raise ValueError(kind)


def accepted(golden_out, golden_in):
    """-> [(name, file bytes, PIL's pixels)] of every accepted file: jpeg_output.npz's, then the new ones."""
    out = [(name, golden_out["out_" + name].tobytes(), golden_in["pix_" + name]) for name, _, _ in M.cases()]
    return out + [(name, golden_in["file_" + name].tobytes(), golden_in["pix_" + name]) for name in NEW]


def load():
    a, b = np.load(M.PATH), np.load(PATH)
    return {k: a[k] for k in a.files}, {k: b[k] for k in b.files}


def main():
    import PIL
    from PIL import Image

    def pixels(data):
        return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))

    def save(img, **options):
        buf = io.BytesIO()
        img.save(buf, "JPEG", **options)
        return buf.getvalue()

    src = np.load(M.PATH)
    out = {"pil_version": np.array(PIL.__version__)}
    stats, stuffed, files = {}, 0, []
    for name, _, _ in M.cases():
        files.append((name, src["out_" + name].tobytes()))
    for name, (shape, kind, seed, options) in NEW.items():
        data = save(Image.fromarray(M.content(kind, shape[0], shape[1], seed)), quality=75, **options)
        out["file_" + name] = np.frombuffer(data, dtype=np.uint8)
        files.append((name, data))
    for name, data in files:
        out["pix_" + name] = pixels(data)
        assert np.array_equal(R.decode(data, stats), out["pix_" + name]), name
        stuffed += R.headers(data)["scan"].count(b"\xff\x00")
    for kind, (mode, options, _) in REFUSED.items():
        img = Image.fromarray(M.content("uniform", 20, 32, 800)).convert(mode)
        out["refused_" + kind] = np.frombuffer(save(img, quality=75, **options), dtype=np.uint8)
    assert stuffed > 0, "no FF 00 pair in any scan"
    assert stats["zrl"] > 0 and stats["eob_only"] > 0, stats
    assert stats["dc_sizes"] == set(range(12)), stats["dc_sizes"]
    standard = R.headers(src["out_37x53_uniform_q75"].tobytes())["huffman"]
    for name in ("17x31_optimize", "20x32_optimize", "37x53_optimize"):
        assert R.headers(out["file_" + name].tobytes())["huffman"] != standard, name
    for name in ("8x8_444", "9x7_444", "33x47_444"):
        assert R.headers(out["file_" + name].tobytes())["factors"] == [(1, 1)] * 3, name
    # small sizes hold the upsampler's special cases (a chroma plane of one or two columns is replicated, not filtered):
    # every size from 1 x 1 to 33 x 7, the restatement against PIL; not stored
    for h in range(1, 34):
        for w in range(1, 8):
            data = save(Image.fromarray(M.content("uniform", h, w, 10 * h + w)), quality=75)
            assert np.array_equal(R.decode(data), pixels(data)), (h, w)
    np.savez_compressed(PATH, **out)
    print("wrote %s (PIL %s, %d accepted files, %d refused, %d bytes; %d stuffed bytes, %d ZRL, %d EOB-only blocks, DC sizes %s)"
          % (PATH, PIL.__version__, len(files), len(REFUSED), os.path.getsize(PATH), stuffed, stats["zrl"],
             stats["eob_only"], sorted(stats["dc_sizes"])))


if __name__ == "__main__":
    main()
