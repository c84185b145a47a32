"""The tracked tile / split-K table (dualdiff_amd/tuned/gfx950.json) against the planner, without a GPU.

Every entry is rebuilt into a dd_gemm descriptor from its key (dummy pointers: the planner dereferences nothing) and
planned by dd_gemm_kernel_name with exactly the entry's tile and split-K.  An entry must name a tile of the library, plan
to a kernel (never "unsupported" / "invalid": the run-time tuner would have had to launch it), and plan the split-K the
normalisation gives: slabs of ceil(chunks / split) K-chunks, so ceil(chunks / ceil(chunks / split)) slabs — with chunks
the 64-wide K steps (the direct conv: the 64-channel chunks), and split 1 for the epilogues that take no split-K."""
import collections
import ctypes

import pytest

from dualdiff_amd import _native
from tests.tuned_table import UP_CONCAT_K1, desc_from_key, expected_split, family, load_table


def test_every_tracked_entry_plans_to_a_kernel():
    lib = _native.load()
    tiles = {lib.dd_gemm_tile_id(i) for i in range(lib.dd_gemm_num_tiles())}
    bad, fams, renorm = [], collections.Counter(), 0
    for key, (tile, split, _form) in load_table():
        if tile != 0 and tile not in tiles:
            bad.append((key, tile, split, "tile %d is not in the library" % tile))
            continue
        plan = lib.dd_gemm_kernel_name(ctypes.byref(desc_from_key(key, tile, split))).decode()
        if plan in ("unsupported", "invalid"):
            bad.append((key, tile, split, plan))
            continue
        got = int(plan.split(" split=")[1].split(" ")[0])
        want = expected_split(key, plan, split)
        if got != want:
            bad.append((key, tile, split, "plans split=%d, normalisation gives %d (%s)" % (got, want, plan)))
        renorm += got != split
        fams[family(plan)] += 1
    print("\n[tuned table] plans per family: %s; %d entries run another split than they name"
          % (dict(sorted(fams.items())), renorm))
    assert not bad, "%d tracked entries no kernel runs as recorded:\n%s" % (len(bad), "\n".join(map(repr, bad[:20])))


def test_table_keys_are_well_formed():
    seen = set()
    for key, v in load_table():
        assert key not in seen, key
        seen.add(key)
        assert key[0] in ("g", "c") and len(v) == 3 and v[2] == 0, (key, v)
        assert v[0] > 0 and v[1] > 0, "entry %r records no launch: %r" % (key, v)


@pytest.mark.parametrize("k", sorted(UP_CONCAT_K1))
def test_up_block_concat_widths(k):
    """The a2 widths the replay assumes are the up blocks' hidden + skip channel counts of the SD UNet."""
    k1 = UP_CONCAT_K1[k]
    assert k1 in (320, 640, 1280) and k - k1 in (320, 640, 1280)
