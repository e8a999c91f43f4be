"""CPU checks of the albedo's packed footprint table (vrenderer_amd/csrc/vr_packed.h), which the fused tile pass reads instead of the
float table: the shipped pack / unpack code as a stand-alone host program, and the numpy model the GPU tests hold the device to."""
import os
import re

import numpy as np

from vrenderer_amd import capi
from tests import packed_model as pk
from tests import tables_model as tm
from tests.host_check import build_host_check, run_host_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_packed_entry_decodes_to_the_float_table_and_its_dirty_rule_holds(tmp_path):
    """tests/host/packed_check.cpp: on random maps, the rim included, an entry's twelve fields give - as byte offsets into a 256-float
    table - the bits of the four float-table entries of its footprint; every rectangle of every map up to 6 x 6 changes nothing outside
    dirty_pack_srgba8_entries, which holds the float table's span and is tight to one entry.  Once more under the address and
    undefined-behaviour sanitizers, as a stand-alone program."""
    r = run_host_check(build_host_check(tmp_path, "packed_check"))
    assert "9 maps decoded, 36 maps of rectangles" in r.stdout, r.stdout[-400:]
    san = build_host_check(tmp_path, "packed_check", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "packed_check_san")
    run_host_check(san, timeout=300, stderr_tail=4000)


def test_the_model_s_entries_decode_to_the_model_of_the_float_table():
    """packed_model against tables_model, which the float table is already held to on the device: for random levels (1 x 1, ragged,
    67 x 61) entry (ix, iy)'s twelve floats are the r, g, b of 'fast' entries (ix, iy) (ix+1, iy) (ix, iy+1) (ix+1, iy+1), as bits -
    where the float table has such a neighbour; the last row and column of entries clamp to the same texels as the ones before."""
    rng = np.random.default_rng(5)
    lut = tm.srgb_lut()
    for h, w in ((1, 1), (1, 4), (5, 3), (64, 64), (61, 67)):
        level = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        table = pk.pack_table(level)
        assert table.shape == (h + 3, w + 3, 4) and table.dtype == np.uint32
        got = pk.decode(table, lut)
        fast = tm.albedo_tables(level, lut)["fast"][..., :3]
        # one more clamped entry per axis, so that every footprint has its right / lower neighbour
        fast = np.pad(fast, ((0, 1), (0, 1), (0, 0)), mode="edge")
        for k, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
            want = fast[dy:dy + h + 3, dx:dx + w + 3]
            assert np.array_equal(got[:, :, k].view(np.uint32), want.view(np.uint32)), (h, w, k)


def test_the_new_table_id_is_declared_and_mirrored():
    header = open(os.path.join(ROOT, "include", "vrterrain.h")).read()
    assert re.search(r"enum\s*\{\s*VR_DEBUG_TABLE_PACK = 5\s*\}", header)
    assert capi.VR_DEBUG_TABLE_PACK == 5 and capi.VR_DEBUG_TABLE_PACK > capi.VR_DEBUG_TABLE_RGBF
