"""CPU tests of vr_terrain_edit: the entry point is declared, mirrored and exported, the kernel ids stay as they were, and
the dirty-rectangle rules of vrenderer_amd/csrc/vr_dirty.h hold against a full rebuild (tests/host/dirty_check.cpp)."""
import os
import re

from vrenderer_amd import capi
from tests.host_check import build_host_check, run_host_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_edit_is_declared_mirrored_and_exported(product_lib):
    header = open(os.path.join(ROOT, "include", "vrterrain.h")).read()
    assert re.search(r"VR_API\s+int\s+vr_terrain_edit\s*\(\s*vr_terrain\*\s*t,\s*int which,\s*int32_t x,\s*int32_t y,\s*int32_t w,\s*int32_t h,"
                     r"\s*const void\*\s*texels,\s*size_t row_pitch_bytes,\s*int device_pointer\)", header)
    assert "vr_terrain_edit" in capi.EXPORTS
    assert hasattr(product_lib, "vr_terrain_edit")
    assert len(product_lib.vr_terrain_edit.argtypes) == 9
    # an edit adds no kernel id: its node-height and pyramid work is timed under the ids there are
    assert capi.VR_K_COUNT == 22 and product_lib.vr_timing_kernel_count() == 22
    hpp = open(os.path.join(ROOT, "include", "vrterrain.hpp")).read()
    assert "Edit(" in hpp and "vr_terrain_edit" in hpp
    # argument checks come before any use of the device: they answer on a machine without one
    assert product_lib.vr_terrain_edit(None, 0, 0, 0, 1, 1, None, 0, 0) == capi.VR_ERR_INVALID_ARGUMENT


def test_dirty_rectangles_hold_what_a_full_rebuild_changes(tmp_path):
    """vr_dirty.h compiles without HIP.  For every rectangle of every map of 1..9 x 1..9 texels and 2000 seeded rectangles each
    of 16 x 16, 17 x 5 and 32 x 32 (tests/host/dirty_check.cpp) whatever a full rebuild changes - chain, the three table shapes,
    the dyadic min / max tree, the query pyramid, at every level - lies inside the predicted rectangle, and the prediction is
    within the program's stated K elements per axis of what changed.  And what creating a terrain rests on: for every map of
    w, h in 1..20 and 31, 32, 33, 64, 67 the rectangle of the whole map is ALL of every structure at every level.  Run once more
    under the address and undefined-behaviour sanitizers, as a stand-alone program."""
    r = run_host_check(build_host_check(tmp_path, "dirty_check"))
    assert "33225 rectangles" in r.stdout, r.stdout[-400:]      # sum over w, h in 1..9 of w (w + 1) / 2 * h (h + 1) / 2 = 165^2, + 3 x 2000
    assert "625 whole maps" in r.stdout, r.stdout[-400:]        # 25 sizes per axis
    san = build_host_check(tmp_path, "dirty_check", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "dirty_check_san")
    run_host_check(san, timeout=300, stderr_tail=4000)
