"""CPU tests of the terrain history: the five entry points are declared, mirrored and exported and refuse NULL without a device;
vr_history_status is 32 bytes in C and in ctypes; and vr_history.h - the ring of records and the step bookkeeping the device code
runs on - holds against a naive model over random operation sequences (tests/host/history_check.cpp), once more under the address
and undefined-behaviour sanitizers as a stand-alone program."""
import ctypes as C
import os
import re
import subprocess

import pytest

from tests.host_check import build_host_check, run_host_check
from vrenderer_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vr_terrain_history_enable", "vr_terrain_history_commit", "vr_terrain_undo", "vr_terrain_redo", "vr_terrain_history_status")


def test_history_is_declared_mirrored_and_exported(product_lib):
    header = open(os.path.join(ROOT, "include", "vrterrain.h")).read()
    for proto in (r"VR_API\s+int\s+vr_terrain_history_enable\s*\(\s*vr_terrain\*\s*t,\s*size_t\s+budget_bytes\)",
                  r"VR_API\s+int\s+vr_terrain_history_commit\s*\(\s*vr_terrain\*\s*t\)",
                  r"VR_API\s+int\s+vr_terrain_undo\s*\(\s*vr_terrain\*\s*t,\s*int32_t\*\s*applied\)",
                  r"VR_API\s+int\s+vr_terrain_redo\s*\(\s*vr_terrain\*\s*t,\s*int32_t\*\s*applied\)",
                  r"VR_API\s+int\s+vr_terrain_history_status\s*\(\s*const vr_terrain\*\s*t,\s*vr_history_status\*\s*out\)"):
        assert re.search(proto, header), proto
    assert re.search(r"#define\s+VR_HISTORY_MAX_RECORDS\s+4096\b", header) and capi.VR_HISTORY_MAX_RECORDS == 4096
    policy = open(os.path.join(ROOT, "vrenderer_amd", "csrc", "vr_history.h")).read()
    assert re.search(r"kHistoryMaxRecords\s*=\s*4096\b", policy)
    for name in NAMES:
        assert name in capi.EXPORTS and hasattr(product_lib, name), name
    assert [len(getattr(product_lib, n).argtypes) for n in NAMES] == [2, 1, 2, 2, 2]
    assert C.sizeof(capi.HistoryStatus) == 32
    assert [f[0] for f in capi.HistoryStatus._fields_] == ["undo_steps", "redo_steps", "open_records", "dropped_steps", "bytes_used", "bytes_budget"]
    # the journal adds no kernel id: capture and swap are untimed, the refresh is timed under the ids there are
    assert capi.VR_K_COUNT == 22 and product_lib.vr_timing_kernel_count() == 22
    # argument checks come before any use of the device: they answer on a machine without one
    applied, st = C.c_int32(7), capi.HistoryStatus()
    assert product_lib.vr_terrain_history_enable(None, 1 << 20) == capi.VR_ERR_INVALID_ARGUMENT
    assert product_lib.vr_terrain_history_commit(None) == capi.VR_ERR_INVALID_ARGUMENT
    assert product_lib.vr_terrain_undo(None, C.byref(applied)) == capi.VR_ERR_INVALID_ARGUMENT
    assert product_lib.vr_terrain_redo(None, None) == capi.VR_ERR_INVALID_ARGUMENT
    assert product_lib.vr_terrain_history_status(None, C.byref(st)) == capi.VR_ERR_INVALID_ARGUMENT


def test_status_struct_size_in_c(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include <vrterrain.h>\nint main(void) { printf("%zu %zu %d\\n", sizeof(vr_history_status), '
                   'offsetof(vr_history_status, bytes_used), (int)VR_HISTORY_MAX_RECORDS); return 0; }\n')
    exe = str(tmp_path / "sizes")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True, capture_output=True, text=True)
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split() == ["32", "16", "4096"]


@pytest.fixture(scope="module")
def history_check(tmp_path_factory):
    return build_host_check(tmp_path_factory.mktemp("history"), "history_check")


def test_ring_and_steps_hold_against_the_naive_model(history_check, tmp_path):
    """vr_history.h compiles without HIP.  Four seeds x 10,000 random operations (append / commit / undo / redo / enable) over a
    4 KB arena and a 24-record table, rectangles from 1 x 1 to a whole 4800-byte map: after every operation the live records lie
    inside the arena, aligned and disjoint, the layout rules hold, the counters and the record list are the model's, and after
    every undo and redo the maps equal the model's whole copies.  Every path is reached: wrap, drop, discarded redo, lost open
    step, oversize record, full record table."""
    r = run_host_check(history_check, expect=" cases, 0 failures")
    assert "40000 cases" in r.stdout, r.stdout[-400:]
    counts = dict(re.findall(r"(\w+) (\d+)", r.stdout.splitlines()[-2]))
    for path in ("recorded", "wraps", "drops", "redo_discards", "lost", "oversize", "table_full", "undos", "redos"):
        assert int(counts[path]) > 0, (path, r.stdout[-400:])
    san = build_host_check(tmp_path, "history_check", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "history_check_san")
    run_host_check(san, timeout=300, expect=" cases, 0 failures", stderr_tail=4000)


@pytest.mark.parametrize("x0, w, h, tb, want", ((0, 1, 1, 1, 16), (3, 37, 5, 1, 5 * 48), (1, 16, 2, 1, 2 * 32), (0, 16, 2, 1, 2 * 16),
                                                (3, 1, 1, 4, 16), (1, 4, 3, 4, 3 * 32), (0, 8192, 8192, 4, 8192 * 8192 * 4)))
def test_record_size(history_check, x0, w, h, tb, want):
    """Rows at a pitch that is a multiple of 16, the first byte x0 * tb mod 16 bytes in."""
    out = subprocess.run([history_check, "size", str(x0), str(w), str(h), str(tb)], capture_output=True, text=True, check=True).stdout
    assert int(out) == want
