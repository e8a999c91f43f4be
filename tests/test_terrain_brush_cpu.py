"""CPU tests of vr_terrain_brush: the entry point is declared, mirrored and exported, the kernel ids stay as they were, the spans
vr_brush.h prepares hold every texel its weight function puts inside a dab (tests/host/brush_check.cpp), and the header's
functions, compiled by g++ and applied to a map on the host, give the bytes of the numpy model (tests/brush_model.py)."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from tests import brush_model as bm
from tests.host_check import build_host_check, run_host_check
from vrenderer_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_brush_is_declared_mirrored_and_exported(product_lib):
    header = open(os.path.join(ROOT, "include", "vrterrain.h")).read()
    assert re.search(r"VR_API\s+int\s+vr_terrain_brush\s*\(\s*vr_terrain\*\s*t,\s*const vr_brush_stroke\*\s*stroke,\s*const vr_brush_dab\*\s*dabs,"
                     r"\s*uint32_t n,\s*int32_t out_rect\[4\]\)", header)
    assert re.search(r"#define\s+VR_MAX_BRUSH_DABS\s+4096\b", header) and capi.VR_MAX_BRUSH_DABS == 4096
    assert re.search(r"VR_BRUSH_RAISE = 0, VR_BRUSH_FLATTEN = 1, VR_BRUSH_SMOOTH = 2, VR_BRUSH_PAINT = 3", header)
    assert (capi.VR_BRUSH_RAISE, capi.VR_BRUSH_FLATTEN, capi.VR_BRUSH_SMOOTH, capi.VR_BRUSH_PAINT) == (0, 1, 2, 3)
    assert (bm.RAISE, bm.FLATTEN, bm.SMOOTH, bm.PAINT) == (0, 1, 2, 3)
    assert C.sizeof(capi.BrushDab) == 32 and C.sizeof(capi.BrushStroke) == 32
    assert "vr_terrain_brush" in capi.EXPORTS
    assert hasattr(product_lib, "vr_terrain_brush")
    assert len(product_lib.vr_terrain_brush.argtypes) == 5
    # a stroke adds no kernel id: the brush kernel is untimed, its node-height and pyramid work is timed under the ids there are
    assert capi.VR_K_COUNT == 22 and product_lib.vr_timing_kernel_count() == 22
    hpp = open(os.path.join(ROOT, "include", "vrterrain.hpp")).read()
    assert "Brush(" in hpp and "vr_terrain_brush" in hpp
    # argument checks come before any use of the device: they answer on a machine without one
    stroke, dab = capi.BrushStroke(op=capi.VR_BRUSH_RAISE), capi.BrushDab(0.0, 0.0, 1.0, 0.0, 1.0)
    assert product_lib.vr_terrain_brush(None, C.byref(stroke), C.byref(dab), 1, None) == capi.VR_ERR_INVALID_ARGUMENT


def test_struct_sizes_in_c(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <vrterrain.h>\nint main(void) { printf("%zu %zu %d\\n", sizeof(vr_brush_dab), sizeof(vr_brush_stroke), '
                   '(int)VR_MAX_BRUSH_DABS); return 0; }\n')
    exe = str(tmp_path / "sizes")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True, capture_output=True, text=True)
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split() == ["32", "32", "4096"]


@pytest.fixture(scope="module")
def brush_check(tmp_path_factory):
    return build_host_check(tmp_path_factory.mktemp("brush"), "brush_check", ["-ffp-contract=off"])


def test_prepared_spans_hold_every_texel_inside_a_dab(brush_check, tmp_path):
    """vr_brush.h compiles without HIP.  Maps of w, h in {1, 2, 3, 8, 17, 33}, 2000 seeded dabs per map (centres outside the map
    included, radii 0.05 .. 40 texels) and five at the ends of fp32's range: every texel with q < 1, by the header's own weight
    function over the whole map, lies inside the prepared span.  Run once more under the address and undefined-behaviour
    sanitizers, as a stand-alone program."""
    r = run_host_check(brush_check, expect=" dabs, 0 failures")
    assert "72180 dabs" in r.stdout, r.stdout[-400:]            # 36 maps x (2000 + 5)
    san = build_host_check(tmp_path, "brush_check", ["-ffp-contract=off", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
                           "brush_check_san")
    run_host_check(san, timeout=300, expect=" dabs, 0 failures", stderr_tail=4000)


def _host_stroke(exe, tmp_path, texels, op, dabs, world, target=0.0, color=(0, 0, 0, 0), channels=0xF):
    h, w = texels.shape[:2]
    dabs = np.ascontiguousarray(dabs, np.float32).reshape(-1, 5)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<5i6f", op, w, h, len(dabs), channels, world, target, *[float(c) for c in color]))
        f.write(dabs.tobytes())
        f.write(np.ascontiguousarray(texels).tobytes())
    subprocess.run([exe, "apply", fin, fout], check=True, timeout=120)
    raw = open(fout, "rb").read()
    return np.frombuffer(raw[16:], np.uint8).reshape(texels.shape), struct.unpack("<4i", raw[:16])


@pytest.mark.parametrize("op", (bm.RAISE, bm.FLATTEN, bm.SMOOTH, bm.PAINT))
@pytest.mark.parametrize("size", ((64, 64), (45, 67), (50, 33), (1, 1), (3, 2)))
def test_header_on_the_host_gives_the_model_s_bytes(brush_check, tmp_path, op, size):
    """40 seeded dabs (radii 0.3 .. 15 texels, hardness 0 .. 0.95, centres inside and outside the map, fractional strengths) on a
    random map: the header's functions under g++ and the numpy model agree in every byte and in the rectangle - the contract the
    device is held to in tests/test_terrain_brush_gpu.py."""
    h, w = size
    rng = np.random.default_rng(1000 * op + 7 * h + w)
    world = 64.0
    texels = rng.integers(0, 256, (h, w, 4) if op == bm.PAINT else (h, w), dtype=np.uint8)
    n = 40
    dabs = np.zeros((n, 5), np.float32)
    dabs[:, 0:2] = rng.uniform(-0.7 * world, 0.7 * world, (n, 2))
    dabs[:, 2] = np.exp(rng.uniform(np.log(0.3), np.log(15.0), n)) * world / max(w, h)
    dabs[:, 3] = rng.choice([0.0, 0.3, 0.7, 0.95], n)
    dabs[:, 4] = rng.uniform(-9.0, 9.0, n) if op == bm.RAISE else rng.uniform(0.0, 1.0, n)
    kw = dict(target=93.5, color=(250.0, 3.25, 128.0, 77.0), channels=0b1011)
    want, want_rect = bm.stroke(texels, op, dabs, world, **kw)
    got, got_rect = _host_stroke(brush_check, tmp_path, texels, op, dabs, world, **kw)
    assert tuple(got_rect) == tuple(want_rect)
    assert np.array_equal(got, want), f"{(got != want).sum()} bytes differ, first {np.argwhere(got != want)[:4].tolist()}"
    if min(h, w) > 8:
        assert (want != texels).sum() >= 30
