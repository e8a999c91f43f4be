"""CPU tests of vr_terrain_erode_hydraulic: the entry point is declared, mirrored and exported and refuses bad arguments without a
device, the header's serial evaluator under g++ (tests/host/hydro_check.cpp) agrees with a tiled, K-sweeps-at-a-time evaluation of
the same header and gives the bytes of the numpy model (tests/hydro_model.py), and the model has the properties the definition
promises."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from tests import hydro_model as hm
from tests.host_check import build_host_check, run_host_check
from tests.erosion_state import full_mask, seeded_dabs
from vrenderer_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORLD = 64.0
SIZES = ((1, 1), (3, 2), (9, 17), (45, 67), (64, 64))                # (h, w)
# (iterations, rain, flow, capacity, dissolve, deposit, evaporation)
CALLS = ((1, 1.0, 0.5, 8.0, 0.5, 0.25, 0.05), (2, 0.5, 1.0, 4.0, 1.0, 1.0, 0.0), (33, 1.0, 0.5, 8.0, 0.5, 0.25, 0.05), (33, 16.0, 0.07, 64.0, 0.1, 0.9, 1.0),
         (12, 0.01, 0.9, 2.0, 0.3, 0.0, 0.5))
GOOD = dict(iterations=8, rain=1.0, flow=0.5, capacity=8.0, dissolve=0.5, deposit=0.25, evaporation=0.05)


def test_hydro_is_declared_mirrored_and_exported(product_lib):
    header = open(os.path.join(ROOT, "include", "vrterrain.h")).read()
    assert re.search(r"VR_API\s+int\s+vr_terrain_erode_hydraulic\s*\(\s*vr_terrain\*\s*t,\s*const vr_hydro_params\*\s*p,\s*const vr_brush_dab\*\s*dabs,"
                     r"\s*uint32_t n,\s*int32_t out_rect\[4\]\)", header)
    assert re.search(r"#define\s+VR_HYDRO_MAX_ITERATIONS\s+1024\b", header) and capi.VR_HYDRO_MAX_ITERATIONS == 1024
    assert re.search(r"VR_API\s+int\s+vr_debug_hydro_config\s*\(\s*int32_t out\[4\]\)", header)
    assert C.sizeof(capi.HydroParams) == 32
    assert "vr_terrain_erode_hydraulic" in capi.EXPORTS and "vr_debug_hydro_config" in capi.EXPORTS
    assert len(product_lib.vr_terrain_erode_hydraulic.argtypes) == 5
    # the call adds no kernel id: its kernels are untimed, like the brush's
    assert capi.VR_K_COUNT == 22 and product_lib.vr_timing_kernel_count() == 22
    hpp = open(os.path.join(ROOT, "include", "vrterrain.hpp")).read()
    assert "ErodeHydraulic(" in hpp and "vr_terrain_erode_hydraulic" in hpp
    cfg = (C.c_int32 * 4)()
    assert product_lib.vr_debug_hydro_config(cfg) == capi.VR_OK and product_lib.vr_debug_hydro_config(None) == capi.VR_ERR_INVALID_ARGUMENT
    tile_w, tile_h, k, zero = list(cfg)
    assert tile_w >= 8 and tile_h >= 8 and zero == 0
    assert k >= 2                                                   # a call of N iterations queues ceil(N / K) step launches, not N
    # the measurement switch takes 0 (the build's K) and 1 .. K
    assert product_lib.vr_debug_hydro_sweeps_per_launch(k + 1) == capi.VR_ERR_INVALID_ARGUMENT
    assert product_lib.vr_debug_hydro_sweeps_per_launch(-1) == capi.VR_ERR_INVALID_ARGUMENT
    assert product_lib.vr_debug_hydro_sweeps_per_launch(1) == capi.VR_OK and product_lib.vr_debug_hydro_sweeps_per_launch(0) == capi.VR_OK


def test_refusals_answer_without_a_device(product_lib):
    """Every refusal comes before any use of the device: a handle that is no terrain is never looked into."""
    lib = product_lib
    fake = C.create_string_buffer(1 << 16)                          # stands in for a terrain; a refused call does not read it
    nan, inf = float("nan"), float("inf")

    def call(t=True, p=True, dabs=True, n=1, reserved=0, d=(0.0, 0.0, 4.0, 0.5, 1.0), **kw):
        hp = capi.HydroParams(**{**GOOD, **kw})
        hp.reserved = reserved
        arr = (capi.BrushDab * max(n, 1))(*[capi.BrushDab(*d)] * max(n, 1))
        rect = (C.c_int32 * 4)()
        return lib.vr_terrain_erode_hydraulic(C.cast(fake, C.c_void_p) if t else None, C.byref(hp) if p else None, arr if dabs else None, n, rect)

    bad = [dict(t=False), dict(p=False), dict(dabs=False), dict(n=capi.VR_MAX_BRUSH_DABS + 1),
           dict(iterations=0), dict(iterations=-3), dict(iterations=capi.VR_HYDRO_MAX_ITERATIONS + 1), dict(reserved=1), dict(reserved=-7),
           dict(rain=-0.1), dict(rain=16.5), dict(flow=0.0), dict(flow=-0.1), dict(flow=1.01), dict(capacity=-1.0), dict(capacity=64.5),
           dict(dissolve=-0.1), dict(dissolve=1.1), dict(deposit=-0.1), dict(deposit=1.1), dict(evaporation=-0.1), dict(evaporation=1.1),
           dict(d=(nan, 0.0, 4.0, 0.5, 1.0)), dict(d=(0.0, inf, 4.0, 0.5, 1.0)), dict(d=(0.0, 0.0, 0.0, 0.5, 1.0)), dict(d=(0.0, 0.0, -1.0, 0.5, 1.0)),
           dict(d=(0.0, 0.0, 4.0, 1.0, 1.0)), dict(d=(0.0, 0.0, 4.0, -0.1, 1.0)), dict(d=(0.0, 0.0, 4.0, 0.5, nan)),
           dict(d=(0.0, 0.0, 4.0, 0.5, 1.5)), dict(d=(0.0, 0.0, 4.0, 0.5, -0.1))]                  # strength is an opacity
    bad += [{name: v} for name in ("rain", "flow", "capacity", "dissolve", "deposit", "evaporation") for v in (nan, inf, -inf)]
    for kw in bad:
        assert call(**kw) == capi.VR_ERR_INVALID_ARGUMENT, kw
    assert bytes(fake) == bytes(1 << 16)


def test_new_declarations_compile_in_c_and_cpp(tmp_path):
    src = tmp_path / "hydro.c"
    src.write_text('#include <stdio.h>\n#include <vrterrain.h>\nint main(void) { vr_hydro_params p = { 8, 1.0f, 0.5f, 8.0f, 0.5f, 0.25f, 0.05f, 0 }; '
                   'int (*f)(vr_terrain*, const vr_hydro_params*, const vr_brush_dab*, uint32_t, int32_t*) = vr_terrain_erode_hydraulic; (void)f; '
                   'printf("%zu %d %d\\n", sizeof(vr_hydro_params), (int)VR_HYDRO_MAX_ITERATIONS, p.iterations); return 0; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "hydro_c.o")],
                   check=True, capture_output=True, text=True)
    cpp = tmp_path / "hydro.cpp"
    cpp.write_text('#include <vrterrain.hpp>\nbool hydro(vRenderer::TerrainPass& tp, const vr_brush_dab* d, int32_t r[4]) '
                   '{ return tp.ErodeHydraulic(d, 1, 8, 1.0f, 0.5f, 8.0f, 0.5f, 0.25f, 0.05f, r); }\n'
                   'static_assert(sizeof(vr_hydro_params) == 32, "vr_hydro_params");\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(cpp), "-o", str(tmp_path / "hydro_cpp.o")],
                   check=True, capture_output=True, text=True)


@pytest.fixture(scope="module")
def hydro_checks(tmp_path_factory):
    """The check program, and the same program under the address and undefined-behaviour sanitizers (stand-alone, nothing preloaded)."""
    d = tmp_path_factory.mktemp("hydro")
    flags = ["-ffp-contract=off"]
    return (build_host_check(d, "hydro_check", flags),
            build_host_check(d, "hydro_check", flags + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "hydro_check_san"))


def test_serial_and_tiled_evaluation_agree_and_keep_the_invariants(hydro_checks):
    """hydro_serial against the tiled K-sweeps-per-pass evaluation in every byte, edge symmetry, nothing outside the rectangle or under
    mask 0 changes, no negative d or s."""
    for exe in hydro_checks:
        r = run_host_check(exe, timeout=300, expect=" edges, 0 failures", stderr_tail=4000)
        assert "392 calls" in r.stdout, r.stdout[-400:]              # 49 maps x 8
        assert int(re.search(r"(\d+) edges", r.stdout).group(1)) > 100000


def _host_hydro(exe, tmp_path, texels, dabs, call):
    h, w = texels.shape
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<4i7f", w, h, len(dabs), call[0], WORLD, *call[1:]))
        f.write(np.ascontiguousarray(dabs, np.float32).tobytes())
        f.write(np.ascontiguousarray(texels).tobytes())
    subprocess.run([exe, "apply", fin, fout], check=True, timeout=120)
    raw = open(fout, "rb").read()
    return np.frombuffer(raw[16:], np.uint8).reshape(texels.shape), struct.unpack("<4i", raw[:16])


@pytest.mark.parametrize("size", SIZES)
def test_header_on_the_host_gives_the_model_s_bytes(hydro_checks, tmp_path, size):
    """Seeded dabs on a random map, five calls that span the parameter ranges (a tiny rain reaches the subnormals): the header's serial
    evaluator under g++ - plain and under the sanitizers - and the numpy model agree in every byte and in the rectangle."""
    h, w = size
    rng = np.random.default_rng(7 * h + w)
    texels = rng.integers(0, 256, (h, w), dtype=np.uint8)
    dabs = seeded_dabs(rng, h, w)
    changed = 0
    for call in CALLS:
        want, want_rect = hm.hydro(texels, dabs, WORLD, *call)
        for exe in hydro_checks:
            got, got_rect = _host_hydro(exe, tmp_path, texels, dabs, call)
            assert tuple(got_rect) == tuple(want_rect), call
            assert np.array_equal(got, want), f"{call}: {(got != want).sum()} bytes differ, first {np.argwhere(got != want)[:4].tolist()}"
        changed = max(changed, int((want != texels).sum()))
    if min(h, w) > 8:
        assert changed >= 30


# ---- the model's own properties ---------------------------------------------------------------------------------------------------
def test_no_mask_no_rain_or_no_capacity_change_nothing():
    """Mask 0 texels keep their byte; with rain = 0 there is no water, and with capacity = 0 water moves but nothing dissolves: the map
    is unchanged.  (Symmetry under a transpose of the map and the dabs is NOT asserted: the neighbour order (0,-1) (-1,0) (1,0) (0,1)
    becomes (-1,0) (0,-1) (0,1) (1,0), another order of the same fp32 sums, so the transposed call may differ in last bits.)"""
    rng = np.random.default_rng(11)
    texels = rng.integers(0, 256, (45, 67), dtype=np.uint8)
    call = CALLS[2]
    zero = np.float32([[3.0, -2.0, 9.0, 0.0, 0.0], [-5.0, 8.0, 6.0, 0.7, 0.0]])                   # dabs that cover texels with strength 0
    out, rect = hm.hydro(texels, zero, WORLD, *call)
    assert rect[2] > 0 and rect[3] > 0 and np.array_equal(out, texels)
    miss = np.float32([[5.0 * WORLD, 0.0, 3.0, 0.0, 1.0]])
    out, rect = hm.hydro(texels, miss, WORLD, *call)
    assert tuple(rect) == (0, 0, 0, 0) and np.array_equal(out, texels)
    out, rect = hm.hydro(texels, np.zeros((0, 5), np.float32), WORLD, *call)                       # n == 0
    assert tuple(rect) == (0, 0, 0, 0) and np.array_equal(out, texels)
    dabs = seeded_dabs(rng, 45, 67, n=5)
    out, rect = hm.hydro(texels, dabs, WORLD, *call)
    mask, mrect = hm.mask_of(texels.shape, dabs, WORLD)
    assert tuple(rect) == tuple(mrect) and (out != texels).sum() >= 30 and not ((out != texels) & (mask == 0)).any()
    x, y, rw, rh = rect
    inside = np.zeros(texels.shape, bool)
    inside[y:y + rh, x:x + rw] = True
    assert not ((out != texels) & ~inside).any()
    it, rain, flow, capacity, dissolve, deposit, evaporation = call
    out, _ = hm.hydro(texels, full_mask(), WORLD, it, 0.0, flow, capacity, dissolve, deposit, evaporation)
    assert np.array_equal(out, texels)
    h, d, s, _, _ = hm.state(texels, full_mask(), WORLD, it, rain, flow, 0.0, dissolve, deposit, evaporation)
    assert np.array_equal(h, texels.astype(np.float32)) and not s.any()
    assert (d != d.flat[0]).any()                                    # the water did move
    out, _ = hm.hydro(texels, full_mask(), WORLD, it, rain, flow, 0.0, dissolve, deposit, evaporation)
    assert np.array_equal(out, texels)


@pytest.mark.parametrize("call", CALLS)
def test_water_and_sediment_stay_finite_and_non_negative(call):
    rng = np.random.default_rng(3)
    texels = rng.integers(0, 256, (45, 67), dtype=np.uint8)
    h, d, s, _, _ = hm.state(texels, full_mask(), WORLD, *call)
    assert np.isfinite(h).all() and np.isfinite(d).all() and np.isfinite(s).all()
    assert (d >= 0).all() and (s >= 0).all()


def test_one_sweep_moves_no_terrain_and_two_do():
    """After one sweep what a texel dissolved is still above it (h' + s' = h): every byte stays.  From the second sweep on the sediment
    travels with the water: a slope loses material above and gains it below."""
    y, x = np.mgrid[0:33, 0:33]
    texels = (40 + 5 * x).astype(np.uint8)                           # a ramp that rises with x
    one, _ = hm.hydro(texels, full_mask(), WORLD, 1, *CALLS[0][1:])
    assert np.array_equal(one, texels)
    out, _ = hm.hydro(texels, full_mask(), WORLD, 24, *CALLS[0][1:])
    delta = out.astype(np.int32) - texels
    assert (delta < 0).sum() >= 30 and (delta > 0).sum() >= 30
    assert delta[:, 20:].sum() < 0 < delta[:, :8].sum()              # carved above, deposited at the foot
