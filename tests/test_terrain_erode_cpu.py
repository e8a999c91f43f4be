"""CPU tests of vr_terrain_erode: the entry point is declared, mirrored and exported and refuses bad arguments without a device, the
header's serial evaluator under g++ (tests/host/erode_check.cpp) agrees with a tiled, K-sweeps-at-a-time evaluation of the same
header and gives the bytes of the numpy model (tests/erode_model.py), and the model has the properties an erosion must have."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from tests import erode_model as em
from tests.erosion_state import full_mask, seeded_dabs
from tests.host_check import build_host_check, run_host_check
from vrenderer_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORLD = 64.0
SIZES = ((1, 1), (3, 2), (9, 17), (45, 67), (64, 64))                # (h, w): maps of 1x1, 2x3, 17x9, 67x45 and 64x64
ITERATIONS, TALUS, RATES = (1, 2, 33), (0.0, 0.5, 3.0), (0.125, 0.03)


def test_erode_is_declared_mirrored_and_exported(product_lib):
    header = open(os.path.join(ROOT, "include", "vrterrain.h")).read()
    assert re.search(r"VR_API\s+int\s+vr_terrain_erode\s*\(\s*vr_terrain\*\s*t,\s*const vr_erode_params\*\s*p,\s*const vr_brush_dab\*\s*dabs,"
                     r"\s*uint32_t n,\s*int32_t out_rect\[4\]\)", header)
    assert re.search(r"#define\s+VR_ERODE_MAX_ITERATIONS\s+1024\b", header) and capi.VR_ERODE_MAX_ITERATIONS == 1024
    assert re.search(r"VR_API\s+int\s+vr_debug_erode_config\s*\(\s*int32_t out\[4\]\)", header)
    assert C.sizeof(capi.ErodeParams) == 32
    assert "vr_terrain_erode" in capi.EXPORTS and "vr_debug_erode_config" in capi.EXPORTS
    assert len(product_lib.vr_terrain_erode.argtypes) == 5
    # an erode adds no kernel id: its kernels are untimed, like the brush's
    assert capi.VR_K_COUNT == 22 and product_lib.vr_timing_kernel_count() == 22
    hpp = open(os.path.join(ROOT, "include", "vrterrain.hpp")).read()
    assert "Erode(" in hpp and "vr_terrain_erode" in hpp
    cfg = (C.c_int32 * 4)()
    assert product_lib.vr_debug_erode_config(cfg) == capi.VR_OK and product_lib.vr_debug_erode_config(None) == capi.VR_ERR_INVALID_ARGUMENT
    tile_w, tile_h, k, zero = list(cfg)
    assert tile_w >= 8 and tile_h >= 8 and zero == 0
    assert k >= 4                                                   # a call of N iterations queues ceil(N / K) step launches, not N


def test_refusals_answer_without_a_device(product_lib):
    """Every refusal comes before any use of the device: a handle that is no terrain is never looked into."""
    lib = product_lib
    fake = C.create_string_buffer(1 << 16)                          # stands in for a terrain; a refused call does not read it
    nan, inf = float("nan"), float("inf")

    def call(t=True, p=True, dabs=True, n=1, iterations=8, talus=1.0, rate=0.125, reserved=(0, 0, 0, 0, 0), d=(0.0, 0.0, 4.0, 0.5, 1.0)):
        ep = capi.ErodeParams(iterations=iterations, talus=talus, rate=rate)
        ep.reserved[:] = reserved
        arr = (capi.BrushDab * max(n, 1))(*[capi.BrushDab(*d)] * max(n, 1))
        rect = (C.c_int32 * 4)()
        return lib.vr_terrain_erode(C.cast(fake, C.c_void_p) if t else None, C.byref(ep) if p else None, arr if dabs else None, n, rect)

    bad = [dict(t=False), dict(p=False), dict(dabs=False), dict(n=capi.VR_MAX_BRUSH_DABS + 1),
           dict(iterations=0), dict(iterations=-3), dict(iterations=capi.VR_ERODE_MAX_ITERATIONS + 1),
           dict(talus=nan), dict(talus=inf), dict(rate=nan), dict(rate=inf), dict(talus=-0.5), dict(talus=255.5),
           dict(rate=0.0), dict(rate=-0.1), dict(rate=0.126), dict(reserved=(0, 0, 0, 0, 1)), dict(reserved=(7, 0, 0, 0, 0)),
           dict(d=(nan, 0.0, 4.0, 0.5, 1.0)), dict(d=(0.0, inf, 4.0, 0.5, 1.0)), dict(d=(0.0, 0.0, 0.0, 0.5, 1.0)), dict(d=(0.0, 0.0, -1.0, 0.5, 1.0)),
           dict(d=(0.0, 0.0, 4.0, 1.0, 1.0)), dict(d=(0.0, 0.0, 4.0, -0.1, 1.0)), dict(d=(0.0, 0.0, 4.0, 0.5, nan)),
           dict(d=(0.0, 0.0, 4.0, 0.5, 1.5)), dict(d=(0.0, 0.0, 4.0, 0.5, -0.1))]                  # strength is an opacity
    for kw in bad:
        assert call(**kw) == capi.VR_ERR_INVALID_ARGUMENT, kw
    assert bytes(fake) == bytes(1 << 16)


def test_new_declarations_compile_in_c_and_cpp(tmp_path):
    src = tmp_path / "erode.c"
    src.write_text('#include <stdio.h>\n#include <vrterrain.h>\nint main(void) { vr_erode_params p = { 8, 1.0f, 0.125f, { 0, 0, 0, 0, 0 } }; '
                   'int (*f)(vr_terrain*, const vr_erode_params*, const vr_brush_dab*, uint32_t, int32_t*) = vr_terrain_erode; (void)f; '
                   'printf("%zu %d %d\\n", sizeof(vr_erode_params), (int)VR_ERODE_MAX_ITERATIONS, p.iterations); return 0; }\n')
    obj = str(tmp_path / "erode_c.o")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", obj], check=True,
                   capture_output=True, text=True)
    cpp = tmp_path / "erode.cpp"
    cpp.write_text('#include <vrterrain.hpp>\nbool erode(vRenderer::TerrainPass& tp, const vr_brush_dab* d, int32_t r[4]) { return tp.Erode(d, 1, 8, 1.0f, 0.125f, r); }\n'
                   'static_assert(sizeof(vr_erode_params) == 32, "vr_erode_params");\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(cpp), "-o", str(tmp_path / "erode_cpp.o")],
                   check=True, capture_output=True, text=True)


@pytest.fixture(scope="module")
def erode_checks(tmp_path_factory):
    """The check program, and the same program under the address and undefined-behaviour sanitizers (stand-alone, nothing preloaded)."""
    d = tmp_path_factory.mktemp("erode")
    flags = ["-ffp-contract=off"]
    return (build_host_check(d, "erode_check", flags),
            build_host_check(d, "erode_check", flags + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "erode_check_san"))


def test_serial_evaluator_keeps_its_invariants(erode_checks):
    """erode_serial's invariants, and erode_serial against the tiled K-sweeps-per-pass evaluation in every byte."""
    for exe in erode_checks:
        r = run_host_check(exe, timeout=300, expect=" calls, 0 failures", stderr_tail=4000)
        assert "740 calls" in r.stdout, r.stdout[-400:]              # (36 maps + the 61 x 61 one) x 20


def _host_erode(exe, tmp_path, texels, dabs, iterations, talus, rate):
    h, w = texels.shape
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<4i3f", w, h, len(dabs), iterations, WORLD, talus, rate))
        f.write(np.ascontiguousarray(dabs, np.float32).tobytes())
        f.write(np.ascontiguousarray(texels).tobytes())
    subprocess.run([exe, "apply", fin, fout], check=True, timeout=120)
    raw = open(fout, "rb").read()
    return np.frombuffer(raw[16:], np.uint8).reshape(texels.shape), struct.unpack("<4i", raw[:16])


@pytest.mark.parametrize("size", SIZES)
def test_header_on_the_host_gives_the_model_s_bytes(erode_checks, tmp_path, size):
    """Seeded dabs on a random map, iterations 1, 2, 33 x talus 0, 0.5, 3 x rate 0.125, 0.03: the header's serial evaluator under
    g++ - plain and under the sanitizers - and the numpy model agree in every byte and in the rectangle."""
    h, w = size
    rng = np.random.default_rng(7 * h + w)
    texels = rng.integers(0, 256, (h, w), dtype=np.uint8)
    dabs = seeded_dabs(rng, h, w)
    changed = 0
    for iterations in ITERATIONS:
        for talus in TALUS:
            for rate in RATES:
                want, want_rect = em.erode(texels, dabs, WORLD, iterations, talus, rate)
                for exe in erode_checks:
                    got, got_rect = _host_erode(exe, tmp_path, texels, dabs, iterations, talus, rate)
                    assert tuple(got_rect) == tuple(want_rect), (iterations, talus, rate)
                    assert np.array_equal(got, want), f"{(iterations, talus, rate)}: {(got != want).sum()} bytes differ, first {np.argwhere(got != want)[:4].tolist()}"
                changed = max(changed, int((want != texels).sum()))
    if min(h, w) > 8:
        assert changed >= 30


# ---- the model's own properties ---------------------------------------------------------------------------------------------------
def test_zero_mask_and_flat_map_change_nothing():
    rng = np.random.default_rng(11)
    texels = rng.integers(0, 256, (45, 67), dtype=np.uint8)
    zero = np.float32([[3.0, -2.0, 9.0, 0.0, 0.0], [-5.0, 8.0, 6.0, 0.7, 0.0]])                   # dabs that cover texels with strength 0
    out, rect = em.erode(texels, zero, WORLD, 33, 0.0, 0.125)
    assert rect[2] > 0 and rect[3] > 0 and np.array_equal(out, texels)
    miss = np.float32([[5.0 * WORLD, 0.0, 3.0, 0.0, 1.0]])
    out, rect = em.erode(texels, miss, WORLD, 33, 0.0, 0.125)
    assert tuple(rect) == (0, 0, 0, 0) and np.array_equal(out, texels)
    out, rect = em.erode(texels, np.zeros((0, 5), np.float32), WORLD, 33, 0.0, 0.125)            # n == 0
    assert tuple(rect) == (0, 0, 0, 0) and np.array_equal(out, texels)
    flat = np.full((45, 67), 93, np.uint8)
    out, rect = em.erode(flat, full_mask(), WORLD, 33, 0.0, 0.125)
    assert tuple(rect) == (0, 0, 67, 45) and np.array_equal(out, flat)


@pytest.mark.parametrize("size", SIZES[2:])
@pytest.mark.parametrize("talus", TALUS)
def test_erosion_stays_inside_its_mask_and_its_range_and_conserves_material(size, talus):
    h, w = size
    rng = np.random.default_rng(100 * h + w)
    texels = rng.integers(0, 256, (h, w), dtype=np.uint8)
    dabs = seeded_dabs(rng, h, w, n=5)
    mask, rect = em.mask_of(texels.shape, dabs, WORLD)
    for iterations, rate in ((1, 0.125), (33, 0.125), (33, 0.03)):
        out, out_rect = em.erode(texels, dabs, WORLD, iterations, talus, rate)
        assert tuple(out_rect) == tuple(rect)
        x, y, rw, rh = rect
        inside = np.zeros((h, w), bool)
        inside[y:y + rh, x:x + rw] = True
        changed = out != texels
        assert not (changed & ~inside).any() and not (changed & (mask == 0)).any()
        window = texels[y:y + rh, x:x + rw]
        assert out[inside].min() >= window.min() and out[inside].max() <= window.max()
        # every edge moves the same amount out of one texel and into the other: the sum changes by the final rounding alone
        assert abs(int(out.astype(np.int64).sum()) - int(texels.astype(np.int64).sum())) <= 0.5 * int(changed.sum()) + 1
    assert changed.sum() >= 10


def test_a_spike_spreads_to_its_eight_neighbours():
    texels = np.full((17, 17), 20, np.uint8)
    texels[8, 8] = 220                                               # a single 200-step spike
    out, _ = em.erode(texels, full_mask(), WORLD, 8, 0.0, 0.125)
    assert out[8, 8] < 220
    ring = [(8 + dy, 8 + dx) for dx, dy in em.NEIGHBOURS]
    assert all(out[p] > 20 for p in ring)


# ---- the fp32 state and its read-back (tests/erosion_state.py, tests/test_terrain_erosion_state_gpu.py) ---------------------------------
def test_the_state_read_back_is_declared_exported_and_refuses_null(product_lib):
    header = open(os.path.join(ROOT, "include", "vrterrain.h")).read()
    assert re.search(r"VR_API\s+int\s+vr_debug_terrain_sweep_state\s*\(\s*vr_terrain\*\s*t,\s*int32_t out_rect\[4\],\s*int32_t\*\s*out_fields,"
                     r"\s*float\*\s*out,\s*size_t capacity_floats\)", header)
    assert "vr_debug_terrain_sweep_state" in capi.EXPORTS and len(product_lib.vr_debug_terrain_sweep_state.argtypes) == 5
    fake = C.create_string_buffer(1 << 16)                          # stands in for a terrain; a refused call does not read it
    t = C.cast(fake, C.c_void_p)
    rect, fields, out = (C.c_int32 * 4)(-1, -1, -1, -1), C.c_int32(-1), (C.c_float * 4)(5, 5, 5, 5)
    fn = product_lib.vr_debug_terrain_sweep_state
    assert fn(None, rect, C.byref(fields), out, 4) == capi.VR_ERR_INVALID_ARGUMENT
    assert fn(t, None, C.byref(fields), out, 4) == capi.VR_ERR_INVALID_ARGUMENT
    assert fn(t, rect, None, out, 4) == capi.VR_ERR_INVALID_ARGUMENT
    assert fn(None, rect, C.byref(fields), None, 0) == capi.VR_ERR_INVALID_ARGUMENT
    assert list(rect) == [-1] * 4 and fields.value == -1 and list(out) == [5.0] * 4 and bytes(fake) == bytes(1 << 16)


@pytest.mark.parametrize("size", SIZES[2:])
def test_state_gives_the_bytes_of_erode(size):
    """erode_model.state: the plane that erode() rounds - its bytes, its mask and its rectangle - and tests/erosion_state.py's view of it."""
    from tests import erosion_state as es
    h, w = size
    rng = np.random.default_rng(7 * h + w)
    texels = rng.integers(0, 256, (h, w), dtype=np.uint8)
    dabs = seeded_dabs(rng, h, w)
    mask, rect = em.mask_of(texels.shape, dabs, WORLD)
    for iterations, talus, rate in ((1, 0.0, 0.125), (2, 0.7, 0.1), (33, 3.0, 0.03)):
        plane, m, r = em.state(texels, dabs, WORLD, iterations, talus, rate)
        want, want_rect = em.erode(texels, dabs, WORLD, iterations, talus, rate)
        assert plane.dtype == np.float32 and plane.shape == texels.shape and np.array_equal(m, mask) and tuple(r) == tuple(rect) == tuple(want_rect)
        stored = np.floor(np.clip(plane.astype(np.float64), 0.0, 255.0) + 0.5).astype(np.uint8)       # (exact in double)
        assert np.array_equal(np.where(mask > 0, stored, texels), want)
        assert np.array_equal(plane[mask == 0], texels[mask == 0].astype(np.float32))
        step = texels.astype(np.float32)
        for _ in range(iterations):
            step = em.sweep(step, mask, talus, rate)
        assert np.array_equal(step.view(np.uint32), plane.view(np.uint32))
        view = es.state("thermal", texels, dabs, WORLD, iterations, (talus, rate))
        assert np.array_equal(view["bytes"], want) and view["rect"] == tuple(want_rect) and np.array_equal(es.bits(view["planes"][0]), es.bits(plane))
    assert (want != texels).sum() >= 30


def test_every_state_case_can_tell_a_wrong_order(oracle, product_lib):
    """The cases of tests/test_terrain_erosion_state_gpu.py on scenes made by the oracle's synthetic heightmaps: each is sensitive - the
    model with two neighbours exchanged differs in at least 30 fp32 cells of the final state - every wrong variant of DESIGN.md 4w's
    table changes the state of every case, and the corner and clamp cases show what they are there for.  (About 10 s of numpy.)"""
    from tests import erosion_state as es
    config = {}
    for kind, fn in (("thermal", product_lib.vr_debug_erode_config), ("hydraulic", product_lib.vr_debug_hydro_config)):
        cfg = (C.c_int32 * 4)()
        assert fn(cfg) == capi.VR_OK
        config[kind] = (cfg[0], cfg[1], cfg[2])
    maps = es.scene_maps(oracle.synth_heightmap)
    cases = es.suite_cases(maps, config)
    assert len(cases) >= 6 + 20 + 4 + 2 + 1
    for name, kind, texels, dabs, world, iterations, params in cases:
        right = es.state(kind, texels, dabs, world, iterations, params)
        assert es.assert_sensitive(kind, texels, dabs, world, iterations, params, right) >= es.SENSITIVE
        if name.startswith(("scene", "borders", "1024")):
            for variant in es.wrong_variants(kind, params):
                cells, _ = es.sensitivity(kind, texels, dabs, world, iterations, params, right, variant)
                assert cells >= 1, (name, kind, iterations, variant)
        if name.startswith("borders"):
            assert es.changes_on_both_sides_of_every_border(texels.astype(np.float32), right["planes"][0], *config[kind][:2]), (name, kind, iterations)
    texels, world = maps["fast64"]
    dabs = np.float32([es.dab(texels.shape, world, 30.0, 28.0, 6.0, 0.0, 1.0)])
    for corner, (params, holds) in es.HYDRO_CORNERS.items():
        holds(es.state("hydraulic", texels, dabs, world, 2 * config["hydraulic"][2] + 1, params), texels)
    for corner, (params, prepare, holds) in es.THERMAL_CORNERS.items():
        holds(es.state("thermal", prepare(texels), dabs, world, 2 * config["thermal"][2] + 1, params), prepare(texels))
    texels, dabs, n, params = es.clamp_case(64.0)
    want = es.state("hydraulic", texels, dabs, 64.0, n, params)
    masked = want["mask"] > 0
    assert (masked & (want["settled"] < 0)).sum() >= 10 and (masked & (want["settled"] > 255)).sum() >= 10
    for name, (dabs, intended) in es.rect_dabs(maps["odd"][1]).items():
        assert es.state("thermal", maps["odd"][0], dabs, maps["odd"][1], 1, es.THERMAL)["rect"] == intended, name
