"""GPU tests of the erosions' fp32 state.  vr_erode.h and vr_hydro.h promise that every cell of every sweep is IEEE fp32 in a fixed
written order, nothing contracted, subnormals kept, so that the device equals the numpy float32 models bit for bit - and the byte
that k_sweep_end rounds the state to hides almost every departure from that (DESIGN.md 4w has the table).  Here the planes the last
erosion call left on the device (vr_debug_terrain_sweep_state: the mask, then h or h, d, s) are compared with the models' state as
bit patterns, cropped to the call's rectangle.  No tolerance anywhere.

The thermal parameters are not dyadic (tests/erosion_state.py), so the arithmetic rounds; and every case that has the edges for it
first shows, on the model alone, that it can tell: the model with the first and the last neighbour of its order exchanged differs
from the right one in at least 30 fp32 cells of the case's final state.  Scenes and helpers are those of
tests/level0_common.py."""
import ctypes as C

import numpy as np
import pytest

from vrenderer_amd import capi
from tests import erosion_state as es
from tests.erosion_state import ITER, assert_state, model
from tests.level0_common import SCENES, assert_bytes, level0, make_scenes, world_of

pytestmark = pytest.mark.gpu

F = np.float32
KINDS = ("thermal", "hydraulic")


@pytest.fixture(scope="module")
def scenes(gpu_ctx):
    return make_scenes(gpu_ctx, SCENES)


@pytest.fixture(scope="module")
def config(gpu_ctx):
    """kind -> (tile width, tile height, sweeps per launch) of this build."""
    out = {}
    for kind, fn in (("thermal", gpu_ctx.lib.vr_debug_erode_config), ("hydraulic", gpu_ctx.lib.vr_debug_hydro_config)):
        cfg = (C.c_int32 * 4)()
        assert fn(cfg) == capi.VR_OK
        out[kind] = (cfg[0], cfg[1], cfg[2])
    return out


def erode(tp, kind, dabs, iterations, params):
    return tp.Erode(dabs, iterations, *params) if kind == "thermal" else tp.ErodeHydraulic(dabs, iterations, **params)


def run_case(sc, kind, texels, dabs, iterations, params, what, sensitive=True):
    """One call on a fresh terrain of `texels` against the model; returns the model's state."""
    world = world_of(sc)
    want = model(kind, texels, dabs, world, iterations, params)
    if sensitive:
        es.assert_sensitive(kind, texels, dabs, world, iterations, params, want)
    a = sc.terrain(texels, sc.al, cast=False, render=False)
    try:
        assert erode(a, kind, dabs, iterations, params) == want["rect"], what
        assert_state(a, want, what)
    finally:
        a.close()
    return want


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", SCENES)
def test_state_on_the_suite_s_scenes(scenes, name, kind):
    """1. The five-dab mask on each scene for 20 iterations: the mask plane is mask_of, h (and d, s) are state(), level 0 is the model's."""
    sc = scenes[name]
    want = run_case(sc, kind, sc.hm, es.five_dabs(sc.hm.shape, world_of(sc)), ITER, es.PARAMS[kind], f"{name}, {kind}")
    assert (want["mask"] > 0).sum() >= 300 and (es.bits(want["planes"][0]) != es.bits(sc.hm.astype(F))).sum() >= 30


@pytest.mark.parametrize("mask", ("full", "soft"))
@pytest.mark.parametrize("kind", KINDS)
def test_tile_borders_and_launch_boundaries_in_fp32(scenes, gpu_ctx, config, kind, mask):
    """2. The 128^2 scene, which the build's tile does not divide, under a mask of 1 and under one whole-map hardness-0 dab (w = min(m_c,
    m_n) fractional on every edge), for 1, K - 1, K, K + 1 and 2K + 1 iterations.  On the model alone: the fp32 h changes on both sides
    of every interior tile border at every count.  The hydraulic flow is 0.07: at 0.5 the first sweep under a mask of 1 is exact.  The
    hydraulic 2K + 1 again at one sweep per launch: the same state."""
    tw, th, k = config[kind]
    sc = scenes["multi"]
    size = sc.hm.shape[0]
    assert sc.hm.shape == (size, size) and size % tw and size % th and es.borders(size, tw) and es.borders(size, th) and k >= 2
    S = world_of(sc)
    dabs = es.full_mask(S) if mask == "full" else es.soft_mask(S)
    params = es.THERMAL if kind == "thermal" else es.HYDRO_SLOW
    m, rect = es.em.mask_of(sc.hm.shape, dabs, S)
    assert tuple(rect) == (0, 0, size, size) and (m > 0).all() and ((m == 1).all() if mask == "full" else len(np.unique(m)) > 1000)
    for n in sorted({1, k - 1, k, k + 1, 2 * k + 1}):
        want = run_case(sc, kind, sc.hm, dabs, n, params, f"{kind}, {mask} mask, {n} iterations, tile {tw} x {th}, K {k}")
        assert es.changes_on_both_sides_of_every_border(sc.hm.astype(F), want["planes"][0], tw, th), (kind, mask, n)
    if kind == "hydraulic":
        n = 2 * k + 1
        want = model(kind, sc.hm, dabs, S, n, params)
        a = sc.terrain(sc.hm, sc.al, cast=False, render=False)
        try:
            assert gpu_ctx.lib.vr_debug_hydro_sweeps_per_launch(1) == capi.VR_OK
            erode(a, kind, dabs, n, params)
            assert_state(a, want, f"hydraulic, {mask} mask, {n} iterations, one sweep per launch")
        finally:
            assert gpu_ctx.lib.vr_debug_hydro_sweeps_per_launch(0) == capi.VR_OK
            a.close()


@pytest.mark.parametrize("kind", KINDS)
def test_rectangles_that_stress_the_load_the_halo_and_the_store(scenes, config, kind):
    """3. On the 67 x 45 scene the narrowest rectangles the dab rule allows (es.rect_dabs says why none is 1 x 1 and why one a texel
    wide has mask 0) and one clipped by the map's right and bottom edges; on the 128^2 scene rectangles exactly one tile wide and one
    tile plus one texel.  The model's rectangle is the one intended.  Only the tile-wide ones have the edges to be order-sensitive."""
    sc = scenes["odd"]
    assert sc.hm.shape == es.ODD_SHAPE
    for name, (dabs, intended) in es.rect_dabs(world_of(sc)).items():
        want = run_case(sc, kind, sc.hm, dabs, ITER, es.PARAMS[kind], f"{kind}, {name}", sensitive=False)
        assert want["rect"] == intended, (name, want["rect"])
        masked = int((want["mask"] > 0).sum())
        assert masked == 0 if "mask 0" in name else masked >= 1, (name, masked)
        x, y, w, h = want["rect"]
        if "clipped" in name:
            assert (x + w, y + h) == sc.hm.shape[::-1] and masked >= 30
    sc = scenes["multi"]
    tw = config[kind][0]
    for width in (tw, tw + 1):
        dabs, rect = es.tile_wide_dabs(sc.hm.shape, world_of(sc), width)
        want = run_case(sc, kind, sc.hm, dabs, ITER, es.PARAMS[kind], f"{kind}, a rectangle {width} wide")
        assert want["rect"] == rect and rect[2] == width


@pytest.mark.parametrize("kind", KINDS)
def test_the_full_iteration_count(scenes, kind):
    """4. 1024 iterations (VR_ERODE_MAX_ITERATIONS, VR_HYDRO_MAX_ITERATIONS) on the 64^2 scene under a dab 20 texels across: 128 or
    256 launches of a one-workgroup grid.  The thermal talus is 0.3: under 0.7 the slopes settle and too few edges stay live for
    the precondition.  The numpy models take 0.4 s (thermal) and 0.9 s (hydraulic) for the 1024 sweeps, three times over with the
    precondition's variant and the cache's miss."""
    assert capi.VR_ERODE_MAX_ITERATIONS == 1024 and capi.VR_HYDRO_MAX_ITERATIONS == 1024
    sc = scenes["fast64"]
    dabs = np.float32([es.dab(sc.hm.shape, world_of(sc), 30.0, 28.0, 10.0, 0.0, 1.0)])
    params = es.THERMAL_LONG if kind == "thermal" else es.HYDRO
    want = run_case(sc, kind, sc.hm, dabs, 1024, params, f"{kind}, 1024 iterations")
    assert 20 <= want["rect"][2] <= 24 and 20 <= want["rect"][3] <= 24


def corner_dabs(sc):
    return np.float32([es.dab(sc.hm.shape, world_of(sc), 30.0, 28.0, 6.0, 0.0, 1.0)])           # 12 texels across


@pytest.mark.parametrize("corner", sorted(es.HYDRO_CORNERS))
def test_hydraulic_parameter_corners(scenes, config, corner):
    """5a. The ends of the hydraulic parameter ranges on the device, 2K + 1 iterations under a 12-texel dab; each with what the model
    must show for the case to mean something (es.HYDRO_CORNERS).  The tiny rain's water is subnormal in at least 30 cells: a build
    that flushes subnormals fails it."""
    sc = scenes["fast64"]
    n = 2 * config["hydraulic"][2] + 1
    params, holds = es.HYDRO_CORNERS[corner]
    want = model("hydraulic", sc.hm, corner_dabs(sc), world_of(sc), n, params)
    assert (want["mask"] > 0).sum() >= 100
    holds(want, sc.hm)
    run_case(sc, "hydraulic", sc.hm, corner_dabs(sc), n, params, f"hydraulic, {corner}", sensitive=False)


@pytest.mark.parametrize("corner", sorted(es.THERMAL_CORNERS))
def test_thermal_parameter_corners(scenes, config, corner):
    """5b. The ends of the thermal parameter ranges, 2K + 1 iterations under a 12-texel dab.  The subnormal rate runs on the scene with
    every other row of the dab's region zeroed: what a zero texel receives is subnormal, in at least 30 cells of the model's h."""
    sc = scenes["fast64"]
    n = 2 * config["thermal"][2] + 1
    params, prepare, holds = es.THERMAL_CORNERS[corner]
    texels = prepare(sc.hm)
    want = model("thermal", texels, corner_dabs(sc), world_of(sc), n, params)
    assert (want["mask"] > 0).sum() >= 100
    holds(want, texels)
    run_case(sc, "thermal", texels, corner_dabs(sc), n, params, f"thermal, {corner}", sensitive=False)


def test_the_clamp_of_the_hydraulic_byte(scenes):
    """6. A 64^2 map of a 0 half and a 255 half under the whole-map soft dab with capacity 64, dissolve 1 and rain 16: after five sweeps
    more than 10 masked texels have h + s below 0 and more than 10 have it above 255 (asserted on the model), so the byte is the
    clamp's.  State and bytes are the model's.  (There is no thermal case: DESIGN.md 4u.)"""
    sc = scenes["fast64"]
    texels, dabs, n, params = es.clamp_case(world_of(sc))
    want = model("hydraulic", texels, dabs, world_of(sc), n, params)
    masked = want["mask"] > 0
    below, above = masked & (want["settled"] < 0), masked & (want["settled"] > 255)
    assert below.sum() >= 10 and above.sum() >= 10, (below.sum(), above.sum())
    assert (want["bytes"][below] == 0).all() and (want["bytes"][above] == 255).all()
    run_case(sc, "hydraulic", texels, dabs, n, params, "the clamp")


def _state_raw(sc, tp, out, capacity):
    rect, fields = (C.c_int32 * 4)(-1, -1, -1, -1), C.c_int32(-1)
    rc = sc.ctx.lib.vr_debug_terrain_sweep_state(tp.handle, rect, C.byref(fields), None if out is None else out.ctypes.data_as(C.c_void_p), capacity)
    return rc, tuple(rect), fields.value


def test_the_read_back_s_own_contract(scenes):
    """7. No record before the first call; the size query; a short capacity is refused and touches nothing; a refused erosion call
    leaves the record of the call before it; a thermal call after a hydraulic one reports one field and its own rectangle; a call
    whose dabs all miss clears the record."""
    sc = scenes["odd"]
    S = world_of(sc)
    five = es.five_dabs(sc.hm.shape, S)
    small = es.rect_dabs(S)["the far corner, clipped"][0]
    first = model("hydraulic", sc.hm, five, S, 5, es.HYDRO)
    second = model("thermal", first["bytes"], small, S, 3, es.THERMAL)
    assert second["rect"] != first["rect"]
    a = sc.terrain(sc.hm, sc.al, cast=False, render=False)
    try:
        assert a.ErosionState() == ((0, 0, 0, 0), None, [])
        sentinel = np.full(8, F(-7.5))
        assert _state_raw(sc, a, sentinel, 8) == (capi.VR_OK, (0, 0, 0, 0), 0) and (sentinel == F(-7.5)).all()
        assert erode(a, "hydraulic", five, 5, es.HYDRO) == first["rect"]
        x, y, w, h = first["rect"]
        assert _state_raw(sc, a, None, 0) == (capi.VR_OK, first["rect"], 3)                       # the size query
        need = 4 * w * h
        buf = np.full(need, F(-7.5))
        rc, rect, fields = _state_raw(sc, a, buf, need - 1)
        assert rc == capi.VR_ERR_INVALID_ARGUMENT and rect == (-1, -1, -1, -1) and fields == -1 and (buf == F(-7.5)).all()
        assert _state_raw(sc, a, None, need)[0] == capi.VR_ERR_INVALID_ARGUMENT
        assert _state_raw(sc, a, buf, need) == (capi.VR_OK, first["rect"], 3)
        es.assert_bits(buf[:w * h].reshape(h, w), es.crop(first["mask"], first["rect"]), "the raw read-back: the mask")
        es.assert_bits(buf[3 * w * h:].reshape(h, w), es.crop(first["planes"][2], first["rect"]), "the raw read-back: s")
        # a refused call (flow above 1; then a dab with a radius of 0) leaves the record
        full = np.zeros((len(five), 8), F)
        full[:, :5] = five
        bad = capi.HydroParams(iterations=9, **{**es.HYDRO, "flow": 1.5})
        out = (C.c_int32 * 4)()
        assert sc.ctx.lib.vr_terrain_erode_hydraulic(a.handle, C.byref(bad), full.ctypes.data_as(C.c_void_p), len(full), out) == capi.VR_ERR_INVALID_ARGUMENT
        full[1, 2] = 0.0
        good = capi.ErodeParams(iterations=3, talus=es.THERMAL[0], rate=es.THERMAL[1])
        assert sc.ctx.lib.vr_terrain_erode(a.handle, C.byref(good), full.ctypes.data_as(C.c_void_p), len(full), out) == capi.VR_ERR_INVALID_ARGUMENT
        assert_state(a, first, "after two refused calls")
        assert erode(a, "thermal", small, 3, es.THERMAL) == second["rect"]
        assert_state(a, second, "a thermal call after a hydraulic one")
        assert len(a.ErosionState()[2]) == 1
        miss = np.float32([es.dab(sc.hm.shape, S, -40.0, 5.0, 3.0, 0.0, 1.0)])
        assert erode(a, "thermal", miss, 3, es.THERMAL) == (0, 0, 0, 0)
        assert a.ErosionState() == ((0, 0, 0, 0), None, []) and _state_raw(sc, a, None, 0) == (capi.VR_OK, (0, 0, 0, 0), 0)
        assert_bytes(level0(a, "height"), second["bytes"], "level 0 after the call that misses")
    finally:
        a.close()
