"""GPU tests of vr_terrain_erode_hydraulic.  The eroded map must equal the numpy float32 model (tests/hydro_model.py) in every byte -
no tolerance anywhere: vr_hydro.h's arithmetic is IEEE fp32 in a fixed order, subnormals kept, and a cell is a pure function of the
sweep before, so neither the tile of the device's kernel nor the number of sweeps it advances per launch may show - and the eroded
terrain must be the one created from the model's map.  Scenes and helpers are those of tests/level0_common.py."""
import ctypes as C

import numpy as np
import pytest

from vrenderer_amd import capi
from tests import brush_model as bm
from tests import erode_model as em
from tests import hydro_model as hm
from tests.level0_common import SCENES, assert_bytes, assert_terrains_equal, borders, dab, five_dabs, full_mask, level0, make_scenes, mask_dabs, world_of

pytestmark = pytest.mark.gpu

# 20 sweeps of these change 250 .. 350 texels of each scene under the five-dab mask, by up to 23 steps, none to 0 or 255 (chosen with
# the model on the CPU; the tests assert what they need of it again)
ITER = 20
P = dict(rain=1.0, flow=0.5, capacity=8.0, dissolve=0.5, deposit=0.25, evaporation=0.05)
TALUS, RATE = 1.5, 0.125                                             # of the thermal calls that share a test with a hydraulic one


@pytest.fixture(scope="module")
def scenes(gpu_ctx):
    return make_scenes(gpu_ctx, SCENES)


_MODEL = {}


def model(sc, dabs, iterations, hm_=None, **kw):
    """The model's (map, rect), computed once per distinct call."""
    src = sc.hm if hm_ is None else hm_
    p = {**P, **kw}
    key = (sc.name, src.tobytes(), np.asarray(dabs, np.float32).tobytes(), iterations, tuple(sorted(p.items())))
    if key not in _MODEL:
        _MODEL[key] = hm.hydro(src, dabs, world_of(sc), iterations, **p)
    return _MODEL[key]


def hydro(tp, dabs, iterations, **kw):
    return tp.ErodeHydraulic(dabs, iterations, **{**P, **kw})


@pytest.mark.parametrize("name", SCENES)
def test_bytes_equal_the_model(scenes, name):
    """1. A five-dab mask on each scene: level 0 equals the model in every byte, the albedo is untouched, the rectangle is the model's."""
    sc = scenes[name]
    dabs = mask_dabs(sc.hm.shape, world_of(sc))
    want, want_rect = model(sc, dabs, ITER)
    changed = want != sc.hm
    assert changed.sum() >= 30 and ((want[changed] > 0) & (want[changed] < 255)).sum() >= 10
    a = sc.terrain(sc.hm, sc.al, cast=False, render=False)
    rect = hydro(a, dabs, ITER)
    assert rect == tuple(want_rect), (rect, want_rect)
    assert_bytes(level0(a, "height"), want, f"{name}, hydraulic")
    assert_bytes(level0(a, "albedo"), sc.al, f"{name}, hydraulic: the albedo")
    a.close()


def ridge_map(size):
    """Ridges 64 texels apart that run obliquely to both axes: the water on their flanks crosses every row and every column."""
    y, x = np.mgrid[0:size, 0:size]
    return (40 + 6 * np.abs((x + 2 * y) % 64 - 32)).astype(np.uint8)


def test_tile_borders_and_launch_boundaries(scenes, gpu_ctx):
    """2. A full mask over the 128^2 map, which the build's tile does not divide, on a noise map and on a ridge map whose water runs
    across the borders, for 1, K - 1, K, K + 1 and 2K + 1 iterations (one launch with a remainder, a full one, a full one and a
    remainder, two and a remainder).  On the model alone: texels change on both sides of every interior tile border at every count -
    at ONE iteration in the fp32 state h, not in the bytes: the definition leaves h' + s' = h after the first sweep, what a texel
    dissolved is still above it, so no byte can change before the second sweep, on any implementation - and the single call of K + 1
    differs in at least 30 texels from a call of K followed by a call of 1: the water and the sediment carried across a launch
    matter.  Then the device's bytes are the model's; and 2K + 1 iterations at one sweep per launch give the same bytes."""
    lib = gpu_ctx.lib
    cfg = (C.c_int32 * 4)()
    assert lib.vr_debug_hydro_config(cfg) == capi.VR_OK
    tw, th, k = cfg[0], cfg[1], cfg[2]
    sc = scenes["multi"]
    size = sc.hm.shape[0]
    assert sc.hm.shape == (size, size)
    bx, by = borders(size, tw), borders(size, th)
    assert len(bx) >= 1 and len(by) >= 1 and len(bx) + len(by) >= 3 and size % tw and size % th, (tw, th, size)
    assert k >= 2
    S = world_of(sc)
    dabs = full_mask(S)
    maps = {"noise": np.random.default_rng(5).integers(0, 256, sc.hm.shape, dtype=np.uint8), "ridge": ridge_map(size)}
    counts = sorted({1, k - 1, k, k + 1, 2 * k + 1})
    for what, src in maps.items():
        for n in counts:
            want, want_rect = model(sc, dabs, n, hm_=src)
            assert tuple(want_rect) == (0, 0, size, size)
            if n == 1:
                changed = hm.state(src, dabs, S, 1, **P)[0] != src.astype(np.float32)
                assert np.array_equal(want, src)
            else:
                changed = want != src
            for b in by:
                assert changed[b - 1, :].any() and changed[b, :].any(), (what, n, b)
            for b in bx:
                assert changed[:, b - 1].any() and changed[:, b].any(), (what, n, b)
            if n == k + 1:
                first, _ = model(sc, dabs, k, hm_=src)
                split, _ = model(sc, dabs, 1, hm_=first)
                assert (split != want).sum() >= 30, (what, (split != want).sum())
            a = sc.terrain(src, sc.al, cast=False, render=False)
            assert hydro(a, dabs, n) == tuple(want_rect)
            assert_bytes(level0(a, "height"), want, f"{what}, {n} iterations, tile {tw} x {th}, K {k}")
            a.close()
    src = maps["ridge"]
    want, _ = model(sc, dabs, 2 * k + 1, hm_=src)
    a = sc.terrain(src, sc.al, cast=False, render=False)
    try:
        assert lib.vr_debug_hydro_sweeps_per_launch(1) == capi.VR_OK
        hydro(a, dabs, 2 * k + 1)
        assert_bytes(level0(a, "height"), want, f"ridge, {2 * k + 1} iterations, one sweep per launch")
    finally:
        assert lib.vr_debug_hydro_sweeps_per_launch(0) == capi.VR_OK
        a.close()


@pytest.mark.parametrize("name", SCENES)
def test_the_terrain_is_the_one_created_from_the_eroded_map(scenes, name):
    """3. A (SetHeight on, pyramid built, one frame rendered; then eroded) against B created from the model's map: every mip level,
    node heights and selections, every G-buffer plane for cameras 0 and 5, sampled heights with normals, 64 ray hits."""
    sc = scenes[name]
    dabs = mask_dabs(sc.hm.shape, world_of(sc))
    want, _ = model(sc, dabs, ITER)
    a = sc.terrain(sc.hm, sc.al)
    hydro(a, dabs, ITER)
    b = sc.terrain(want, sc.al)
    assert_terrains_equal(sc, a, b, name)
    a.close(); b.close()


def test_history(scenes):
    """4. Enable, erode, commit, undo: the original bytes; redo: the model's.  One call is one record; a hydraulic and a thermal call
    in one step undo together."""
    sc = scenes["odd"]
    S = world_of(sc)
    dabs = mask_dabs(sc.hm.shape, S)
    want, _ = model(sc, dabs, ITER)
    a = sc.terrain(sc.hm, sc.al, cast=False, render=False)
    a.EnableHistory(1 << 20)
    hydro(a, dabs, ITER)
    assert a.HistoryStatus()["open_records"] == 1
    a.CommitHistory()
    assert_bytes(level0(a, "height"), want, "eroded")
    assert a.Undo()
    assert_bytes(level0(a, "height"), sc.hm, "undone")
    assert a.Redo()
    assert_bytes(level0(a, "height"), want, "redone")
    again, _ = model(sc, dabs, 7, hm_=want)
    both, _ = em.erode(again, dabs, S, 3, 0.0, RATE)
    assert (again != want).sum() >= 30 and (both != again).sum() >= 30
    hydro(a, dabs, 7)
    a.Erode(dabs, 3, 0.0, RATE)
    assert a.HistoryStatus()["open_records"] == 2
    a.CommitHistory()
    assert_bytes(level0(a, "height"), both, "a hydraulic and a thermal erosion")
    assert a.Undo()
    assert_bytes(level0(a, "height"), want, "the step of two undone")
    assert a.Undo() and not a.Undo()
    assert_bytes(level0(a, "height"), sc.hm, "everything undone")
    a.close()


@pytest.mark.parametrize("second_stream", (False, True))
def test_a_stroke_a_hydraulic_and_a_thermal_call_with_nothing_between(scenes, gpu_ctx, second_stream):
    """5. A RAISE stroke, a hydraulic erosion over an overlapping rectangle and a thermal erosion of the same mask (all three reuse the
    terrain's dab buffers), with no synchronisation between: the model of the calls in sequence.  Again with the context on a second
    stream."""
    import torch
    sc = scenes["fast64"]
    S = world_of(sc)
    raise_dabs = five_dabs(sc.hm.shape, S, bm.RAISE)
    mask = np.float32([dab(sc.hm.shape, S, 24.0, 30.0, 20.0, 0.0, 1.0), dab(sc.hm.shape, S, 50.0, 12.0, 9.0, 0.7, 0.6)])
    m1, r1 = bm.stroke(sc.hm, bm.RAISE, raise_dabs, S)
    m2, r2 = hm.hydro(m1, mask, S, ITER, **P)
    m3, r3 = em.erode(m2, mask, S, 5, TALUS, RATE)
    assert (m2 != m1).sum() >= 30 and (m3 != m2).sum() >= 30
    assert r1[0] < r2[0] + r2[2] and r2[0] < r1[0] + r1[2] and r1[1] < r2[1] + r2[3] and r2[1] < r1[1] + r1[3]         # the rectangles overlap
    a = sc.terrain(sc.hm, sc.al)
    gpu_ctx.synchronize()
    side = torch.cuda.Stream() if second_stream else None
    try:
        if side is not None:
            gpu_ctx.set_stream(side.cuda_stream)
        a.Brush("raise", raise_dabs)
        assert hydro(a, mask, ITER) == tuple(r2)
        assert a.Erode(mask, 5, TALUS, RATE) == tuple(r3)
        gpu_ctx.synchronize()
        assert_bytes(level0(a, "height"), m3, f"stroke, hydraulic, thermal (second stream: {second_stream})")
    finally:
        torch.cuda.synchronize()
        gpu_ctx.set_stream(0)
        a.close()


@pytest.mark.parametrize("second_stream", (False, True))
def test_the_shared_block_grows_behind_a_pending_call(scenes, gpu_ctx, second_stream):
    """6. Both erosions keep their planes in one block.  A thermal call under a mask of about 20 x 20 texels (three planes: the block
    stays at its initial 64 KiB), a hydraulic call under a whole-map mask (seven planes of 64 x 64: the block must grow while the
    first call may still be pending) and the small thermal call again, with nothing between: level 0 is the models applied in
    sequence, and the scratch bytes grew at the second call and not at the third.  Again with the context on a second stream."""
    import torch
    sc = scenes["fast64"]
    S = world_of(sc)
    small = np.float32([dab(sc.hm.shape, S, 30.0, 28.0, 9.0, 0.0, 1.0)])
    whole = full_mask(S)
    m1, r1 = em.erode(sc.hm, small, S, ITER, 0.0, RATE)
    m2, r2 = hm.hydro(m1, whole, S, ITER, **P)
    m3, r3 = em.erode(m2, small, S, ITER, 0.0, RATE)
    assert (m1 != sc.hm).sum() >= 30 and (m2 != m1).sum() >= 30 and (m3 != m2).sum() >= 30
    assert 18 <= r1[2] <= 22 and 18 <= r1[3] <= 22 and tuple(r2) == (0, 0, 64, 64) and tuple(r3) == tuple(r1)
    assert 3 * 4 * (r1[2] * r1[3] + 63) <= 1 << 16 < 7 * 4 * r2[2] * r2[3]
    a = sc.terrain(sc.hm, sc.al)
    gpu_ctx.synchronize()
    side = torch.cuda.Stream() if second_stream else None
    try:
        if side is not None:
            gpu_ctx.set_stream(side.cuda_stream)
        assert a.Erode(small, ITER, 0.0, RATE) == tuple(r1)
        s1 = a.memory_bytes()["scratch"]
        assert hydro(a, whole, ITER) == tuple(r2)
        s2 = a.memory_bytes()["scratch"]
        assert a.Erode(small, ITER, 0.0, RATE) == tuple(r3)
        s3 = a.memory_bytes()["scratch"]
        gpu_ctx.synchronize()
        assert_bytes(level0(a, "height"), m3, f"thermal, hydraulic, thermal (second stream: {second_stream})")
        assert s2 > s1 and s3 == s2, (s1, s2, s3)
    finally:
        torch.cuda.synchronize()
        gpu_ctx.set_stream(0)
        a.close()


def test_a_refused_call_leaves_no_trace(scenes):
    """7. A refused call (flow above 1) between two good ones: VR_ERR_INVALID_ARGUMENT, and the map is the model's of the two good
    calls.  n == 0 and dabs that all miss the map are VR_OK with the rectangle {0, 0, 0, 0} and change nothing.  The seven planes of
    the rectangle are counted under scratch."""
    sc = scenes["odd"]
    S = world_of(sc)
    dabs = mask_dabs(sc.hm.shape, S)
    first, _ = model(sc, dabs, 5)
    second, rect2 = model(sc, dabs, 9, hm_=first, rain=2.0, evaporation=0.2)
    assert (first != sc.hm).sum() >= 30 and (second != first).sum() >= 30
    a = sc.terrain(sc.hm, sc.al, cast=False, render=False)
    before = a.memory_bytes()["scratch"]
    hydro(a, dabs, 5)
    full = np.zeros((len(dabs), 8), np.float32)
    full[:, :5] = dabs
    params = capi.HydroParams(iterations=9, **{**P, "flow": 1.5})
    rect = (C.c_int32 * 4)(-1, -1, -1, -1)
    assert sc.ctx.lib.vr_terrain_erode_hydraulic(a.handle, C.byref(params), full.ctypes.data_as(C.c_void_p), len(full), rect) == capi.VR_ERR_INVALID_ARGUMENT
    assert_bytes(level0(a, "height"), first, "after the refused call")
    miss = np.float32([dab(sc.hm.shape, S, -40.0, 5.0, 3.0, 0.0, 1.0), dab(sc.hm.shape, S, 10.5, 12.5, 0.2, 0.0, 1.0)])
    assert hydro(a, miss, 9) == (0, 0, 0, 0) and hydro(a, np.zeros((0, 5), np.float32), 9) == (0, 0, 0, 0)
    assert_bytes(level0(a, "height"), first, "after calls that miss")
    assert hydro(a, dabs, 9, rain=2.0, evaporation=0.2) == tuple(rect2)
    assert_bytes(level0(a, "height"), second, "after the second good call")
    assert a.memory_bytes()["scratch"] - before >= 7 * 4 * rect2[2] * rect2[3]
    a.close()
