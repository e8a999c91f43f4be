"""GPU tests of vr_terrain_brush.  The stroked map must equal the numpy float32 model (tests/brush_model.py) in every byte - no
tolerance anywhere: vr_brush.h's arithmetic is IEEE fp32 in a fixed order - and the stroked terrain must be the one created from
the model's maps.  Scenes and the state under test are those of tests/level0_common.py: 64^2 + 64^2, 67x45 height + 33x50
albedo (a dab is an ellipse in texel space) and the 2x2-surface world of 128 on 128^2 maps; frames are 256x144."""
import ctypes as C

import numpy as np
import pytest

from vrenderer_amd import capi
from tests import brush_model as bm
from tests.level0_common import (BRUSH_OPS, SCENES, STROKE_KW, assert_bytes, assert_terrains_equal, check_stroke_preconditions, dab, five_dabs, level0, make_scenes,
                                 order_dabs, world_of)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scenes(gpu_ctx):
    return make_scenes(gpu_ctx, SCENES)


@pytest.mark.parametrize("op", sorted(BRUSH_OPS))
@pytest.mark.parametrize("name", SCENES)
def test_bytes_equal_the_model(scenes, name, op):
    """1. Each op on each scene, a stroke of five dabs: level 0 equals the model in every byte, the other map is untouched, the
    returned rectangle is the model's."""
    sc = scenes[name]
    which = "albedo" if op == bm.PAINT else "height"
    before = sc.al if op == bm.PAINT else sc.hm
    dabs = five_dabs(before.shape, world_of(sc), op)
    want, want_rect = bm.stroke(before, op, dabs, world_of(sc), **STROKE_KW[op])
    check_stroke_preconditions(before, want, op)
    a = sc.terrain(sc.hm, sc.al, cast=False, render=False)
    rect = a.Brush(BRUSH_OPS[op], dabs, **STROKE_KW[op])
    assert rect == tuple(want_rect), (rect, want_rect)
    assert_bytes(level0(a, which), want, f"{name}, {BRUSH_OPS[op]}")
    other = "height" if which == "albedo" else "albedo"
    assert_bytes(level0(a, other), sc.hm if other == "height" else sc.al, f"{name}, {BRUSH_OPS[op]}: the other map")
    a.close()


def test_order_and_chunking(scenes):
    """2. 300 dabs, more than 256 of which meet one 32 x 8 tile (a chunk boundary and an ordered compaction across it), in a
    rectangle with tiles no dab meets and rows below it no dab reaches.  A stroke has ONE target, and FLATTEN steps towards one
    target commute up to rounding, so the order is made visible by RAISE with alternating strengths +200 / -200, whose clamps do
    not commute: the device equals the model, and the model of the reversed list differs.  FLATTEN at opacity 0.5 over the same
    300 dabs equals the model too."""
    sc = scenes["fast64"]
    S = world_of(sc)
    hm = np.full_like(sc.hm, 100)
    hm[::3, ::2] = 130
    dabs = order_dabs(hm.shape, S, (200.0, -200.0))
    prepared = [bm.prepare(d, S, 64, 64) for d in dabs]
    assert sum(d["x0"] < 32 and d["x1"] > 0 and d["y0"] < 8 and d["y1"] > 0 for d in prepared) > 256
    want, want_rect = bm.stroke(hm, bm.RAISE, dabs, S)
    assert want_rect[1] + want_rect[3] <= 48 and np.array_equal(want[48:], hm[48:])            # nothing touches the bottom rows
    assert np.array_equal(want[24:32, 40:64], hm[24:32, 40:64]) and want_rect[0] + want_rect[2] > 56 and want_rect[3] > 36     # an untouched tile inside the rectangle
    reversed_, _ = bm.stroke(hm, bm.RAISE, dabs[::-1], S)
    assert (reversed_ != want).sum() >= 30                                                    # the test can see order
    a = sc.terrain(hm, sc.al, cast=False, render=False)
    assert a.Brush("raise", dabs) == tuple(want_rect)
    assert_bytes(level0(a, "height"), want, "300 dabs, RAISE +-200")
    a.close()
    fl = order_dabs(hm.shape, S, (0.5,))
    want, want_rect = bm.stroke(sc.hm, bm.FLATTEN, fl, S, target=40.0)
    a = sc.terrain(sc.hm, sc.al, cast=False, render=False)
    assert a.Brush("flatten", fl, target=40.0) == tuple(want_rect)
    assert_bytes(level0(a, "height"), want, "300 dabs, FLATTEN")
    a.close()


def test_accumulation_inside_a_stroke(scenes):
    """3. Eight coincident RAISE dabs of strength 0.2 in ONE stroke: the centre texel gains 2 (1.6, rounded once).  The same dabs as
    eight calls leave the map as it was (0.2 rounds away every time) - as the model says of both."""
    sc = scenes["fast64"]
    S = world_of(sc)
    hm = np.clip(sc.hm, 20, 230).astype(np.uint8)
    dabs = np.float32([dab(hm.shape, S, 21.0, 33.0, 3.0, 0.7, 0.2)] * 8)
    want, _ = bm.stroke(hm, bm.RAISE, dabs, S)
    assert int(want[33, 21]) == int(hm[33, 21]) + 2 and (want != hm).sum() >= 5
    a = sc.terrain(hm, sc.al, cast=False, render=False)
    a.Brush("raise", dabs)
    assert_bytes(level0(a, "height"), want, "8 dabs in one stroke")
    a.close()
    each = hm
    for d in dabs:
        each, _ = bm.stroke(each, bm.RAISE, d[None, :], S)
    assert np.array_equal(each, hm)
    a = sc.terrain(hm, sc.al, cast=False, render=False)
    for d in dabs:
        a.Brush("raise", d[None, :])
    assert_bytes(level0(a, "height"), hm, "8 strokes of one dab")
    a.close()


def test_smooth_reads_the_snapshot(scenes):
    """4. Two overlapping SMOOTH dabs of opacity 1 over a one-texel spike: the means are those of the map before the stroke."""
    sc = scenes["fast64"]
    S = world_of(sc)
    hm = np.full_like(sc.hm, 100)
    hm[30, 31] = 255
    hm[0, 0] = 10                                                    # and a clamped neighbourhood, at the map's corner
    dabs = np.float32([dab(hm.shape, S, 30.0, 30.0, 5.0, 0.7, 1.0), dab(hm.shape, S, 33.0, 31.0, 5.0, 0.0, 1.0), dab(hm.shape, S, 0.0, 0.0, 3.0, 0.5, 1.0)])
    want, want_rect = bm.stroke(hm, bm.SMOOTH, dabs, S)
    assert int(want[30, 31]) == 117 and int(want[29, 30]) == 117     # 100 + 155 / 9 on the spike and beside it: not a running mean
    assert (want != hm).sum() >= 9
    a = sc.terrain(hm, sc.al, cast=False, render=False)
    assert a.Brush("smooth", dabs) == tuple(want_rect)
    assert_bytes(level0(a, "height"), want, "SMOOTH over a spike")
    a.close()


@pytest.mark.parametrize("name", SCENES)
def test_the_terrain_is_the_one_created_from_the_stroked_maps(scenes, name):
    """5. A (SetHeight on, pyramid built, one frame rendered; then RAISE and PAINT) against B created from the model's maps: every
    mip level, node heights and selections, every G-buffer plane for cameras 0 and 5, sampled heights with normals, 64 ray hits."""
    sc = scenes[name]
    S = world_of(sc)
    hd, ad = five_dabs(sc.hm.shape, S, bm.RAISE), five_dabs(sc.al.shape, S, bm.PAINT)
    hm, _ = bm.stroke(sc.hm, bm.RAISE, hd, S)
    al, _ = bm.stroke(sc.al, bm.PAINT, ad, S, **STROKE_KW[bm.PAINT])
    a = sc.terrain(sc.hm, sc.al)
    a.Brush("raise", hd)
    a.Brush("paint", ad, **STROKE_KW[bm.PAINT])
    b = sc.terrain(hm, al)
    assert_terrains_equal(sc, a, b, name)
    a.close(); b.close()


def test_nothing_outside_nothing_on_a_miss(scenes):
    """6. Dabs that all miss the map - beside it, and one of radius 0.2 texels between four texel centres - are VR_OK with the
    rectangle {0, 0, 0, 0} and leave level 0 alone; so is n = 0.  One dab of radius 4 S changes the whole map, as the model says."""
    sc = scenes["odd"]
    S = world_of(sc)
    a = sc.terrain(sc.hm, sc.al, cast=False, render=False)
    for which, m in (("height", sc.hm), ("albedo", sc.al)):
        h, w = m.shape[:2]
        miss = np.float32([dab(m.shape, S, -9.0, 5.0, 3.0, 0.0, 1.0), dab(m.shape, S, 5.0, h + 30.0, 6.0, 0.7, 1.0),
                           dab(m.shape, S, 10.5, 12.5, 0.2, 0.0, 1.0), [1.0e30, -1.0e30, 1.0, 0.0, 1.0]])
        op = bm.PAINT if which == "albedo" else bm.FLATTEN
        kw = dict(color=(255.0, 255.0, 255.0, 255.0)) if which == "albedo" else dict(target=255.0)
        want, want_rect = bm.stroke(m, op, miss, S, **kw)
        assert tuple(want_rect) == (0, 0, 0, 0) and np.array_equal(want, m)
        assert a.Brush(BRUSH_OPS[op], miss, **kw) == (0, 0, 0, 0)
        assert a.Brush(BRUSH_OPS[op], np.zeros((0, 5), np.float32), **kw) == (0, 0, 0, 0)
        assert_bytes(level0(a, which), m, f"{which} after strokes that miss")
    whole = np.float32([[0.3, -0.2, 4.0 * S, 0.5, 30.0]])
    want, want_rect = bm.stroke(sc.hm, bm.RAISE, whole, S)
    assert tuple(want_rect) == (0, 0, 67, 45) and (want != sc.hm).mean() > 0.9
    assert a.Brush("raise", whole) == (0, 0, 67, 45)
    assert_bytes(level0(a, "height"), want, "one dab of radius 4 S")
    a.close()


def test_refusals_leave_the_terrain_alone(scenes):
    """7. Every invalid argument returns VR_ERR_INVALID_ARGUMENT; level 0 of both maps downloads unchanged afterwards."""
    sc = scenes["odd"]
    a = sc.terrain(sc.hm, sc.al)
    lib, hnd = sc.ctx.lib, a.handle
    nan, inf = float("nan"), float("inf")

    def call(op=capi.VR_BRUSH_RAISE, mask=0xF, target=0.0, color=(0.0, 0.0, 0.0, 0.0), d=(0.0, 0.0, 4.0, 0.5, 1.0), n=1, t=hnd, stroke=True, dabs=True):
        st = capi.BrushStroke(op=op, channel_mask=mask, target=target)
        st.color[:] = color
        arr = (capi.BrushDab * max(n, 1))(*[capi.BrushDab(*d)] * max(n, 1))
        rect = (C.c_int32 * 4)()
        return lib.vr_terrain_brush(t, C.byref(st) if stroke else None, arr if dabs else None, n, rect)

    assert call() == capi.VR_OK and call(n=0, dabs=False) == capi.VR_OK          # the calls below differ from a valid one in one thing
    a.Edit("height", 0, 0, sc.hm)                                                # (undo the valid stroke)
    bad = [dict(t=None), dict(stroke=False), dict(dabs=False), dict(n=capi.VR_MAX_BRUSH_DABS + 1),
           dict(op=4), dict(op=-1),
           dict(d=(nan, 0.0, 4.0, 0.5, 1.0)), dict(d=(0.0, inf, 4.0, 0.5, 1.0)), dict(d=(0.0, 0.0, nan, 0.5, 1.0)), dict(d=(0.0, 0.0, inf, 0.5, 1.0)),
           dict(d=(0.0, 0.0, 4.0, nan, 1.0)), dict(d=(0.0, 0.0, 4.0, 0.5, nan)), dict(d=(0.0, 0.0, 4.0, 0.5, -inf)),
           dict(target=nan), dict(target=inf, op=capi.VR_BRUSH_FLATTEN), dict(color=(0.0, nan, 0.0, 0.0), op=capi.VR_BRUSH_PAINT),
           dict(d=(0.0, 0.0, 0.0, 0.5, 1.0)), dict(d=(0.0, 0.0, -1.0, 0.5, 1.0)),                                     # radius <= 0
           dict(d=(0.0, 0.0, 4.0, 1.0, 1.0)), dict(d=(0.0, 0.0, 4.0, -0.1, 1.0)), dict(d=(0.0, 0.0, 4.0, 1.5, 1.0)),  # hardness outside [0, 1)
           dict(d=(0.0, 0.0, 4.0, 0.5, 255.5)), dict(d=(0.0, 0.0, 4.0, 0.5, -256.0)),                                 # RAISE: |strength| > 255
           dict(op=capi.VR_BRUSH_FLATTEN, d=(0.0, 0.0, 4.0, 0.5, 1.5)), dict(op=capi.VR_BRUSH_SMOOTH, d=(0.0, 0.0, 4.0, 0.5, -0.1)),
           dict(op=capi.VR_BRUSH_PAINT, d=(0.0, 0.0, 4.0, 0.5, 2.0)),
           dict(op=capi.VR_BRUSH_FLATTEN, target=-1.0), dict(op=capi.VR_BRUSH_FLATTEN, target=255.5),
           dict(op=capi.VR_BRUSH_PAINT, color=(0.0, 0.0, 256.0, 0.0)), dict(op=capi.VR_BRUSH_PAINT, color=(-0.5, 0.0, 0.0, 0.0)),
           dict(op=capi.VR_BRUSH_PAINT, mask=0), dict(op=capi.VR_BRUSH_PAINT, mask=16)]
    for kw in bad:
        assert call(**kw) == capi.VR_ERR_INVALID_ARGUMENT, kw
    assert_bytes(level0(a, "height"), sc.hm, "height after the refusals")
    assert_bytes(level0(a, "albedo"), sc.al, "albedo after the refusals")
    a.close()


def test_the_caller_s_array_is_free_on_return(scenes):
    """8. The dab array is overwritten with NaNs straight after the call, before anything is synchronised: the map is the model's
    of the original dabs."""
    sc = scenes["fast64"]
    S = world_of(sc)
    rng = np.random.default_rng(8)
    n = 2000
    buf = np.zeros((n, 8), np.float32)
    buf[:, 0:2] = rng.uniform(-0.5 * S, 0.5 * S, (n, 2))
    buf[:, 2] = rng.uniform(0.5, 4.0, n)
    buf[:, 3] = rng.choice([0.0, 0.7], n)
    buf[:, 4] = rng.uniform(-3.0, 3.0, n)
    original = buf.copy()
    want, want_rect = bm.stroke(sc.hm, bm.RAISE, original, S)
    assert (want != sc.hm).sum() >= 30
    a = sc.terrain(sc.hm, sc.al)
    sc.ctx.synchronize()
    rect = a.Brush("raise", buf)
    buf[:] = np.nan
    sc.ctx.synchronize()
    assert rect == tuple(want_rect)
    assert_bytes(level0(a, "height"), want, "after the caller reused its array")
    a.close()
