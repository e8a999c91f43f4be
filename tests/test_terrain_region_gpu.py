"""GPU tests of vr_terrain_region.  The map with the region in it must equal the numpy float32 model (tests/region_model.py) in every
byte - no tolerance anywhere: vr_region.h's arithmetic is IEEE fp32 in a fixed order, and a texel is a pure function of its own byte,
its coordinates and the call, so neither the rectangle nor the tile nor the device's order of edges may show.  Scenes and helpers are
those of tests/test_terrain_path_gpu.py; the calls are tests/region_cases.py's, whose preconditions are asserted on the model's output
(and, without a device, in tests/test_region_model_cpu.py)."""
import numpy as np
import pytest

import vrenderer_amd as vr
from tests import brush_model as bm
from tests import erode_model as em
from tests import noise_cases as nc
from tests import region_cases as rc
from tests import region_model as rm
from tests import test_gbuffer_lazy_gpu as gl
from tests import test_terrain_edit_gpu as te
from tests.common import params
from tests.fusion_common import PLANES, assert_same_frame, terrain_fixture
from tests.test_terrain_brush_gpu import assert_bytes, five_dabs, level0, world_of
from tests.test_terrain_texture_gpu import ExtraScene

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scenes(gpu_ctx):
    out = {n: (te.Scene if n in te.SCENES else ExtraScene)(gpu_ctx, n) for n in rc.SCENES}
    for n, sc in out.items():
        assert world_of(sc) == rc.WORLD[n]
    return out


def apply(tp, which, pts, contours, p):
    """One vr_terrain_region with the parameters of tests/region_model.params."""
    return tp.Region(which, pts, op=p["op"], target=p["target"], feather=p["feather"], opacity=p["opacity"], color=p["color"], channels=p["channel_mask"],
                     feather_inside=p["feather_inside"], contours=contours)


_MODEL = {}


def model(texels, pts, contours, p, world):
    """The model's (texels, rect, detail) of one call, computed once per distinct call."""
    key = (texels.tobytes(), texels.shape, np.asarray(pts, np.float32).tobytes(), contours, repr(sorted(p.items())), world)
    if key not in _MODEL:
        _MODEL[key] = rc.run_model(texels, pts, contours, p, world)
    return _MODEL[key]


def _height_op(sc, op, mode="skirt"):
    name, S = sc.name, world_of(sc)
    pts, contours, p = rc.height_case(name, sc.hm, op, mode)
    want, want_rect, detail = model(sc.hm, pts, contours, p, S)
    what = f"{name}, {rm.OP_IDS[op]}, {mode}"
    print(what, rc.check_preconditions(sc.hm, want, p, detail, what))
    a = sc.terrain(sc.hm, sc.al, cast=False, render=False)
    rect = apply(a, "height", pts, contours, p)
    assert rect == tuple(want_rect), (rect, want_rect)
    assert_bytes(level0(a, "height"), want, what)
    assert_bytes(level0(a, "albedo"), sc.al, f"{what}: the albedo")
    b = sc.terrain(want, sc.al, cast=False, render=False)
    te._assert_tables_equal(a, b, what)
    a.close(); b.close()


@pytest.mark.parametrize("mode", rc.MODES)
@pytest.mark.parametrize("op", rc.HEIGHT_OPS, ids=[rm.OP_IDS[o] for o in rc.HEIGHT_OPS])
def test_each_op_on_fast64(scenes, op, mode):
    """1. LEVEL, CUT, FILL and RAISE inside the six-vertex polygon with two reflex vertices, with the skirt, with the feather inside and
    with a hard edge: level 0 equals the model in every byte, the rectangle is the model's, the albedo is untouched, and the decoded
    tables are those of a terrain created from the model's map."""
    _height_op(scenes["fast64"], op, mode)


@pytest.mark.parametrize("name", [n for n in rc.SCENES if n != "fast64"])
def test_the_other_scenes(scenes, name):
    """2. One op each on the odd sizes, the 2 x 2-surface world and the 512x32 map, whose polygon spans every tile column."""
    sc = scenes[name]
    if name == "wide":
        pts = rc.scene_polygon(name, sc.hm.shape)[0]
        tex = (pts[:, 0] + rc.WORLD[name] / 2) / rc.WORLD[name] * sc.hm.shape[1] - 0.5
        assert tex.min() < 0 and tex.max() > sc.hm.shape[1] - 1
    _height_op(sc, rc.scene_op(name))


@pytest.mark.parametrize("name", rc.SCENES)
def test_paint(scenes, name):
    """3. PAINT on the albedo with channel_mask 5: channels 0 and 2 equal the model, channels 1 and 3 and the heightmap are untouched,
    and the mip chain is that of a terrain created from the model's albedo."""
    sc = scenes[name]
    S = world_of(sc)
    pts, contours, p = rc.albedo_case(name, sc.al)
    want, want_rect, detail = model(sc.al, pts, contours, p, S)
    print(name, rc.check_preconditions(sc.al, want, p, detail, f"{name}, paint"))
    assert np.array_equal(want[..., 1], sc.al[..., 1]) and np.array_equal(want[..., 3], sc.al[..., 3])
    a = sc.terrain(sc.hm, sc.al, cast=False, render=False)
    assert apply(a, "albedo", pts, contours, p) == tuple(want_rect)
    assert_bytes(level0(a, "albedo"), want, f"{name}, a painted region")
    assert_bytes(level0(a, "height"), sc.hm, f"{name}, a painted region: the heightmap")
    b = sc.terrain(sc.hm, want, cast=False, render=False)
    te._assert_chains_equal(a, b, f"{name}, a painted region")
    a.close(); b.close()


def _one_call(sc, pts, contours, p, what):
    S = world_of(sc)
    want, want_rect, d = model(sc.hm, pts, contours, p, S)
    assert (want != sc.hm).sum() >= 200, what
    a = sc.terrain(sc.hm, sc.al, cast=False, render=False)
    assert apply(a, "height", pts, contours, p) == tuple(want_rect), what
    assert_bytes(level0(a, "height"), want, what)
    a.close()
    return want_rect, d


def test_three_hundred_edges(scenes):
    """4. A 300-edge sawtooth whose teeth all cross the rows 8 .. 15 of fast64: two chunks of the walk, and on the model inside texels
    of the tile [32, 64) x [8, 16) with crossings to their left from edges both below and above index 256."""
    sc = scenes["fast64"]
    pts, p = rc.sawtooth(sc.hm.shape, world_of(sc)), rc.sawtooth_params()
    d = model(sc.hm, pts, None, p, world_of(sc))[2]
    assert rc.sawtooth_precondition(d, sc.hm.shape) >= 5
    _one_call(sc, pts, None, p, "300 edges")


def test_tiles_that_see_an_edge_through_its_span_alone(scenes):
    """5. On 512x32, a rectangle whose left edge is at least 96 texels left of inside texels, with a small feather: some tiles hold
    inside texels and no texel nearer than the feather to any edge."""
    sc = scenes["wide"]
    pts, contours, p = rc.shadow_case(sc.hm.shape, world_of(sc))
    d = model(sc.hm, pts, contours, p, world_of(sc))[2]
    tiles = rc.shadow_precondition(d)
    assert tiles and all(tx - min(float(e["ax"]) for e in d["edges"]) >= 96 for tx, _ in tiles)
    _one_call(sc, pts, contours, p, "shadow-only tiles")


@pytest.mark.parametrize("shape", ("island", "hole in hole", "bow-tie", "off all sides", "contains the map", "on texel centres", "aligned on texel centres"))
def test_shapes(scenes, shape):
    """6. An island (two contours); a hole within a hole (three); a bow-tie; a polygon partly off the map on all four sides; a polygon
    that contains the whole map - every edge outside it, the rectangle the whole map; a square with its vertices exactly on texel
    centres, turned and axis-aligned."""
    sc = scenes["fast64"]
    S = world_of(sc)
    pts, contours, p = rc.aligned_square(sc.hm.shape, S) if shape.startswith("aligned") else rc.shape_cases(sc.hm.shape, S)[shape]
    rect, d = _one_call(sc, pts, contours, p, shape)
    h, w = sc.hm.shape
    if shape in ("off all sides", "contains the map"):
        assert rect == (0, 0, w, h)
    if shape == "contains the map":
        assert d["inside"].all() and all(float(e["ax"]) < 0 for e in d["edges"])
    if shape in ("island", "hole in hole"):
        assert not d["inside"][h // 2, w // 2] if shape == "island" else d["inside"][h // 2, w // 2]


def test_order_with_nothing_between(scenes):
    """7. A stroke, a region and an erosion queued back to back, no host wait between: the region sees the stroked map and the erosion
    the map with the region in it - the model's chain, which differs from the chain with the region left out or applied to the map
    before the stroke."""
    sc = scenes["odd"]
    S = world_of(sc)
    stroke = five_dabs(sc.hm.shape, S, bm.RAISE)
    pts, contours, p = rc.height_case("odd", sc.hm, rm.CUT)
    mask = nc.five_dabs(sc.hm.shape, S)
    brushed, _ = bm.stroke(sc.hm, bm.RAISE, stroke, S)
    cut, region_rect, _ = model(brushed, pts, contours, p, S)
    want, erode_rect = em.erode(cut, mask, S, 20, 0.5, 0.125)
    first = bm.stroke(model(sc.hm, pts, contours, p, S)[0], bm.RAISE, stroke, S)[0]
    assert (first != cut).sum() >= 30 and (em.erode(brushed, mask, S, 20, 0.5, 0.125)[0] != want).sum() >= 30 and (want != cut).sum() >= 30
    assert (em.erode(first, mask, S, 20, 0.5, 0.125)[0] != want).sum() >= 30
    a = sc.terrain(sc.hm, sc.al)
    a.Brush("raise", stroke)
    assert apply(a, "height", pts, contours, p) == tuple(region_rect)
    assert a.Erode(mask, 20, 0.5, 0.125) == tuple(erode_rect)
    assert_bytes(level0(a, "height"), want, "brush, region, erode")
    assert_bytes(level0(a, "albedo"), sc.al, "brush, region, erode: the albedo")
    a.close()


def test_history(scenes):
    """8. Enable, region, commit, undo: the original bytes; redo: the model's.  One call is one record, and two calls before one commit
    are one step."""
    sc = scenes["odd"]
    S = world_of(sc)
    pts, contours, p = rc.height_case("odd", sc.hm, rm.FILL)
    want = model(sc.hm, pts, contours, p, S)[0]
    assert (want != sc.hm).sum() >= 200
    a = sc.terrain(sc.hm, sc.al, cast=False, render=False)
    a.EnableHistory(1 << 20)
    apply(a, "height", pts, contours, p)
    assert a.HistoryStatus()["open_records"] == 1
    a.CommitHistory()
    st = a.HistoryStatus()
    assert (st["undo_steps"], st["redo_steps"], st["open_records"]) == (1, 0, 0)
    assert_bytes(level0(a, "height"), want, "with the region")
    assert a.Undo()
    assert_bytes(level0(a, "height"), sc.hm, "undone")
    assert a.Redo() and not a.Redo()
    assert_bytes(level0(a, "height"), want, "redone")
    assert_bytes(level0(a, "albedo"), sc.al, "the albedo")
    a.close()
    p2 = dict(p, op=rm.RAISE, target=-30.0, feather_inside=True)
    second = model(want, pts, contours, p2, S)[0]
    assert (second != want).sum() >= 30
    a = sc.terrain(sc.hm, sc.al, cast=False, render=False)
    a.EnableHistory(1 << 20)
    apply(a, "height", pts, contours, p)
    apply(a, "height", pts, contours, p2)
    assert a.HistoryStatus()["open_records"] == 2
    a.CommitHistory()
    st = a.HistoryStatus()
    assert (st["undo_steps"], st["redo_steps"], st["open_records"]) == (1, 0, 0)
    assert_bytes(level0(a, "height"), second, "two calls")
    assert a.Undo() and not a.Undo()
    assert_bytes(level0(a, "height"), sc.hm, "two calls undone in one step")
    assert a.Redo()
    assert_bytes(level0(a, "height"), second, "two calls redone")
    a.close()


def test_calls_that_launch_nothing(scenes):
    """9. n == 0, a region beside the map, and calls refused on a real terrain (PAINT on the heightmap; a contour of two points): every
    byte and the history's status stay as they were.  Then a good call still gives the model's bytes."""
    sc = scenes["odd"]
    S = world_of(sc)
    pts, contours, p = rc.height_case("odd", sc.hm, rm.LEVEL)
    a = sc.terrain(sc.hm, sc.al, cast=False, render=False)
    a.EnableHistory(1 << 20)
    before = a.HistoryStatus()
    beside = np.float32([rc.vertex(sc.hm.shape, S, -40.0, 5.0), rc.vertex(sc.hm.shape, S, -30.0, 60.0), rc.vertex(sc.hm.shape, S, -12.0, 20.0)])
    assert model(sc.hm, beside, None, p, S)[1] == (0, 0, 0, 0)
    assert apply(a, "height", beside, None, p) == (0, 0, 0, 0)
    assert apply(a, "height", np.zeros((0, 2), np.float32), None, p) == (0, 0, 0, 0)
    for bad_pts, bad_contours, bad in ((pts, None, dict(p, op=rm.PAINT)), (pts, (4, 2), p)):
        with pytest.raises(Exception) as e:
            apply(a, "height", bad_pts, bad_contours, bad)
        assert "vr_terrain_region" in str(e.value), e.value
    assert_bytes(level0(a, "height"), sc.hm, "after calls that launch nothing")
    assert_bytes(level0(a, "albedo"), sc.al, "after calls that launch nothing: the albedo")
    assert a.HistoryStatus() == before
    want, want_rect, _ = model(sc.hm, pts, contours, p, S)
    assert apply(a, "height", pts, contours, p) == tuple(want_rect)
    assert_bytes(level0(a, "height"), want, "after a good call")
    a.close()


def test_a_region_with_a_lazily_fused_frame_pending():
    """10. A fused frame that left its colour planes to their first reader, then Region, then a G-buffer download: the planes are those
    of the eager path (VR_OPT_GBUFFER_LAZY off) - the frame on the terrain as it was; the next frame shows the region, and is the frame
    of a terrain created from the model's map."""
    w, h = 96, 64
    with terrain_fixture(256) as fx:
        v = gl._views(w, h)
        hm = fx["h"]
        pts = np.float32([rc.vertex(hm.shape, 256.0, fx_ * 256, fy * 256) for fx_, fy in ((0.05, 0.1), (0.5, 0.3), (0.95, 0.08), (0.9, 0.9), (0.5, 0.7), (0.1, 0.95))])
        p = rm.params(op=rm.LEVEL, target=240.0, feather=20.0, opacity=1.0)
        want_map, _ = rm.region(hm, pts, p, 256.0)
        assert (want_map != hm).sum() >= hm.size // 4

        def script(scn, lazy):
            out = {}
            try:
                scn.submit(v[1])
                apply(scn.tp, "height", pts, None, p)
                out["before the region"] = gl._capture(scn.rt, scn.hdr)
                scn.submit(v[1])
                out["after the region"] = gl._capture(scn.rt, scn.hdr)
            finally:
                scn.tp.Edit("height", 0, 0, hm)
            return out
        want, _ = gl._both(fx, w, h, script)
        assert not np.array_equal(want["before the region"]["normals"], want["after the region"]["normals"]), "the region is not in view"
        tb = vr.TerrainPass(fx["ctx"], params(256)).Init(want_map, vr.synth_albedo(fx["ctx"], 256, hm))
        scn = gl.Scene(dict(ctx=fx["ctx"], tp=tb), 1, w, h)
        try:
            scn.submit(v[1])
            assert_same_frame(want["after the region"], gl._capture(scn.rt, scn.hdr), "the frame of a terrain created from the model's map", PLANES + ("hdr",))
        finally:
            scn.close()
            tb.close()
