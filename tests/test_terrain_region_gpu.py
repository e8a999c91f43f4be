"""GPU tests of vr_terrain_region.  The map with the region in it must equal the numpy float32 model (tests/region_model.py) in every
byte - no tolerance anywhere: vr_region.h's arithmetic is IEEE fp32 in a fixed order, and a texel is a pure function of its own byte,
its coordinates and the call, so neither the rectangle nor the tile nor the device's order of edges may show.  Scenes and test bodies
are those of tests/level0_common.py; the calls (pts, contours, p) are tests/region_cases.py's, whose preconditions are asserted on the
model's output (and, without a device, in tests/test_region_model_cpu.py)."""
import numpy as np
import pytest

from tests import level0_common as lc
from tests import region_cases as rc
from tests import region_model as rm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scenes(gpu_ctx):
    return lc.make_scenes(gpu_ctx, rc.SCENES, rc.WORLD)


def apply(tp, which, call):
    """One vr_terrain_region with the parameters of tests/region_model.params."""
    pts, contours, p = call
    return tp.Region(which, pts, op=p["op"], target=p["target"], feather=p["feather"], opacity=p["opacity"], color=p["color"], channels=p["channel_mask"],
                     feather_inside=p["feather_inside"], contours=contours)


REGION = lc.Level0Op("vr_terrain_region", apply, lambda texels, call, world: rc.run_model(texels, *call, world))


def preconditions(call):
    return lambda before, want, detail, what: rc.check_preconditions(before, want, call[2], detail, what)


def _height_op(sc, op, mode="skirt"):
    call = rc.height_case(sc.name, sc.hm, op, mode)
    lc.check_height_call(sc, REGION, call, f"{sc.name}, {rm.OP_IDS[op]}, {mode}", preconditions(call))


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
    call = rc.albedo_case(name, sc.al)
    lc.check_albedo_call(sc, REGION, call, f"{name}, a painted region", preconditions(call))


def test_three_hundred_edges(scenes):
    """4. A 300-edge sawtooth whose teeth all cross the rows 8 .. 15 of fast64: two chunks of the walk, and on the model inside texels
    of the tile [32, 64) x [8, 16) with crossings to their left from edges both below and above index 256."""
    sc = scenes["fast64"]
    call = (rc.sawtooth(sc.hm.shape, lc.world_of(sc)), None, rc.sawtooth_params())
    d = REGION.model(sc.hm, call, lc.world_of(sc))[2]
    assert rc.sawtooth_precondition(d, sc.hm.shape) >= 5
    lc.check_one_call(sc, REGION, call, "300 edges")


def test_tiles_that_see_an_edge_through_its_span_alone(scenes):
    """5. On 512x32, a rectangle whose left edge is at least 96 texels left of inside texels, with a small feather: some tiles hold
    inside texels and no texel nearer than the feather to any edge."""
    sc = scenes["wide"]
    call = rc.shadow_case(sc.hm.shape, lc.world_of(sc))
    d = REGION.model(sc.hm, call, lc.world_of(sc))[2]
    tiles = rc.shadow_precondition(d)
    assert tiles and all(tx - min(float(e["ax"]) for e in d["edges"]) >= 96 for tx, _ in tiles)
    lc.check_one_call(sc, REGION, call, "shadow-only tiles")


@pytest.mark.parametrize("shape", ("island", "hole in hole", "bow-tie", "off all sides", "contains the map", "on texel centres", "aligned on texel centres"))
def test_shapes(scenes, shape):
    """6. An island (two contours); a hole within a hole (three); a bow-tie; a polygon partly off the map on all four sides; a polygon
    that contains the whole map - every edge outside it, the rectangle the whole map; a square with its vertices exactly on texel
    centres, turned and axis-aligned."""
    sc = scenes["fast64"]
    S = lc.world_of(sc)
    call = rc.aligned_square(sc.hm.shape, S) if shape.startswith("aligned") else rc.shape_cases(sc.hm.shape, S)[shape]
    rect, d = lc.check_one_call(sc, REGION, call, shape)
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
    lc.check_order_with_nothing_between(sc, REGION, rc.height_case("odd", sc.hm, rm.CUT), "region")


def test_history(scenes):
    """8. Enable, region, commit, undo: the original bytes; redo: the model's.  One call is one record, and two calls before one commit
    are one step."""
    sc = scenes["odd"]
    pts, contours, p = rc.height_case("odd", sc.hm, rm.FILL)
    second = (pts, contours, dict(p, op=rm.RAISE, target=-30.0, feather_inside=True))
    lc.check_history(sc, REGION, [(pts, contours, p)], (pts, contours, p), second)


def test_calls_that_launch_nothing(scenes):
    """9. n == 0, a region beside the map, and calls refused on a real terrain (PAINT on the heightmap; a contour of two points): every
    byte and the history's status stay as they were.  Then a good call still gives the model's bytes."""
    sc = scenes["odd"]
    S = lc.world_of(sc)
    pts, contours, p = rc.height_case("odd", sc.hm, rm.LEVEL)
    beside = np.float32([rc.vertex(sc.hm.shape, S, -40.0, 5.0), rc.vertex(sc.hm.shape, S, -30.0, 60.0), rc.vertex(sc.hm.shape, S, -12.0, 20.0)])
    lc.check_calls_that_launch_nothing(sc, REGION, (pts, contours, p), misses=[(beside, None, p), (np.zeros((0, 2), np.float32), None, p)],
                                       refused=[(pts, None, dict(p, op=rm.PAINT)), (pts, (4, 2), p)])


def test_a_region_with_a_lazily_fused_frame_pending():
    """10. A fused frame that left its colour planes to their first reader, then Region, then a G-buffer download: the planes are those
    of the eager path (VR_OPT_GBUFFER_LAZY off) - the frame on the terrain as it was; the next frame shows the region, and is the frame
    of a terrain created from the model's map."""
    pts = np.float32([rc.vertex((256, 256), 256.0, fx * 256, fy * 256) for fx, fy in ((0.05, 0.1), (0.5, 0.3), (0.95, 0.08), (0.9, 0.9), (0.5, 0.7), (0.1, 0.95))])
    p = rm.params(op=rm.LEVEL, target=240.0, feather=20.0, opacity=1.0)
    lc.check_with_a_lazily_fused_frame_pending(REGION, (pts, None, p), lambda hm: rm.region(hm, pts, p, 256.0)[0], "region", min_changed=256 * 256 // 4)
