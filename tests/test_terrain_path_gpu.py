"""GPU tests of vr_terrain_path.  The map with the path in it must equal the numpy float32 model (tests/path_model.py) in every byte -
no tolerance anywhere: vr_path.h's arithmetic is IEEE fp32 in a fixed order, and a texel is a pure function of its own byte, its
coordinates and the call, so neither the rectangle nor the tile nor the device's order of segments may show.  Scenes and test bodies
are those of tests/level0_common.py; the calls (pts, p) are tests/path_cases.py's, whose preconditions are asserted on the model's
output (and, without a device, in tests/test_path_model_cpu.py)."""
import numpy as np
import pytest

from tests import level0_common as lc
from tests import path_cases as pc
from tests import path_model as pm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scenes(gpu_ctx):
    return lc.make_scenes(gpu_ctx, pc.SCENES, pc.WORLD)


def apply(tp, which, call):
    """One vr_terrain_path with the parameters of tests/path_model.params."""
    pts, p = call
    return tp.Path(which, pts, p["radius"], hardness=p["hardness"], opacity=p["opacity"], op=p["op"], color=p["color"], channels=p["channel_mask"], closed=p["closed"])


PATH = lc.Level0Op("vr_terrain_path", apply, lambda texels, call, world: pc.run_model(texels, *call, world))


def preconditions(call):
    return lambda before, want, detail, what: pc.check_preconditions(before, want, call[1], detail, what)


def _height_op(sc, op):
    call = pc.height_case(sc.name, sc.hm, op)
    lc.check_height_call(sc, PATH, call, f"{sc.name}, {pc.OP_IDS[op]}", preconditions(call))


@pytest.mark.parametrize("op", pc.HEIGHT_OPS, ids=[pc.OP_IDS[o] for o in pc.HEIGHT_OPS])
def test_each_op_on_fast64(scenes, op):
    """1. LEVEL, CUT and FILL along the five-point bent path, a different height at every point and one bend sharper than 90 degrees:
    level 0 equals the model in every byte, the rectangle is the model's, the albedo is untouched, and the decoded tables are those of
    a terrain created from the model's map."""
    _height_op(scenes["fast64"], op)


@pytest.mark.parametrize("name", [n for n in pc.SCENES if n != "fast64"])
def test_the_other_scenes(scenes, name):
    """2. One op each on the odd sizes, the 2 x 2-surface world and the 512x32 map, whose path runs the whole length of the map and
    crosses every tile column."""
    _height_op(scenes[name], pc.scene_op(name))


@pytest.mark.parametrize("name", pc.SCENES)
def test_paint(scenes, name):
    """3. PAINT on the albedo with channel_mask 5: channels 0 and 2 equal the model, channels 1 and 3 and the heightmap are untouched,
    and the mip chain is that of a terrain created from the model's albedo."""
    sc = scenes[name]
    call = pc.albedo_case(name, sc.al)
    lc.check_albedo_call(sc, PATH, call, f"{name}, a painted path", preconditions(call))


def test_three_hundred_segments(scenes):
    """4. A 300-segment zigzag inside one 32 x 8 tile of fast64: two chunks of the walk, more than 256 segments on that tile, and on
    the model winners from both below and above index 256 within it."""
    sc = scenes["fast64"]
    call = (pc.zigzag(sc.hm.shape, lc.world_of(sc)), pc.zigzag_params())
    d = PATH.model(sc.hm, call, lc.world_of(sc))[2]
    win = d["winner"][8:16, 0:32]
    assert len(d["segments"]) == 300 and (win[win >= 0] < 256).sum() >= 20 and (win >= 256).sum() >= 20
    lc.check_one_call(sc, PATH, call, "300 segments", min_changed=100)


@pytest.mark.parametrize("shape", ("closed", "single", "repeated", "leaves"))
def test_degenerate_shapes(scenes, shape):
    """5. A closed loop; n == 1; a path with a repeated point; a path that leaves the map and re-enters."""
    sc = scenes["fast64"]
    lc.check_one_call(sc, PATH, pc.degenerate_cases(sc.hm.shape, lc.world_of(sc))[shape], shape)


def test_order_with_nothing_between(scenes):
    """6. A stroke, a path and an erosion queued back to back, no host wait between: the path sees the stroked map and the erosion
    the map with the path in it - the model's chain, which differs from the chain with the path left out or laid on the map before the
    stroke."""
    sc = scenes["odd"]
    lc.check_order_with_nothing_between(sc, PATH, pc.height_case("odd", sc.hm, pm.LEVEL), "path")


def test_history(scenes):
    """7. Enable, path, commit, undo: the original bytes; redo: the model's.  One call is one record, and two calls before one commit
    are one step."""
    sc = scenes["odd"]
    pts, p = pc.height_case("odd", sc.hm, pm.FILL)
    second = (pts[::-1], dict(p, op=pm.CUT, radius=float(np.float32(0.5 * p["radius"]))))
    lc.check_history(sc, PATH, [(pts, p)], (pts, p), second)


def test_calls_that_launch_nothing(scenes):
    """8. n == 0, a path beside the map, and calls refused on a real terrain (PAINT on the heightmap; a closed path of two points):
    every byte and the history's status stay as they were.  Then a good call still gives the model's bytes."""
    sc = scenes["odd"]
    S = lc.world_of(sc)
    pts, p = pc.height_case("odd", sc.hm, pm.LEVEL)
    beside = np.float32([pc.point(sc.hm.shape, S, -40.0, 5.0, 10.0), pc.point(sc.hm.shape, S, -30.0, 60.0, 90.0), pc.point(sc.hm.shape, S, 20.0, 90.0, 90.0)])
    lc.check_calls_that_launch_nothing(sc, PATH, (pts, p), misses=[(beside, p), (np.zeros((0, 3), np.float32), p)],
                                       refused=[(pts, dict(p, op=pm.PAINT)), (pts[:2], dict(p, closed=True))])


def test_a_path_with_a_lazily_fused_frame_pending():
    """9. A fused frame that left its colour planes to their first reader, then Path, then a G-buffer download: the planes are those
    of the eager path (VR_OPT_GBUFFER_LAZY off) - the frame on the terrain as it was; the next frame shows the path, and is the frame
    of a terrain created from the model's map."""
    pts = np.float32([pc.point((256, 256), 256.0, fx * 256, fy * 256, hh) for fx, fy, hh in
                      ((0.05, 0.1, 250.0), (0.5, 0.35, 20.0), (0.3, 0.7, 240.0), (0.9, 0.55, 10.0), (0.6, 0.95, 200.0))])
    p = pm.params(40.0, hardness=0.3, opacity=1.0, op=pm.LEVEL)
    lc.check_with_a_lazily_fused_frame_pending(PATH, (pts, p), lambda hm: pm.path(hm, pts, p, 256.0)[0], "path", min_changed=256 * 256 // 4)
