"""GPU tests of vr_terrain_path.  The map with the path in it must equal the numpy float32 model (tests/path_model.py) in every byte -
no tolerance anywhere: vr_path.h's arithmetic is IEEE fp32 in a fixed order, and a texel is a pure function of its own byte, its
coordinates and the call, so neither the rectangle nor the tile nor the device's order of segments may show.  Scenes and helpers are
those of tests/test_terrain_noise_gpu.py; the calls are tests/path_cases.py's, whose preconditions are asserted on the model's output
(and, without a device, in tests/test_path_model_cpu.py)."""
import numpy as np
import pytest

import vrenderer_amd as vr
from tests import brush_model as bm
from tests import erode_model as em
from tests import noise_cases as nc
from tests import path_cases as pc
from tests import path_model as pm
from tests import test_gbuffer_lazy_gpu as gl
from tests import test_terrain_edit_gpu as te
from tests.common import params
from tests.fusion_common import PLANES, assert_same_frame, terrain_fixture
from tests.test_terrain_brush_gpu import assert_bytes, five_dabs, level0, world_of
from tests.test_terrain_texture_gpu import ExtraScene

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scenes(gpu_ctx):
    out = {n: (te.Scene if n in te.SCENES else ExtraScene)(gpu_ctx, n) for n in pc.SCENES}
    for n, sc in out.items():
        assert world_of(sc) == pc.WORLD[n]
    return out


def apply(tp, which, pts, p):
    """One vr_terrain_path with the parameters of tests/path_model.params."""
    return tp.Path(which, pts, p["radius"], hardness=p["hardness"], opacity=p["opacity"], op=p["op"], color=p["color"], channels=p["channel_mask"], closed=p["closed"])


_MODEL = {}


def model(texels, pts, p, world):
    """The model's (texels, rect, detail) of one call, computed once per distinct call."""
    key = (texels.tobytes(), texels.shape, np.asarray(pts, np.float32).tobytes(), repr(sorted(p.items())), world)
    if key not in _MODEL:
        _MODEL[key] = pc.run_model(texels, pts, p, world)
    return _MODEL[key]


def _height_op(sc, op):
    name, S = sc.name, world_of(sc)
    pts, p = pc.height_case(name, sc.hm, op)
    want, want_rect, detail = model(sc.hm, pts, p, S)
    what = f"{name}, {pc.OP_IDS[op]}"
    print(what, pc.check_preconditions(sc.hm, want, p, detail, what))
    a = sc.terrain(sc.hm, sc.al, cast=False, render=False)
    rect = apply(a, "height", pts, p)
    assert rect == tuple(want_rect), (rect, want_rect)
    assert_bytes(level0(a, "height"), want, what)
    assert_bytes(level0(a, "albedo"), sc.al, f"{what}: the albedo")
    b = sc.terrain(want, sc.al, cast=False, render=False)
    te._assert_tables_equal(a, b, what)
    a.close(); b.close()


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
    S = world_of(sc)
    pts, p = pc.albedo_case(name, sc.al)
    want, want_rect, detail = model(sc.al, pts, p, S)
    print(name, pc.check_preconditions(sc.al, want, p, detail, f"{name}, paint"))
    assert np.array_equal(want[..., 1], sc.al[..., 1]) and np.array_equal(want[..., 3], sc.al[..., 3])
    a = sc.terrain(sc.hm, sc.al, cast=False, render=False)
    assert apply(a, "albedo", pts, p) == tuple(want_rect)
    assert_bytes(level0(a, "albedo"), want, f"{name}, a painted path")
    assert_bytes(level0(a, "height"), sc.hm, f"{name}, a painted path: the heightmap")
    b = sc.terrain(sc.hm, want, cast=False, render=False)
    te._assert_chains_equal(a, b, f"{name}, a painted path")
    a.close(); b.close()


def test_three_hundred_segments(scenes):
    """4. A 300-segment zigzag inside one 32 x 8 tile of fast64: two chunks of the walk, more than 256 segments on that tile, and on
    the model winners from both below and above index 256 within it."""
    sc = scenes["fast64"]
    S = world_of(sc)
    pts, p = pc.zigzag(sc.hm.shape, S), pc.zigzag_params()
    want, want_rect, d = model(sc.hm, pts, p, S)
    win = d["winner"][8:16, 0:32]
    assert len(d["segments"]) == 300 and (win[win >= 0] < 256).sum() >= 20 and (win >= 256).sum() >= 20 and (want != sc.hm).sum() >= 100
    a = sc.terrain(sc.hm, sc.al, cast=False, render=False)
    assert apply(a, "height", pts, p) == tuple(want_rect)
    assert_bytes(level0(a, "height"), want, "300 segments")
    a.close()


@pytest.mark.parametrize("shape", ("closed", "single", "repeated", "leaves"))
def test_degenerate_shapes(scenes, shape):
    """5. A closed loop; n == 1; a path with a repeated point; a path that leaves the map and re-enters."""
    sc = scenes["fast64"]
    S = world_of(sc)
    pts, p = pc.degenerate_cases(sc.hm.shape, S)[shape]
    want, want_rect, _ = model(sc.hm, pts, p, S)
    assert (want != sc.hm).sum() >= 200
    a = sc.terrain(sc.hm, sc.al, cast=False, render=False)
    assert apply(a, "height", pts, p) == tuple(want_rect)
    assert_bytes(level0(a, "height"), want, shape)
    a.close()


def test_order_with_nothing_between(scenes):
    """6. A stroke, a path and an erosion queued back to back, no host wait between: the path sees the stroked map and the erosion
    the map with the path in it - the model's chain, which differs from the chain with the path left out or laid on the map before the
    stroke."""
    sc = scenes["odd"]
    S = world_of(sc)
    stroke = five_dabs(sc.hm.shape, S, bm.RAISE)
    pts, p = pc.height_case("odd", sc.hm, pm.LEVEL)
    mask = nc.five_dabs(sc.hm.shape, S)
    brushed, _ = bm.stroke(sc.hm, bm.RAISE, stroke, S)
    pathed, path_rect, _ = model(brushed, pts, p, S)
    want, erode_rect = em.erode(pathed, mask, S, 20, 0.5, 0.125)
    stale = model(sc.hm, pts, p, S)[0]
    assert (stale != pathed).sum() >= 30 and (em.erode(brushed, mask, S, 20, 0.5, 0.125)[0] != want).sum() >= 30 and (want != pathed).sum() >= 30
    a = sc.terrain(sc.hm, sc.al)
    a.Brush("raise", stroke)
    assert apply(a, "height", pts, p) == tuple(path_rect)
    assert a.Erode(mask, 20, 0.5, 0.125) == tuple(erode_rect)
    assert_bytes(level0(a, "height"), want, "brush, path, erode")
    assert_bytes(level0(a, "albedo"), sc.al, "brush, path, erode: the albedo")
    a.close()


def test_history(scenes):
    """7. Enable, path, commit, undo: the original bytes; redo: the model's.  One call is one record, and two calls before one commit
    are one step."""
    sc = scenes["odd"]
    S = world_of(sc)
    pts, p = pc.height_case("odd", sc.hm, pm.FILL)
    want = model(sc.hm, pts, p, S)[0]
    assert (want != sc.hm).sum() >= 200
    a = sc.terrain(sc.hm, sc.al, cast=False, render=False)
    a.EnableHistory(1 << 20)
    apply(a, "height", pts, p)
    assert a.HistoryStatus()["open_records"] == 1
    a.CommitHistory()
    st = a.HistoryStatus()
    assert (st["undo_steps"], st["redo_steps"], st["open_records"]) == (1, 0, 0)
    assert_bytes(level0(a, "height"), want, "with the path")
    assert a.Undo()
    assert_bytes(level0(a, "height"), sc.hm, "undone")
    assert a.Redo() and not a.Redo()
    assert_bytes(level0(a, "height"), want, "redone")
    assert_bytes(level0(a, "albedo"), sc.al, "the albedo")
    a.close()
    p2 = dict(p, op=pm.CUT, radius=float(np.float32(0.5 * p["radius"])))
    second = model(want, pts[::-1], p2, S)[0]
    assert (second != want).sum() >= 30
    a = sc.terrain(sc.hm, sc.al, cast=False, render=False)
    a.EnableHistory(1 << 20)
    apply(a, "height", pts, p)
    apply(a, "height", pts[::-1], p2)
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
    """8. n == 0, a path beside the map, and calls refused on a real terrain (PAINT on the heightmap; a closed path of two points):
    every byte and the history's status stay as they were.  Then a good call still gives the model's bytes."""
    sc = scenes["odd"]
    S = world_of(sc)
    pts, p = pc.height_case("odd", sc.hm, pm.LEVEL)
    a = sc.terrain(sc.hm, sc.al, cast=False, render=False)
    a.EnableHistory(1 << 20)
    before = a.HistoryStatus()
    beside = np.float32([pc.point(sc.hm.shape, S, -40.0, 5.0, 10.0), pc.point(sc.hm.shape, S, -30.0, 60.0, 90.0), pc.point(sc.hm.shape, S, 20.0, 90.0, 90.0)])
    assert model(sc.hm, beside, p, S)[1] == (0, 0, 0, 0)
    assert apply(a, "height", beside, p) == (0, 0, 0, 0)
    assert apply(a, "height", np.zeros((0, 3), np.float32), p) == (0, 0, 0, 0)
    for bad_pts, bad in ((pts, dict(p, op=pm.PAINT)), (pts[:2], dict(p, closed=True))):
        with pytest.raises(Exception) as e:
            apply(a, "height", bad_pts, bad)
        assert "vr_terrain_path" in str(e.value), e.value
    assert_bytes(level0(a, "height"), sc.hm, "after calls that launch nothing")
    assert_bytes(level0(a, "albedo"), sc.al, "after calls that launch nothing: the albedo")
    assert a.HistoryStatus() == before
    want, want_rect, _ = model(sc.hm, pts, p, S)
    assert apply(a, "height", pts, p) == tuple(want_rect)
    assert_bytes(level0(a, "height"), want, "after a good call")
    a.close()


def test_a_path_with_a_lazily_fused_frame_pending():
    """9. A fused frame that left its colour planes to their first reader, then Path, then a G-buffer download: the planes are those
    of the eager path (VR_OPT_GBUFFER_LAZY off) - the frame on the terrain as it was; the next frame shows the path, and is the frame
    of a terrain created from the model's map."""
    w, h = 96, 64
    with terrain_fixture(256) as fx:
        v = gl._views(w, h)
        hm = fx["h"]
        pts = np.float32([pc.point(hm.shape, 256.0, fx_ * 256, fy * 256, hh) for fx_, fy, hh in
                          ((0.05, 0.1, 250.0), (0.5, 0.35, 20.0), (0.3, 0.7, 240.0), (0.9, 0.55, 10.0), (0.6, 0.95, 200.0))])
        p = pm.params(40.0, hardness=0.3, opacity=1.0, op=pm.LEVEL)
        want_map, _ = pm.path(hm, pts, p, 256.0)
        assert (want_map != hm).sum() >= hm.size // 4

        def script(scn, lazy):
            out = {}
            try:
                scn.submit(v[1])
                apply(scn.tp, "height", pts, p)
                out["before the path"] = gl._capture(scn.rt, scn.hdr)
                scn.submit(v[1])
                out["after the path"] = gl._capture(scn.rt, scn.hdr)
            finally:
                scn.tp.Edit("height", 0, 0, hm)
            return out
        want, _ = gl._both(fx, w, h, script)
        assert not np.array_equal(want["before the path"]["normals"], want["after the path"]["normals"]), "the path is not in view"
        tb = vr.TerrainPass(fx["ctx"], params(256)).Init(want_map, vr.synth_albedo(fx["ctx"], 256, hm))
        scn = gl.Scene(dict(ctx=fx["ctx"], tp=tb), 1, w, h)
        try:
            scn.submit(v[1])
            assert_same_frame(want["after the path"], gl._capture(scn.rt, scn.hdr), "the frame of a terrain created from the model's map", PLANES + ("hdr",))
        finally:
            scn.close()
            tb.close()
