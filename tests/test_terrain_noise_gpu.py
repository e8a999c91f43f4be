"""GPU tests of vr_terrain_noise.  The noised map must equal the numpy float32 / uint32 model (tests/noise_model.py) in every byte - no
tolerance anywhere: vr_noise.h's arithmetic is IEEE fp32 and uint32 in a fixed order, and a texel is a pure function of its own byte,
its coordinates, the parameters and its mask, so neither the rectangle nor the tile may show.  Scenes and helpers are those of
tests/test_terrain_edit_gpu.py and tests/test_terrain_brush_gpu.py, with tests/texture_cases.py's "wide"; the calls are
tests/noise_cases.py's, whose preconditions are asserted on the model's output (and, without a device, in
tests/test_noise_model_cpu.py)."""
import numpy as np
import pytest

import vrenderer_amd as vr
from tests import brush_model as bm
from tests import erode_model as em
from tests import noise_cases as nc
from tests import noise_model as nm
from tests import test_gbuffer_lazy_gpu as gl
from tests import test_terrain_edit_gpu as te
from tests.common import params
from tests.fusion_common import PLANES, assert_same_frame, terrain_fixture
from tests.test_terrain_brush_gpu import assert_bytes, five_dabs, level0, order_dabs, world_of
from tests.test_terrain_texture_gpu import ExtraScene

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scenes(gpu_ctx):
    out = {n: (te.Scene if n in te.SCENES else ExtraScene)(gpu_ctx, n) for n in nc.SCENES}
    for n, sc in out.items():
        assert world_of(sc) == nc.WORLD[n]
    return out


def apply(tp, which, p, dabs=None, whole_map=False):
    """One vr_terrain_noise with the parameters of tests/noise_model.params."""
    return tp.Noise(which, p["frequency"], p["amplitude"], octaves=p["octaves"], lacunarity=p["lacunarity"], gain=p["gain"], offset=(p["offset_x"], p["offset_z"]),
                    seed=p["seed"], basis=p["basis"], fractal=p["fractal"], op=p["op"], base=p["base"], channels=p["channel_mask"], dabs=dabs, whole_map=whole_map)


_MODEL = {}


def model(name, texels, p, world, dabs=None, whole_map=False):
    """The model's (texels, rect, detail) of one call, computed once per distinct call."""
    key = (name, texels.tobytes(), repr(sorted(p.items())), None if dabs is None else np.asarray(dabs, np.float32).tobytes(), whole_map)
    if key not in _MODEL:
        _MODEL[key] = nc.run_model(texels, p, world, dabs=dabs, whole_map=whole_map)
    return _MODEL[key]


def _under_five_dabs(sc, basis, fractal):
    name, S = sc.name, world_of(sc)
    p = nc.height_params(name, basis, fractal)
    dabs = nc.five_dabs(sc.hm.shape, S)
    want, want_rect, detail = model(name, sc.hm, p, S, dabs=dabs)
    what = f"{name}, {basis}-{fractal} under five dabs"
    print(what, nc.check_preconditions(sc.hm, want, p, detail, what))
    a = sc.terrain(sc.hm, sc.al, cast=False, render=False)
    rect = apply(a, "height", p, dabs)
    assert rect == tuple(want_rect), (rect, want_rect)
    assert_bytes(level0(a, "height"), want, what)
    assert_bytes(level0(a, "albedo"), sc.al, f"{what}: the albedo")
    b = sc.terrain(want, sc.al, cast=False, render=False)
    te._assert_tables_equal(a, b, what)
    a.close(); b.close()


@pytest.mark.parametrize("combo", nc.COMBOS, ids=nc.COMBO_IDS)
def test_every_basis_and_fractal_under_five_dabs(scenes, combo):
    """1. The heightmap of fast64 under five dabs, ADD, each basis x fractal: level 0 equals the model in every byte, the rectangle is
    the model's, the albedo is untouched, and the decoded tables are those of a terrain created from the model's map."""
    _under_five_dabs(scenes["fast64"], *combo)


@pytest.mark.parametrize("name", [n for n in nc.SCENES if n != "fast64"])
def test_the_other_scenes_under_five_dabs(scenes, name):
    """1, the rest: one basis x fractal on each other scene - odd sizes, the 2 x 2-surface world, the 512x32 map."""
    _under_five_dabs(scenes[name], *nc.scene_combo(name))


@pytest.mark.parametrize("name", nc.SCENES)
def test_the_whole_map(scenes, name):
    """2. VR_NOISE_WHOLE_MAP, BLEND, 12 octaves: every byte equals the model, the rectangle is the map, and every mip level is that of a
    terrain created from the result.  One kernel serves every map (the four-texel variant of DESIGN.md 4z was measured and not
    kept), so the 67-texel rows of `odd` and the rows that are a multiple of four run the same code."""
    sc = scenes[name]
    S, p = world_of(sc), nc.whole_params(name)
    want, want_rect, detail = model(name, sc.hm, p, S, whole_map=True)
    print(name, nc.check_preconditions(sc.hm, want, p, detail, name, masked=False))
    a = sc.terrain(sc.hm, sc.al, cast=False, render=False)
    rect = apply(a, "height", p, whole_map=True)
    assert rect == tuple(want_rect) == (0, 0, sc.hm.shape[1], sc.hm.shape[0]), (rect, want_rect)
    assert_bytes(level0(a, "height"), want, f"{name}, noise over the whole map")
    assert_bytes(level0(a, "albedo"), sc.al, f"{name}, noise: the albedo")
    b = sc.terrain(want, sc.al, cast=False, render=False)
    te._assert_chains_equal(a, b, f"{name}, noise over the whole map")
    te._assert_tables_equal(a, b, f"{name}, noise over the whole map")
    a.close(); b.close()


@pytest.mark.parametrize("name", nc.SCENES)
def test_the_albedo(scenes, name):
    """3. The albedo under five dabs with channel_mask 5: channels 0 and 2 equal the model, channels 1 and 3 and the heightmap are
    untouched."""
    sc = scenes[name]
    S, p = world_of(sc), nc.albedo_params(name)
    dabs = nc.five_dabs(sc.al.shape, S)
    want, want_rect, detail = model(name, sc.al, p, S, dabs=dabs)
    print(name, nc.check_preconditions(sc.al, want, p, detail, f"{name}, albedo"))
    assert np.array_equal(want[..., 1], sc.al[..., 1]) and np.array_equal(want[..., 3], sc.al[..., 3])
    a = sc.terrain(sc.hm, sc.al, cast=False, render=False)
    assert apply(a, "albedo", p, dabs) == tuple(want_rect)
    assert_bytes(level0(a, "albedo"), want, f"{name}, noise on the albedo")
    assert_bytes(level0(a, "height"), sc.hm, f"{name}, noise on the albedo: the heightmap")
    b = sc.terrain(sc.hm, want, cast=False, render=False)
    te._assert_chains_equal(a, b, f"{name}, noise on the albedo")
    a.close(); b.close()


def test_three_hundred_dabs_in_either_order(scenes):
    """4. 300 dabs, which span two chunks of the walk, more than 256 of them on one tile: the model's bytes, and the same bytes from the
    reversed list - a mask texel is a maximum, which has no order."""
    sc = scenes["fast64"]
    S = world_of(sc)
    p = nc.height_params("fast64", nm.VALUE, nm.BILLOW)
    dabs = order_dabs(sc.hm.shape, S, (0.9, 0.3, 0.65, 1.0, 0.15))
    want, want_rect, detail = model("fast64", sc.hm, p, S, dabs=dabs)
    m = detail["mask"]
    assert (want != sc.hm).sum() >= 200 and ((m > 0) & (m < 1)).sum() >= 100
    assert np.array_equal(want, model("fast64", sc.hm, p, S, dabs=dabs[::-1])[0])
    got = []
    for rows in (dabs, dabs[::-1]):
        a = sc.terrain(sc.hm, sc.al, cast=False, render=False)
        assert apply(a, "height", p, np.ascontiguousarray(rows)) == tuple(want_rect)
        got.append(level0(a, "height"))
        a.close()
    assert_bytes(got[0], want, "300 dabs")
    assert_bytes(got[1], got[0], "300 dabs reversed")


def test_order_with_nothing_between(scenes):
    """5. A stroke, a noise call and an erosion queued back to back, no host wait between: the noise sees the stroked map and the
    erosion the noised one - the model's chain, which differs from the chain with the noise left out or applied to the map before the
    stroke."""
    sc = scenes["odd"]
    S = world_of(sc)
    stroke = five_dabs(sc.hm.shape, S, bm.RAISE)
    p = nc.height_params("odd", nm.GRADIENT, nm.FBM, op=nm.BLEND)
    mask = nc.five_dabs(sc.hm.shape, S)
    brushed, _ = bm.stroke(sc.hm, bm.RAISE, stroke, S)
    noised, noise_rect, _ = model("odd", brushed, p, S, dabs=mask)
    want, erode_rect = em.erode(noised, mask, S, 20, 0.5, 0.125)
    stale = model("odd", sc.hm, p, S, dabs=mask)[0]
    assert (stale != noised).sum() >= 30 and (em.erode(brushed, mask, S, 20, 0.5, 0.125)[0] != want).sum() >= 30 and (want != noised).sum() >= 30
    a = sc.terrain(sc.hm, sc.al)
    a.Brush("raise", stroke)
    assert apply(a, "height", p, mask) == tuple(noise_rect)
    assert a.Erode(mask, 20, 0.5, 0.125) == tuple(erode_rect)
    assert_bytes(level0(a, "height"), want, "brush, noise, erode")
    assert_bytes(level0(a, "albedo"), sc.al, "brush, noise, erode: the albedo")
    a.close()


def test_history(scenes):
    """6. Enable, noise, commit, undo: the original bytes; redo: the model's.  One call is one record - under dabs and over the whole
    map - and two calls before one commit are one step."""
    sc = scenes["odd"]
    S = world_of(sc)
    dabs = nc.five_dabs(sc.hm.shape, S)
    for p, kw in ((nc.height_params("odd", nm.VALUE, nm.RIDGED), dict(dabs=dabs)), (nc.whole_params("odd"), dict(whole_map=True))):
        want = model("odd", sc.hm, p, S, **kw)[0]
        assert (want != sc.hm).sum() >= 200
        a = sc.terrain(sc.hm, sc.al, cast=False, render=False)
        a.EnableHistory(1 << 20)
        apply(a, "height", p, **kw)
        assert a.HistoryStatus()["open_records"] == 1
        a.CommitHistory()
        st = a.HistoryStatus()
        assert (st["undo_steps"], st["redo_steps"], st["open_records"]) == (1, 0, 0)
        assert_bytes(level0(a, "height"), want, "noised")
        assert a.Undo()
        assert_bytes(level0(a, "height"), sc.hm, "undone")
        assert a.Redo() and not a.Redo()
        assert_bytes(level0(a, "height"), want, "redone")
        assert_bytes(level0(a, "albedo"), sc.al, "the albedo")
        a.close()
    p1, p2 = nc.height_params("odd", nm.VALUE, nm.RIDGED), nc.whole_params("odd")
    first = model("odd", sc.hm, p1, S, dabs=dabs)[0]
    second = model("odd", first, p2, S, whole_map=True)[0]
    a = sc.terrain(sc.hm, sc.al, cast=False, render=False)
    a.EnableHistory(1 << 20)
    apply(a, "height", p1, dabs)
    apply(a, "height", p2, whole_map=True)
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
    """7. n == 0, dabs that all miss the map, and a call refused on a real terrain (a lattice coordinate beyond 2^22 on this map; an
    unknown basis): every byte and the history's status stay as they were.  Then a good call still gives the model's bytes."""
    sc = scenes["odd"]
    S = world_of(sc)
    p = nc.height_params("odd", nm.GRADIENT, nm.RIDGED)
    a = sc.terrain(sc.hm, sc.al, cast=False, render=False)
    a.EnableHistory(1 << 20)
    before = a.HistoryStatus()
    miss = np.float32([nc.dab(sc.hm.shape, S, -40.0, 5.0, 3.0, 0.0, 1.0), nc.dab(sc.hm.shape, S, 10.5, 12.5, 0.2, 0.0, 1.0)])
    assert nc.model(sc.hm, p, S, dabs=miss)[1] == (0, 0, 0, 0)
    assert apply(a, "height", p, miss) == (0, 0, 0, 0)
    assert apply(a, "height", p, np.zeros((0, 5), np.float32)) == (0, 0, 0, 0)
    far = dict(p, frequency=float(np.float32(3.0e5)))
    assert not nm.in_range(nm.prepare(far, S, sc.hm.shape[1], sc.hm.shape[0]), sc.hm.shape[1], sc.hm.shape[0])
    for bad, kw in ((far, dict(dabs=nc.five_dabs(sc.hm.shape, S))), (far, dict(whole_map=True)), (dict(p, basis=2), dict(whole_map=True))):
        with pytest.raises(Exception) as e:
            apply(a, "height", bad, **kw)
        assert "vr_terrain_noise" in str(e.value), e.value
    assert_bytes(level0(a, "height"), sc.hm, "after calls that launch nothing")
    assert_bytes(level0(a, "albedo"), sc.al, "after calls that launch nothing: the albedo")
    assert a.HistoryStatus() == before
    want, want_rect, _ = model("odd", sc.hm, p, S, whole_map=True)
    assert apply(a, "height", p, whole_map=True) == tuple(want_rect)
    assert_bytes(level0(a, "height"), want, "after a good call")
    a.close()


def test_a_noise_call_with_a_lazily_fused_frame_pending():
    """8. A fused frame that left its colour planes to their first reader, then Noise, then a G-buffer download: the planes are those
    of the eager path (VR_OPT_GBUFFER_LAZY off) - the frame on the terrain as it was; the next frame shows the noise, and is the frame
    of a terrain created from the model's map."""
    w, h = 96, 64
    with terrain_fixture(256) as fx:
        v = gl._views(w, h)
        hm = fx["h"]
        p = nm.params(1.0 / 40.0, 160.0, octaves=5, offset=(11.0, -6.0), seed=4, basis=nm.GRADIENT, fractal=nm.RIDGED, op=nm.BLEND, base=90.0)
        want_map, _ = nm.noise(hm, p, 256.0, whole_map=True)
        assert (want_map != hm).sum() >= hm.size // 2

        def script(scn, lazy):
            out = {}
            try:
                scn.submit(v[1])
                apply(scn.tp, "height", p, whole_map=True)
                out["before the noise"] = gl._capture(scn.rt, scn.hdr)
                scn.submit(v[1])
                out["after the noise"] = gl._capture(scn.rt, scn.hdr)
            finally:
                scn.tp.Edit("height", 0, 0, hm)
            return out
        want, _ = gl._both(fx, w, h, script)
        assert not np.array_equal(want["before the noise"]["normals"], want["after the noise"]["normals"]), "the noise is not in view"
        tb = vr.TerrainPass(fx["ctx"], params(256)).Init(want_map, vr.synth_albedo(fx["ctx"], 256, hm))
        scn = gl.Scene(dict(ctx=fx["ctx"], tp=tb), 1, w, h)
        try:
            scn.submit(v[1])
            assert_same_frame(want["after the noise"], gl._capture(scn.rt, scn.hdr), "the frame of a terrain created from the model's map", PLANES + ("hdr",))
        finally:
            scn.close()
            tb.close()
