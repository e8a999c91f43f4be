"""GPU tests of vr_terrain_noise.  The noised map must equal the numpy float32 / uint32 model (tests/noise_model.py) in every byte - no
tolerance anywhere: vr_noise.h's arithmetic is IEEE fp32 and uint32 in a fixed order, and a texel is a pure function of its own byte,
its coordinates, the parameters and its mask, so neither the rectangle nor the tile may show.  Scenes and test bodies are those of
tests/level0_common.py, with tests/texture_cases.py's "wide"; the calls (p, dabs, whole_map) are tests/noise_cases.py's, whose
preconditions are asserted on the model's output (and, without a device, in tests/test_noise_model_cpu.py)."""
import numpy as np
import pytest

from tests import level0_common as lc
from tests import noise_cases as nc
from tests import noise_model as nm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scenes(gpu_ctx):
    return lc.make_scenes(gpu_ctx, nc.SCENES, nc.WORLD)


def apply(tp, which, call):
    """One vr_terrain_noise with the parameters of tests/noise_model.params."""
    p, dabs, whole_map = call
    return tp.Noise(which, p["frequency"], p["amplitude"], octaves=p["octaves"], lacunarity=p["lacunarity"], gain=p["gain"], offset=(p["offset_x"], p["offset_z"]),
                    seed=p["seed"], basis=p["basis"], fractal=p["fractal"], op=p["op"], base=p["base"], channels=p["channel_mask"], dabs=dabs, whole_map=whole_map)


NOISE = lc.Level0Op("vr_terrain_noise", apply, lambda texels, call, world: nc.run_model(texels, call[0], world, dabs=call[1], whole_map=call[2]))


def preconditions(call, **kw):
    return lambda before, want, detail, what: nc.check_preconditions(before, want, call[0], detail, what, **kw)


def _under_five_dabs(sc, basis, fractal):
    call = (nc.height_params(sc.name, basis, fractal), nc.five_dabs(sc.hm.shape, lc.world_of(sc)), False)
    lc.check_height_call(sc, NOISE, call, f"{sc.name}, {basis}-{fractal} under five dabs", preconditions(call))


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
    call = (nc.whole_params(name), None, True)
    want, want_rect, detail = NOISE.model(sc.hm, call, lc.world_of(sc))
    print(name, nc.check_preconditions(sc.hm, want, call[0], detail, name, masked=False))
    a = sc.terrain(sc.hm, sc.al, cast=False, render=False)
    rect = apply(a, "height", call)
    assert rect == tuple(want_rect) == (0, 0, sc.hm.shape[1], sc.hm.shape[0]), (rect, want_rect)
    lc.assert_bytes(lc.level0(a, "height"), want, f"{name}, noise over the whole map")
    lc.assert_bytes(lc.level0(a, "albedo"), sc.al, f"{name}, noise: the albedo")
    b = sc.terrain(want, sc.al, cast=False, render=False)
    lc.assert_chains_equal(a, b, f"{name}, noise over the whole map")
    lc.assert_tables_equal(a, b, f"{name}, noise over the whole map")
    a.close(); b.close()


@pytest.mark.parametrize("name", nc.SCENES)
def test_the_albedo(scenes, name):
    """3. The albedo under five dabs with channel_mask 5: channels 0 and 2 equal the model, channels 1 and 3 and the heightmap are
    untouched."""
    sc = scenes[name]
    call = (nc.albedo_params(name), nc.five_dabs(sc.al.shape, lc.world_of(sc)), False)
    lc.check_albedo_call(sc, NOISE, call, f"{name}, noise on the albedo", preconditions(call))


def test_three_hundred_dabs_in_either_order(scenes):
    """4. 300 dabs, which span two chunks of the walk, more than 256 of them on one tile: the model's bytes, and the same bytes from the
    reversed list - a mask texel is a maximum, which has no order."""
    sc = scenes["fast64"]
    S = lc.world_of(sc)
    p = nc.height_params("fast64", nm.VALUE, nm.BILLOW)
    dabs = lc.order_dabs(sc.hm.shape, S, (0.9, 0.3, 0.65, 1.0, 0.15))
    want, want_rect, detail = NOISE.model(sc.hm, (p, dabs, False), S)
    m = detail["mask"]
    assert (want != sc.hm).sum() >= 200 and ((m > 0) & (m < 1)).sum() >= 100
    assert np.array_equal(want, NOISE.model(sc.hm, (p, dabs[::-1], False), S)[0])
    got = []
    for rows in (dabs, dabs[::-1]):
        a = sc.terrain(sc.hm, sc.al, cast=False, render=False)
        assert apply(a, "height", (p, np.ascontiguousarray(rows), False)) == tuple(want_rect)
        got.append(lc.level0(a, "height"))
        a.close()
    lc.assert_bytes(got[0], want, "300 dabs")
    lc.assert_bytes(got[1], got[0], "300 dabs reversed")


def test_order_with_nothing_between(scenes):
    """5. A stroke, a noise call and an erosion queued back to back, no host wait between: the noise sees the stroked map and the
    erosion the noised one - the model's chain, which differs from the chain with the noise left out or applied to the map before the
    stroke."""
    sc = scenes["odd"]
    call = (nc.height_params("odd", nm.GRADIENT, nm.FBM, op=nm.BLEND), nc.five_dabs(sc.hm.shape, lc.world_of(sc)), False)
    lc.check_order_with_nothing_between(sc, NOISE, call, "noise")


def test_history(scenes):
    """6. Enable, noise, commit, undo: the original bytes; redo: the model's.  One call is one record - under dabs and over the whole
    map - and two calls before one commit are one step."""
    sc = scenes["odd"]
    under_dabs = (nc.height_params("odd", nm.VALUE, nm.RIDGED), nc.five_dabs(sc.hm.shape, lc.world_of(sc)), False)
    whole = (nc.whole_params("odd"), None, True)
    lc.check_history(sc, NOISE, [under_dabs, whole], under_dabs, whole)


def test_calls_that_launch_nothing(scenes):
    """7. n == 0, dabs that all miss the map, and a call refused on a real terrain (a lattice coordinate beyond 2^22 on this map; an
    unknown basis): every byte and the history's status stay as they were.  Then a good call still gives the model's bytes."""
    sc = scenes["odd"]
    S = lc.world_of(sc)
    p = nc.height_params("odd", nm.GRADIENT, nm.RIDGED)
    miss = np.float32([nc.dab(sc.hm.shape, S, -40.0, 5.0, 3.0, 0.0, 1.0), nc.dab(sc.hm.shape, S, 10.5, 12.5, 0.2, 0.0, 1.0)])
    far = dict(p, frequency=float(np.float32(3.0e5)))
    assert not nm.in_range(nm.prepare(far, S, sc.hm.shape[1], sc.hm.shape[0]), sc.hm.shape[1], sc.hm.shape[0])
    lc.check_calls_that_launch_nothing(sc, NOISE, (p, None, True), misses=[(p, miss, False), (p, np.zeros((0, 5), np.float32), False)],
                                       refused=[(far, nc.five_dabs(sc.hm.shape, S), False), (far, None, True), (dict(p, basis=2), None, True)])


def test_a_noise_call_with_a_lazily_fused_frame_pending():
    """8. A fused frame that left its colour planes to their first reader, then Noise, then a G-buffer download: the planes are those
    of the eager path (VR_OPT_GBUFFER_LAZY off) - the frame on the terrain as it was; the next frame shows the noise, and is the frame
    of a terrain created from the model's map."""
    p = nm.params(1.0 / 40.0, 160.0, octaves=5, offset=(11.0, -6.0), seed=4, basis=nm.GRADIENT, fractal=nm.RIDGED, op=nm.BLEND, base=90.0)
    lc.check_with_a_lazily_fused_frame_pending(NOISE, (p, None, True), lambda hm: nm.noise(hm, p, 256.0, whole_map=True)[0], "noise", min_changed=256 * 256 // 2)
