"""GPU tests of vr_deferred_light_tiled_ex: the tiled lighting pass for every light type, with the sun's shadow term.

The 256 world in a 256x144 frame: 2x2 macro tiles with a 16-row partial bottom tile, 8x5 light tiles, a 256^2 shadow map.
Every tolerance is one the suite already asserts for the same quantity (test_gpu_parity.py): per-channel RMS <= 1e-4 and
max error <= 2e-3 * max(1, max reference) against the fp32 oracle, RMS <= 1e-5 between the tiled and the streaming pass.
The light lists keep the frame below 1, where those bounds hold for an RGBA16F output."""
import ctypes as C

import numpy as np
import pytest

import vrenderer_amd as vr
from tests import f64_shading as fs
from tests import frontend_common as fc
from tests.common import AMBIENT_BOTTOM, AMBIENT_TOP, CAMERAS, params, scaled_camera
from vrenderer_amd.passes import frame_detile, partition_info

pytestmark = pytest.mark.gpu

W, H, SIZE = 256, 144, 256
TILES_X, TILES_Y = 8, 5
PLANES = ("depth", "diffuse", "specular", "normals", "emissive")
BLACK = (0.0, 0.0, 0.0)


def _world_positions(view, depth):
    """World position of every pixel centre (float64), as ReconstructWorldPosition gives it."""
    m = np.array(view.clip_to_world[:], np.float64).reshape(4, 4)
    ys, xs = np.mgrid[0:H, 0:W]
    cx, cy = (xs + 0.5) * (2.0 / W) - 1.0, 1.0 - (ys + 0.5) * (2.0 / H)
    e = cx[..., None] * m[0] + cy[..., None] * m[1] + depth.astype(np.float64)[..., None] * m[2] + m[3]
    return e[..., :3] / e[..., 3:4]


def _all_type_lights(wp, covered, n, seed):
    """The all-type list of the float64 tests (f64_shading.all_type_lights says how it is built and why every light stays 5
    units from the surface)."""
    return fs.all_type_lights(vr, wp, covered, n, seed)


@pytest.fixture(scope="module")
def st(oracle, gpu_ctx):
    """The scene, its G-buffer on both sides, the shadow map and the oracle's frames - computed once, never changed."""
    h = oracle.synth_heightmap(SIZE)
    a = oracle.synth_albedo(SIZE, h)
    tp = vr.TerrainPass(gpu_ctx, params(SIZE)).Init(h, a)
    v = vr.make_view(*scaled_camera(CAMERAS[7], SIZE), W, H)        # terrain and sky: 31 of the 40 light tiles are covered
    rt = vr.RenderTargets(gpu_ctx).Init(W, H)
    tp.Render(v, v, rt, vr.default_render_params(400.0))
    gb = oracle.GBufferHost(W, H)
    for name in PLANES:
        getattr(gb, name)[...] = rt.download(name).reshape(getattr(gb, name).shape)
    sm = vr.CascadedShadowMap(gpu_ctx, vr.default_shadow_params(float(SIZE), resolution=256))
    lv = fc.light_view_of(lambda light, cam, p: sm.SetupForPlanarViewStable(light, cam), SIZE)
    sm.Clear()
    sm.RenderTerrain(tp)                                # the depth-only pass (bit-exact against the oracle elsewhere)
    sdepth = sm.download_depth()
    assert sdepth.shape == (256, 256) and (sdepth < 1.0).any()
    covered = gb.depth < 1.0
    assert 0.5 < covered.mean() < 0.8
    wp = _world_positions(v, gb.depth)
    lights = _all_type_lights(wp, covered, 40, 20261019)
    s = dict(tp=tp, v=v, rt=rt, gb=gb, sm=sm, lv=lv, sdepth=sdepth, covered=covered, wp=wp, lights=lights, cache={})
    yield s
    for o in (sm, rt, tp):
        o.close()


def _oracle(st, oracle, key, lights, shadow_bias=None, ambient=(AMBIENT_TOP, AMBIENT_BOTTOM)):
    if key not in st["cache"]:
        shadow = None if shadow_bias is None else (st["lv"], st["sdepth"], 0, shadow_bias)
        st["cache"][key] = oracle.deferred(st["v"], st["gb"], lights, ambient[0], ambient[1], f32=True, shadow=shadow)
        st["cache"][key].setflags(write=False)
    return st["cache"][key]


def _render_ex(st, gpu_ctx, lights, bias=None, part=None, out=None, ambient=(AMBIENT_TOP, AMBIENT_BOTTOM), rt=None):
    hdr = out or vr.HdrImage(gpu_ctx, W, H)
    if bias is not None:
        st["sm"].params.depth_bias = bias
    vr.TiledDeferredLightingPass(gpu_ctx).Render(st["v"], rt or st["rt"], lights, ambient[0], ambient[1], hdr, part, all_light_types=True,
                                                 shadow_map=st["sm"] if bias is not None else None)
    if out is not None:
        return None
    got = hdr.download()
    hdr.close()
    return got


def _assert_close(oracle, got_u16, ref32, what):
    got = oracle.half_to_float(got_u16).astype(np.float64)
    rms = [float(np.sqrt(np.mean((got[..., c] - ref32[..., c]) ** 2))) for c in range(3)]
    mx = float(np.abs(got[..., :3] - ref32[..., :3]).max())
    bound = 2e-3 * max(1.0, float(ref32.max()))
    print(f"{what}: per-channel RMS {rms}, max error {mx:.3e} (bound {bound:.3e}), reference max {float(ref32.max()):.3f}")
    assert max(rms) <= 1e-4, (what, rms)
    assert mx <= bound, (what, mx, bound)


def _lists(gpu_ctx):
    t = vr.TiledDeferredLightingPass(gpu_ctx)
    return {(x, y): set(t.tile_light_list(x, y).tolist()) for y in range(TILES_Y) for x in range(TILES_X)}


def test_every_light_type_matches_the_oracle(st, oracle, gpu_ctx):
    lights = st["lights"]
    kinds = {(l.type, l.radius > 0, l.angular_size_or_inv_range > 0) for l in lights[1:]}
    assert len(lights) == 40 and len(kinds) >= 5
    ref = _oracle(st, oracle, "all", lights)
    plain = _oracle(st, oracle, "plain", lights[:2])
    assert np.abs(ref - plain).max() > 1e-3, "the spot and spherical lights must contribute for the test to mean anything"
    _assert_close(oracle, _render_ex(st, gpu_ctx, lights), ref, "40 lights of all types")
    vr.TiledDeferredLightingPass(gpu_ctx).Status()


@pytest.mark.parametrize("bias", [0.0, 1e-3])
def test_every_light_type_under_the_suns_shadow_matches_the_oracle(st, oracle, gpu_ctx, bias):
    lights = st["lights"]
    ref = _oracle(st, oracle, ("shadow", bias), lights, shadow_bias=bias)
    unshadowed = _oracle(st, oracle, "all", lights)
    assert np.abs(ref - unshadowed).max() > 1e-3, "the frame has no shadowed pixels"
    _assert_close(oracle, _render_ex(st, gpu_ctx, lights, bias=bias), ref, f"40 lights, shadow bias {bias}")
    # the binding's conditions are those of vr_deferred_light_shadowed: the light must be directional
    hdr = vr.HdrImage(gpu_ctx, W, H)
    with pytest.raises(vr.VrError):
        vr.TiledDeferredLightingPass(gpu_ctx).Render(st["v"], st["rt"], lights, AMBIENT_TOP, AMBIENT_BOTTOM, hdr, shadow_map=st["sm"],
                                                     shadow_light_index=1)
    hdr.close()


def test_agrees_with_the_streaming_pass_on_sixteen_lights(st, oracle, gpu_ctx):
    lights = st["lights"][:16]
    a = oracle.half_to_float(_render_ex(st, gpu_ctx, lights, bias=1e-3)).astype(np.float64)
    hdr = vr.HdrImage(gpu_ctx, W, H)
    vr.DeferredLightingPass(gpu_ctx).Render(st["v"], st["rt"], lights, AMBIENT_TOP, AMBIENT_BOTTOM, hdr, shadow_map=st["sm"])
    b = oracle.half_to_float(hdr.download()).astype(np.float64)
    hdr.close()
    rms = float(np.sqrt(np.mean((a - b) ** 2)))
    print(f"tiled_ex vs streaming, 16 lights with the shadow: RMS {rms:.3e}")
    assert rms <= 1e-5, rms


def test_a_light_that_reaches_a_tile_is_in_its_list(st, oracle, gpu_ctx):
    """Exact, every light and every tile: where the oracle's frame with light i alone differs from the lightless frame (ambient
    0) at any pixel of a light tile, i is in that tile's list."""
    lights = _all_type_lights(st["wp"], st["covered"], 24, 77)
    none = _oracle(st, oracle, "none", [], ambient=(BLACK, BLACK))
    _render_ex(st, gpu_ctx, lights, ambient=(BLACK, BLACK))
    lists = _lists(gpu_ctx)
    reached = 0
    for i, l in enumerate(lights):
        alone = _oracle(st, oracle, ("alone", i), [l], ambient=(BLACK, BLACK))
        differs = (alone != none).any(axis=2)
        for (x, y), members in lists.items():
            if differs[y * 32:(y + 1) * 32, x * 32:(x + 1) * 32].any():
                reached += 1
                assert i in members, f"light {i} (type {l.type}) lights tile ({x}, {y}) but is not in its list"
    assert reached > len(lights), reached
    assert any(len(m) < len(lights) for m in lists.values()), "nothing was culled: the lists say nothing"


def test_the_cone_test_drops_a_narrow_spot_from_most_tiles(st, oracle, gpu_ctx):
    ys, xs = np.nonzero(st["covered"])
    k = len(ys) // 2
    pos = st["wp"][ys[k], xs[k]] + np.array([0.0, 15.0, 0.0])
    lights = [vr.point_light(pos, 100.0, 1000.0), vr.spot_light(pos, (0.0, -1.0, 0.0), 100.0, 1000.0, 5.0, 10.0)]
    _render_ex(st, gpu_ctx, lights)
    lists = _lists(gpu_ctx)
    covered = [(x, y) for (x, y) in lists if st["covered"][y * 32:(y + 1) * 32, x * 32:(x + 1) * 32].any()]
    assert len(covered) >= 20
    assert all(0 in lists[t] for t in covered), "premise: the point light's range spans the scene"
    with_spot = [t for t in covered if 1 in lists[t]]
    print(f"spot listed in {len(with_spot)} of {len(covered)} covered tiles")
    assert 1 <= len(with_spot) < len(covered) / 2, (len(with_spot), len(covered))


def test_more_than_256_lights_in_one_tile(st, oracle, gpu_ctx):
    """300 spot and spherical lights above one spot of the terrain: a tile's list takes two staging rounds."""
    ys, xs = np.nonzero(st["covered"])
    k = len(ys) // 2
    centre = st["wp"][ys[k], xs[k]]
    rng = np.random.default_rng(300)
    lights, surface = [], st["wp"][st["covered"]]
    while len(lights) < 300:
        i = len(lights)
        pos = centre + np.array([rng.uniform(-6, 6), rng.uniform(8, 20), rng.uniform(-6, 6)])
        if np.sqrt(((surface - pos) ** 2).sum(axis=1)).min() < 5.0:          # (as in _all_type_lights)
            continue
        col = rng.uniform(0.1, 1.0, 3)
        if i % 2:
            lights.append(vr.spot_light(pos, (rng.uniform(-0.3, 0.3), -1.0, rng.uniform(-0.3, 0.3)), 1.5, 80.0, 20.0, 60.0, col,
                                        radius=1.0 if i % 4 == 1 else 0.0))
        else:
            lights.append(vr.point_light(pos, 0.6, 80.0, col, radius=rng.uniform(0.5, 2.0)))
    ref = _oracle(st, oracle, "300", lights)
    assert np.abs(ref - _oracle(st, oracle, "300 none", [])).max() > 1e-3
    got = _render_ex(st, gpu_ctx, lights)
    vr.TiledDeferredLightingPass(gpu_ctx).Status()           # no tile exceeds the cap
    longest = max(len(m) for m in _lists(gpu_ctx).values())
    assert longest > 256, longest
    _assert_close(oracle, got, ref, "300 lights over one tile")


@pytest.mark.parametrize("world", [2, 3])
def test_packed_tiles_reassemble_to_the_unsplit_frame(st, gpu_ctx, world):
    lights = st["lights"]
    full = _render_ex(st, gpu_ctx, lights, bias=1e-3)
    info = partition_info(W, H, 0, world)
    gathered = np.zeros(world * info["packed_bytes"] // 2, np.uint16)
    for r in range(world):
        packed = vr.HdrImage(gpu_ctx, 128, info["max_owned"] * 128)
        _render_ex(st, gpu_ctx, lights, bias=1e-3, part=vr.Partition(r, world), out=packed)
        gathered[r * info["packed_bytes"] // 2:(r + 1) * info["packed_bytes"] // 2] = packed.download(info["packed_bytes"])
        packed.close()
    big = vr.HdrImage(gpu_ctx, 128, world * info["max_owned"] * 128)
    big.upload(gathered)
    out = vr.HdrImage(gpu_ctx, W, H)
    frame_detile(gpu_ctx, big.device_ptr, world, out)
    got = out.download()
    big.close(); out.close()
    assert np.array_equal(got, full)


def test_frame_submit_queues_the_new_pass_for_tiled_2_and_the_old_one_for_tiled_1(st, gpu_ctx):
    tp, v, sm = st["tp"], st["v"], st["sm"]
    sm.params.depth_bias = 1e-3
    rp = vr.default_render_params(400.0, assume_cleared=1)
    rt = vr.RenderTargets(gpu_ctx).Init(W, H)
    hdr = vr.HdrImage(gpu_ctx, W, H)
    tiled = vr.TiledDeferredLightingPass(gpu_ctx)
    plain = [l for l in st["lights"] if l.type != vr.capi.VR_LIGHT_SPOT and not l.radius > 0]
    assert len(plain) >= 8

    def per_call(lights, **kw):
        tp.Render(v, v, rt, rp)
        tiled.Render(v, rt, lights, AMBIENT_TOP, AMBIENT_BOTTOM, hdr, **kw)
        return hdr.download().copy()

    def submit(lights, mode):
        vr.Frame(tp, rt, rp, lights, AMBIENT_TOP, AMBIENT_BOTTOM, tiled=mode, shadow_map=sm).submit(v, hdr)
        gpu_ctx.synchronize()
        return hdr.download().copy()

    want_all = per_call(st["lights"], shadow_map=sm)
    assert np.array_equal(submit(st["lights"], 2), want_all), "tiled = 2, every light type and the shadow"
    want_ex, want_old = per_call(plain, shadow_map=sm), per_call(plain)
    assert not np.array_equal(want_ex, want_old), "premise: the shadow changes the frame"
    assert np.array_equal(submit(plain, 2), want_ex), "tiled = 2 applies the shadow binding"
    assert np.array_equal(submit(plain, 1), want_old), "tiled = 1 ignores the shadow binding, as before"
    assert np.array_equal(submit(plain, True), want_old), "tiled = True means 1"
    hdr.close(); rt.close()


def test_plane_tracking_and_depth_ranges_do_not_change_the_frame(st, gpu_ctx):
    """Bytes are compared across the plane tracking on / off and the tile pass's depth ranges asked for / not.  Which culling
    instantiation a call took (ranges consumed, or the depth plane re-read) cannot be seen from outside - the timing ids do not
    separate them - so this shows that the settings agree, not that the ranges were used; that a fresh tile pass's ranges are
    taken is what vr_gbuffer_consume_ranges is tested for with the old entry point, which shares the call."""
    tp, v, lights = st["tp"], st["v"], st["lights"]
    rt = vr.RenderTargets(gpu_ctx).Init(W, H)
    out = {}
    try:
        for tracking in (True, False):
            gpu_ctx.set_plane_tracking(tracking)
            for ranges in (0, 1):
                rt.Clear()
                tp.Render(v, v, rt, vr.default_render_params(400.0, assume_cleared=1, depth_ranges=ranges))
                out[(tracking, ranges)] = _render_ex(st, gpu_ctx, lights, bias=1e-3, rt=rt)
    finally:
        gpu_ctx.set_plane_tracking(True)
        rt.close()
    first = out[(True, 0)]
    assert first.any()
    for key, frame in out.items():
        assert np.array_equal(frame, first), key
