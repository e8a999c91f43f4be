"""vr_deferred_light_tiled_ex - k_deferred_tiled<.., EXTRA, SHADOW> and k_light_cull<RANGES, CONE> - against the float64 model
(tests/f64_shading.py).  Every assertion on a frame goes through f64_shading.reference and f64_shading.check (TiledCase); no kernel
is compared with another kernel or with the oracle.  The oracle's worst ratio for the same input is printed beside the kernel's;
tests/test_tiled_ex_f64_cpu.py holds the oracle to the same reference, caps and masks, which is what makes the caps conditions on
the inputs.  Each docstring names the LightVariant and LightCull value the case selects under light_plan() (vr_light_plan.h) and
the facts that select it; the facts are asserted as premises."""
import contextlib

import numpy as np
import pytest

import vrenderer_amd as vr
from tests import f64_shading as fs
from tests.common import AMBIENT_BOTTOM, AMBIENT_TOP, CAMERAS, params, scaled_camera
from tests.common import hdr_rgb as _rgb, packed_frame as _packed, upload_planes as _upload

pytestmark = pytest.mark.gpu

AMBIENT = (AMBIENT_TOP, AMBIENT_BOTTOM)
_CASES, _ORACLE = {}, {}


def _case(key, build):
    """The case's input and float64 reference: computed once, shared by the tests that run it, never changed."""
    if key not in _CASES:
        _CASES[key] = build()
    return _CASES[key]


def _edge(width, lights_name):
    return _case(("edge", width, lights_name), lambda: fs.tiled_edge_case(vr, AMBIENT, width, lights_name))


def _pcf(lists, w_scale=1.0):
    return _case(("pcf", lists, w_scale), lambda: fs.tiled_pcf_case(vr, AMBIENT, lists, w_scale))


def _check(case, oracle, frame, what):
    res = case.check(frame, what, report=False)
    if case.name not in _ORACLE:                     # printed, not asserted here: test_tiled_ex_f64_cpu.py asserts it
        try:
            _ORACLE[case.name] = f"{case.check(case.oracle_frame(oracle), 'oracle', report=False)['worst']:.4f}"
        except AssertionError as e:
            _ORACLE[case.name] = f"outside ({str(e)[:80]})"
    print(f"{case.name}: {what}: kernel worst ratio {res['worst']:.4f}, oracle {_ORACLE[case.name]}, classes {res['counts']}"
          + (f", coverage {res['coverage']}" if "coverage" in res else ""))
    return res


@contextlib.contextmanager
def _tracking(gpu_ctx, on):
    gpu_ctx.set_plane_tracking(on)
    try:
        yield
    finally:
        gpu_ctx.set_plane_tracking(True)


def _shadow_map(gpu_ctx, case):
    """The case's map behind a binding, uploaded as test_lighting_f64._pcf_setup does."""
    sm = vr.CascadedShadowMap(gpu_ctx, vr.default_shadow_params(256.0, resolution=fs.PCF_RES, depth_bias=fs.PCF_BIAS))
    sm.view = case.light_view
    sm.targets.upload("depth", case.shadow_map)
    return sm


def _frame(gpu_ctx, case, world=None, sm=None, ex=True):
    """The case through vr_deferred_light_tiled_ex (ex=False: vr_deferred_light_tiled): row-major, or - world given - every rank's
    packed owner tiles de-tiled on the host.  Returns ((h, w, 3) float64, the pass)."""
    tl = vr.TiledDeferredLightingPass(gpu_ctx)
    kw = dict(all_light_types=True) if ex else {}
    if sm is not None:
        kw.update(shadow_map=sm, shadow_light_index=case.shadow[2])
    rt = _upload(gpu_ctx, case.planes)
    render = lambda out, part=None: tl.Render(case.view, rt, case.lights, AMBIENT_TOP, AMBIENT_BOTTOM, out, part, **kw)   # noqa: E731
    if world is None:
        hdr = vr.HdrImage(gpu_ctx, case.w, case.h)
        render(hdr)
        got = _rgb(hdr, case.w, case.h)
        hdr.close()
    else:
        got = _packed(gpu_ctx, case.w, case.h, world, render)
    tl.Status()                                      # no tile's list overflowed
    rt.close()
    return got, tl


def _premises(case, extra, cone, shadow):
    """The facts vr_light_check hands to light_plan(): a spot or radius > 0 light in the list; a spot with outer_angle below
    pi / 2 and a unit axis; a binding on a directional light."""
    facts = fs.plan_facts(case.lights)
    assert facts["extra"] == extra and facts["cone"] == cone, facts
    assert (case.shadow is not None) == shadow
    if shadow:
        assert case.lights[case.shadow[2]].type == fs.VR_LIGHT_DIRECTIONAL


def _edge_rows(case, got, lit):
    c0, c1 = case.rows["cleared"]
    assert (got[c0:c1] == 0).all() and not np.signbit(got[c0:c1]).any(), "cleared texels stay +0"
    if lit:
        y0 = case.rows["far_plane"][0]
        amb = fs.reference(fs.Pixels.from_planes(case.planes, np.arange(case.w), np.full(case.w, y0)), case.view, [], *AMBIENT)["ref"]
        assert (np.abs(got[y0] - amb) > 1e-3).mean() > 0.2, "texels at depth 1.0 with real planes must be lit"


# ---- cases 1 and 2: the edge-case frame -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tracking", [False, True], ids=["untracked", "tracked"])
@pytest.mark.parametrize("lights_name", ["extra", "all"])
def test_edge_frame_extra_row_major(gpu_ctx, oracle, lights_name, tracking):
    """LV_TILED_ROW_EXTRA with LC_DEPTH_CONE.  Facts: the entry is vr_deferred_light_tiled_ex (all_light_types), no partition,
    no binding; the list (`extra`, or the 13 lights suns + points + extra) holds spot and spherical lights (extra) and spots
    with outer_angle below pi / 2 and a unit axis (cone); an uploaded G-buffer carries no depth ranges.  The edge-case frame at
    512x128: far-plane texels with real planes, single cleared texels inside a lit wave, roughness -1, emissive Inf and NaN -
    through bg[] and the TiledExtra staging, with the plane tracking off and on (on: every region's state is 'unknown')."""
    case = _edge(512, lights_name)
    _premises(case, extra=True, cone=True, shadow=False)
    assert len(case.lights) == dict(extra=5, all=13)[lights_name]
    with _tracking(gpu_ctx, tracking):
        got, _ = _frame(gpu_ctx, case)
    _check(case, oracle, got, f"row-major, tracking {tracking}")
    _edge_rows(case, got, lit=lights_name == "all")


@pytest.mark.parametrize("lights_name", ["extra", "all"])
def test_partial_light_tile_column_row_major(gpu_ctx, oracle, lights_name):
    """LV_TILED_ROW_EXTRA with LC_DEPTH_CONE at width 508 (a multiple of 4, not of 32): the last column of light tiles is 28
    pixels wide - `inside` in x, the culling boxes' min(cx1, w).  Facts as above: tiled_ex, no partition, no binding, spot
    and spherical lights, a culled cone, no ranges."""
    case = _edge(508, lights_name)
    _premises(case, extra=True, cone=True, shadow=False)
    assert case.w % 4 == 0 and case.w % 32 == 28
    got, _ = _frame(gpu_ctx, case)
    _check(case, oracle, got, "row-major")
    _edge_rows(case, got, lit=lights_name == "all")


@pytest.mark.parametrize("world", [2, 3])
def test_partial_light_tile_column_packed(gpu_ctx, oracle, world):
    """LV_TILED_PACKED_EXTRA with LC_DEPTH_CONE at width 508: a partition is given (packed), the 13-light list holds spot and
    spherical lights and culled cones, no binding, no ranges.  The last owner tile is 124 pixels wide; every rank's tiles are
    de-tiled on the host."""
    case = _edge(508, "all")
    _premises(case, extra=True, cone=True, shadow=False)
    got, _ = _frame(gpu_ctx, case, world=world)
    _check(case, oracle, got, f"packed, world {world}")
    _edge_rows(case, got, lit=True)


def test_partial_light_tile_column_plain_tiled(gpu_ctx, oracle):
    """LV_TILED_ROW with LC_DEPTH at width 508: the entry is vr_deferred_light_tiled, the list (suns + points) has no spot and
    no spherical light, no partition - the old kernel at the same edge."""
    case = _edge(508, "tiled")
    _premises(case, extra=False, cone=False, shadow=False)
    got, _ = _frame(gpu_ctx, case, ex=False)
    _check(case, oracle, got, "vr_deferred_light_tiled, row-major")
    _edge_rows(case, got, lit=True)


# ---- cases 3 to 6: the PCF frame ----------------------------------------------------------------------------------------------------
def _pcf_run(gpu_ctx, oracle, case, world=None):
    sm = _shadow_map(gpu_ctx, case)
    got, tl = _frame(gpu_ctx, case, world=world, sm=sm)
    sm.close()
    assert not np.isnan(got).any(), "every pixel belongs to one rank's tiles"
    _check(case, oracle, got, "row-major" if world is None else f"packed, world {world}")
    return tl


@pytest.mark.parametrize("w_scale", [1.0, 2.0])
def test_pcf_frame_shadow_row_major(gpu_ctx, oracle, w_scale):
    """LV_TILED_ROW_SHADOW with LC_DEPTH.  Facts: vr_deferred_light_tiled_ex with a binding on light 0 (the sun, directional),
    the list [sun, directional] has no spot and no spherical light, no partition, no ranges (uploaded).  shadow_factor in
    front of the light loop on every pixel of the exact-geometry PCF frame at 2048x64, an orthographic (w = 1) and a general
    (w = 2) light matrix: more than 99 % of the values checked, every coverage key hit."""
    case = _pcf("sun_first", w_scale)
    _premises(case, extra=False, cone=False, shadow=True)
    assert case.shadow[2] == 0 and (case.w, case.h) == (2048, 64)
    _pcf_run(gpu_ctx, oracle, case)


@pytest.mark.parametrize("world", [1, 2, 3])
def test_pcf_frame_shadow_packed(gpu_ctx, oracle, world):
    """LV_TILED_PACKED_SHADOW with LC_DEPTH: the same with a partition of 1, 2 and 3 ranks (packed), a binding on the sun, no
    spot and no spherical light."""
    case = _pcf("sun_first")
    _premises(case, extra=False, cone=False, shadow=True)
    _pcf_run(gpu_ctx, oracle, case, world=world)


@pytest.mark.parametrize("lists", ["sun_second", "twice"])
def test_shadow_light_not_first(gpu_ctx, oracle, lists):
    """LV_TILED_ROW_SHADOW with LC_DEPTH, shadow_light_index 1 of [directional, sun] and 3 of [directional, sun, directional,
    sun]: a binding on a directional light that is not light 0, no spot and no spherical light, no partition.  The model gets
    the index through the shadow tuple; a flag on another staged slot, or on every directional light, moves a quarter of the
    frame by the whole sun."""
    case = _pcf(lists)
    _premises(case, extra=False, cone=False, shadow=True)
    assert case.shadow[2] == dict(sun_second=1, twice=3)[lists] == len(case.lights) - 1
    _pcf_run(gpu_ctx, oracle, case)


@pytest.mark.parametrize("world", [None, 2], ids=["row_major", "packed2"])
def test_pcf_frame_every_light_type_under_the_shadow(gpu_ctx, oracle, world):
    """LV_TILED_ROW_EXTRA_SHADOW and LV_TILED_PACKED_EXTRA_SHADOW (a partition of 2 ranks) with LC_DEPTH_CONE.  Facts: a binding
    on the sun (list index 3, behind two ranged lights: a tile that culls one stages the sun in another slot than its index);
    the list holds a punctual point light, spots with and without a range, a spherical point and a spherical spot (extra); the
    spots have outer_angle below pi / 2 and unit axes (cone); no ranges.  Every light is at least 5 units from every
    receiver (asserted on the CPU side too)."""
    case = _pcf("all_types")
    _premises(case, extra=True, cone=True, shadow=True)
    assert fs.plan_facts(case.lights)["kinds"] == fs.ALL_KINDS and case.shadow[2] == 3
    tl = _pcf_run(gpu_ctx, oracle, case, world=world)
    if world is None:
        lists = [tl.tile_light_list(x, 0).tolist() for x in range(case.w // 32)]
        assert any(l.index(3) < 3 for l in lists) and any(l.index(3) == 3 for l in lists), "the sun's slot varies with the culling"


def test_more_than_256_lights_with_the_sun_in_the_second_staging_round(gpu_ctx, oracle):
    """LV_TILED_ROW_EXTRA_SHADOW with LC_DEPTH_CONE on the PCF frame of width 256: 300 weak spot and spherical lights over the
    light tile PCF_CROWD_TILE, the unshadowed directional light in front, the sun last with the binding on it - in that tile's
    list it stands beyond position 256, so kTlShadowed is set in the second staging round.  Facts: a binding, spot and
    spherical lights, culled cones, no partition, no ranges.  Checked on the 4096 pixels of pcf_crowd_mask: the tile and a
    sample of its neighbours."""
    case = _pcf("crowd")
    _premises(case, extra=True, cone=True, shadow=True)
    li = case.shadow[2]
    assert li == len(case.lights) - 1 == fs.PCF_CROWD_N + 1 and len(case.pix) == 4096
    tl = _pcf_run(gpu_ctx, oracle, case)
    hot = tl.tile_light_list(*fs.PCF_CROWD_TILE)
    assert len(hot) > 256 and int(np.flatnonzero(hot == li)[0]) >= 256, (len(hot), hot[-3:])
    assert len(hot) == len(case.lights), "the 300 lights, the directional one and the sun"


# ---- case 7: the tile pass's ranges and the tracked hints ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def terrain(gpu_ctx):
    size, w, h = 256, 256, 144
    hm = vr.synth_heightmap(gpu_ctx, size)
    tp = vr.TerrainPass(gpu_ctx, params(size)).Init(hm, vr.synth_albedo(gpu_ctx, size, hm))
    view = vr.make_view(*scaled_camera(CAMERAS[7], size), w, h)
    rt = vr.RenderTargets(gpu_ctx).Init(w, h)
    tp.Render(view, view, rt, vr.default_render_params(400.0))           # the G-buffer the model shades (the tile pass is bit-exact)
    planes = {k: rt.download(k) for k in rt.PLANES}
    rt.close()
    yield tp, view, fs.tiled_terrain_case(vr, AMBIENT, view, planes)
    tp.close()


@pytest.mark.parametrize("tracking", [True, False], ids=["tracked", "untracked"])
def test_terrain_frame_with_the_tile_pass_ranges(gpu_ctx, oracle, terrain, tracking):
    """LV_TILED_ROW_EXTRA with LC_RANGES_CONE.  Facts: vr_deferred_light_tiled_ex, no partition, no binding; the 40 lights of
    all_type_lights hold every kind (extra) and spots with outer_angle below pi / 2 and unit axes (cone); the tile pass left
    ranges.  That last fact cannot be seen from outside (the library exposes neither the ranges' state nor the culling variant
    a call took): it rests on raster_plan()'s conditions, as in test_tiled_1024_lights - depth_ranges = 1 and assume_cleared = 1
    (the only two the test can assert), the fast tile-pass variant this terrain gets, a fresh G-buffer whose pointers never
    left the library, and nothing that touches it between the tile pass and the lighting call.  The 256^2 terrain at 256x144 from CAMERAS[7]: with the tracking on, sky regions
    (kRegionClear), constant-specular regions and mixed ones reach the EXTRA kernel as hints."""
    tp, view, case = terrain
    _premises(case, extra=True, cone=True, shadow=False)
    assert len(case.lights) == 40 and fs.plan_facts(case.lights)["kinds"] >= fs.ALL_KINDS
    with _tracking(gpu_ctx, tracking):
        rp = vr.default_render_params(400.0, assume_cleared=1, depth_ranges=1)
        assert rp.depth_ranges == 1 and rp.assume_cleared == 1
        rt = vr.RenderTargets(gpu_ctx).Init(case.w, case.h)
        hdr = vr.HdrImage(gpu_ctx, case.w, case.h)
        tp.Render(view, view, rt, rp)
        tl = vr.TiledDeferredLightingPass(gpu_ctx)
        tl.Render(view, rt, case.lights, AMBIENT_TOP, AMBIENT_BOTTOM, hdr, all_light_types=True)
        tl.Status()
        census = rt.region_census()
        got = _rgb(hdr, case.w, case.h)
        for k in rt.PLANES:
            assert np.array_equal(rt.download(k), case.planes[k]), f"premise: the model shades this G-buffer ({k})"
        hdr.close(); rt.close()
    if tracking:
        assert census["clear"] > 0 and census["specular_constant"] > 0 and census["unknown"] > 0, census
    else:
        assert census["unknown"] == census["total"], census
    _check(case, oracle, got, f"tile-pass ranges, tracking {tracking}")
