"""Every lighting-pass kernel against the float64 model (tests/f64_shading.py): the streaming and the hinted kernel
(with and without the spot / spherical variant), the scalar kernel for widths that are not a multiple of 4, the
shadowed variants, the tiled pass, and the fused RenderLit on terrain frames.  No kernel is compared with another.

Coverage of the instantiations vr_light_plan.h names, together with tests/test_tiled_ex_f64.py: 21 of 21 shading variants
(LightVariant) and 4 of 4 culling variants (LightCull).  This module reaches the twelve streaming and hinted variants (the
packed ones in test_packed_output), LV_SCALAR, LV_TILED_ROW, LV_TILED_PACKED, LC_DEPTH and LC_RANGES; test_tiled_ex_f64.py
reaches the six EXTRA / SHADOW variants of k_deferred_tiled, LC_DEPTH_CONE and LC_RANGES_CONE."""
import numpy as np
import pytest

import vrenderer_amd as vr
from tests import f64_shading as fs
from tests.common import AMBIENT_BOTTOM, AMBIENT_TOP, CAMERAS, params, scaled_camera
from tests.common import hdr_rgb as _rgb, packed_frame as _packed, upload_planes as _upload

pytestmark = pytest.mark.gpu

EDGE_W, EDGE_H = 512, 128


@pytest.fixture(scope="module")
def terrain(gpu_ctx):
    out = {}
    for size in (256, 2048):
        h = vr.synth_heightmap(gpu_ctx, size)
        a = vr.synth_albedo(gpu_ctx, size, h)
        out[size] = vr.TerrainPass(gpu_ctx, params(size)).Init(h, a)
    yield out
    for tp in out.values():
        tp.close()


def _edge(w):
    view, planes, rows = fs.edge_case_frame(vr, w, EDGE_H)
    return view, planes, rows, fs.edge_lights(vr, view, planes, rows)


def _check_frame(got, planes, view, lights, what, shadow=None, caps=fs.EDGE_CAPS, mask=None):
    if mask is None:
        pix = fs.Pixels.from_planes(planes)
        got = got.reshape(-1, 3)
    else:
        py, px = np.nonzero(mask)
        pix = fs.Pixels.from_planes(planes, px, py)
        got = got[py, px]
    r = fs.reference(pix, view, lights, AMBIENT_TOP, AMBIENT_BOTTOM, shadow=shadow)
    res = fs.check(got, r, pix, what, caps=caps)
    print(f"{what}: worst ratio {res['worst']:.3f}, classes {res['counts']}")
    assert res["checked"] > 0.9 * got.size, res
    return res


@pytest.mark.parametrize("tracking", [False, True], ids=["stream", "hinted"])
@pytest.mark.parametrize("lights_name", ["suns", "points", "extra", "max"])
def test_edge_frame_streaming_and_hinted_kernels(gpu_ctx, tracking, lights_name):
    """k_deferred_stream (nothing known about the planes) and k_deferred (plane tracking on: the wave early-out over
    cleared texels), the EXTRA variant for the spot / spherical lists."""
    view, planes, rows, L = _edge(EDGE_W)
    gpu_ctx.set_plane_tracking(tracking)
    try:
        rt = _upload(gpu_ctx, planes)
        hdr = vr.HdrImage(gpu_ctx, EDGE_W, EDGE_H)
        vr.DeferredLightingPass(gpu_ctx).Render(view, rt, L[lights_name], AMBIENT_TOP, AMBIENT_BOTTOM, hdr)
        got = _rgb(hdr, EDGE_W, EDGE_H)
        _check_frame(got, planes, view, L[lights_name], f"{'hinted' if tracking else 'stream'}, {lights_name}")
        hdr.close(); rt.close()
    finally:
        gpu_ctx.set_plane_tracking(True)


@pytest.mark.parametrize("w", [EDGE_W - 3, EDGE_W - 2, EDGE_W - 1])
def test_edge_frame_scalar_widths(gpu_ctx, w):
    """Widths = 1, 2, 3 (mod 4): k_deferred_scalar."""
    view, planes, rows, L = _edge(w)
    rt = _upload(gpu_ctx, planes)
    hdr = vr.HdrImage(gpu_ctx, w, EDGE_H)
    vr.DeferredLightingPass(gpu_ctx).Render(view, rt, L["extra"], AMBIENT_TOP, AMBIENT_BOTTOM, hdr)
    _check_frame(_rgb(hdr, w, EDGE_H), planes, view, L["extra"], f"width {w}")
    hdr.close(); rt.close()


def _pcf_setup(gpu_ctx, width, w_scale):
    cam, lv, smap, planes = fs.pcf_frame(vr, w_scale, width)
    sm = vr.CascadedShadowMap(gpu_ctx, vr.default_shadow_params(256.0, resolution=fs.PCF_RES, depth_bias=fs.PCF_BIAS))
    sm.view = lv
    sm.targets.upload("depth", smap)
    sun = vr.reference_sun()
    lights = [sun, vr.directional_light((0.3, -1.0, 0.2), 0.5, 0.0)]
    return cam, sm, planes, lights, (lv, smap, 0, fs.PCF_BIAS, sun.out_of_bounds_shadow)


def _pcf_check(got, planes, cam, lights, sh, width, what):
    pix = fs.Pixels.from_planes(planes)
    r = fs.reference(pix, cam, lights, AMBIENT_TOP, AMBIENT_BOTTOM, shadow=sh,
                     exact_geometry=True if width % 256 == 0 else "vz")
    res = fs.check(got.reshape(-1, 3), r, pix, what)
    cov = fs.pcf_coverage(r["shadow_geo"], W=width)
    print(f"{what}: worst ratio {res['worst']:.3f}, classes {res['counts']}, coverage {cov}")
    assert res["checked"] > 0.99 * got.size
    for k in ("v0", "v1", "z0", "z1", "edge", "outside") + (("u0", "u1") if width % 256 == 0 else ()):
        assert cov[k] > 0, cov
    return cov


@pytest.mark.parametrize("width,w_scale,tracking", [(2048, 1.0, False), (2048, 1.0, True), (2048, 2.0, False),
                                                    (2045, 1.0, False), (2046, 2.0, False), (2047, 1.0, True)])
def test_pcf_frame(gpu_ctx, width, w_scale, tracking):
    """The shadowed kernels (stream / hinted quad kernels, k_deferred_scalar at widths 1, 2, 3 mod 4) on the PCF frame:
    the shadow factor against the float64 tent on every pixel - ramp, checkerboard, constants 0 and 1, receivers exactly
    on a stored depth, footprints over every edge and corner, u / v / zc exactly 0 and 1 (u: power-of-two widths), an
    orthographic (w = 1) and a general (w = 2) light matrix.  Both load paths of the quad kernels carry > 1000 pixels."""
    cam, sm, planes, lights, sh = _pcf_setup(gpu_ctx, width, w_scale)
    gpu_ctx.set_plane_tracking(tracking)
    try:
        rt = _upload(gpu_ctx, planes)
        hdr = vr.HdrImage(gpu_ctx, width, fs.PCF_H)
        vr.DeferredLightingPass(gpu_ctx).Render(cam, rt, lights, AMBIENT_TOP, AMBIENT_BOTTOM, hdr, shadow_map=sm)
        cov = _pcf_check(_rgb(hdr, width, fs.PCF_H), planes, cam, lights, sh, width, f"PCF frame {width}, w = {w_scale}")
        if width % 4 == 0:
            assert cov["clamp_path"] > 1000 and cov["row_path"] > 1000, cov
        hdr.close(); rt.close(); sm.close()
    finally:
        gpu_ctx.set_plane_tracking(True)


@pytest.mark.parametrize("world", [1, 2, 3])
@pytest.mark.parametrize("kind", ["stream", "hinted", "tiled", "shadow", "stream_suns", "hinted_suns", "shadow_hinted"])
def test_packed_output(gpu_ctx, world, kind):
    """The PACKED instantiations (a vr_partition of 1, 2 and 3 ranks): k_deferred_stream, k_deferred, k_deferred_tiled on
    the edge-case frame and the shadowed stream kernel on the PCF frame, every rank's owner tiles de-tiled on the host.
    "stream" and "hinted" run the 16-light `max` list (spot and spherical lights: LV_STREAM_PACKED_EXTRA with the tracking
    off, LV_HINTED_PACKED_EXTRA with it on); "stream_suns" and "hinted_suns" the four suns (no spot, no spherical light, no
    binding: LV_STREAM_PACKED with the tracking off, LV_HINTED_PACKED with it on); "shadow" runs with the tracking off
    (LV_STREAM_PACKED_SHADOW), "shadow_hinted" with it on (a binding, the region array as a hint: LV_HINTED_PACKED_SHADOW)."""
    if kind in ("shadow", "shadow_hinted"):
        cam, sm, planes, lights, sh = _pcf_setup(gpu_ctx, fs.PCF_W, 1.0)
        assert all(l.type == fs.VR_LIGHT_DIRECTIONAL for l in lights)
        rt = _upload(gpu_ctx, planes)
        gpu_ctx.set_plane_tracking(kind == "shadow_hinted")
        try:
            got = _packed(gpu_ctx, fs.PCF_W, fs.PCF_H, world, lambda buf, part: vr.DeferredLightingPass(gpu_ctx).Render(
                cam, rt, lights, AMBIENT_TOP, AMBIENT_BOTTOM, buf, part, shadow_map=sm))
        finally:
            gpu_ctx.set_plane_tracking(True)
        assert not np.isnan(got).any(), "every pixel belongs to one rank's tiles"
        _pcf_check(got, planes, cam, lights, sh, fs.PCF_W, f"packed shadowed ({kind}), world {world}")
        rt.close(); sm.close()
        return
    view, planes, rows, L = _edge(EDGE_W)
    lights = L["tiled" if kind == "tiled" else "suns" if kind.endswith("_suns") else "max"]
    assert fs.plan_facts(lights)["extra"] == (kind in ("stream", "hinted"))
    gpu_ctx.set_plane_tracking(not kind.startswith("stream"))
    try:
        rt = _upload(gpu_ctx, planes)
        if kind == "tiled":
            tl = vr.TiledDeferredLightingPass(gpu_ctx)
            render = lambda buf, part: tl.Render(view, rt, lights, AMBIENT_TOP, AMBIENT_BOTTOM, buf, part)  # noqa: E731
        else:
            render = lambda buf, part: vr.DeferredLightingPass(gpu_ctx).Render(  # noqa: E731
                view, rt, lights, AMBIENT_TOP, AMBIENT_BOTTOM, buf, part)
        got = _packed(gpu_ctx, EDGE_W, EDGE_H, world, render)
    finally:
        gpu_ctx.set_plane_tracking(True)
    # NaN is a legitimate output (emissive NaN): coverage is checked on the depth plane's pixels through the model
    _check_frame(got, planes, view, lights, f"packed {kind}, world {world}")
    rt.close()


@pytest.mark.parametrize("tracking", [False, True], ids=["untracked", "tracked"])
def test_edge_frame_tiled_pass_lights_the_far_plane(gpu_ctx, tracking):
    """k_light_cull + k_deferred_tiled on the edge-case frame (directional and punctual lights): texels at depth 1.0 that
    carry real planes are lit like any other, cleared texels stay +0."""
    view, planes, rows, L = _edge(EDGE_W)
    gpu_ctx.set_plane_tracking(tracking)
    try:
        rt = _upload(gpu_ctx, planes)
        hdr = vr.HdrImage(gpu_ctx, EDGE_W, EDGE_H)
        tl = vr.TiledDeferredLightingPass(gpu_ctx)
        tl.Render(view, rt, L["tiled"], AMBIENT_TOP, AMBIENT_BOTTOM, hdr)
        tl.Status()
        got = _rgb(hdr, EDGE_W, EDGE_H)
        _check_frame(got, planes, view, L["tiled"], "tiled")
        y0, y1 = rows["far_plane"]
        amb = fs.reference(fs.Pixels.from_planes(planes, np.arange(EDGE_W), np.full(EDGE_W, y0)), view, [], AMBIENT_TOP,
                           AMBIENT_BOTTOM)["ref"]
        assert (np.abs(got[y0] - amb) > 1e-3).mean() > 0.2, "texels at depth 1.0 with real planes must be lit"
        c0, c1 = rows["cleared"]
        assert (got[c0:c1] == 0).all()
        hdr.close(); rt.close()
    finally:
        gpu_ctx.set_plane_tracking(True)


def _five_lights(size):
    s = size / 256.0
    return [vr.reference_sun(), vr.point_light((10.0 * s, 40.0, -5.0 * s), 3000.0, 120.0 * s, (1.0, 0.5, 0.25)),
            vr.spot_light((-20.0 * s, 60.0, 10.0 * s), (0.3, -1.0, -0.2), 6000.0, 200.0 * s, 12.0, 25.0, (0.2, 1.0, 0.4)),
            vr.point_light((30.0 * s, 35.0, -30.0 * s), 2000.0, 150.0 * s, (0.9, 0.9, 1.0), radius=6.0),
            vr.spot_light((0.0, 80.0, -40.0 * s), (0.0, -1.0, 0.3), 9000.0, 0.0, 5.0, 40.0, (1.0, 0.2, 0.2), radius=3.0)]


@pytest.mark.parametrize("fused", [False, True], ids=["render+lighting", "render_lit"])
@pytest.mark.parametrize("n_lights", [1, 5])
@pytest.mark.parametrize("size", [256, 2048])
def test_terrain_frames(gpu_ctx, terrain, size, n_lights, fused):
    """Terrain G-buffers at 640x360 through the hinted k_deferred (tile pass + lighting) and through the fused
    vr_terrain_render_lit; the class caps are the default 1e-4 of the checked values."""
    w, h = 640, 360
    tp = terrain[size]
    eye, tgt = scaled_camera(CAMERAS[0], size)
    view = vr.make_view(eye, tgt, w, h)
    lights = _five_lights(size)[:n_lights]
    rp = vr.default_render_params(400.0, assume_cleared=1)
    rt = vr.RenderTargets(gpu_ctx).Init(w, h)
    hdr = vr.HdrImage(gpu_ctx, w, h)
    tp.Render(view, view, rt, rp)                              # the G-buffer the model shades (the tile pass is bit-exact)
    planes = {k: rt.download(k) for k in rt.PLANES}
    if fused:
        tp.RenderLit(view, rt, rp, lights, AMBIENT_TOP, AMBIENT_BOTTOM, hdr)
    else:
        vr.DeferredLightingPass(gpu_ctx).Render(view, rt, lights, AMBIENT_TOP, AMBIENT_BOTTOM, hdr)
    assert (planes["depth"] < 1.0).mean() > 0.05
    _check_frame(_rgb(hdr, w, h), planes, view, lights, f"{size}^2, {n_lights} lights, {'fused' if fused else 'two passes'}",
                 caps=None)
    hdr.close(); rt.close()


@pytest.mark.parametrize("depth_ranges", [0, 1], ids=["depth_re_read", "tile_pass_ranges"])
def test_tiled_1024_lights(gpu_ctx, terrain, depth_ranges):
    """The tiled pass with 1024 point lights at 256x144 (plus the sun), culling on the depth plane re-read and on the
    ranges the tile pass leaves (k_raster's RANGES variant)."""
    w, h, size = 256, 144, 256
    tp = terrain[size]
    eye, tgt = scaled_camera(CAMERAS[0], size)
    view = vr.make_view(eye, tgt, w, h)
    hm = vr.synth_heightmap(gpu_ctx, size)
    lights = [vr.reference_sun()] + list(vr.synthetic_point_lights(1023, float(size), hm))
    rt = vr.RenderTargets(gpu_ctx).Init(w, h)
    tp.Render(view, view, rt, vr.default_render_params(400.0, assume_cleared=1, depth_ranges=depth_ranges))
    hdr = vr.HdrImage(gpu_ctx, w, h)
    tl = vr.TiledDeferredLightingPass(gpu_ctx)
    tl.Render(view, rt, lights, AMBIENT_TOP, AMBIENT_BOTTOM, hdr)
    tl.Status()
    planes = {k: rt.download(k) for k in rt.PLANES}
    _check_frame(_rgb(hdr, w, h), planes, view, lights, "tiled, 1024 lights", caps=None)
    hdr.close(); rt.close()


def test_8k_frame_sample(gpu_ctx, terrain):
    """The bench's 8K frame (2048^2 scene, reference sun, tracked path): a seeded sample of 2^20 pixels."""
    w, h, size = 7680, 4320, 2048
    tp = terrain[size]
    eye, tgt = scaled_camera(CAMERAS[0], size)
    view = vr.make_view(eye, tgt, w, h)
    lights = [vr.reference_sun()]
    rt = vr.RenderTargets(gpu_ctx).Init(w, h)
    tp.Render(view, view, rt, vr.default_render_params(400.0, assume_cleared=1))
    hdr = vr.HdrImage(gpu_ctx, w, h)
    vr.DeferredLightingPass(gpu_ctx).Render(view, rt, lights, AMBIENT_TOP, AMBIENT_BOTTOM, hdr)
    got = _rgb(hdr, w, h)
    planes = {k: rt.download(k) for k in rt.PLANES}
    rng = np.random.default_rng(8)
    idx = rng.choice(w * h, 1 << 20, replace=False)
    py, px = np.divmod(idx, w)
    mask = np.zeros((h, w), bool)
    mask[py, px] = True
    _check_frame(got, planes, view, lights, "8K sample", caps=None, mask=mask)
    hdr.close(); rt.close()
