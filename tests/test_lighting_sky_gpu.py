"""Every lighting path against the kernel that always shades (k_deferred_stream: plane tracking off, whole frame), bit for bit on
the half words, at the extremes of the lighting model's domain and outside it (tests/sky_classes.py; the domain:
vrenderer_amd/csrc/vr_light_domain.h).  Frames are small on purpose: the shortcuts are per wave (256 consecutive pixels) and per
8x32 region, so each frame has waves that are all sky, mixed, and without sky.

Nothing is kept off the device.  What was read before the finite extremes went there: the lighting kernels compute no index or
trip count from a float that the view or a light reaches, except shadow_factor's footprint, which sits behind comparisons that a
NaN fails and is clamped to the map; k_light_cull turns its boxes into booleans only.  The tile pass (the fused entries run it
under the infinite-far-plane and the 2^20 views too) reads world_to_clip, which is an ordinary finite matrix for both; its one
conversion of a view-dependent float is snap_vertex's, clamped to +-1e9 in front of the cast (a NaN takes the lower bound),
and tri_setup clamps every pixel box to the viewport before a bin or a pixel is addressed.  Which kernel a call launched is read
back (Context.last_light_variant), so that an equality cannot hold for want of the path it is about."""
import numpy as np
import pytest

import vrenderer_amd as vr
from tests import sky_classes as sc
from tests.common import AMBIENT_BOTTOM, AMBIENT_TOP, CAMERAS, flythrough_camera, packed_frame, scaled_camera, upload_planes
from tests.fusion_common import FUSED, terrain_fixture

pytestmark = pytest.mark.gpu

W, H, SKY_ROWS, SKY_PIXEL = 128, 96, 40, (40, 10)
SENTINEL = 0x3c00                                               # 1.0 in every half of HdrColor
INVALID = vr.capi.VR_ERR_INVALID_ARGUMENT


def _planes(w, h, seed=11, sky_rows=SKY_ROWS):
    """Random surface data as the fuzz test draws it, rows 0 .. sky_rows - 1 cleared."""
    rng = np.random.default_rng(seed)
    n = rng.normal(size=(h, w, 3)); n /= np.linalg.norm(n, axis=-1, keepdims=True)
    p = dict(depth=rng.uniform(0.2, 0.999, size=(h, w)).astype(np.float32),
             diffuse=rng.integers(0, 2 ** 32, size=(h, w), dtype=np.uint32), specular=rng.integers(0, 2 ** 32, size=(h, w), dtype=np.uint32),
             normals=np.round(np.concatenate([n, rng.uniform(0, 1, size=(h, w, 1))], -1) * 32767.0).astype(np.int16).view(np.uint16),
             emissive=np.abs(rng.normal(0, 0.05, size=(h, w, 4))).astype(np.float16).view(np.uint16))
    for k, a in p.items():
        a[:sky_rows] = 1.0 if k == "depth" else 0
    return p


def _words(hdr, w, h):
    return hdr.download().view(np.uint16).reshape(h, w, 4).copy()


def _light(ctx, rt, case, w, h, *, tiled=None, shadow=None, part=None, hdr=None):
    """One lighting call into an image prefilled with SENTINEL; the half words (h, w, 4), or the packed image's when part is given."""
    own = hdr is None
    if own:
        hdr = vr.HdrImage(ctx, w, h)
    try:
        hdr.upload(np.full(hdr.width * hdr.height * 4, SENTINEL, np.uint16))
        if tiled is None:
            vr.DeferredLightingPass(ctx).Render(case.view, rt, case.lights, case.top, case.bottom, hdr, part, shadow_map=shadow)
        else:
            vr.TiledDeferredLightingPass(ctx).Render(case.view, rt, case.lights, case.top, case.bottom, hdr, part, all_light_types=tiled == "ex", shadow_map=shadow)
        return _words(hdr, hdr.width, hdr.height) if own else None
    finally:
        if own:
            hdr.close()


def _stream(ctx, planes, case, w, h, shadow=None):
    """The reference: k_deferred_stream (k_deferred_scalar at a width that is no multiple of 4) - nothing known about the planes."""
    ctx.set_plane_tracking(False)
    try:
        rt = upload_planes(ctx, planes)
        try:
            return _light(ctx, rt, case, w, h, shadow=shadow)
        finally:
            rt.close()
    finally:
        ctx.set_plane_tracking(True)


def _same(want, got, what):
    assert want.shape == got.shape and np.array_equal(want, got), f"{what}: {(want != got).any(-1).sum()} pixels differ, first {np.argwhere((want != got).any(-1))[:3].tolist()}"


def _rgb(words):
    return words[..., :3].view(np.float16).astype(np.float64)


@pytest.fixture(scope="module")
def cases(product_lib):
    return {c.name: c for c in sc.cases(W, H, SKY_PIXEL)}


@pytest.fixture(scope="module")
def planes():
    return _planes(W, H)


@pytest.fixture(scope="module")
def fx():
    with terrain_fixture(256) as f:
        yield f


@pytest.fixture(scope="module")
def shadow_map(fx):
    """The sun's shadow map of the 256^2 terrain (the lighting kernels only read its depth plane and the light view)."""
    ctx = fx["ctx"]
    sm = vr.CascadedShadowMap(ctx, vr.default_shadow_params(256.0, resolution=256))
    sm.SetupForPlanarViewStable(vr.reference_sun(), vr.make_view(sc.EYE, sc.TARGET, W, H))
    sm.Clear()
    sm.RenderTerrain(fx["tp"])
    yield sm
    sm.close()


# (the names as literals: collecting the tests must not build the library; _case() checks each against tests/sky_classes.py)
_ALL_NAMES = ["in: sun, intensity and color at 2^40", "in: sun at 2^40 with out_of_bounds_shadow at 2^40", "out: sun at 1e9 with out_of_bounds_shadow at 1e30",
              "in: unranged point light at 2^40", "in: spot light at 2^40 looking at the sky",
              "in: spherical source at 2^40", "in: unranged point light nearest to the far plane", "in: ranged light whose range ends on the far plane",
              "in: ambient colours at 6e4", "in: world coordinates at 2^20", "out: the 3e38 x 10 sun", "out: infinite far plane, unranged point light",
              "out: infinite far plane, sun only", "out: point light on a far-plane pixel's reconstructed position"]


def _case(cases, name):
    hit = [c for n, c in cases.items() if n == name or (name.endswith("nearest to the far plane") and "nearest" in n)]
    assert len(hit) == 1, name
    return hit[0]


def _family(ctx):
    """The kernel family of the context's last lighting pass, by vr_light_plan.h's LightVariant, and whether its culling stage took the depth ranges."""
    shade, cull = ctx.last_light_variant()
    return ("stream" if 0 <= shade < 6 else "hinted" if shade < 12 else "scalar" if shade == 12 else "tiled"), cull in (1, 3)


def _expect_kernel(ctx, case, what):
    """Inside sky_is_zero a call with something known about the planes runs k_deferred; outside it k_deferred_stream, whatever is known."""
    assert _family(ctx)[0] == ("hinted" if case.kind == "in" else "stream"), f"{what}: ran {ctx.last_light_variant()}"


_WITH_SUN = [n for n in _ALL_NAMES if "sun" in n or "nearest" in n or "6e4" in n or "2^20" in n or "infinite far plane, unranged" in n]


def _plain_list(case):
    return all(l.type == vr.capi.VR_LIGHT_DIRECTIONAL or (l.type == vr.capi.VR_LIGHT_POINT and l.radius == 0.0) for l in case.lights)


@pytest.mark.parametrize("name", _ALL_NAMES)
def test_the_streaming_paths_equal_the_kernel_that_always_shades(gpu_ctx, cases, planes, name):
    """128x96, rows 0 .. 39 cleared.  Tracking on with the planes uploaded (the clear not known: k_deferred looks at the texels),
    an all-sky frame behind a lazy Clear (the clear known), the 127-wide frame (k_deferred_scalar, tracked against untracked) and
    a 256x128 frame under Partition(r, 2) (packed, both ranks): each equals the untracked pass bit for bit on every pixel.
    With the emissive plane known zero (a Clear, then four planes uploaded) and behind the Clear alone the kernel is read back:
    k_deferred inside sky_is_zero, k_deferred_stream outside it.
    Inside sky_is_zero the reference's sky pixels are exactly +0; outside it the model's domain check sent every call to the
    kernels that shade - the equality is then not the shortcut's merit."""
    case = _case(cases, name)
    ref = _stream(gpu_ctx, planes, case, W, H)
    assert not (ref[..., :3] == SENTINEL).all(-1).any(), "a pixel was not written"
    if case.kind == "in":
        assert not ref[:SKY_ROWS, :, :3].any(), f"{name}: a sky pixel of the reference is not +0: {_rgb(ref)[:SKY_ROWS][ref[:SKY_ROWS, :, :3].any(-1)][:3]}"
    assert np.isfinite(_rgb(ref)[SKY_ROWS:]).any()
    rt = upload_planes(gpu_ctx, planes)
    try:
        _same(ref, _light(gpu_ctx, rt, case, W, H), f"{name}: tracked, clear not known")
    finally:
        rt.close()
    assert _family(gpu_ctx)[0] in ("hinted", "stream")
    # the same with the emissive plane known zero: the question is asked (k_deferred), the regions are unknown, the texels decide
    dark = dict(planes, emissive=np.zeros_like(planes["emissive"]))
    want = _stream(gpu_ctx, dark, case, W, H)
    assert _family(gpu_ctx)[0] == "stream"
    rt = vr.RenderTargets(gpu_ctx).Init(W, H)
    try:
        rt.Clear()
        for k in ("depth", "diffuse", "specular", "normals"):
            rt.upload(k, dark[k])
        assert rt.plane_known_zero("emissive")
        _same(want, _light(gpu_ctx, rt, case, W, H), f"{name}: tracked, emissive known zero, clear not known")
        _expect_kernel(gpu_ctx, case, f"{name}: emissive known zero")
    finally:
        rt.close()
    # the clear known: a lazy Clear, nothing else
    sky = sc.cleared_planes(W, H)
    want = _stream(gpu_ctx, sky, case, W, H)
    rt = vr.RenderTargets(gpu_ctx).Init(W, H)
    try:
        rt.Clear()
        _same(want, _light(gpu_ctx, rt, case, W, H), f"{name}: tracked, clear known")
        _expect_kernel(gpu_ctx, case, f"{name}: clear known")
    finally:
        rt.close()
    # the scalar kernel
    ws = 127
    odd = {k: np.ascontiguousarray(a[:, :ws]) for k, a in planes.items()}
    c127 = _case({c.name: c for c in sc.cases(ws, H, SKY_PIXEL)}, name)
    want = _stream(gpu_ctx, odd, c127, ws, H)
    if case.kind == "in":
        assert not want[:SKY_ROWS, :, :3].any(), f"{name}: scalar kernel, sky not +0"
    rt = upload_planes(gpu_ctx, odd)
    try:
        _same(want, _light(gpu_ctx, rt, c127, ws, H), f"{name}: scalar kernel, tracked")
        assert _family(gpu_ctx)[0] == "scalar"
    finally:
        rt.close()
    # packed, world = 2
    wp, hp = 256, 128
    big = _planes(wp, hp, seed=12)
    cp = _case({c.name: c for c in sc.cases(wp, hp, SKY_PIXEL)}, name)
    want = _stream(gpu_ctx, big, cp, wp, hp)
    rt = upload_planes(gpu_ctx, big)
    try:
        def render(buf, part):
            buf.upload(np.zeros(buf.width * buf.height * 4, np.uint16))
            _light(gpu_ctx, rt, cp, wp, hp, part=part, hdr=buf)
        got = packed_frame(gpu_ctx, wp, hp, 2, render)
        assert np.array_equal(got, _rgb(want), equal_nan=True) and np.array_equal(np.signbit(got), np.signbit(_rgb(want))), f"{name}: packed, world = 2"
    finally:
        rt.close()


@pytest.mark.parametrize("name", _WITH_SUN)
def test_the_shadowed_paths_equal_the_kernel_that_always_shades(fx, shadow_map, cases, planes, name):
    """The shadow term on the list's sun (every case whose list has one; a far-plane pixel is outside the map and gets the light's
    out_of_bounds_shadow - at 2^40 with the intensity at 2^40 in one class, overflowing the product in another): shadowed stream
    against the shadowed tracked pass on uploaded planes and behind a lazy Clear, bit for bit, the kernel read back; and
    vr_deferred_light_tiled_ex with the binding: its sky rows equal the stream kernel's inside sky_is_zero, it refuses outside."""
    ctx, case = fx["ctx"], _case(cases, name)
    assert any(l.type == vr.capi.VR_LIGHT_DIRECTIONAL for l in case.lights), name
    li = [i for i, l in enumerate(case.lights) if l.type == vr.capi.VR_LIGHT_DIRECTIONAL][0]
    if li != 0:
        case = sc.Case(case.name, case.kind, case.view, [case.lights[li]] + [l for i, l in enumerate(case.lights) if i != li], case.top, case.bottom)
    ref = _stream(ctx, planes, case, W, H, shadow=shadow_map)
    if case.kind == "in":
        assert not ref[:SKY_ROWS, :, :3].any(), f"{name}: a sky pixel of the shadowed reference is not +0"
    rt = upload_planes(ctx, planes)
    try:
        _same(ref, _light(ctx, rt, case, W, H, shadow=shadow_map), f"{name}: shadowed, tracked")
        hdr = vr.HdrImage(ctx, W, H)
        try:
            if case.kind == "in":
                _light(ctx, rt, case, W, H, tiled="ex", shadow=shadow_map, hdr=hdr)
                assert _family(ctx)[0] == "tiled"
                _same(ref[:SKY_ROWS], _words(hdr, W, H)[:SKY_ROWS], f"{name}: shadowed tiled_ex, sky rows")
            else:
                with pytest.raises(vr.VrError) as err:
                    _light(ctx, rt, case, W, H, tiled="ex", shadow=shadow_map, hdr=hdr)
                assert err.value.code == INVALID and "use vr_deferred_light" in str(err.value), str(err.value)
                assert (_words(hdr, W, H) == SENTINEL).all()
        finally:
            hdr.close()
    finally:
        rt.close()
    want = _stream(ctx, sc.cleared_planes(W, H), case, W, H, shadow=shadow_map)
    if name == "out: sun at 1e9 with out_of_bounds_shadow at 1e30":
        # why the bound exists: the far plane is outside the map, intensity * out_of_bounds_shadow = Inf, 0 * Inf = NaN
        assert np.isnan(_rgb(want)).any(), "the class does not overflow under the binding: it shows nothing"
    rt = vr.RenderTargets(ctx).Init(W, H)
    try:
        rt.Clear()
        _same(want, _light(ctx, rt, case, W, H, shadow=shadow_map), f"{name}: shadowed, clear known")
        _expect_kernel(ctx, case, f"{name}: shadowed, clear known")
    finally:
        rt.close()


@pytest.mark.parametrize("name", _ALL_NAMES)
def test_the_tiled_paths_at_the_sky(gpu_ctx, cases, planes, name):
    """k_deferred_tiled gives a background pixel no light, whatever the host knows.  Inside sky_is_zero its sky pixels equal the
    streaming kernel's bit for bit (+0), through vr_deferred_light_tiled (plain lists) and _tiled_ex, tracked and untracked;
    outside it both entries refuse, name the entry to use and leave HdrColor alone."""
    case = _case(cases, name)
    entries = (["plain"] if _plain_list(case) else []) + ["ex"]
    hdr = vr.HdrImage(gpu_ctx, W, H)
    try:
        if case.kind == "out":
            rt = upload_planes(gpu_ctx, planes)
            try:
                for e in entries:
                    with pytest.raises(vr.VrError) as err:
                        _light(gpu_ctx, rt, case, W, H, tiled=e, hdr=hdr)
                    assert err.value.code == INVALID and "use vr_deferred_light" in str(err.value), str(err.value)
                    assert (_words(hdr, W, H) == SENTINEL).all()
            finally:
                rt.close()
            return
        ref = _stream(gpu_ctx, planes, case, W, H)
        for tracking in (False, True):
            gpu_ctx.set_plane_tracking(tracking)
            rt = upload_planes(gpu_ctx, planes)
            try:
                for e in entries:
                    _light(gpu_ctx, rt, case, W, H, tiled=e, hdr=hdr)
                    got = _words(hdr, W, H)
                    _same(ref[:SKY_ROWS], got[:SKY_ROWS], f"{name}: tiled ({e}), tracking {tracking}, sky rows")
                    assert not (got[..., :3] == SENTINEL).all(-1).any()
                vr.TiledDeferredLightingPass(gpu_ctx).Status()
            finally:
                rt.close()
                gpu_ctx.set_plane_tracking(True)
    finally:
        hdr.close()


@pytest.mark.parametrize("name", [n for n in _ALL_NAMES if n.startswith("out:")])
def test_the_streaming_kernel_s_sky_against_the_model(gpu_ctx, cases, planes, name):
    """Outside sky_is_zero: the class (zero, NaN, Inf, finite) of every sky pixel of k_deferred_stream's output against the float64
    model's (tests/test_lighting_sky_cpu.py prints the table; a case may name single pixels where fp32 coincidences decide).
    Both are printed before the comparison."""
    case = _case(cases, name)
    got = sc.classify(_rgb(_stream(gpu_ctx, planes, case, W, H))[:SKY_ROWS])
    want = sc.model_classes(case, W, H)[:SKY_ROWS]
    count = lambda c: dict(zip(*np.unique(c.astype(str), return_counts=True)))      # noqa: E731
    print(f"{name}: device {count(got)}, float64 model {count(want)}")
    assert (got == want).all(), f"{name}: device {count(got)} against the model's {count(want)}; first {np.argwhere(got != want)[:3].tolist()}"


# ---- the fused entries: a rendered terrain with a horizon in view --------------------------------------------------------------
FW, FH = 256, 144
FUSED_NAMES = _ALL_NAMES


def _terrain_case(name, w, h, sky_pixel):
    eye, tgt = scaled_camera(flythrough_camera(0), 256)
    return _case({c.name: c for c in sc.cases(w, h, sky_pixel, eye, tgt)}, name)


def _pair(ctx, tp, case, w, h):
    """vr_terrain_render + vr_deferred_light with the tracking off: (HdrColor words, the five planes)."""
    ctx.set_plane_tracking(False)
    rt = vr.RenderTargets(ctx).Init(w, h)
    try:
        rt.Clear()
        tp.Render(case.view, case.view, rt, vr.default_render_params(400.0))
        hdr = _light(ctx, rt, case, w, h)
        return hdr, {k: rt.download(k).copy() for k in ("depth", "diffuse", "specular", "normals", "emissive")}
    finally:
        rt.close()
        ctx.set_plane_tracking(True)


def _sky_pixel(ctx, tp, w, h):
    """A sky pixel of the flythrough view, and the proof that the frame has all three kinds of wave."""
    eye, tgt = scaled_camera(flythrough_camera(0), 256)
    rt = vr.RenderTargets(ctx).Init(w, h)
    try:
        v = vr.make_view(eye, tgt, w, h)
        tp.Render(v, v, rt, vr.default_render_params(400.0))
        sky = rt.download("depth") == 1.0
    finally:
        rt.close()
    assert sky.any() and not sky.all(), "the view has no horizon"
    ys, xs = np.nonzero(sky)
    return int(xs[len(xs) // 2]), int(ys[len(ys) // 2])


@pytest.mark.parametrize("w", [FW, 332])
@pytest.mark.parametrize("name", FUSED_NAMES)
def test_the_fused_entries_equal_the_unfused_pair(fx, name, w):
    """A 256^2 terrain under a band of sky, 256 and 332 pixels wide.  Inside sky_is_zero vr_terrain_render_lit (32- and 64-pixel
    tiles) and vr_frame_submit (KEEP, and with the lazy G-buffer) give the unfused pair's HdrColor bit for bit - the pair lit by
    the kernel that always shades.  Outside it vr_frame_submit still does, without fusing, and vr_terrain_render_lit refuses,
    names the pair, and leaves HdrColor's sentinel, the five planes and the region census as they were.
    Then the tiled entries behind a tile pass that left its depth ranges (depth_ranges = 1): vr_deferred_light_tiled (plain lists)
    and _tiled_ex take the ranges (read back), then re-read the depth plane on a second call; inside sky_is_zero their sky pixels
    equal the pair's bit for bit both times; outside it they refuse, HdrColor keeps its sentinel and the ranges are still there
    for the next ordinary call."""
    ctx, tp, h = fx["ctx"], fx["tp"], FH
    case = _terrain_case(name, w, h, _sky_pixel(ctx, tp, w, h))
    want, want_planes = _pair(ctx, tp, case, w, h)
    sky = want_planes["depth"] == 1.0
    if case.kind == "in":
        assert not want[sky][:, :3].any(), f"{name}: a sky pixel of the unfused pair is not +0"
    rp = vr.default_render_params(400.0, assume_cleared=1)
    hdr = vr.HdrImage(ctx, w, h)
    try:
        for tile in (32, 64):
            ctx.set_raster_tile(tile)
            rt = vr.RenderTargets(ctx).Init(w, h)
            try:
                rt.upload("diffuse", np.full((h, w), 0x01020304, np.uint32))
                rt.Clear()
                hdr.upload(np.full(w * h * 4, SENTINEL, np.uint16))
                if case.kind == "in":
                    tp.RenderLit(case.view, rt, rp, case.lights, case.top, case.bottom, hdr)
                    _same(want, _words(hdr, w, h), f"{name}: vr_terrain_render_lit, {tile}-pixel tiles")
                else:
                    with pytest.raises(vr.VrError) as err:
                        tp.RenderLit(case.view, rt, rp, case.lights, case.top, case.bottom, hdr)
                    assert err.value.code == INVALID and "use vr_terrain_render + vr_deferred_light" in str(err.value), str(err.value)
                    assert (_words(hdr, w, h) == SENTINEL).all()
                    census = rt.region_census()
                    assert census["clear"] == census["total"] > 0, census          # the lazy clear is still pending or was applied: all clear
                    assert not rt.download("diffuse").any() and (rt.download("depth") == 1.0).all()
            finally:
                rt.close()
                ctx.set_raster_tile(0)
        for lazy in (0, 1):
            ctx.set_gbuffer_lazy(lazy)
            rt = vr.RenderTargets(ctx).Init(w, h)
            try:
                hdr.upload(np.full(w * h * 4, SENTINEL, np.uint16))
                fr = vr.Frame(tp, rt, rp, case.lights, case.top, case.bottom)
                ctx.timing_enable(2)
                fr.submit(case.view, hdr)
                ctx.synchronize()
                ran = ctx.timing_collect()
                ctx.timing_enable(0)
                assert (FUSED in ran) == (case.kind == "in" and _plain_list(case)), f"{name}: lazy {lazy}: ran {sorted(ran)}"
                _same(want, _words(hdr, w, h), f"{name}: vr_frame_submit, lazy {lazy}")
                for k, a in want_planes.items():
                    assert np.array_equal(a.view(np.uint8), rt.download(k).view(np.uint8)), f"{name}: vr_frame_submit, lazy {lazy}: {k}"
            finally:
                rt.close()
                ctx.set_gbuffer_lazy(1)
        rpr = vr.default_render_params(400.0, assume_cleared=1, depth_ranges=1)
        ordinary = sc.Case("ordinary", "in", vr.make_view(*scaled_camera(flythrough_camera(0), 256), w, h), [vr.reference_sun()])
        for e in (["plain"] if _plain_list(case) else []) + ["ex"]:
            rt = vr.RenderTargets(ctx).Init(w, h)
            try:
                tp.Render(case.view, case.view, rt, rpr)
                if case.kind == "in":
                    for ranges in (True, False):                # the first call consumes the ranges, the second re-reads the depth plane
                        _light(ctx, rt, case, w, h, tiled=e, hdr=hdr)
                        assert _family(ctx) == ("tiled", ranges), f"{name}: tiled ({e}): ran {ctx.last_light_variant()}"
                        got = _words(hdr, w, h)
                        assert np.array_equal(want[sky], got[sky]), f"{name}: tiled ({e}), ranges {ranges}: sky pixels differ from the stream kernel's"
                        assert not (got[..., :3] == SENTINEL).all(-1).any()
                    vr.TiledDeferredLightingPass(ctx).Status()
                else:
                    with pytest.raises(vr.VrError) as err:
                        _light(ctx, rt, case, w, h, tiled=e, hdr=hdr)
                    assert err.value.code == INVALID and "use vr_deferred_light" in str(err.value), str(err.value)
                    assert (_words(hdr, w, h) == SENTINEL).all()
                    _light(ctx, rt, ordinary, w, h, tiled=e, hdr=hdr)
                    assert _family(ctx) == ("tiled", True), f"{name}: the refused call took the depth ranges: {ctx.last_light_variant()}"
            finally:
                rt.close()
    finally:
        hdr.close()


# ---- non-finite values: refused by every entry, no trace ------------------------------------------------------------------------
def _bad_inputs():
    """(what the message must name, a function that returns (view, lights, top, bottom) with one value replaced by `bad`)."""
    sun = vr.reference_sun
    spot = lambda: vr.spot_light((5.0, 10.0, -3.0), (0.3, -1.0, 0.2), 3000.0, 250.0, 20.0, 35.0)      # noqa: E731
    point = lambda: vr.point_light((5.0, 40.0, -3.0), 800.0, 150.0, radius=2.0)                       # noqa: E731
    fields = {"sun": (sun, ["direction", "color", "intensity", "angular_size_or_inv_range", "out_of_bounds_shadow"]),
              "point": (point, ["position", "color", "intensity", "angular_size_or_inv_range", "radius"]),
              "spot": (spot, ["direction", "position", "color", "intensity", "angular_size_or_inv_range", "radius", "inner_angle", "outer_angle"])}
    out = []
    for kind, (make, names) in fields.items():
        for f in names:
            def build(bad, make=make, f=f):
                l = make()
                if f in ("direction", "position", "color"):
                    getattr(l, f)[1] = bad
                else:
                    setattr(l, f, bad)
                return None, [vr.reference_sun(), l], AMBIENT_TOP, AMBIENT_BOTTOM
            out.append((f"{kind}.{f}", "light." + f, build))
    for c in range(3):
        out.append((f"ambient_top[{c}]", "ambient_top", lambda bad, c=c: (None, [vr.reference_sun()], tuple(bad if k == c else x for k, x in enumerate(AMBIENT_TOP)), AMBIENT_BOTTOM)))
        out.append((f"ambient_bottom[{c}]", "ambient_bottom", lambda bad, c=c: (None, [vr.reference_sun()], AMBIENT_TOP, tuple(bad if k == c else x for k, x in enumerate(AMBIENT_BOTTOM)))))
    out.append(("camera_pos", "view.camera_pos", lambda bad: (("camera_pos", 1, bad), [vr.reference_sun()], AMBIENT_TOP, AMBIENT_BOTTOM)))
    out.append(("clip_to_world", "view.clip_to_world", lambda bad: (("clip_to_world", 9, bad), [vr.reference_sun()], AMBIENT_TOP, AMBIENT_BOTTOM)))
    return out


def test_non_finite_values_are_refused_by_every_entry_and_leave_no_trace(fx, shadow_map):
    """NaN, +Inf and -Inf in turn in every field of every light type that the type reads, in each ambient channel, in camera_pos
    and in one clip_to_world entry: vr_deferred_light, _shadowed, _tiled (fields of lights it takes), _tiled_ex,
    vr_terrain_render_lit and vr_frame_submit (fused, and tiled = 2) answer VR_ERR_INVALID_ARGUMENT and name the field.  HdrColor
    keeps its sentinel, a pending lazy clear stays pending (the planes read as cleared, every region counts as clear), the depth
    ranges a tile pass left are still taken by the next tiled pass, and the next ordinary call gives the ordinary frame."""
    ctx, tp = fx["ctx"], fx["tp"]
    w, h = FW, FH
    eye, tgt = scaled_camera(flythrough_camera(0), 256)
    rp = vr.default_render_params(400.0, assume_cleared=1)
    rt = vr.RenderTargets(ctx).Init(w, h)
    hdr = vr.HdrImage(ctx, w, h)
    hdr.upload(np.full(w * h * 4, SENTINEL, np.uint16))
    rt.upload("diffuse", np.full((h, w), 0x01020304, np.uint32))
    rt.Clear()                                                  # lazy: pending through every refusal below
    stream, tiled = vr.DeferredLightingPass(ctx), vr.TiledDeferredLightingPass(ctx)
    calls = 0
    try:
        for what, names, build in _bad_inputs():
            for bad in (float("nan"), float("inf"), float("-inf")):
                patch, lights, top, bottom = build(bad)
                v = vr.make_view(eye, tgt, w, h)
                if patch:
                    getattr(v, patch[0])[patch[1]] = patch[2]
                plain = all(l.type == vr.capi.VR_LIGHT_DIRECTIONAL or (l.type == vr.capi.VR_LIGHT_POINT and l.radius == 0.0) for l in lights)
                entries = {"vr_deferred_light": lambda: stream.Render(v, rt, lights, top, bottom, hdr),
                           "vr_deferred_light_shadowed": lambda: stream.Render(v, rt, lights, top, bottom, hdr, shadow_map=shadow_map),
                           "vr_deferred_light_tiled_ex": lambda: tiled.Render(v, rt, lights, top, bottom, hdr, all_light_types=True, shadow_map=shadow_map),
                           "vr_terrain_render_lit": lambda: tp.RenderLit(v, rt, rp, lights, top, bottom, hdr),
                           "vr_frame_submit": lambda: vr.Frame(tp, rt, rp, lights, top, bottom).submit(v, hdr),
                           "vr_frame_submit (tiled = 2)": lambda: vr.Frame(tp, rt, rp, lights, top, bottom, tiled=2, shadow_map=shadow_map).submit(v, hdr)}
                if plain:
                    entries["vr_deferred_light_tiled"] = lambda: tiled.Render(v, rt, lights, top, bottom, hdr)
                for entry, call in entries.items():
                    with pytest.raises(vr.VrError) as err:
                        call()
                    assert err.value.code == INVALID and names in str(err.value), f"{entry}, {what} = {bad}: {err.value}"
                    calls += 1
        assert calls >= 3 * 6 * 26
        assert (_words(hdr, w, h) == SENTINEL).all(), "a refused call wrote HdrColor"
        census = rt.region_census()
        assert census["clear"] == census["total"] > 0, census
        assert not rt.download("diffuse").any() and (rt.download("depth") == 1.0).all()
        # the next ordinary frame is the ordinary frame
        case = sc.Case("ordinary", "in", vr.make_view(eye, tgt, w, h), [vr.reference_sun()])
        want, want_planes = _pair(ctx, tp, case, w, h)
        vr.Frame(tp, rt, rp, case.lights, case.top, case.bottom).submit(case.view, hdr)
        _same(want, _words(hdr, w, h), "the frame after the refusals")
        for k, a in want_planes.items():
            assert np.array_equal(a.view(np.uint8), rt.download(k).view(np.uint8)), k
        # depth ranges: left by a tile pass, still VALID behind a refused tiled call - the lists equal those of a sequence without it
        lights = [vr.reference_sun()] + [vr.point_light((10.0 * i - 60.0, 30.0, 7.0 * i - 40.0), 50.0, 25.0) for i in range(12)]
        nan_lights = list(lights)
        nan_lights[3] = vr.point_light((float("nan"), 30.0, 0.0), 50.0, 25.0)
        rpr = vr.default_render_params(400.0, assume_cleared=1, depth_ranges=1)
        v, v2 = vr.make_view(eye, tgt, w, h), vr.make_view(*scaled_camera(CAMERAS[5], 256), w, h)

        def sequence(with_refused_call):
            g = vr.RenderTargets(ctx).Init(w, h)
            try:
                tp.Render(v, v, g, rpr)
                if with_refused_call:
                    with pytest.raises(vr.VrError):
                        tiled.Render(v, g, nan_lights, AMBIENT_TOP, AMBIENT_BOTTOM, hdr)
                tiled.Render(v, g, lights, AMBIENT_TOP, AMBIENT_BOTTOM, hdr)
                tp.Render(v2, v2, g, rpr)
                tiled.Render(v2, g, lights, AMBIENT_TOP, AMBIENT_BOTTOM, hdr)
                tiled.Status()
                return {(x, y): tiled.tile_light_list(x, y).tolist() for y in range((h + 31) // 32) for x in range(w // 32)}, _words(hdr, w, h)
            finally:
                g.close()
        la, ha = sequence(True)
        lb, hb = sequence(False)
        assert la == lb and any(len(m) < len(lights) for m in lb.values())
        _same(hb, ha, "tiled lighting behind a refused tiled call")
    finally:
        hdr.close(); rt.close()
