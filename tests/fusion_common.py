"""What the GPU tests of the fused frame kernel share: frames through vr_frame_submit with VR_OPT_FRAME_FUSION on or off, which
of the two kernels ran (from the timing records), everything a frame left behind, and comparison bit for bit.  The unfused
pair of passes is the reference throughout."""
import contextlib

import numpy as np

import vrenderer_amd as vr
from tests.common import AMBIENT_BOTTOM, AMBIENT_TOP, CAMERAS, flythrough_camera, packed_hdr, params, scaled_camera

FUSED, LIGHTING = "k_raster (fused with lighting)", "k_deferred"
PLANES = ("depth", "diffuse", "specular", "normals", "emissive")
FRAME_KEYS = PLANES + ("hdr", "census", "emissive_known_zero")


@contextlib.contextmanager
def terrain_fixture(size):
    """A context of the caller's own (the fusion option is per context) with a synthetic size^2 terrain."""
    ctx = vr.Context(0)
    h = vr.synth_heightmap(ctx, size)
    tp = vr.TerrainPass(ctx, params(size)).Init(h, vr.synth_albedo(ctx, size, h))
    try:
        yield dict(ctx=ctx, tp=tp, h=h, size=size)
    finally:
        tp.close()
        ctx.close()


def region_kinds(depth):
    """Number of 8-row x 32-pixel regions (a wave's share of a 32-pixel tile) that are all terrain / all sky / mixed."""
    h, w = depth.shape
    cov = depth < 1.0
    k = dict(terrain=0, sky=0, mixed=0)
    for y in range(0, h, 8):
        for x in range(0, w, 32):
            r = cov[y:y + 8, x:x + 32]
            k["terrain" if r.all() else "mixed" if r.any() else "sky"] += 1
    return k


def download_frame(rt, hdr, nbytes=None):
    """The five planes and HdrColor (its first nbytes) as host copies."""
    f = {p: rt.download(p).copy() for p in PLANES}
    f["hdr"] = hdr.download(nbytes).copy()
    return f


def submit_frames(fx, fusion, w, h, views, lights=None, *, clear=False, before=None, ahead=0, part=None, tiled=False, tile=0,
                  hdr_fill=0, **rpkw):
    """Renders `views` one after the other into fresh targets through vr_frame_submit; per frame: everything the frame left
    behind (FRAME_KEYS) and which of the two kernels ran (`fused`, `lighting`; `ran` holds every timed name).
    hdr_fill is the 16-bit pattern HdrColor holds beforehand.  Zeros are uploaded once: a packed image needs them (pixels of a
    partial edge tile outside the frame are never written), and a later frame starts from what the one before it left.  A
    sentinel such as 0x3c00 is renewed before every frame."""
    ctx, tp = fx["ctx"], fx["tp"]
    lights = [vr.reference_sun()] if lights is None else lights
    rpkw.setdefault("assume_cleared", 1)
    rp = vr.default_render_params(400.0, **rpkw)
    ctx.set_frame_fusion(fusion)
    ctx.set_raster_tile(tile)
    rt = vr.RenderTargets(ctx).Init(w, h)
    hdr, nbytes = (vr.HdrImage(ctx, w, h), None) if part is None else packed_hdr(ctx, w, h, part)
    out = []
    try:
        fr = vr.Frame(tp, rt, rp, lights, AMBIENT_TOP, AMBIENT_BOTTOM, part, tiled)
        for i, v in enumerate(views):
            if i == 0 or hdr_fill:
                hdr.upload(np.full(hdr.width * hdr.height * 4, hdr_fill, np.uint16))
            if clear:
                rt.Clear()
            if before is not None:
                before(i, rt)
            ctx.timing_enable(2)
            fr.submit(v, hdr, views[i + 1:i + 1 + ahead])
            ctx.synchronize()
            ran = ctx.timing_collect()
            ctx.timing_enable(0)
            f = download_frame(rt, hdr, nbytes)
            f.update(census=rt.region_census(), emissive_known_zero=rt.plane_known_zero("emissive"),
                     fused=FUSED in ran, lighting=LIGHTING in ran, ran=sorted(ran))
            assert not (f["fused"] and f["lighting"]), f["ran"]
            out.append(f)
    finally:
        ctx.set_frame_fusion(1)
        ctx.set_raster_tile(0)
        hdr.close()
        rt.close()
    return out


def expect_kernels(frames, fused, what=""):
    """Every frame ran exactly one of the two kernels: the fused tile pass if `fused`, the streaming lighting pass if not."""
    for i, f in enumerate(frames):
        assert f["fused"] == fused and f["lighting"] != fused, f"{what}: frame {i} ran {f['ran']}"


def assert_same_bits(a, b, what):
    x, y = np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8)
    assert x.shape == y.shape, f"{what}: {x.shape} against {y.shape} bytes"
    assert np.array_equal(x, y), f"{what} differs in {(x != y).sum()} bytes"


def assert_same_frame(want, got, what, keys=FRAME_KEYS):
    """Arrays bit for bit, everything else (the region census, what is known of the emissive plane) by equality."""
    for k in keys:
        if isinstance(want[k], np.ndarray):
            assert_same_bits(want[k], got[k], f"{what}, {k}")
        else:
            assert want[k] == got[k], f"{what}, {k}: {want[k]} != {got[k]}"


def assert_same_frames(want, got, what, keys=FRAME_KEYS):
    assert len(want) == len(got), f"{what}: {len(want)} frames against {len(got)}"
    for i, (a, b) in enumerate(zip(want, got)):
        assert_same_frame(a, b, f"{what}: frame {i}", keys)


@contextlib.contextmanager
def _targets(ctx, w, h, part, hdr_fill, rt):
    """The caller's G-buffer or a fresh one, and an HdrColor image holding hdr_fill: whole frame, or `part`'s packed tiles (of
    which only the first nbytes are live)."""
    own = rt is None
    if own:
        rt = vr.RenderTargets(ctx).Init(w, h)
    hdr, nbytes = (vr.HdrImage(ctx, w, h), None) if part is None else packed_hdr(ctx, w, h, part)
    try:
        hdr.upload(np.full(hdr.width * hdr.height * 4, hdr_fill, np.uint16))
        yield rt, hdr, nbytes
    finally:
        hdr.close()
        if own:
            rt.close()


def render_unfused(ctx, tp, v, w, h, lights, part=None, *, rt=None, hdr_fill=0):
    """(HdrColor words, depth) of vr_terrain_render + vr_deferred_light."""
    rp = vr.default_render_params(400.0, assume_cleared=1)
    with _targets(ctx, w, h, part, hdr_fill, rt) as (rt, hdr, nbytes):
        tp.Render(v, v, rt, rp, part)
        vr.DeferredLightingPass(ctx).Render(v, rt, lights, AMBIENT_TOP, AMBIENT_BOTTOM, hdr, part)
        return hdr.download(nbytes).copy(), rt.download("depth").copy()


def render_lit(ctx, tp, v, w, h, lights, part=None, *, rt=None, hdr_fill=0):
    """(HdrColor words, depth) of vr_terrain_render_lit."""
    rp = vr.default_render_params(400.0, assume_cleared=1)
    with _targets(ctx, w, h, part, hdr_fill, rt) as (rt, hdr, nbytes):
        tp.RenderLit(v, rt, rp, lights, AMBIENT_TOP, AMBIENT_BOTTOM, hdr, part)
        return hdr.download(nbytes).copy(), rt.download("depth").copy()


def lit_pair(ctx, tp, v, w, h, lights, part=None):
    """render_unfused, then render_lit into the same G-buffer: ((HdrColor, depth) wanted, (HdrColor, depth) got)."""
    rt = vr.RenderTargets(ctx).Init(w, h)
    try:
        want = render_unfused(ctx, tp, v, w, h, lights, part, rt=rt)
        rt.Clear()                                             # (the fused pass must not depend on what the other planes hold)
        return want, render_lit(ctx, tp, v, w, h, lights, part, rt=rt)
    finally:
        rt.close()


def views(w, h):
    """Two flythrough views (terrain under a band of sky) and the top-down camera (no sky at all)."""
    return [vr.make_view(*scaled_camera(flythrough_camera(0), 256), w, h), vr.make_view(*scaled_camera(CAMERAS[4], 256), w, h),
            vr.make_view(*scaled_camera(flythrough_camera(5), 256), w, h)]


def timed(ctx, fn):
    ctx.timing_enable(2)
    try:
        out = fn()
        ctx.synchronize()
        return out, ctx.timing_collect()
    finally:
        ctx.timing_enable(0)


def capture(rt, hdr):
    f = {p: rt.download(p).copy() for p in PLANES}
    f.update(hdr=hdr.download().copy(), census=rt.region_census(), emissive_known_zero=rt.plane_known_zero("emissive"))
    return f


class LazyScene:
    """Fresh targets and a Frame on the fixture's terrain, with the option set to `lazy`."""

    def __init__(self, fx, lazy, w, h):
        self.ctx, self.tp, self.w, self.h = fx["ctx"], fx["tp"], w, h
        self.ctx.set_gbuffer_lazy(lazy)
        self.rt = vr.RenderTargets(self.ctx).Init(w, h)
        self.hdr, self.hdr2 = vr.HdrImage(self.ctx, w, h), vr.HdrImage(self.ctx, w, h)
        self.rp = vr.default_render_params(400.0, assume_cleared=1)
        self.lights = [vr.reference_sun()]
        self.fr = vr.Frame(self.tp, self.rt, self.rp, self.lights, AMBIENT_TOP, AMBIENT_BOTTOM)

    def submit(self, v, fused=True):
        """One frame; returns the names of the stamped kernels it queued."""
        _, ran = timed(self.ctx, lambda: self.fr.submit(v, self.hdr))
        assert (FUSED in ran) == fused and (LIGHTING in ran) != fused, sorted(ran)
        return ran

    def close(self):
        self.ctx.set_gbuffer_lazy(1)
        for o in (self.hdr, self.hdr2, self.rt):
            o.close()


def both(fx, w, h, script):
    """script(scene, lazy) -> dict of results, with the option off and on; the two must agree bit for bit."""
    outs = []
    for lazy in (0, 1):
        sc = LazyScene(fx, lazy, w, h)
        try:
            outs.append(script(sc, lazy))
        finally:
            sc.close()
    want, got = outs
    assert want.keys() == got.keys()
    for k in want:
        if isinstance(want[k], dict) and "depth" in want[k]:
            assert_same_frame(want[k], got[k], f"{w}x{h}, {k}", [q for q in FRAME_KEYS + ("hdr2",) if q in want[k]])
        elif isinstance(want[k], np.ndarray):
            assert_same_bits(want[k], got[k], f"{w}x{h}, {k}")
        else:
            assert want[k] == got[k], f"{w}x{h}, {k}: {want[k]} != {got[k]}"
    return want, got
