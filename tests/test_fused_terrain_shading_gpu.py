"""The TERRAIN flavour of the shading in the fused resolve of k_raster (vr_deferred_dev.h, vr_terrain_surface.h): both fused
flavours - vr_frame_submit under VR_OPT_FRAME_FUSION (G-buffer kept) and vr_terrain_render_lit (whole frame and a rank's packed
tiles) - against the unfused pair of passes, which shades every texel with the generic decode.  Every comparison is exact.

Frames of 256x144 and 252x132 (partial edge tiles) on a 256^2 terrain; flythrough views 0 and 7 hold all three kinds of 8 x 32
region at both sizes (checked with the CPU oracle when the views were chosen, asserted here from the downloaded depth plane):
all terrain, all sky, and mixed - the last is where an uncovered pixel is given +0 by lane instead of being shaded."""
import numpy as np
import pytest

import vrenderer_amd as vr
from tests.common import AMBIENT_BOTTOM, AMBIENT_TOP, flythrough_camera, params, scaled_camera, upload_planes

pytestmark = pytest.mark.gpu

FUSED, LIGHTING = "k_raster (fused with lighting)", "k_deferred"
PLANES = ("depth", "diffuse", "specular", "normals", "emissive")
SIZES = [(256, 144), (252, 132)]
VIEWS = (0, 7)
SIZE = 256


@pytest.fixture(scope="module")
def fx(product_lib):
    ctx = vr.Context(0)
    h = vr.synth_heightmap(ctx, SIZE)
    a = vr.synth_albedo(ctx, SIZE, h)
    tp = vr.TerrainPass(ctx, params(SIZE)).Init(h, a)
    yield dict(ctx=ctx, tp=tp, h=h)
    tp.close()
    ctx.close()


def _view(i, w, h):
    return vr.make_view(*scaled_camera(flythrough_camera(i), SIZE), w, h)


def _light_lists(heightmap):
    """The lists the fused path admits (<= 16 lights, directional and punctual, no shadow term)."""
    sun = vr.reference_sun()
    pts = vr.synthetic_point_lights(16, float(SIZE), heightmap, 400.0, seed=9001)
    # a lamp over the middle of the terrain whose range ends inside the frame: pixels within it and pixels beyond it (the
    # attenuation's early-out); any positional light makes the pass reconstruct positions in the exact order (exact_pos)
    lamp = vr.point_light((0.0, 60.0, 0.0), 3000.0, 70.0, (1.0, 0.5, 0.25))
    dirs = [vr.directional_light(d, irradiance=e, angular_size_deg=s, color=c)
            for d, e, s, c in (((0.3, -1.0, 0.1), 0.5, 2.0, (1.0, 0.9, 0.8)), ((0.0, -0.2, -1.0), 0.25, 0.0, (0.2, 0.4, 1.0)),
                               ((1.0, -0.05, 0.0), 0.75, 10.0, (1.0, 1.0, 1.0)), ((-0.5, 0.5, 0.5), 1.0, 0.53, (0.5, 1.0, 0.5)),
                               ((0.1, -1.0, -0.1), 2.0, 30.0, (1.0, 0.2, 0.2)))]
    mixed = [sun, pts[0], dirs[0], pts[1], lamp, dirs[1], pts[2], pts[3], dirs[2], pts[4], pts[5], dirs[3], pts[6], pts[7], dirs[4], pts[8]]
    assert len(mixed) == 16
    return {
        "reference sun": [sun],
        "sun of zero angular size": [vr.directional_light((-0.9, -0.25, 0.35), irradiance=1.0, angular_size_deg=0.0)],
        "sun and a point light with a range": [sun, lamp],
        "sixteen directional and point lights": mixed,
        "a light of intensity 0": [sun, vr.point_light((0.0, 60.0, 0.0), 0.0, 70.0), vr.directional_light((0.3, -1.0, 0.1), irradiance=0.0)],
    }


LIST_NAMES = ["reference sun", "sun of zero angular size", "sun and a point light with a range", "sixteen directional and point lights",
              "a light of intensity 0"]


def _region_kinds(depth):
    """Number of 8-row x 32-pixel regions (a wave's share of a 32-pixel tile) that are all terrain / all sky / mixed."""
    h, w = depth.shape
    cov = depth < 1.0
    k = dict(terrain=0, sky=0, mixed=0)
    for y in range(0, h, 8):
        for x in range(0, w, 32):
            r = cov[y:y + 8, x:x + 32]
            k["terrain" if r.all() else "mixed" if r.any() else "sky"] += 1
    return k


def _submit(fx, fusion, w, h, views, lights):
    """`views` one after the other through vr_frame_submit into fresh targets; per frame everything the frame left behind."""
    ctx, tp = fx["ctx"], fx["tp"]
    ctx.set_frame_fusion(fusion)
    rt, hdr = vr.RenderTargets(ctx).Init(w, h), vr.HdrImage(ctx, w, h)
    fr = vr.Frame(tp, rt, vr.default_render_params(400.0, assume_cleared=1), lights, AMBIENT_TOP, AMBIENT_BOTTOM)
    out = []
    try:
        for v in views:
            hdr.upload(np.full(w * h * 4, 0x3c00, np.uint16))
            ctx.timing_enable(2)
            fr.submit(v, hdr)
            ctx.synchronize()
            ran = ctx.timing_collect()
            ctx.timing_enable(0)
            assert (FUSED in ran) == bool(fusion) and (LIGHTING in ran) != bool(fusion), sorted(ran)
            f = {p: rt.download(p).copy() for p in PLANES}
            f.update(hdr=hdr.download().copy(), census=rt.region_census(), emissive_known_zero=rt.plane_known_zero("emissive"))
            out.append(f)
    finally:
        ctx.set_frame_fusion(1)
        hdr.close()
        rt.close()
    return out


def _same_frames(want, got, what):
    for i, (a, b) in enumerate(zip(want, got)):
        for p in PLANES + ("hdr",):
            x, y = a[p].view(np.uint8), b[p].view(np.uint8)
            assert np.array_equal(x, y), f"{what}: frame {i}, {p} differs in {(x != y).sum()} bytes"
        assert a["census"] == b["census"], f"{what}: frame {i}, region census {a['census']} != {b['census']}"
        assert a["emissive_known_zero"] == b["emissive_known_zero"], f"{what}: frame {i}, emissive plane knowledge"


def _lit_pair(fx, v, w, h, lights, part=None):
    """(HdrColor, depth) of vr_terrain_render + vr_deferred_light and of vr_terrain_render_lit."""
    from vrenderer_amd.passes import partition_info
    ctx, tp = fx["ctx"], fx["tp"]
    rp = vr.default_render_params(400.0, assume_cleared=1)
    rt = vr.RenderTargets(ctx).Init(w, h)
    if part is None:
        imgs, nbytes = [vr.HdrImage(ctx, w, h) for _ in range(2)], None
    else:
        info = partition_info(w, h, part.rank, part.world_size)
        rows = (info["packed_bytes"] + vr.VR_OWNER_TILE * 8 - 1) // (vr.VR_OWNER_TILE * 8)
        imgs, nbytes = [vr.HdrImage(ctx, vr.VR_OWNER_TILE, rows) for _ in range(2)], info["owned"] * 128 * 128 * 6
    try:
        for img in imgs:                                    # (pixels of a partial edge tile outside the frame are never written)
            img.upload(np.zeros(img.width * img.height * 4, np.uint16))
        tp.Render(v, v, rt, rp, part)
        vr.DeferredLightingPass(ctx).Render(v, rt, lights, AMBIENT_TOP, AMBIENT_BOTTOM, imgs[0], part)
        want = (imgs[0].download(nbytes).copy(), rt.download("depth").copy())
        rt.Clear()
        tp.RenderLit(v, rt, rp, lights, AMBIENT_TOP, AMBIENT_BOTTOM, imgs[1], part)
        got = (imgs[1].download(nbytes).copy(), rt.download("depth").copy())
    finally:
        for o in imgs + [rt]:
            o.close()
    return want, got


@pytest.mark.parametrize("w,h", SIZES)
def test_frame_submit_fusion_on_equals_fusion_off(fx, w, h):
    """HdrColor, the five planes, the region census and the emissive plane's knowledge, two consecutive views; every frame holds
    all-terrain, all-sky and mixed regions."""
    views = [_view(i, w, h) for i in VIEWS]
    lights = [vr.reference_sun()]
    off, on = _submit(fx, 0, w, h, views, lights), _submit(fx, 1, w, h, views, lights)
    for i, f in enumerate(off):
        k = _region_kinds(f["depth"])
        assert k["terrain"] > 0 and k["sky"] > 0 and k["mixed"] > 0, f"frame {i}: {k}"
        assert not (f["hdr"].reshape(h, w, 4)[f["depth"] == 1.0] != 0).any(), f"frame {i}: a sky pixel is not +0"
    _same_frames(off, on, f"{w}x{h}")


@pytest.mark.parametrize("w,h", SIZES)
def test_render_lit_equals_render_plus_lighting(fx, w, h):
    """The whole frame and the packed tiles of both ranks of a 2-way split, same views."""
    lights = [vr.reference_sun()]
    for i in VIEWS:
        v = _view(i, w, h)
        for part in (None, vr.Partition(0, 2), vr.Partition(1, 2)):
            what = f"{w}x{h} view {i} part {None if part is None else (part.rank, part.world_size)}"
            (hdr_a, d_a), (hdr_b, d_b) = _lit_pair(fx, v, w, h, lights, part)
            assert np.array_equal(d_a.view(np.uint32), d_b.view(np.uint32)), "depth: " + what
            assert np.array_equal(hdr_a, hdr_b), f"HdrColor differs at {(hdr_a != hdr_b).sum()} halfs: " + what
            if part is None:
                k = _region_kinds(d_a)
                assert k["terrain"] > 0 and k["sky"] > 0 and k["mixed"] > 0, what + f": {k}"


@pytest.mark.parametrize("name", LIST_NAMES)
def test_light_lists_through_both_fused_flavours(fx, name):
    """252x132 (partial edge tiles), view 0.  The list must light something, and - for the lamp - not everything."""
    w, h = 252, 132
    lights = _light_lists(fx["h"])[name]
    v = _view(0, w, h)
    off, on = _submit(fx, 0, w, h, [v], lights), _submit(fx, 1, w, h, [v], lights)
    _same_frames(off, on, name)
    (hdr_a, d_a), (hdr_b, d_b) = _lit_pair(fx, v, w, h, lights)
    assert np.array_equal(d_a.view(np.uint32), d_b.view(np.uint32)), name + ": depth"
    assert np.array_equal(hdr_a, hdr_b), f"{name}: render_lit's HdrColor differs at {(hdr_a != hdr_b).sum()} halfs"
    assert np.array_equal(off[0]["hdr"], hdr_a), name + ": the two unfused references differ"
    cov = off[0]["depth"] < 1.0
    assert off[0]["hdr"].reshape(h, w, 4)[cov].any(), name + ": nothing is lit"
    if name == "sun and a point light with a range":
        sun_only = _submit(fx, 0, w, h, [v], lights[:1])[0]["hdr"].reshape(h, w, 4)
        changed = (sun_only != off[0]["hdr"].reshape(h, w, 4)).any(axis=2)
        assert changed[cov].any() and not changed[cov].all(), f"the lamp reaches {changed[cov].sum()} of {cov.sum()} terrain pixels"
        assert not changed[~cov].any()


def _cleared(w, h):
    return dict(depth=np.ones((h, w), np.float32), diffuse=np.zeros((h, w), np.uint32), specular=np.zeros((h, w), np.uint32),
                normals=np.zeros((h, w, 4), np.uint16), emissive=np.zeros((h, w, 4), np.uint16))


@pytest.mark.parametrize("name", LIST_NAMES)
def test_a_cleared_texel_shades_to_plus_zero(fx, name):
    """What giving an uncovered pixel +0 by lane rests on.  Plane tracking off (nothing is known of the planes: the lighting pass
    reads every texel), each light list, both sizes:
      - a cleared G-buffer: every HdrColor word is 0x0000 - all pixels, no exclusions;
      - the streaming kernel still stores +0 without shading for a wave whose 256 texels ALL read as cleared, so once more with
        one drawn texel in every run of 256 pixels: its wave then runs the model on the 255 cleared texels around it, and
        every word of those is 0x0000 (the drawn texels themselves are lit, and checked to be)."""
    ctx = fx["ctx"]
    lights = _light_lists(fx["h"])[name]
    ctx.set_plane_tracking(0)
    try:
        for w, h in SIZES:
            v = _view(0, w, h)
            for seeded in (False, True):
                planes = _cleared(w, h)
                drawn = np.zeros(w * h, bool)
                if seeded:
                    drawn[5::256] = True
                    planes["depth"].reshape(-1)[drawn] = 0.5
                    planes["diffuse"].reshape(-1)[drawn] = 0xff80c0ff
                    planes["specular"].reshape(-1)[drawn] = 0xff0a0a0a
                    planes["normals"].reshape(-1, 4)[drawn] = (0, 32767, 0, 32767)
                rt, hdr = upload_planes(ctx, planes), vr.HdrImage(ctx, w, h)
                try:
                    hdr.upload(np.full(w * h * 4, 0x3c00, np.uint16))
                    vr.DeferredLightingPass(ctx).Render(v, rt, lights, AMBIENT_TOP, AMBIENT_BOTTOM, hdr)
                    out = hdr.download().view(np.uint16).reshape(w * h, 4)
                finally:
                    hdr.close()
                    rt.close()
                bad = (out[~drawn] != 0).any(axis=1)
                assert not bad.any(), f"{name}, {w}x{h}, seeded {seeded}: {bad.sum()} cleared texels do not shade to +0, first words {out[~drawn][bad][:4]}"
                if seeded:
                    assert out[drawn][:, :3].any(axis=1).all(), f"{name}, {w}x{h}: a drawn texel is not lit"
    finally:
        ctx.set_plane_tracking(1)
