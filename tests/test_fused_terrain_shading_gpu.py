"""The TERRAIN flavour of the shading in the fused resolve of k_raster (vr_deferred_dev.h, vr_terrain_surface.h): both fused
flavours - vr_frame_submit under VR_OPT_FRAME_FUSION (G-buffer kept) and vr_terrain_render_lit (whole frame and a rank's packed
tiles) - against the unfused pair of passes, which shades every texel with the generic decode.  Every comparison is exact.

Frames of 256x144 and 252x132 (partial edge tiles) on a 256^2 terrain; flythrough views 0 and 7 hold all three kinds of 8 x 32
region at both sizes (checked with the CPU oracle when the views were chosen, asserted here from the downloaded depth plane):
all terrain, all sky, and mixed - the last is where an uncovered pixel is given +0 by lane instead of being shaded."""
import numpy as np
import pytest

import vrenderer_amd as vr
from tests.common import AMBIENT_BOTTOM, AMBIENT_TOP, flythrough_camera, scaled_camera, upload_planes
from tests.fusion_common import assert_same_frames, expect_kernels, lit_pair, region_kinds, submit_frames, terrain_fixture

pytestmark = pytest.mark.gpu

SIZES = [(256, 144), (252, 132)]
VIEWS = (0, 7)
SIZE = 256


@pytest.fixture(scope="module")
def fx(product_lib):
    with terrain_fixture(SIZE) as f:
        yield f


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


def _submit(fx, fusion, w, h, views, lights):
    """`views` through vr_frame_submit over an HdrColor of 0x3c00; the fused kernel ran exactly when the option is on."""
    frames = submit_frames(fx, fusion, w, h, views, lights, hdr_fill=0x3c00)
    expect_kernels(frames, bool(fusion), f"fusion {fusion}")
    return frames


@pytest.mark.parametrize("w,h", SIZES)
def test_frame_submit_fusion_on_equals_fusion_off(fx, w, h):
    """HdrColor, the five planes, the region census and the emissive plane's knowledge, two consecutive views; every frame holds
    all-terrain, all-sky and mixed regions."""
    views = [_view(i, w, h) for i in VIEWS]
    lights = [vr.reference_sun()]
    off, on = _submit(fx, 0, w, h, views, lights), _submit(fx, 1, w, h, views, lights)
    for i, f in enumerate(off):
        k = region_kinds(f["depth"])
        assert k["terrain"] > 0 and k["sky"] > 0 and k["mixed"] > 0, f"frame {i}: {k}"
        assert not (f["hdr"].reshape(h, w, 4)[f["depth"] == 1.0] != 0).any(), f"frame {i}: a sky pixel is not +0"
    assert_same_frames(off, on, f"{w}x{h}")


@pytest.mark.parametrize("w,h", SIZES)
def test_render_lit_equals_render_plus_lighting(fx, w, h):
    """The whole frame and the packed tiles of both ranks of a 2-way split, same views."""
    lights = [vr.reference_sun()]
    for i in VIEWS:
        v = _view(i, w, h)
        for part in (None, vr.Partition(0, 2), vr.Partition(1, 2)):
            what = f"{w}x{h} view {i} part {None if part is None else (part.rank, part.world_size)}"
            (hdr_a, d_a), (hdr_b, d_b) = lit_pair(fx["ctx"], fx["tp"], v, w, h, lights, part)
            assert np.array_equal(d_a.view(np.uint32), d_b.view(np.uint32)), "depth: " + what
            assert np.array_equal(hdr_a, hdr_b), f"HdrColor differs at {(hdr_a != hdr_b).sum()} halfs: " + what
            if part is None:
                k = region_kinds(d_a)
                assert k["terrain"] > 0 and k["sky"] > 0 and k["mixed"] > 0, what + f": {k}"


@pytest.mark.parametrize("name", LIST_NAMES)
def test_light_lists_through_both_fused_flavours(fx, name):
    """252x132 (partial edge tiles), view 0.  The list must light something, and - for the lamp - not everything."""
    w, h = 252, 132
    lights = _light_lists(fx["h"])[name]
    v = _view(0, w, h)
    off, on = _submit(fx, 0, w, h, [v], lights), _submit(fx, 1, w, h, [v], lights)
    assert_same_frames(off, on, name)
    (hdr_a, d_a), (hdr_b, d_b) = lit_pair(fx["ctx"], fx["tp"], v, w, h, lights)
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
