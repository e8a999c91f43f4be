"""The first light of the list in the fused resolve of k_raster (LightFirst, vr_deferred_dev.h): read once per workgroup and
shaded in front of the loop over lights 1 .. n - 1.  Both fused flavours - vr_frame_submit under VR_OPT_FRAME_FUSION (G-buffer
kept) and vr_terrain_render_lit - against the unfused pair of passes, element for element: nothing here has a tolerance.

Frames of 96x64 (whole 32-pixel tiles), 70x50 and 68x50 (partial last tile column and row) on a 64^2 terrain.  The tile pass
fuses only where the frame's width is a multiple of four (vr_raster_plan.h), so a 70-pixel row is queued as the unfused pair
with fusion on as well - that frame is held to the same equality, and to that fact; 68x50 is the partial-tile frame whose
pixels the fused kernel shades.  The view is the first
of the flythrough's whose frame holds all three kinds of 8 x 32 region (a wave's share of a tile): all terrain, all sky, mixed;
that one exists is asserted.  The unfused frames are rendered once per size and light list and shared."""
import numpy as np
import pytest

import vrenderer_amd as vr
from tests.common import flythrough_camera, scaled_camera
from tests.fusion_common import (PLANES, assert_same_bits, assert_same_frame, expect_kernels, region_kinds, render_lit,
                                 submit_frames, terrain_fixture)

pytestmark = pytest.mark.gpu

SIZES = [(96, 64), (70, 50), (68, 50)]
SIZE = 64
MAX_HEIGHT = 400.0


@pytest.fixture(scope="module")
def fx(product_lib):
    with terrain_fixture(SIZE) as f:
        yield dict(f, views={}, unfused={})


def _sun():
    return vr.reference_sun()


def _lamp():
    """Over the middle of the terrain, no range limit (inv_range = 0)."""
    return vr.point_light((0.0, 60.0, 0.0), 3000.0, 0.0, (1.0, 0.5, 0.25))


def _ranged_lamp():
    """A range that ends inside the frame."""
    return vr.point_light((2.0, 40.0, -3.0), 2000.0, 45.0, (0.3, 0.6, 1.0))


def _far_lamp():
    """Five thousand units above a 64-unit world with a range of 10: the attenuation is 0 at every pixel."""
    return vr.point_light((0.0, 5000.0, 0.0), 3000.0, 10.0, (1.0, 1.0, 1.0))


def _sixteen(heightmap):
    pts = vr.synthetic_point_lights(8, float(SIZE), heightmap, MAX_HEIGHT, seed=9001)
    dirs = [vr.directional_light(d, irradiance=e, angular_size_deg=s, color=c)
            for d, e, s, c in (((-0.9, -0.25, 0.35), 1.0, 0.53, (1.0, 1.0, 1.0)), ((0.3, -1.0, 0.1), 0.5, 2.0, (1.0, 0.9, 0.8)),
                               ((0.0, -0.2, -1.0), 0.25, 0.0, (0.2, 0.4, 1.0)), ((1.0, -0.05, 0.0), 0.75, 10.0, (1.0, 1.0, 1.0)),
                               ((-0.5, 0.5, 0.5), 1.0, 0.53, (0.5, 1.0, 0.5)), ((0.1, -1.0, -0.1), 2.0, 30.0, (1.0, 0.2, 0.2)),
                               ((0.7, -0.7, 0.0), 0.3, 1.0, (0.9, 0.9, 0.2)), ((-0.2, -0.9, -0.4), 0.1, 5.0, (0.2, 0.9, 0.9)))]
    out = [l for pair in zip(dirs, pts) for l in pair]
    assert len(out) == 16 and out[0].type == vr.VR_LIGHT_DIRECTIONAL and out[1].type == vr.VR_LIGHT_POINT
    return out


LISTS = {
    "a no lights": lambda h: [],
    "b sun": lambda h: [_sun()],
    "c point light without a range": lambda h: [_lamp()],
    "d point light out of range, then sun": lambda h: [_far_lamp(), _sun()],
    "e sun, then point light": lambda h: [_sun(), _ranged_lamp()],
    "f point light, then sun": lambda h: [_ranged_lamp(), _sun()],
    "g sixteen, directional and point alternating": _sixteen,
}
CASES = [(w, h, name) for (w, h) in SIZES for name in LISTS]


def _submit(fx, fusion, w, h, v, lights, expect_fused=None):
    """One frame through vr_frame_submit over an HdrColor of 0x3c00: everything the frame left behind.  Unless told otherwise,
    the fused kernel ran exactly when the option is on and the width is a multiple of four."""
    frames = submit_frames(fx, fusion, w, h, [v], lights, hdr_fill=0x3c00)
    expect_kernels(frames, (bool(fusion) and w % 4 == 0) if expect_fused is None else expect_fused, f"{w}x{h}, fusion {fusion}")
    return frames[0]


def _render_lit(fx, w, h, v, lights):
    """(HdrColor, depth) of vr_terrain_render_lit, whole frame, over an HdrColor of 0x3c00."""
    return render_lit(fx["ctx"], fx["tp"], v, w, h, lights, hdr_fill=0x3c00)


def _view(fx, w, h):
    """The first flythrough view whose frame holds all-terrain, all-sky and mixed regions (from the unfused depth plane)."""
    if (w, h) not in fx["views"]:
        found = None
        for i in range(8):
            v = vr.make_view(*scaled_camera(flythrough_camera(i), SIZE), w, h)
            k = region_kinds(_submit(fx, 0, w, h, v, [])["depth"])
            if k["terrain"] > 0 and k["sky"] > 0 and k["mixed"] > 0:
                found = v
                break
        assert found is not None, f"{w}x{h}: no flythrough view holds all-terrain, all-sky and mixed regions"
        fx["views"][(w, h)] = found
    return fx["views"][(w, h)]


def _unfused(fx, w, h, name):
    """vr_terrain_render + the streaming lighting pass under vr_frame_submit with fusion off: the reference, rendered once."""
    key = (w, h, name)
    if key not in fx["unfused"]:
        f = _submit(fx, 0, w, h, _view(fx, w, h), LISTS[name](fx["h"]))
        for a in f.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        fx["unfused"][key] = f
    return fx["unfused"][key]


@pytest.mark.parametrize("w,h,name", CASES)
def test_keep_flavour_equals_unfused_pair(fx, w, h, name):
    """vr_frame_submit with fusion on: HdrColor, the five planes and the region census are those of the unfused pair."""
    want = _unfused(fx, w, h, name)
    k = region_kinds(want["depth"])
    assert k["terrain"] > 0 and k["sky"] > 0 and k["mixed"] > 0, k
    got = _submit(fx, 1, w, h, _view(fx, w, h), LISTS[name](fx["h"]))
    assert_same_frame(want, got, f"{name}, {w}x{h}", ("hdr",) + PLANES + ("census",))
    cov = want["depth"] < 1.0
    lit = want["hdr"].reshape(h, w, 4)[cov][:, :3].any()
    assert lit, f"{name}: no terrain pixel is lit (the ambient term alone lights them)"


@pytest.mark.parametrize("w,h,name", CASES)
def test_lit_flavour_equals_unfused_pair(fx, w, h, name):
    """vr_terrain_render_lit: HdrColor and depth are those of the unfused pair."""
    want = _unfused(fx, w, h, name)
    hdr, depth = _render_lit(fx, w, h, _view(fx, w, h), LISTS[name](fx["h"]))
    assert_same_bits(want["depth"], depth, f"{name}, {w}x{h}: depth")
    assert_same_bits(want["hdr"], hdr, f"{name}, {w}x{h}: HdrColor")


@pytest.mark.parametrize("w,h", SIZES)
def test_out_of_range_first_light_leaves_the_sun_alone(fx, w, h):
    """List (d): the point light in front reaches no pixel (att == 0 skips that light only), so the frame is the sun's."""
    v = _view(fx, w, h)
    sun = _unfused(fx, w, h, "b sun")
    both = LISTS["d point light out of range, then sun"](fx["h"])
    keep = _submit(fx, 1, w, h, v, both)
    hdr, _ = _render_lit(fx, w, h, v, both)
    n_keep = int((keep["hdr"].view(np.uint16) != sun["hdr"].view(np.uint16)).sum())
    n_lit = int((hdr.view(np.uint16) != sun["hdr"].view(np.uint16)).sum())
    print(f"{w}x{h}: halfs that differ from the sun alone: frame submit {n_keep}, render_lit {n_lit} of {sun['hdr'].size}")
    assert_same_bits(sun["hdr"], keep["hdr"], f"{w}x{h}: frame submit, out-of-range light + sun against the sun alone")
    assert_same_bits(sun["hdr"], hdr, f"{w}x{h}: render_lit, out-of-range light + sun against the sun alone")
    assert sun["hdr"].reshape(h, w, 4)[sun["depth"] < 1.0][:, :3].any()


@pytest.mark.parametrize("kind", ["spot", "sphere"])
def test_spot_or_spherical_first_light_is_queued_unfused(fx, kind):
    """The fused resolve admits directional and punctual lights only: such a list runs the tile pass and the lighting kernel."""
    w, h = SIZES[2]
    first = (vr.spot_light((0.0, 60.0, 0.0), (0.1, -1.0, 0.2), 3000.0, 0.0, 20.0, 35.0) if kind == "spot"
             else vr.point_light((0.0, 60.0, 0.0), 3000.0, 0.0, radius=2.0))
    lights = [first, _sun()]
    v = _view(fx, w, h)
    off = _submit(fx, 0, w, h, v, lights)
    on = _submit(fx, 1, w, h, v, lights, expect_fused=False)          # asserts: k_deferred ran, the fused kernel did not
    assert_same_frame(off, on, f"{kind} first", ("hdr",) + PLANES)
