"""The inputs of tests/test_tiled_ex_f64.py, proven on the CPU: for every (frame, light list, shadow) combination that module
runs through the all-light-type tiled kernels, the fp32 oracle (oracle/vr_oracle.c) goes through the same float64 reference,
the same check, the same caps and the same masks (f64_shading.TiledCase).  The caps are conditions on the input: where the oracle
alone left a class cap or the bound, the lights or the mask were moved, never a cap.  Needs the oracle and the model only."""
import numpy as np
import pytest

import vrenderer_amd as vr
from tests import f64_shading as fs
from tests.common import AMBIENT_BOTTOM, AMBIENT_TOP, CAMERAS, params, scaled_camera

AMBIENT = (AMBIENT_TOP, AMBIENT_BOTTOM)


def _surface_distance(case):
    """The least distance of a positional light from a reconstructed surface point of the checked pixels."""
    p = case.pix
    wp = fs.world_position(case.view, case.w, case.h, p.px, p.py, p.depth)
    pos = np.array([l.position[:3] for l in case.lights if l.type != fs.VR_LIGHT_DIRECTIONAL], np.float64)
    return min(float(np.sqrt(((wp - q) ** 2).sum(-1)).min()) for q in pos)


@pytest.mark.parametrize("lights_name", ["extra", "all", "tiled"])
@pytest.mark.parametrize("width", [512, 508])
def test_oracle_on_the_edge_case_frame(oracle, width, lights_name):
    """Cases 1 and 2: the edge-case frame at 512 and at 508 (a last light-tile column of 28 pixels) under `extra`, the 13
    lights suns + points + extra, and - for vr_deferred_light_tiled - suns + points; EDGE_CAPS, more than 90 % checked."""
    case = fs.tiled_edge_case(vr, AMBIENT, width, lights_name)
    facts = fs.plan_facts(case.lights)
    assert facts["extra"] == facts["cone"] == (lights_name != "tiled")
    assert len(case.lights) == dict(extra=5, all=13, tiled=8)[lights_name]
    got = case.oracle_frame(oracle)
    case.check(got, "oracle")
    c0, c1 = case.rows["cleared"]
    assert (got[c0:c1] == 0).all() and not np.signbit(got[c0:c1]).any()
    if lights_name != "extra":                                   # (no light of `extra` reaches the far plane)
        y0 = case.rows["far_plane"][0]
        amb = fs.reference(fs.Pixels.from_planes(case.planes, np.arange(width), np.full(width, y0)), case.view, [], *AMBIENT)["ref"]
        assert (np.abs(got[y0] - amb) > 1e-3).mean() > 0.2, "texels at depth 1.0 with real planes are lit"


@pytest.mark.parametrize("lists,w_scale", [("sun_first", 1.0), ("sun_first", 2.0), ("sun_second", 1.0), ("twice", 1.0),
                                           ("all_types", 1.0), ("crowd", 1.0)])
def test_oracle_on_the_pcf_frame(oracle, lists, w_scale):
    """Cases 3 to 6: the exact-geometry PCF frame with the shadowed sun first, second, and fourth of four; with one light
    of every kind around it; and behind 300 weak lights over one light tile (a mask of 4096 pixels).  More than 99 %
    checked, default caps, every coverage key hit on the whole frames."""
    case = fs.tiled_pcf_case(vr, AMBIENT, lists, w_scale)
    li = case.shadow[2]
    assert case.lights[li].type == fs.VR_LIGHT_DIRECTIONAL and case.lights[li].out_of_bounds_shadow == 1.0
    facts = fs.plan_facts(case.lights)
    got = case.oracle_frame(oracle)
    case.check(got, "oracle")
    if lists in ("all_types", "crowd"):
        assert facts["extra"] and facts["cone"]
        assert _surface_distance(case) >= 5.0
    if lists == "all_types":
        assert facts["kinds"] == fs.ALL_KINDS
    if lists == "sun_second":
        # the index matters: the same list with the other light shadowed is another frame
        lv, smap, _, bias = case.shadow
        other = fs.TiledCase("", case.view, case.planes, case.lights, AMBIENT, shadow=(lv, smap, 0, bias)).oracle_frame(oracle)
        assert (np.abs(other - got) > 1e-2).mean() > 0.1
    if lists == "crowd":
        assert len(case.lights) == fs.PCF_CROWD_N + 2 and li == len(case.lights) - 1 and len(case.pix) == 4096
        # the sun's shadow term shows on the checked pixels: against the same list unshadowed, far beyond a tolerance
        plain = fs.TiledCase("", case.view, case.planes, case.lights, AMBIENT).oracle_frame(oracle)
        d = np.abs(plain - got)[case.pix.py, case.pix.px]
        assert (d > 1e-2).any(-1).sum() > 500
        # ... and so do the 300 lights
        bare = fs.TiledCase("", case.view, case.planes, [case.lights[0], case.lights[-1]], AMBIENT,
                            shadow=case.shadow[:2] + (1,) + case.shadow[3:]).oracle_frame(oracle)
        hot = (case.pix.px // 32 == fs.PCF_CROWD_TILE[0]) & (case.pix.py // 32 == fs.PCF_CROWD_TILE[1])
        assert (np.abs(bare - got)[case.pix.py, case.pix.px][hot] > 1e-2).any(-1).mean() > 0.5


def test_oracle_on_the_terrain_frame(oracle):
    """Case 7: the 256^2 terrain at 256x144 from CAMERAS[7] (terrain and sky) under the 40 lights of all_type_lights; default caps."""
    w, h, size = 256, 144, 256
    hm = oracle.synth_heightmap(size)
    t = oracle.OracleTerrain(params(size), hm, oracle.synth_albedo(size, hm))
    view = vr.make_view(*scaled_camera(CAMERAS[7], size), w, h)
    gb = oracle.GBufferHost(w, h)
    t.render(view, gb, vr.default_render_params(400.0))
    planes = {k: np.array(getattr(gb, k)).reshape((h, w) + ((4,) if k in ("normals", "emissive") else ())) for k in ("depth", "diffuse", "specular", "normals", "emissive")}
    t.close()
    covered = planes["depth"] < 1.0
    assert 0.5 < covered.mean() < 0.8, "terrain and sky"
    case = fs.tiled_terrain_case(vr, AMBIENT, view, planes)
    facts = fs.plan_facts(case.lights)
    assert len(case.lights) == 40 and facts["extra"] and facts["cone"] and facts["kinds"] >= fs.ALL_KINDS
    case.check(case.oracle_frame(oracle), "oracle")
