"""CPU test of the terrain's surface constants (vrenderer_amd/csrc/vr_terrain_surface.h) through tests/host/terrain_surface_check.cpp."""
import re

from tests.host_check import build_host_check, run_host_check


def test_terrain_surface_constants_and_the_facts_the_folds_rest_on(tmp_path):
    """vr_terrain_surface.h compiles without HIP (its static_asserts hold for the host compiler too).  The constants equal
    decode_surface's generic expressions evaluated in float at run time; the normal decode's fmaxf(., -1) is an identity for all
    65,535 codes in [-32767, 32767]; x * 0 + 1 == 1, separately rounded and fused, over a dense sweep of [0, 1] with both
    endpoints, the denormals and the last floats below 1."""
    r = run_host_check(build_host_check(tmp_path, "terrain_surface_check", ["-ffp-contract=off"]))
    m = re.search(r"(\d+) cases", r.stdout)
    assert m and int(m.group(1)) == 11, r.stdout[-400:]           # 7 on the constants, 3 on the normal decode, 1 on the sweep
