"""CPU test of the lighting pass's host plan (vrenderer_amd/csrc/vr_light_plan.h) through tests/host/light_plan_check.cpp."""
import re

import pytest

from tests.host_check import build_host_check, run_host_check


@pytest.mark.parametrize("sanitize", [False, True])
def test_light_plan_matches_the_transcribed_launch_sites_and_invariants(tmp_path, sanitize):
    """vr_light_plan.h compiles without HIP.  For every combination of its boolean inputs and the three entry points, over light
    counts 0, 1, VR_TILE_LIGHT_CAP, VR_TILE_LIGHT_CAP + 1 and 65536, a rank that owns nothing or something and six frame sizes,
    light_plan() and light_width_ok() name the kernel instantiation, grids, list layout and refusal that the launch sites of
    deferred_light and deferred_light_tiled held written out, keep the invariants of tests/host/light_plan_check.cpp against a
    table of each variant's compiled-in flags, and every enum value is chosen by some input.  Over the same inputs with
    sky_not_zero set (vr_light_domain.h) the streaming pass gets the plan of the same call with nothing known about the planes -
    k_deferred_stream or k_deferred_scalar, never k_deferred - and both tiled entry points are refused.  Once more as the same
    stand-alone program under the address and undefined-behaviour sanitizers."""
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    r = run_host_check(build_host_check(tmp_path, "light_plan_check", extra, "light_plan_check_san" if sanitize else None))
    # 3 entry points x 2^7 bools x 5 light counts x 2 owner-tile counts x 3 sizes per width class; of the half whose width is no
    # multiple of 4 the tiled passes refuse all and the streaming pass the packed half: 5/12 of the cases
    m = re.search(r"(\d+) cases \((\d+) refused widths", r.stdout)
    assert m and int(m.group(1)) == 11520 and int(m.group(2)) == 11520 * 5 // 12, r.stdout[-400:]
    # with sky_not_zero: the 7/12 with an accepted width, of which the tiled entry points' share (their 1/2 of 2/3 = 4/7) is refused
    m = re.search(r"outside sky_is_zero: (\d+) accepted widths \((\d+) refused", r.stdout)
    assert m and int(m.group(1)) == 11520 * 7 // 12 and int(m.group(2)) == 11520 // 3, r.stdout[-400:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-2000:]
