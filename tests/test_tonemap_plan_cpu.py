"""CPU test of the tone-map stage's host plan (vrenderer_amd/csrc/vr_tonemap_plan.h) through tests/host/tonemap_plan_check.cpp."""
import re

import pytest

from tests.host_check import build_host_check, run_host_check


@pytest.mark.parametrize("sanitize", [False, True])
def test_tonemap_plan_matches_the_transcribed_checks_and_launch_sites(tmp_path, sanitize):
    """vr_tonemap_plan.h compiles without HIP.  For the four vr_tonemap_* entry points and vr_frame_submit's stage, packed and
    row-major, over 34 frame sizes (widths of both classes, pixel counts on both sides of 2^26 and 2^32 - 1, two that are no
    size), a rank that owns nothing, one tile or the most, both capacities one byte under and at their limits, each parameter
    condition violated alone and every presence / absence combination of the pointers, tm_refusal() names the message the
    parent's code reported first and tm_plan() the kernel family, both grids, the block count, `launch` and Q of its launch
    sites; every refusal and every family is produced by some input, and a refused input never yields a plan that launches.
    Once more as the same stand-alone program under the address and undefined-behaviour sanitizers."""
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    r = run_host_check(build_host_check(tmp_path, "tonemap_plan_check", extra, "tonemap_plan_check_san" if sanitize else None))
    # 2 layouts x 34 sizes x 3 owner-tile counts x 4 capacity pairs x 6 parameter sets, times the boolean facts: ldr, device, tables
    # and - the four entry points - tone mapper, image (2^5 each), or - the frame - communicator, gathered, ldr_frame, RCCL (2^7)
    m = re.search(r"(\d+) cases \((\d+) accepted\)", r.stdout)
    assert m and int(m.group(1)) == 2 * 34 * 3 * 4 * 6 * (4 * 2 ** 5 + 2 ** 7) and int(m.group(2)) > 0, r.stdout[-400:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-2000:]
