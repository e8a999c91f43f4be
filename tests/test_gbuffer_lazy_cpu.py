"""VR_OPT_GBUFFER_LAZY without a GPU: the option's value in the header and its mirrors, and the state and policy code
(vr_gbuffer_state.h, vr_raster_plan.h) against a model that keeps whole eager copies (tests/host/gbuffer_lazy_check.cpp), once more
under the address and undefined-behaviour sanitizers as a stand-alone program."""
import os
import re

import pytest

import vrenderer_amd as vr
from tests.host_check import build_host_check, run_host_check
from vrenderer_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_option_is_declared_and_mirrored(product_lib):
    header = open(os.path.join(ROOT, "include", "vrterrain.h")).read()
    assert re.search(r"VR_OPT_GBUFFER_LAZY = 7\b", header) and capi.VR_OPT_GBUFFER_LAZY == 7
    assert "VR_OPT_GBUFFER_LAZY" in open(os.path.join(ROOT, "include", "vrterrain.hpp")).read() and hasattr(vr.Context, "set_gbuffer_lazy")
    assert product_lib.vr_context_set_option(None, capi.VR_OPT_GBUFFER_LAZY, 0) != 0
    assert "ctx is NULL" in product_lib.vr_last_error().decode()
    assert capi.VR_K_COUNT == product_lib.vr_timing_kernel_count() == 22      # a materialisation is timed under the tile pass's own id


@pytest.fixture(scope="module")
def lazy_check(tmp_path_factory):
    return build_host_check(tmp_path_factory.mktemp("gbuffer_lazy"), "gbuffer_lazy_check")


def test_lazy_state_holds_against_the_eager_model(lazy_check, tmp_path):
    """40,000 random sequences of 24 calls (frames, readers, partial writers, clears, uploads, edits, resizes, option flips,
    refused materialisations) on two targets and two terrains: at every reader nothing is pending and planes, depth, census
    and plane knowledge are the eager model's; sticky-off holds; a terrain holds exactly the target whose record names it; a refused call changes nothing.  Every path is reached."""
    r = run_host_check(lazy_check, expect=" cases, 0 failures")
    assert "40000 sequences, 960000 cases" in r.stdout, r.stdout[-400:]
    counts = dict(re.findall(r"(\w+) (\d+)", r.stdout.splitlines()[-2]))
    for path in ("lazy_frames", "materialised", "replaced", "refused"):
        assert int(counts[path]) > 1000, (path, r.stdout[-400:])
    san = build_host_check(tmp_path, "gbuffer_lazy_check", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "gbuffer_lazy_check_san")
    run_host_check(san, "4000", timeout=300, expect=" cases, 0 failures", stderr_tail=4000)


@pytest.mark.parametrize("rule", [1, 2, 3, 4, 5, 6])
def test_the_check_notices_a_broken_rule(lazy_check, rule):
    """With one of the host's rules broken (an edit, the census or an upload that does not materialise, a partial writer that
    replaces the record, a forgotten sticky-off, a terrain left holding a target whose record names another terrain) the same
    sequences report failures."""
    r = run_host_check(lazy_check, "break", str(rule), expect="broken rule: ")
    assert int(re.search(r"(\d+) failures", r.stdout).group(1)) > 0, r.stdout[-400:]
