"""VR_OPT_FRAME_FUSION without a GPU: the option's value in the header, in the ctypes mirror and in the C++ wrapper, and the
ABI it must leave alone."""
import os
import re

import pytest

import vrenderer_amd as vr
from vrenderer_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header(name):
    with open(os.path.join(ROOT, "include", name)) as f:
        return f.read()


def test_option_round_trips_between_header_and_mirrors(product_lib):
    opts = dict(re.findall(r"(VR_OPT_[A-Z_]+) = (\d+)", _header("vrterrain.h")))
    assert opts["VR_OPT_FRAME_FUSION"] == "6" and capi.VR_OPT_FRAME_FUSION == 6
    for name, value in opts.items():
        assert getattr(capi, name) == int(value), name
    assert len(set(opts.values())) == len(opts)
    assert "VR_OPT_FRAME_FUSION" in _header("vrterrain.hpp") and hasattr(vr.Context, "set_frame_fusion")
    # the library knows the option: without a context the call fails on the context, not on the option
    assert product_lib.vr_context_set_option(None, capi.VR_OPT_FRAME_FUSION, 0) != 0
    assert "ctx is NULL" in product_lib.vr_last_error().decode()


def test_product_build_and_kernel_ids_are_unchanged(product_lib):
    assert product_lib.vr_build_experiments() == 0
    assert capi.VR_K_COUNT == 22
    m = re.search(r"enum \{ VR_K_SELECT.*?VR_K_COUNT \};", _header("vrterrain.h"), re.S)
    assert m and len(re.findall(r"VR_K_[A-Z_0-9]+", m.group(0))) == capi.VR_K_COUNT + 1
    names = [product_lib.vr_kernel_name(i).decode() for i in range(capi.VR_K_COUNT)]
    assert "k_raster (fused with lighting)" in names and "k_deferred" in names and len(set(names)) == capi.VR_K_COUNT
