"""GPU tests of the albedo's packed footprint table (vrenderer_amd/csrc/vr_packed.h), which the fused flavours of the tile pass read
with ONE 16-byte fetch per footprint and decode through the sRGB table in LDS, where the unfused and materialising variants go on
reading four decoded texels from the float table.

  1. frames: both fused flavours (vr_frame_submit under VR_OPT_FRAME_FUSION, vr_terrain_render_lit on both tile edges) against the same
     frames of the unfused pair of passes, which runs on the float tables and is anchored to the oracle elsewhere - depth and HdrColor
     byte for byte (vr_frame_submit: the planes, the region census and the plane knowledge as well).  Cameras and what each has to show:
     tests/packed_cases.py; every claim is counted from the oracle's per-pixel LOD and world position and asserted.
  2. freshness: after vr_terrain_edit at an edge and a corner, a brush stroke, a stamp, an undo and a redo the fused frame is the
     unfused one and the table is the model of the device's own chain (tests/packed_model.py).
  3. the table itself, every level and entry with the clamped rim, on a 64^2 and a 67 x 61 map.

Every comparison is exact."""
import numpy as np
import pytest

import vrenderer_amd as vr
from tests import packed_cases as pc
from tests import packed_model as pk
from tests.common import params
from tests.fusion_common import assert_same_bits, assert_same_frames, expect_kernels, render_lit, render_unfused, submit_frames

pytestmark = pytest.mark.gpu

SIZES = (64, 256)
# Both fused entry points fuse where the frame's width is a multiple of four (raster_plan): 333 x 211 runs - and is compared - as the
# unfused pair under either setting, so 332 x 211 stands beside it: the partial edge tiles of both tile edges through the fused kernels.
LIT_FRAMES = pc.FRAMES + ((332, 211),)


@pytest.fixture(scope="module")
def scenes(product_lib, oracle):
    """Per map size: a context of its own (the fusion option is per context), the terrain, the maps and the oracle's terrain."""
    out = {}
    for size in SIZES:
        ctx = vr.Context(0)
        hm, al = pc.maps(size)
        out[size] = dict(ctx=ctx, tp=vr.TerrainPass(ctx, params(size)).Init(hm, al), h=hm, al=al, size=size, ot=pc.oracle_terrain(oracle, size, hm, al))
    yield out
    for fx in out.values():
        fx["tp"].close()
        fx["ot"].close()
        fx["ctx"].close()


def _fused_equals_unfused(fx, views, w, h, what):
    """The three fused launches of one frame list against the unfused pair."""
    lights = [vr.reference_sun()]
    off, on = submit_frames(fx, 0, w, h, views, lights, hdr_fill=0x3c00), submit_frames(fx, 1, w, h, views, lights, hdr_fill=0x3c00)
    expect_kernels(off, False, what)
    expect_kernels(on, w % 4 == 0, what)          # (a frame whose width is no multiple of four is not fused by either entry point)
    assert_same_frames(off, on, f"{what}, vr_frame_submit")
    ctx, tp = fx["ctx"], fx["tp"]
    for i, v in enumerate(views):
        want_hdr, want_depth = render_unfused(ctx, tp, v, w, h, lights)
        assert_same_bits(off[i]["hdr"], want_hdr, f"{what}, view {i}: the two unfused references")
        for tile in (32, 64):
            ctx.set_raster_tile(tile)
            try:
                hdr, depth = render_lit(ctx, tp, v, w, h, lights)
            finally:
                ctx.set_raster_tile(0)
            assert_same_bits(want_depth, depth, f"{what}, view {i}, vr_terrain_render_lit on {tile}-pixel tiles: depth")
            assert_same_bits(want_hdr, hdr, f"{what}, view {i}, vr_terrain_render_lit on {tile}-pixel tiles: HdrColor")
    return off


@pytest.mark.parametrize("name", list(pc.CAMERAS))
@pytest.mark.parametrize("size", SIZES)
def test_fused_frames_on_the_packed_table_equal_unfused_frames_on_the_float_table(scenes, oracle, size, name):
    fx = scenes[size]
    levels = fx["tp"].mip_levels("albedo")
    for w, h in LIT_FRAMES:
        v = pc.view(name, size, w, h)
        claim = pc.claim(name, size, w, h) if (w, h) in pc.FRAMES else None
        if claim is not None:
            f = pc.facts(oracle, fx["ot"], size, v, w, h, levels)
            assert claim(f), f"{size}^2 map, {name}, {w}x{h}: the camera misses its case: {f}"
        off = _fused_equals_unfused(fx, [v], w, h, f"{size}^2 map, {name}, {w}x{h}")
        assert (off[0]["depth"] < 1.0).any(), f"{size}^2 map, {name}, {w}x{h}: nothing drawn"


def test_a_non_square_map(product_lib, oracle):
    """96 x 64 texels over a square world (vr_terrain_create admits it; both maps of one size, so the tile pass takes the fast variant):
    rows of 99 entries, 67 of them - the row pitch and the level sizes differ per axis at every level."""
    ctx = vr.Context(0)
    hm, al = pc.maps(96, 64)
    tp = vr.TerrainPass(ctx, params(64)).Init(hm, al)
    try:
        fx = dict(ctx=ctx, tp=tp, h=hm, size=64)
        for name in ("corner and edges", "grazing"):
            for w, h in LIT_FRAMES:
                off = _fused_equals_unfused(fx, [pc.view(name, 64, w, h)], w, h, f"96x64 map, {name}, {w}x{h}")
                assert (off[0]["depth"] < 1.0).any()
        pk.assert_packed_is_the_model(tp, "96x64 map")
    finally:
        tp.close()
        ctx.close()


# ---- freshness ------------------------------------------------------------------------------------------------------------------------
def _fresh(fx, what):
    """The table is the model of the chain as it is now, and a fused frame that looks at the edited places is the unfused one."""
    pk.assert_packed_is_the_model(fx["tp"], what)
    for name in ("corner and edges", "grazing"):
        w, h = LIT_FRAMES[2]
        _fused_equals_unfused(fx, [pc.view(name, fx["size"], w, h)], w, h, f"{what}: {name}")


def test_the_table_follows_every_kind_of_writer(product_lib, oracle):
    """On a 64^2 map with history on: vr_terrain_edit of the albedo in a rectangle that touches the right edge, one in the lower left
    corner, one of a single inner texel (its halo: the entries in front of it hold it too); a paint stroke; an albedo stamp; undo; redo.
    After each the read-back is the model - so every entry that holds a changed texel was refreshed, the clamped rim included - and it
    differs from the read-back before (the writer did write)."""
    size = 64
    ctx = vr.Context(0)
    hm, al = pc.maps(size)
    tp = vr.TerrainPass(ctx, params(size)).Init(hm, al)
    stamp = None
    try:
        fx = dict(ctx=ctx, tp=tp, h=hm, size=size)
        tp.EnableHistory(8 << 20)
        rng = np.random.default_rng(11)
        last = [pk.assert_packed_is_the_model(tp, "created")]

        def changed(what):
            _fresh(fx, what)
            got = tp.PackedTables()
            assert any((a != b).any() for a, b in zip(got, last[0])), f"{what}: the table did not change"
            last[0] = got

        for what, x, y, ew, eh in (("right edge", 50, 20, 14, 9), ("lower left corner", 0, 57, 5, 7), ("one texel", 31, 8, 1, 1)):
            tp.Edit("albedo", x, y, rng.integers(0, 256, (eh, ew, 4), dtype=np.uint8))
            tp.CommitHistory()
            changed(f"edit, {what}")
        assert tp.Brush("paint", [(5.0, -9.0, 7.5, 0.3, 0.8)], color=(250.0, 10.0, 120.0, 255.0))[2] > 0
        tp.CommitHistory()
        changed("brush stroke")
        stamp = vr.Stamp(ctx, rng.integers(0, 256, (9, 13, 4), dtype=np.uint8))
        assert tp.Stamp("albedo", stamp, -20.0, 24.0, 18.0, 12.0, rotation=0.4)[2] > 0
        tp.CommitHistory()
        changed("stamp")
        before_undo = last[0]
        assert tp.Undo()
        changed("undo")
        assert tp.Redo()
        changed("redo")
        assert all(np.array_equal(a, b) for a, b in zip(last[0], before_undo)), "redo: not the table in front of the undo"
        # a heightmap edit leaves the albedo's table alone
        tp.Edit("height", 3, 3, np.full((5, 5), 9, np.uint8))
        assert all(np.array_equal(a, b) for a, b in zip(tp.PackedTables(), last[0]))
        _fresh(fx, "heightmap edit")
    finally:
        if stamp is not None:
            stamp.close()
        tp.close()
        ctx.close()


# ---- the table itself -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", ((64, 64), (67, 61)))
def test_the_created_table_is_the_model_bit_for_bit(gpu_ctx, oracle, w, h):
    """Every level down to 1 x 1, every entry, the clamped rim included; the heightmap has no such table."""
    import ctypes as C
    from vrenderer_amd import capi
    hm, al = pc.maps(w, h, seed=23)
    tp = vr.TerrainPass(gpu_ctx, params(64)).Init(hm, al)
    try:
        got = pk.assert_packed_is_the_model(tp, f"{w}x{h}")
        assert got[0].shape == (h + 3, w + 3, 4) and got[-1].shape == (4, 4, 4) and len(got) == tp.mip_levels("albedo")
        dims = (C.c_int32 * 2)(-1, -1)
        assert gpu_ctx.lib.vr_debug_terrain_tables(tp.handle, 0, capi.VR_DEBUG_TABLE_PACK, 0, dims, None, 0) == capi.VR_OK and list(dims) == [0, 0]
    finally:
        tp.close()
