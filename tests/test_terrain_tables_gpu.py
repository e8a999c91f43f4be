"""GPU tests of the decoded tables themselves - quad, quadf and fast of the heightmap, fast and rgbf of the albedo, per mip level -
read back with vr_debug_terrain_tables (TerrainPass.Tables) and held to tests/tables_model.py bit for bit: after create, and after
in-place refreshes at the places where a refresh goes wrong.  Every frame's tile pass and every height query read the terrain through
these tables, yet frames and samples see only the entries some pixel or point happens to select: a stale entry at a coarse level's
clamped rim, an entry just outside a dirty rectangle, a wrong quad beside a right quadf, or a wrong table of the raster variant the
terrain does not take, show in none of them.

Every comparison is against the model applied to the device's own level (download_mip), level by level, so mip rounding is not in
question; floats are compared as uint32 and no tolerance appears anywhere."""
import ctypes as C

import numpy as np
import pytest

import vrenderer_amd as vr
from vrenderer_amd import capi
from tests import frontend_common as fc
from tests import tables_model as tm
from tests.common import params
from tests.level0_common import Maps, Scene

pytestmark = pytest.mark.gpu

REFRESH_SCENES = ("odd", "fast64")               # 67x45 + 33x50 (odd, ragged at every level, the general raster variant) and 64x64 + 64x64
WHICH = tm.WHICH
read_tables, assert_tables_are_the_model, assert_tables_equal, tables_differ = tm.read_tables, tm.assert_tables_are_the_model, tm.assert_tables_equal, tm.tables_differ


# ---- 1. created terrains ------------------------------------------------------------------------------------------------------------------
def _created_cases(gpu_ctx):
    maps = [fc.random_texture(w, h, fc.CREATE_SEED) for w, h in fc.CREATE_SHAPES]
    cases = [(f"{w}x{h}", maps[k][0], maps[(k + 1) % len(maps)][1], fc.CREATE_WORLD) for k, (w, h) in enumerate(fc.CREATE_SHAPES)]
    for name in ("odd", "fast64", "multi"):
        sc = Scene(gpu_ctx, name)
        cases.append((name, sc.hm, sc.al, sc))
    return cases


def test_a_created_terrain_s_tables_are_the_model_bit_for_bit(gpu_ctx):
    """The CREATE_SHAPES maps paired as in tests/test_terrain_create_gpu.py (1x1, 5x5, 7x2, 2x7, 33x17: heightmap k under the albedo of
    shape k + 1) and the odd (67x45 / 33x50), fast64 and multi (128^2, 2 x 2 surfaces) scenes of the edit tests: for every level of
    both maps every table has the model's shape and bits - out to the clamped rim, whichever raster variant the pair takes."""
    for name, hm, al, sc in _created_cases(gpu_ctx):
        tp = vr.TerrainPass(gpu_ctx, sc.p if isinstance(sc, Scene) else params(sc)).Init(hm, al)
        try:
            assert np.array_equal(tp.download_mip("height", 0), hm) and np.array_equal(tp.download_mip("albedo", 0), al)
            got = assert_tables_are_the_model(tp, name)
            (h, w), (ah, aw) = hm.shape, al.shape[:2]
            assert got["height"][0]["quad"].shape == (h + 2, w + 2) and got["height"][0]["fast"].shape == (h + 3, w + 3, 4)
            assert got["albedo"][0]["rgbf"].shape == (ah, aw, 4) and got["albedo"][0]["fast"].shape == (ah + 3, aw + 3, 4)
            assert sorted(got["height"][-1]) == ["fast", "quad", "quadf"] and got["height"][-1]["quad"].shape == (3, 3)
            assert sorted(got["albedo"][-1]) == ["fast", "rgbf"] and got["albedo"][-1]["rgbf"].shape == (1, 1, 4)
        finally:
            tp.close()


# ---- 2. in-place refresh where it goes wrong ---------------------------------------------------------------------------------------------
def refresh_rectangles(w, h):
    """(name, x, y, ew, eh) of the level-0 rectangles of a w x h map that are filled and restored:
      - pyramid_model.refresh_edits, cut to the map: corners, the odd last column and row alone (an empty level-1 rectangle), a column,
        a row, 7 x 9;
      - single texels 30 .. 33 by 6 .. 9, all sixteen: entries either side of column 32 and row 8 of the tables kernel's 32 x 8 workgroups
        in ENTRY space (entry = texel + 0 or + 1) at level 0, and the level-0 texels (2x, 2y) that carry the four diagonal ones to level 1,
        where the map has them.  (The workgroups tile a level's dirty entries from the rectangle's first entry, so a single texel is one
        workgroup per level: what these hold is the entry arithmetic around those indices, the rectangle below the tiling itself);
      - a texel whose dirty span ends exactly at w - 1 (texel w - 2: the rim entries need no refresh) and one whose span ends at w
        (texel w - 1: entries w, w + 1 and w + 2 all read it), on both axes;
      - a rectangle of 41 x 27 texels at (13, 9), cut to the map: on a 64 x 64 map 2 x 4 workgroups at level 0, 1 x 2 at level 1, one at each
        level below - at least three levels with non-empty spans and another first_block for each, so the workgroup-to-level lookup and
        the 32 x 8 tiling are exercised."""
    out = tm.refresh_rectangles(w, h)
    out += [(f"texel ({x}, {y})", x, y, 1, 1) for y in (6, 7, 8, 9) for x in (30, 31, 32, 33) if x < w and y < h]
    out += [(f"texel ({2 * x}, {2 * y}), level-1 texel ({x}, {y})", 2 * x, 2 * y, 1, 1) for x, y in ((30, 6), (31, 7), (32, 8), (33, 9)) if 2 * x < w and 2 * y < h]
    out += [("span ends at w - 1", w - 2, h // 2, 1, 1), ("span ends at w", w - 1, h // 2, 1, 1),
            ("span ends at h - 1", w // 2, h - 2, 1, 1), ("span ends at h", w // 2, h - 1, 1, 1)]
    out.append(("41 x 27 at (13, 9)", 13, 9, min(41, w - 13), min(27, h - 9)))
    return out


@pytest.mark.parametrize("which", WHICH)
@pytest.mark.parametrize("name", REFRESH_SCENES)
def test_in_place_refresh_at_the_places_that_go_wrong(gpu_ctx, name, which):
    """Each rectangle of refresh_rectangles is filled with 255 (the albedo: 0xFFFFFFFF), then with 0, then restored.  After each edit all
    tables of all levels of both maps are the model of the edited chain; after a fill they differ from the bits read before the edits
    (the maps are clipped to 20 .. 230 first, so that 255 and 0 are new everywhere); after the restore they are those bits again."""
    sc = Scene(gpu_ctx, name)
    hm, al = np.clip(sc.hm, 20, 230).astype(np.uint8), np.clip(sc.al, 20, 230).astype(np.uint8)
    a = sc.terrain(hm, al, render=False)
    try:
        maps = Maps(sc)
        maps.hm, maps.al = hm.copy(), al.copy()
        full = hm if which == "height" else al
        h, w = full.shape[:2]
        base = assert_tables_are_the_model(a, f"{name}, before the edits")
        lv = a.mip_levels(which)
        assert lv >= 6
        for what, x, y, ew, eh in refresh_rectangles(w, h):
            assert 0 <= x and 0 <= y and ew >= 1 and eh >= 1 and x + ew <= w and y + eh <= h, what
            for value in (255, 0, None):
                texels = full[y:y + eh, x:x + ew].copy() if value is None else np.full((eh, ew) + full.shape[2:], value, np.uint8)
                maps.edit(a, which, x, y, texels)
                label = f"{name}, {which}, {what} -> {'restored' if value is None else value}"
                assert np.array_equal(a.download_mip(which, 0), maps.hm if which == "height" else maps.al), label
                got = assert_tables_are_the_model(a, label)
                if value is None:
                    assert_tables_equal(got, base, f"{label}: against the bits read before the edits")
                else:
                    assert tables_differ(got, base), label
    finally:
        a.close()


# ---- 4. the entry itself ------------------------------------------------------------------------------------------------------------------
def test_size_queries_absent_tables_and_refusals(gpu_ctx):
    """On the odd scene (67x45 / 33x50): a size query gives the dims and writes nothing; quad and quadf of the albedo, rgbf of the
    heightmap and a level beyond the chain give VR_OK, zero dims and leave `out` alone; a capacity one byte short, NULL out with a
    capacity and the other argument errors are refused with out_dims and `out` untouched; an exact capacity fills exactly the level's
    bytes and nothing behind them."""
    sc = Scene(gpu_ctx, "odd")
    tp = vr.TerrainPass(gpu_ctx, sc.p).Init(sc.hm, sc.al)
    try:
        fn, hnd = gpu_ctx.lib.vr_debug_terrain_tables, tp.handle
        dims = (C.c_int32 * 2)()
        guard = np.full(1 << 20, 0xA5, np.uint8)
        out = guard.ctypes.data_as(C.c_void_p)
        Q, QF, F, R = capi.VR_DEBUG_TABLE_QUAD, capi.VR_DEBUG_TABLE_QUADF, capi.VR_DEBUG_TABLE_FAST, capi.VR_DEBUG_TABLE_RGBF
        sizes = {(0, Q, 0): (69, 47, 4), (0, QF, 0): (69, 47, 16), (0, F, 0): (70, 48, 16), (1, F, 0): (36, 53, 16), (1, R, 0): (33, 50, 16),
                 (0, Q, 1): (35, 24, 4), (0, F, 6): (4, 4, 16), (1, R, 5): (1, 1, 16), (1, F, 2): (11, 15, 16)}
        for (which, table, level), (cols, rows, entry) in sizes.items():
            dims[0] = dims[1] = -1
            assert fn(hnd, which, table, level, dims, None, 0) == capi.VR_OK and list(dims) == [cols, rows], (which, table, level, list(dims))
            need = cols * rows * entry
            dims[0] = dims[1] = -1
            assert fn(hnd, which, table, level, dims, out, need - 1) == capi.VR_ERR_INVALID_ARGUMENT and list(dims) == [-1, -1]
            assert b"capacity" in gpu_ctx.lib.vr_last_error()
            assert fn(hnd, which, table, level, dims, None, need) == capi.VR_ERR_INVALID_ARGUMENT and list(dims) == [-1, -1]
            assert (guard == 0xA5).all(), (which, table, level)
            assert fn(hnd, which, table, level, dims, out, need) == capi.VR_OK and list(dims) == [cols, rows]
            assert (guard[need:] == 0xA5).all() and (guard[:need] != 0xA5).any()
            guard[:] = 0xA5
        assert tp.mip_levels("height") == 7 and tp.mip_levels("albedo") == 6
        for which, table, level in ((1, Q, 0), (1, QF, 0), (0, R, 0), (0, Q, 7), (0, F, 7), (1, R, 6), (1, F, 15), (0, QF, 16), (0, F, 2**31 - 1)):
            for args in ((None, 0), (out, guard.nbytes)):
                dims[0] = dims[1] = -1
                assert fn(hnd, which, table, level, dims, *args) == capi.VR_OK and list(dims) == [0, 0], (which, table, level)
        dims[0] = dims[1] = -1
        for args in ((None, 0, F, 0, dims, out, guard.nbytes), (hnd, 2, F, 0, dims, out, guard.nbytes), (hnd, 0, 4, 0, dims, out, guard.nbytes),
                     (hnd, 0, -1, 0, dims, out, guard.nbytes), (hnd, 0, F, -1, dims, out, guard.nbytes), (hnd, 0, F, 0, None, out, guard.nbytes)):
            assert fn(*args) == capi.VR_ERR_INVALID_ARGUMENT, args[1:4]
        assert list(dims) == [-1, -1] and (guard == 0xA5).all()
    finally:
        tp.close()


def test_an_edit_on_one_stream_is_read_back_on_another(gpu_ctx):
    """Eight device-pointer edits of each map of the 64^2 scene are queued on stream A - whole-map fills, the last one the maps the
    model expects - then the context moves to stream B with what vr_context_set_stream asks of the host (B waits for A: no host
    synchronisation) and the tables are read back at once: they are the model of the last edit, every level and table, and equal what
    is read again after the device has been synchronised."""
    import torch
    sc = Scene(gpu_ctx, "fast64")
    rng = np.random.default_rng(17)
    dev = f"cuda:{gpu_ctx.device}"
    fills = [(rng.integers(0, 256, (64, 64), dtype=np.uint8), rng.integers(0, 256, (64, 64, 4), dtype=np.uint8)) for _ in range(8)]
    d_fills = [(torch.from_numpy(h).to(dev), torch.from_numpy(a).to(dev)) for h, a in fills]
    a = sc.terrain(sc.hm, sc.al, render=False)
    gpu_ctx.synchronize()
    torch.cuda.synchronize()
    A, B = torch.cuda.Stream(), torch.cuda.Stream()
    try:
        before = read_tables(a)
        gpu_ctx.set_stream(A.cuda_stream)
        for dh, da in d_fills:
            a.Edit("height", 0, 0, device_ptr=dh.data_ptr(), w=64, h=64)
            a.Edit("albedo", 0, 0, device_ptr=da.data_ptr(), w=64, h=64)
        B.wait_stream(A)
        gpu_ctx.set_stream(B.cuda_stream)
        got = read_tables(a)
        gpu_ctx.synchronize()
        torch.cuda.synchronize()
        assert np.array_equal(a.download_mip("height", 0), fills[-1][0]) and np.array_equal(a.download_mip("albedo", 0), fills[-1][1])
        want = {"height": [tm.height_tables(a.download_mip("height", l)) for l in range(a.mip_levels("height"))],
                "albedo": [tm.albedo_tables(a.download_mip("albedo", l)) for l in range(a.mip_levels("albedo"))]}
        assert_tables_equal(got, want, "read back on B behind the edits on A: against the model of the last edit")
        assert_tables_equal(got, assert_tables_are_the_model(a, "after the synchronise"), "read back on B: against the tables after the synchronise")
        assert tables_differ(got, before)
    finally:
        torch.cuda.synchronize()
        gpu_ctx.set_stream(0)
        a.close()
