"""GPU tests of the query pyramid itself - the min / max pyramid vr_terrain_cast_rays walks, read back with
vr_debug_terrain_query_pyramid (TerrainPass.QueryPyramid) and held to tests/pyramid_model.py byte for byte: after the first cast of a
created terrain, and after in-place refreshes at the places where a refresh goes wrong.  Ray hits cannot show most of this: a bound
that is too loose only makes the walk longer, and the lo plane is read only under a negative max_height.  No tolerance appears in
any byte comparison; the one bound (the device's own sampler inside the device's own cells) is the walk's own slack, 2^-14.

The last test runs the second trip of the grid-stride loops of k_query_heights and k_query_rays (more than 16384 x 256 elements)."""
import ctypes as C

import numpy as np
import pytest

import vrenderer_amd as vr
from vrenderer_amd import capi
from tests import frontend_common as fc
from tests import pyramid_model as pm
from tests import queries_common as qc
from tests.common import params
from tests.f64_queries import Surface64
from tests.level0_common import Maps, Scene

pytestmark = pytest.mark.gpu

REFRESH_SCENES = ("odd", "fast64")               # 67x45 (odd, ragged at every level) and 64x64


def device_pair(tp):
    """Levels 0 and 1 of the heightmap as they are on the device (a one-level chain: level 0 twice)."""
    l0 = tp.download_mip("height", 0)
    return l0, (tp.download_mip("height", 1) if tp.mip_levels("height") > 1 else l0)


def assert_pyramid_is(got, want, what):
    assert got is not None, f"{what}: no pyramid"
    assert [a.shape for a in got] == [a.shape for a in want], f"{what}: levels {[a.shape[:2] for a in got]}, the model's {[a.shape[:2] for a in want]}"
    for l, (a, b) in enumerate(zip(got, want)):
        bad = np.argwhere((a != b).any(-1))
        assert bad.size == 0, (f"{what}: level {l} ({a.shape[1]} x {a.shape[0]} cells) differs in {len(bad)} cells, first (iz, ix) {bad[:4].tolist()}: "
                               f"device {a[tuple(bad[0])].tolist()}, model {b[tuple(bad[0])].tolist()}")


def assert_pyramid_is_the_model(tp, what):
    """Every byte of every level against the model of the device's own levels 0 and 1; returns the pyramid."""
    got = tp.QueryPyramid()
    assert_pyramid_is(got, pm.levels(*device_pair(tp)), what)
    return got


def _one_cast(tp, mh):
    tp.CastRays(np.float32([[0.0, 4.0 * abs(mh) + 1.0, 0.0]]), np.float32([[0.1, -1.0, 0.2]]), np.inf, mh)


def _created_cases(gpu_ctx):
    cases = [(f"{w}x{h}", fc.random_texture(w, h, fc.CREATE_SEED)[0], float(fc.CREATE_WORLD)) for w, h in fc.CREATE_SHAPES]
    cases += [("67x45", Scene(gpu_ctx, "odd").hm, 64.0), ("64x64", Scene(gpu_ctx, "fast64").hm, 64.0)]
    special = {n: (hm, ws) for n, hm, ws, _ in qc.special_maps()}
    cases += [(n, special[n][0], special[n][1]) for n in ("ragged 96x40", "all zero", "all 255")]
    return cases


def test_a_created_terrain_s_pyramid_is_the_model_byte_for_byte(gpu_ctx):
    """4a.  The maps of frontend_common.CREATE_SHAPES (1x1, 5x5, 7x2, 2x7, 33x17), 67x45, 64x64, the ragged 96x40 map and the all-zero
    and all-255 64^2 maps: no pyramid before the first cast; after one cast the number of levels, every level's cells and every byte
    of every level are pyramid_model.levels of the device's own levels 0 and 1."""
    for name, hm, ws in _created_cases(gpu_ctx):
        tp = vr.TerrainPass(gpu_ctx, params(int(ws))).Init(hm, np.zeros(hm.shape + (4,), np.uint8))
        try:
            assert tp.QueryPyramid() is None, f"{name}: a pyramid before the first cast"
            tp.SampleHeights(np.zeros((4, 2), np.float32), 10.0)
            assert tp.QueryPyramid() is None, f"{name}: a height query built the pyramid"
            _one_cast(tp, 10.0)
            assert np.array_equal(tp.download_mip("height", 0), hm)
            got = assert_pyramid_is_the_model(tp, name)
            h, w = hm.shape
            assert got[0].shape == (h + 1, w + 1, 2) and got[-1].shape == (1, 1, 2)
        finally:
            tp.close()


@pytest.mark.parametrize("name", REFRESH_SCENES)
def test_the_device_s_sampler_stays_inside_the_device_s_bounds(gpu_ctx, name):
    """4b.  At every leaf cell's points of pyramid_model.cell_points (texel-centre offsets 0 .. 1 in quarters per axis and the cell's
    level-1 footprint cuts) SampleHeights with max_height = 1 - hv itself - lies in r8[lo] - 2^-14 .. r8[hi] + 2^-14 of the cell read
    back from the device, r8[b] = float32(b) / 255: the slack is the walk's own (slack_mh of k_query_rays), not tuned here.
    A point on a cell's rim may be moved across the boundary by the fp32 rounding of its world coordinate and of the sampler's uv: by
    a few 1e-6 texel.  H / max_height is continuous with a slope of at most 1 per texel, so the move changes hv by a few 1e-6 at the
    most, far below the slack of 6.1e-5, and every point is held to each cell it was generated for.
    Measured on the MI355X: worst excess over [r8[lo], r8[hi]] itself 0.0 on both scenes (153,272 and 207,025 points) - some point
    attains its cell's bound exactly, none leaves it."""
    sc = Scene(gpu_ctx, name)
    tp = vr.TerrainPass(gpu_ctx, sc.p).Init(sc.hm, sc.al)
    try:
        _one_cast(tp, sc.mh)
        pyr = tp.QueryPyramid()
        l0, l1 = device_pair(tp)
        (h0, w0), (h1, w1) = l0.shape, l1.shape
        x, z = pm.cell_points(w0, h0, w1, h1, float(sc.world))
        pts = np.stack([x, z], -1).reshape(-1, 2).astype(np.float32)
        hv = tp.SampleHeights(pts, 1.0).reshape(x.shape)
        r8 = (np.arange(256, dtype=np.float32) / np.float32(255.0)).astype(np.float64)
        lo, hi = r8[pyr[0][..., 0]][:, :, None, None], r8[pyr[0][..., 1]][:, :, None, None]
        worst = float(max((lo - hv).max(), (hv - hi).max()))
        print(f"\n{name}: {hv.size} points, worst excess of hv over the device's [r8[lo], r8[hi]] = {worst:.3e} (slack {pm.SLACK:.3e})")
        assert worst <= pm.SLACK, worst
        # the model's surface at the same points, inside the same cells (3a on the device's own bytes)
        assert pm.excess(pyr[0], Surface64(l0, l1, float(sc.world), 1.0).H(x, z)) <= pm.SLACK
    finally:
        tp.close()


@pytest.mark.parametrize("name", REFRESH_SCENES)
def test_in_place_refresh_at_the_places_that_go_wrong(gpu_ctx, name):
    """4c.  Heights clipped to 20 .. 230, so that 255 and 0 are new extremes of the whole map and move hi, then lo, at every level up to
    the top cell (tests/test_queries_cpu.py shows it on the model); the pyramid is built first.  Each rectangle of
    pyramid_model.refresh_edits - single texels at the corners, in the odd last column and last row alone (an empty level-1 rectangle),
    either side of a level-1 footprint boundary and on both sides of the kernels' 64 x 4 tile edges, then a column, a row and 7 x 9 -
    is filled with 255, with 0 and restored: after each edit every level is the model of the edited map, after the restoring one
    the original pyramid (a bound must come down again).  And the first edit on a terrain with no pyramid yet, then one cast."""
    sc = Scene(gpu_ctx, name)
    hm = pm.clipped(sc.hm)
    h, w = hm.shape
    a = sc.terrain(hm, sc.al, render=False)
    try:
        maps = Maps(sc)
        maps.hm = hm.copy()
        base = assert_pyramid_is_the_model(a, f"{name}, before the edits")
        edits = pm.refresh_edits(w, h)
        for what, x, y, ew, eh in edits:
            for value in (255, 0, None):
                texels = hm[y:y + eh, x:x + ew].copy() if value is None else np.full((eh, ew), value, np.uint8)
                maps.edit(a, "height", x, y, texels)
                label = f"{name}, {what} -> {'restored' if value is None else value}"
                assert np.array_equal(a.download_mip("height", 0), maps.hm), label
                got = assert_pyramid_is_the_model(a, label)
                if value is None:
                    assert_pyramid_is(got, base, f"{label}: against the original pyramid")
                else:
                    assert any(not np.array_equal(p, q) for p, q in zip(got, base)), label
        # no pyramid yet: the edit has nothing to refresh, the first cast builds it from the edited map
        what, x, y, ew, eh = edits[0]
        b = sc.terrain(hm, sc.al, cast=False, render=False)
        try:
            b.Edit("height", x, y, np.full((eh, ew), 255, np.uint8))
            assert b.QueryPyramid() is None
            _one_cast(b, sc.mh)
            edited = hm.copy()
            edited[y:y + eh, x:x + ew] = 255
            assert np.array_equal(b.download_mip("height", 0), edited)
            assert_pyramid_is_the_model(b, f"{name}, {what} -> 255 before the first cast")
        finally:
            b.close()
    finally:
        a.close()


def test_the_second_trip_of_the_grid_stride_loops(gpu_ctx):
    """4e.  n = 4,194,304 + 257 elements in device-pointer mode on the 64^2 scene: the grid is capped at 16384 workgroups of 256, so the
    last 257 elements are the loops' second trip.  The inputs are the scene's 4096 seeded points / rays tiled on the device; every
    output element i equals element i % 4096 of a 4096-element call bit for bit - heights with normals, and hits - and the 4096
    sentinel bytes behind element n - 1 of every output buffer stay as they were."""
    import torch
    sc = Scene(gpu_ctx, "fast64")
    tp = vr.TerrainPass(gpu_ctx, sc.p).Init(sc.hm, sc.al)
    dev = f"cuda:{gpu_ctx.device}"
    m, n, guard = 4096, 4194304 + 257, 4096
    reps = (n + m - 1) // m

    def tiled(host, row_bytes):
        base = torch.from_numpy(np.ascontiguousarray(host).view(np.uint8).reshape(m, row_bytes).copy()).to(dev)
        return base, base.repeat(reps, 1)[:n].contiguous()

    def out_buffer(rows, row_bytes):
        return torch.full((rows * row_bytes + guard,), 0xA5, dtype=torch.uint8, device=dev)

    def check(big, small, row_bytes, what):
        assert bool((big[n * row_bytes:] == 0xA5).all()) and bool((small[m * row_bytes:] == 0xA5).all()), f"{what}: bytes behind the last element were written"
        want = small[:m * row_bytes].view(m, row_bytes).repeat(reps, 1)[:n]
        differ = (big[:n * row_bytes].view(n, row_bytes) != want).any(1)
        assert not bool(differ.any()), f"{what}: {int(differ.sum())} of {n} elements differ, first {differ.nonzero()[:4].flatten().tolist()}"
        assert bool((small[:m * row_bytes] != 0xA5).any())

    try:
        lib, ptr = gpu_ctx.lib, lambda t: C.c_void_p(t.data_ptr())
        # heights with normals
        _, xz_big = tiled(qc.uniform_points(sc.world), 8)
        xz_small = xz_big[:m].contiguous()
        h_big, n_big, h_small, n_small = out_buffer(n, 4), out_buffer(n, 12), out_buffer(m, 4), out_buffer(m, 12)
        torch.cuda.synchronize()
        capi.check(lib.vr_terrain_query_heights(tp.handle, ptr(xz_small), m, sc.mh, ptr(h_small), ptr(n_small), 1), "vr_terrain_query_heights")
        capi.check(lib.vr_terrain_query_heights(tp.handle, ptr(xz_big), n, sc.mh, ptr(h_big), ptr(n_big), 1), "vr_terrain_query_heights")
        gpu_ctx.synchronize()
        check(h_big, h_small, 4, "heights")
        check(n_big, n_small, 12, "normals")
        hh, nn = tp.SampleHeights(qc.uniform_points(sc.world), sc.mh, normals=True)
        assert h_small[:m * 4].cpu().numpy().tobytes() == hh.tobytes() and n_small[:m * 12].cpu().numpy().tobytes() == nn.tobytes()
        del xz_big, h_big, n_big
        # rays
        surf = Surface64(*device_pair(tp), sc.world, sc.mh)
        o, d, tm = qc.make_rays(surf, sc.world)
        rays = np.zeros(m, vr.RAY_DTYPE)
        rays["origin"], rays["dir"], rays["t_max"] = o, d, tm
        _, r_big = tiled(rays, 32)
        r_small = r_big[:m].contiguous()
        o_big, o_small = out_buffer(n, 32), out_buffer(m, 32)
        torch.cuda.synchronize()
        capi.check(lib.vr_terrain_cast_rays(tp.handle, ptr(r_small), m, sc.mh, ptr(o_small), 1), "vr_terrain_cast_rays")
        capi.check(lib.vr_terrain_cast_rays(tp.handle, ptr(r_big), n, sc.mh, ptr(o_big), 1), "vr_terrain_cast_rays")
        gpu_ctx.synchronize()
        check(o_big, o_small, 32, "hits")
        host = tp.cast_ray_array(rays, sc.mh)
        assert o_small[:m * 32].cpu().numpy().tobytes() == host.tobytes()
        assert (host["status"] == capi.VR_RAY_HIT).mean() > 0.3 and not (host["status"] == capi.VR_RAY_STEP_LIMIT).any()
    finally:
        tp.close()
