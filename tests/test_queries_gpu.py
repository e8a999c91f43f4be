"""GPU tests of the terrain queries (vr_terrain_query_heights, vr_terrain_cast_rays): heights bit-exact against the vertex
stage through the oracle, heights / normals / ray hits against the float64 model of tests/f64_queries.py.

The tests print the worst |error| / tolerance they find (pytest -s); the bounds are tests/f64_queries.py's height_tol / ray_tol.
DESIGN.md 4q is where the device's figures belong."""
import ctypes as C

import numpy as np
import pytest

import vrenderer_amd as vr
from vrenderer_amd import capi
from tests.common import CAMERAS, params, scaled_camera
from tests import queries_common as qc
from tests.f64_queries import HIT, INVALID, MISS, Surface64

pytestmark = pytest.mark.gpu

SIZES = (64, 256)


class Scene:
    def __init__(self, ctx, oracle, size):
        self.size, self.mh = size, qc.scaled_max_height(size)
        self.hm = vr.synth_heightmap(ctx, size)
        self.al = vr.synth_albedo(ctx, size, self.hm)
        self.tp = vr.TerrainPass(ctx, params(size)).Init(self.hm, self.al)
        self.ot = oracle.OracleTerrain(params(size), self.hm, self.al)
        self.surf = Surface64(self.tp.download_mip("height", 0), self.tp.download_mip("height", 1), size, self.mh)
        self._rays = None

    def rays(self):
        """The ray set and its model, computed once and shared."""
        if self._rays is None:
            o, d, tm = qc.make_rays(self.surf, self.size)
            self._rays = (o, d, tm, qc.model_of_rays(self.surf, o, d, tm))
        return self._rays

    def close(self):
        self.tp.close(); self.ot.close()


@pytest.fixture(scope="module")
def scenes(gpu_ctx, oracle):
    s = {size: Scene(gpu_ctx, oracle, size) for size in SIZES}
    yield s
    for v in s.values():
        v.close()


def _device_array(ctx, host):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(host).view(np.uint8).reshape(-1).copy()).to(f"cuda:{ctx.device}")
    return t


@pytest.mark.parametrize("size", SIZES)
def test_heights_are_the_vertex_stage_s_bit_for_bit(scenes, size):
    """SampleHeights(world.xz) == world.y for all 1,089 vertices of up to 8 selected instances under two cameras: the anchor
    to the oracle's vertex stage (OracleTerrain.vertex)."""
    sc = scenes[size]
    mh = 400.0
    for cam in (CAMERAS[0], CAMERAS[5]):
        eye, tgt = scaled_camera(cam, size)
        view = vr.make_view(eye, tgt, 640, 360)
        n, _, inst = sc.ot.select(view, mh)
        assert n >= 1
        for i in range(min(n, 8)):
            world = np.array([sc.ot.vertex(view, mh, inst[i], vx, vz)[1] for vz in range(33) for vx in range(33)], np.float32)
            got = sc.tp.SampleHeights(world[:, [0, 2]], mh)
            assert np.array_equal(got.view(np.uint32), world[:, 1].view(np.uint32)), (size, cam, i, int((got != world[:, 1]).sum()))


def test_heights_outside_the_world_odd_counts_and_device_pointers(scenes, gpu_ctx):
    sc = scenes[64]
    surf, tp, ws, mh = sc.surf, sc.tp, 64.0, sc.mh
    rng = np.random.default_rng(11)
    # clamp addressing outside uv in [0, 1]^2: the height of the nearest border point
    out = rng.uniform(-3.0 * ws, 3.0 * ws, (4096, 2)).astype(np.float32)
    h = tp.SampleHeights(out, mh)
    inside = np.clip(out, -0.5 * ws, 0.5 * ws)
    assert np.array_equal(h, tp.SampleHeights(inside, mh))
    x, z = out[:, 0].astype(np.float64), out[:, 1].astype(np.float64)
    assert (np.abs(h - surf.H(x, z)) <= surf.height_tol(x, z)).all()
    # n = 1, 63, 65, 4096: every count is the prefix of the largest
    for n in (1, 63, 65, 4096):
        hn, nn = tp.SampleHeights(out[:n], mh, normals=True)
        assert hn.shape == (n,) and nn.shape == (n, 3) and np.array_equal(hn, h[:n])
    assert tp.SampleHeights(np.zeros((0, 2), np.float32), mh).shape == (0,)
    # device-pointer mode == host mode (stream-ordered: the copies below run on the context's stream order via synchronise)
    import torch
    n = 4096
    d_xz, d_h, d_n = _device_array(gpu_ctx, out), torch.zeros(n * 4, dtype=torch.uint8, device=f"cuda:{gpu_ctx.device}"), torch.zeros(n * 12, dtype=torch.uint8, device=f"cuda:{gpu_ctx.device}")
    torch.cuda.synchronize()
    capi.check(gpu_ctx.lib.vr_terrain_query_heights(tp.handle, C.c_void_p(d_xz.data_ptr()), n, mh, C.c_void_p(d_h.data_ptr()), C.c_void_p(d_n.data_ptr()), 1),
               "vr_terrain_query_heights")
    gpu_ctx.synchronize()
    hh, nn = tp.SampleHeights(out, mh, normals=True)
    assert np.array_equal(d_h.cpu().numpy().view(np.float32), hh) and np.array_equal(d_n.cpu().numpy().view(np.float32).reshape(n, 3), nn)
    # rays likewise
    o, d, tm, _ = sc.rays()
    rays = np.zeros(512, vr.RAY_DTYPE)
    rays["origin"], rays["dir"], rays["t_max"] = o[::8], d[::8], tm[::8]
    d_r, d_o = _device_array(gpu_ctx, rays), torch.zeros(512 * 32, dtype=torch.uint8, device=f"cuda:{gpu_ctx.device}")
    torch.cuda.synchronize()
    capi.check(gpu_ctx.lib.vr_terrain_cast_rays(tp.handle, C.c_void_p(d_r.data_ptr()), 512, mh, C.c_void_p(d_o.data_ptr()), 1), "vr_terrain_cast_rays")
    gpu_ctx.synchronize()
    assert d_o.cpu().numpy().tobytes() == tp.cast_ray_array(rays, mh).tobytes()


@pytest.mark.parametrize("size", SIZES)
def test_heights_and_normals_against_float64(scenes, size):
    """4096 uniform points: |h - H64| <= 8 (ulp32(world_size) S + ulp32(max_height)); normals within 1e-3 rad away from
    the cell boundaries (at most 2 % of the points are left out)."""
    sc = scenes[size]
    pts = qc.uniform_points(size)
    h, nrm = sc.tp.SampleHeights(pts, sc.mh, normals=True)
    x, z = pts[:, 0].astype(np.float64), pts[:, 1].astype(np.float64)
    ratio = np.abs(h - sc.surf.H(x, z)) / sc.surf.height_tol(x, z)
    ok = qc.away_from_cell_boundaries(sc.surf, x, z)
    ang = np.arccos(np.clip((nrm.astype(np.float64) * sc.surf.normal(x, z)).sum(1), -1.0, 1.0))
    print(f"\n{size}^2: worst |h - H64| / tol = {ratio.max():.4f}; worst normal angle {ang[ok].max():.3e} rad; {1 - ok.mean():.2%} of the points left out")
    assert (ratio <= 1.0).all(), ratio.max()
    assert 1.0 - ok.mean() <= 0.02
    assert (ang[ok] <= 1e-3).all(), ang[ok].max()
    assert np.abs(np.linalg.norm(nrm, axis=1) - 1.0).max() <= 1e-6


@pytest.mark.parametrize("size", SIZES)
def test_ray_hits_against_float64(scenes, size):
    """4096 rays per map (tests/queries_common.py: make_rays); every HIT and MISS within the model's bounds, the statuses
    as the model's except on grazing rays (at most 3 %), no ray at the step limit.  Check (c) holds position.x and .z to
    4 ulp32 of the largest term; position.y, the sampler's value, to 4 ulp32 plus the sampler's step ulp32(world_size) S for
    hits inside the segment, and to the height tolerance from above for rays that start under the surface or leave through the
    floor (tests/queries_common.py: check_ray_hits gives the argument)."""
    sc = scenes[size]
    o, d, tm, model = sc.rays()
    assert model["grazing"].mean() <= 0.03, model["grazing"].mean()
    hits = sc.tp.CastRays(o, d, tm, sc.mh)
    worst = qc.check_ray_hits(sc.surf, o, d, tm, hits, model, f"{size}^2")
    print(f"\n{size}^2: statuses {np.bincount(hits['status'], minlength=4).tolist()}; worst ratios {worst}")
    assert (hits["status"] == HIT).mean() > 0.3


def test_shapes_that_break_pyramids(gpu_ctx):
    """A ragged 96 x 40 map, a 1 x 1 map, an all-zero and an all-255 map, max_height = 0 (a plane at y = 0 that is hit) and a
    negative max_height: 512 rays each, checked like test_ray_hits_against_float64."""
    for name, hmap, ws, mh in qc.special_maps():
        p = params(int(ws))
        tp = vr.TerrainPass(gpu_ctx, p).Init(hmap, np.zeros(hmap.shape + (4,), np.uint8))
        lv = tp.mip_levels("height")
        l0 = tp.download_mip("height", 0)
        surf = Surface64(l0, tp.download_mip("height", 1) if lv > 1 else l0, ws, mh)
        o, d, tm = qc.make_rays(surf, ws, 512)
        model = qc.model_of_rays(surf, o, d, tm)
        hits = tp.CastRays(o, d, tm, mh)
        worst = qc.check_ray_hits(surf, o, d, tm, hits, model, name)
        print(f"\n{name}: statuses {np.bincount(hits['status'], minlength=4).tolist()}; worst ratios {worst}")
        pts = qc.uniform_points(ws, 512)
        h = tp.SampleHeights(pts, mh)
        x, z = pts[:, 0].astype(np.float64), pts[:, 1].astype(np.float64)
        assert (np.abs(h - surf.H(x, z)) <= surf.height_tol(x, z)).all(), name
        if mh == 0.0:
            # the plane y = 0: every ray that comes down onto it inside the world is a hit on it, at -origin.y / dir.y
            down = (o[:, 1] > 0) & (d[:, 1] < 0) & (model["status"] == HIT)
            assert down.sum() > 100 and (hits["status"][down] == HIT).all()
            t = -o[down, 1].astype(np.float64) / d[down, 1].astype(np.float64)
            assert (np.abs(hits["t"][down] - t) <= 4 * np.spacing(t.astype(np.float32))).all()
            assert not hits["position"][down, 1].any() and np.array_equal(hits["normal"][down], np.tile(np.float32([0, 1, 0]), (down.sum(), 1)))
        tp.close()


def test_bad_rays_are_invalid_and_leave_their_neighbours_alone(scenes):
    """NaN / Inf / zero directions, NaN origins, t_max < 0 and t_max = 0, mixed one by one into a wave of valid rays: those
    lanes return VR_RAY_INVALID (a MISS for t_max = 0 above the ground), the others' hits are identical to a run without."""
    sc = scenes[64]
    o, d, tm, _ = sc.rays()
    base = np.zeros(256, vr.RAY_DTYPE)
    base["origin"], base["dir"], base["t_max"] = o[1400:1656], d[1400:1656], tm[1400:1656]       # random rays from above
    clean = sc.tp.cast_ray_array(base, sc.mh)
    assert (clean["status"] == HIT).sum() > 16
    nan, inf = np.float32("nan"), np.float32("inf")
    bad = [("dir", (nan, -1, 0)), ("dir", (0, nan, 0)), ("dir", (1, -1, nan)), ("dir", (inf, -1, 0)), ("dir", (0, -inf, 0)), ("dir", (0, 0, 0)),
           ("dir", (-0.0, 0.0, -0.0)), ("origin", (nan, 50, 0)), ("origin", (0, nan, 0)), ("origin", (0, 50, nan)), ("origin", (inf, 50, 0)),
           ("t_max", -1.0), ("t_max", nan), ("t_max", -inf), ("t_max", -0.0), ("t_max", 0.0)]
    for k, (field, value) in enumerate(bad):
        lane = 3 + 13 * k
        rays = base.copy()
        if field == "origin":
            rays["dir"][lane] = (0.0, -1.0, 0.0)
        if field == "t_max":
            rays["origin"][lane], rays["dir"][lane] = (1.0, 4.0 * sc.mh, -2.0), (0.0, -1.0, 0.0)
        rays[field][lane] = value
        hits = sc.tp.cast_ray_array(rays, sc.mh)
        others = np.arange(256) != lane
        assert hits[others].tobytes() == clean[others].tobytes(), (field, value)
        want = MISS if field == "t_max" and value == 0.0 else INVALID
        assert hits["status"][lane] == want, (field, value, int(hits["status"][lane]))
        assert not hits["position"][lane].any() and not hits["normal"][lane].any()
        assert np.array_equal(hits["t"][lane:lane + 1], rays["t_max"][lane:lane + 1], equal_nan=True)
    # extreme but finite values spin nowhere: every lane comes back with a status
    wild = base.copy()
    wild["dir"][::7] *= np.float32(1e30); wild["dir"][1::7] *= np.float32(1e-30); wild["origin"][2::7] *= np.float32(1e20); wild["t_max"][3::7] = np.float32(1e-30)
    hits = sc.tp.cast_ray_array(wild, sc.mh)
    assert (hits["status"] <= 2).all()
    keep = np.ones(256, bool)
    for s in range(4):
        keep[s::7] = False
    assert hits[keep].tobytes() == clean[keep].tobytes()


def test_queries_do_not_disturb_rendering(scenes, gpu_ctx):
    """Render, query on the same stream, render again: the G-buffer planes are the first frame's, and the terrain grew by the
    pyramid (textures) and the staging memory (scratch) only."""
    size = 256
    tp = vr.TerrainPass(gpu_ctx, params(size)).Init(scenes[size].hm, scenes[size].al)
    eye, tgt = scaled_camera(CAMERAS[0], size)
    w, h = 320, 180
    view = vr.make_view(eye, tgt, w, h)
    rp = vr.default_render_params(400.0)
    rt = vr.RenderTargets(gpu_ctx).Init(w, h)
    rt.Clear(); tp.Render(view, view, rt, rp)
    first = {p: rt.download(p) for p in vr.RenderTargets.PLANES}
    before = tp.memory_bytes()
    o, d, tm, _ = scenes[size].rays()
    rt.Clear(); tp.Render(view, view, rt, rp)
    hits = tp.CastRays(o[:1024], d[:1024], tm[:1024], 400.0)
    pts = qc.uniform_points(size, 1024)
    hh = tp.SampleHeights(pts, 400.0)
    rt.Clear(); tp.Render(view, view, rt, rp)
    for p, want in first.items():
        assert np.array_equal(rt.download(p), want), p
    after = tp.memory_bytes()
    cells, wc, hc = 0, size + 1, size + 1
    while True:
        cells += wc * hc
        if wc == 1 and hc == 1:
            break
        wc, hc = (wc + 1) // 2, (hc + 1) // 2
    assert after["textures"] - before["textures"] == 2 * cells                       # one uint8 pair per cell of every level
    assert after["node_heights"] == before["node_heights"]
    assert 0 < after["scratch"] - before["scratch"] <= 4 * 1024 * 64                  # the staging of 1024 rays, doubled at most twice
    assert after["total"] == after["textures"] + after["scratch"] + after["node_heights"]
    # and the answers do not depend on what was rendered in between
    assert tp.CastRays(o[:1024], d[:1024], tm[:1024], 400.0).tobytes() == hits.tobytes() and np.array_equal(tp.SampleHeights(pts, 400.0), hh)
    assert tp.memory_bytes() == after                                                # nothing is allocated per call once it is large enough
    # the query kernels are timed like every other (vr_timing_*); the pyramid is not built a second time
    gpu_ctx.timing_enable(1)
    tp.CastRays(o[:64], d[:64], tm[:64], 400.0); tp.SampleHeights(pts[:64], 400.0)
    t = gpu_ctx.timing_collect()
    gpu_ctx.timing_enable(0)
    assert t["k_query_rays"][1] == 1 and t["k_query_heights"][1] == 1 and "k_query_pyramid (all levels)" not in t
    rt.close(); tp.close()
