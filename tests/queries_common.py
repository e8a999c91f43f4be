"""Shared by tests/test_queries_cpu.py and tests/test_queries_gpu.py: the point and ray sets of the terrain-query tests
and the checks of a batch of ray hits against the float64 model (tests/f64_queries.py).  Everything is seeded; the CPU
tests verify that the seeds keep the shares the GPU tests rely on (points near cell boundaries, grazing rays)."""
import numpy as np

import vrenderer_amd as vr
from tests.common import CAMERAS, scaled_camera
from tests.f64_queries import HIT, INVALID, MISS, STEP_LIMIT, Surface64, ulp32

POINT_SEED = 20251
RAY_SEED = 77003
N_POINTS = 4096
N_RAYS = 4096
RAY_CAMERAS = (0, 4, 6)


def scaled_max_height(size):
    """EditorParams::m_MaxHeight = 400 is authored for the 2048 world, like the cameras."""
    return 400.0 * size / 2048.0


def mip_pair(levels):
    """(level 0, level 1) of a chain given as a list of (h, w) uint8 arrays; a one-level chain samples level 0 twice."""
    return levels[0], levels[1] if len(levels) > 1 else levels[0]


def uniform_points(world_size, n=N_POINTS, seed=POINT_SEED):
    rng = np.random.default_rng(seed)
    return rng.uniform(-0.5 * world_size, 0.5 * world_size, (n, 2)).astype(np.float32)


def away_from_cell_boundaries(surf, x, z, margin=2.0 ** -10):
    """True where (x, z) is further than `margin` texels from every level-0 and level-1 cell boundary (where the
    analytic normal jumps)."""
    x, z = np.asarray(x, np.float64), np.asarray(z, np.float64)
    u, v = (x + 0.5 * surf.ws) / surf.ws, (z + 0.5 * surf.ws) / surf.ws
    ok = np.ones(x.shape, bool)
    for tex in (surf.l0, surf.l1):
        h, w = tex.shape
        for c in (u * w - 0.5, v * h - 0.5):
            ok &= np.abs(c - np.round(c)) > margin
    return ok


def make_rays(surf, size, n=N_RAYS, seed=RAY_SEED):
    """(origins, dirs, t_max) as float32: one third pixel rays of cameras 0, 4 and 6 at 64 x 64, one third random origins
    above the box with random downward directions, and ninths of vertical rays, axis-parallel rays with an exact zero
    component, and rays that start below the surface."""
    rng = np.random.default_rng(seed)
    ws, mh = surf.ws, surf.mh
    third = n // 3
    o, d, tm = [], [], []
    per_cam = [third // 3 + (1 if k < third % 3 else 0) for k in range(3)]
    for cam, cnt in zip(RAY_CAMERAS, per_cam):
        eye, tgt = scaled_camera(CAMERAS[cam], size)
        view = vr.make_view(eye, tgt, 64, 64)
        for p in rng.choice(64 * 64, cnt, replace=False):
            r = vr.pixel_ray(view, float(p % 64), float(p // 64))
            o.append(list(r.origin)); d.append(list(r.dir)); tm.append(r.t_max)
    top = max(abs(mh), 1e-3 * ws)
    # random origins above the box (some beside it), random downward directions of any length
    k = third
    oo = np.stack([rng.uniform(-0.6 * ws, 0.6 * ws, k), rng.uniform(1.05, 3.0, k) * top + max(mh, 0.0), rng.uniform(-0.6 * ws, 0.6 * ws, k)], 1)
    dd = np.stack([rng.normal(size=k), -np.abs(rng.normal(size=k)) - 0.05, rng.normal(size=k)], 1) * rng.uniform(0.5, 4.0, (k, 1))
    o += oo.tolist(); d += dd.tolist(); tm += [np.inf] * k
    rest = n - 2 * third
    nv, na = rest // 3, rest // 3
    nb = rest - nv - na
    # vertical: three quarters down from above, one quarter up from under the box
    xz = rng.uniform(-0.5 * ws, 0.5 * ws, (nv, 2))
    up = np.arange(nv) % 4 == 3
    oo = np.stack([xz[:, 0], np.where(up, min(mh, 0.0) - 0.25 * top, max(mh, 0.0) + rng.uniform(0.1, 2.0, nv) * top), xz[:, 1]], 1)
    dd = np.stack([np.zeros(nv), np.where(up, 1.0, -1.0) * rng.uniform(0.5, 3.0, nv), np.zeros(nv)], 1)
    o += oo.tolist(); d += dd.tolist(); tm += [np.inf] * nv
    # axis-parallel: half horizontal along +-x / +-z at an altitude inside the box, half in a plane z = const or x = const
    alt = rng.uniform(0.0, 1.0, na) * mh
    ax = rng.integers(0, 4, na)
    sgn = np.where(ax % 2 == 0, 1.0, -1.0)
    side = rng.uniform(-0.5 * ws, 0.5 * ws, na)
    planar = np.arange(na) % 2 == 1
    oo = np.where((ax < 2)[:, None], np.stack([-0.7 * ws * sgn, alt, side], 1), np.stack([side, alt, -0.7 * ws * sgn], 1))
    dd = np.where((ax < 2)[:, None], np.stack([sgn, np.zeros(na), np.zeros(na)], 1), np.stack([np.zeros(na), np.zeros(na), sgn], 1))
    oo[planar, 1] = max(mh, 0.0) + rng.uniform(0.2, 1.5, planar.sum()) * top
    dd[planar, 1] = -rng.uniform(0.05, 1.0, planar.sum())
    o += oo.tolist(); d += (dd * rng.uniform(0.5, 2.0, (na, 1))).tolist(); tm += [np.inf] * na
    # below the surface, inside the box, any direction
    xz = rng.uniform(-0.5 * ws, 0.5 * ws, (nb, 2)).astype(np.float32).astype(np.float64)
    hh, floor = surf.H(xz[:, 0], xz[:, 1]), min(mh, 0.0)
    oo = np.stack([xz[:, 0], floor + (hh - floor) * rng.uniform(0.1, 0.95, nb), xz[:, 1]], 1)
    dd = rng.normal(size=(nb, 3))
    o += oo.tolist(); d += dd.tolist(); tm += [np.inf] * nb
    return np.asarray(o, np.float32), np.asarray(d, np.float32), np.asarray(tm, np.float32)


def special_maps():
    """Shapes that break pyramids: (name, heightmap, world size, max_height)."""
    rng = np.random.default_rng(5150)
    ragged = rng.integers(0, 256, (40, 96), dtype=np.uint8)
    ragged[8:30, 10:80] = (ragged[8:30, 10:80] // 8) + 100             # a plateau among the noise
    noise = rng.integers(0, 256, (64, 64), dtype=np.uint8)
    return [("ragged 96x40", ragged, 128.0, 30.0),
            ("1x1", np.full((1, 1), 200, np.uint8), 64.0, 20.0),
            ("all zero", np.zeros((64, 64), np.uint8), 64.0, 12.5),
            ("all 255", np.full((64, 64), 255, np.uint8), 64.0, 12.5),
            ("max_height 0", noise, 64.0, 0.0),
            ("max_height < 0", noise, 64.0, -12.5)]


def model_of_rays(surf, o, d, tm):
    """first_hit64 of the float32 rays plus `grazing`: the model's own closest approach before its hit (or over the whole
    segment of a miss) is inside the tolerance there - the status of such a ray is not the kernel's to decide."""
    o64, d64, tm64 = o.astype(np.float64), d.astype(np.float64), tm.astype(np.float64)
    m = surf.first_hit64(o64, d64, tm64)
    os_, ds_ = np.where(np.isfinite(o64), o64, 0.0), np.where(np.isfinite(d64), d64, 1.0)
    grazing = np.isfinite(m["gmin"]) & (np.abs(m["gmin"]) < surf.ray_tol(os_, ds_, np.where(np.isfinite(m["t_at"]), m["t_at"], 0.0)))
    m["grazing"] = grazing
    return m


def check_ray_hits(surf, o, d, tm, hits, model=None, label=""):
    """Checks (a)-(d) of every HIT, the bound of every MISS and the agreement of the statuses with the model; returns
    the worst ratios found (|error| / tolerance)."""
    model = model or model_of_rays(surf, o, d, tm)
    o64, d64 = o.astype(np.float64), d.astype(np.float64)
    st = hits["status"]
    assert not (st == STEP_LIMIT).any(), f"{label}: {(st == STEP_LIMIT).sum()} rays reached the step limit"
    assert np.array_equal(st == INVALID, model["status"] == INVALID), f"{label}: INVALID statuses differ from the model"
    texel_t = 1.0 / np.maximum(np.hypot(d64[:, 0] * surf.w0, d64[:, 2] * surf.h0) / surf.ws, 1e-300)     # t per texel along the ray
    worst = dict(a=0.0, b=0.0, y=0.0, y_ulp=0.0, miss=0.0)
    h = np.nonzero(st == HIT)[0]
    if h.size:
        t = hits["t"][h].astype(np.float64)
        pos, nrm = hits["position"][h].astype(np.float64), hits["normal"][h].astype(np.float64)
        oh, dh = o64[h], d64[h]
        assert ((t >= 0) & (t <= tm[h].astype(np.float64)) & (t >= model["t0"][h] - 4 * ulp32(t)) & (t <= model["t1"][h] + 4 * ulp32(t))).all(), f"{label}: t outside the clipped segment"
        tol = surf.ray_tol(oh, dh, t)
        # (a) the reported height is the surface's at the reported point
        ea = np.abs(pos[:, 1] - surf.H(pos[:, 0], pos[:, 2])) / tol
        worst["a"] = float(ea.max())
        assert (ea <= 1.0).all(), f"{label}: (a) height at the hit off by {ea.max():.2f} x tol (ray {h[ea.argmax()]})"
        # (c) the point is the ray's: position == origin + t dir within 4 ulp32 of the largest term.  x and z are held to exactly
        # that.  position.y is by definition the sampler's fp32 value at position.xz, and that value is a step function of the
        # point: the sampler rounds x + world_size / 2 to fp32, so H moves in steps of up to ulp32(world_size) S, and where g
        # changes sign across such a step no t has a smaller |origin.y + t dir.y - position.y| than half of it.  The bound for y is
        # therefore 4 ulp32(largest term) + ulp32(world_size) S: the issue's own first-order term of the uv rounding, without
        # its margin of 8 and without the max_height and |t| |dir| terms of the height tolerance.  Two classes of hit cannot be
        # near the ray in y at all and are held to the height tolerance from above only: a ray that starts at or below the surface
        # is reported at its first t inside the box, any depth under the surface, and so is one that leaves through the floor.
        for k in (0, 2):
            big = np.maximum(np.abs(oh[:, k]), np.maximum(np.abs(t * dh[:, k]), np.abs(pos[:, k])))
            assert (np.abs(pos[:, k] - (oh[:, k] + t * dh[:, k])) <= 4 * ulp32(big)).all(), f"{label}: (c) position[{k}] is not origin + t dir"
        gy = oh[:, 1] + t * dh[:, 1] - pos[:, 1]
        big = np.maximum(np.abs(oh[:, 1]), np.maximum(np.abs(t * dh[:, 1]), np.abs(pos[:, 1])))
        started_below = t <= model["t0"][h] + 0.125 * texel_t[h] + 4 * ulp32(t)
        at_exit = t >= model["t1"][h] - 4 * ulp32(t)
        inner = ~started_below & ~at_exit
        step = ulp32(surf.ws) * surf.slope_bound(pos[inner, 0], pos[inner, 2])
        uy = np.abs(gy[inner]) / (4 * ulp32(big[inner]) + step)
        worst["y"] = float(uy.max(initial=0.0))
        worst["y_ulp"] = float((np.abs(gy[inner]) / ulp32(big[inner])).max(initial=0.0))     # in ulp32 of the largest term alone
        assert (uy <= 1.0).all(), f"{label}: (c) position.y is {uy.max():.2f} x (4 ulp32 + the sampler's step) from origin.y + t dir.y (ray {h[inner][uy.argmax()]})"
        assert (gy[~inner] <= tol[~inner] + 4 * ulp32(big[~inner])).all(), f"{label}: (c) a ray that starts under the surface or leaves through the floor is reported above the surface"
        # (b) no earlier hit: the model's g stays above -tol up to 1/8 texel before the reported t
        gm, _ = surf.gmin_upto(model, h, t - 0.125 * texel_t[h])
        eb = np.where(np.isfinite(gm), -gm / tol, 0.0)
        worst["b"] = float(eb.max())
        assert (eb <= 1.0).all(), f"{label}: (b) an earlier crossing {eb.max():.2f} x tol deep was missed (ray {h[eb.argmax()]})"
        # (d) the normal, away from the lines where it jumps
        ok = away_from_cell_boundaries(surf, pos[:, 0], pos[:, 2])
        ang = np.arccos(np.clip((nrm * surf.normal(pos[:, 0], pos[:, 2])).sum(1), -1.0, 1.0))
        assert (ang[ok] <= 1e-3).all(), f"{label}: (d) normal off by {ang[ok].max():.2e} rad"
    m = np.nonzero(st == MISS)[0]
    if m.size:
        assert np.array_equal(hits["t"][m], tm[m], equal_nan=True) and not hits["position"][m].any() and not hits["normal"][m].any(), f"{label}: a MISS carries more than t_max"
        inside = model["t1"][m] >= model["t0"][m]
        mm = m[inside]
        gm, t_at = model["gall"][mm], model["t_all"][mm]
        em = -gm / surf.ray_tol(o64[mm], d64[mm], t_at)
        worst["miss"] = float(em.max(initial=0.0))
        assert (em <= 1.0).all(), f"{label}: a MISS passes {em.max():.2f} x tol under the surface (ray {mm[em.argmax()]})"
    differ = (st != model["status"]) & ~model["grazing"]
    assert not differ.any(), f"{label}: {differ.sum()} statuses differ from the model outside grazing rays, first {np.nonzero(differ)[0][:8].tolist()}"
    return worst
