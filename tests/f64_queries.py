"""float64 model of the terrain queries, written from the definition of the queried surface (include/vrterrain.h,
"terrain queries"), not from the kernels:

    H(x, z) = SampleLevel(heightmap, linear-clamp, uv, 0.1).r * max_height,   uv = ((x, z) + world_size / 2) / world_size
            = (0.9 * bilinear(level 0) + 0.1 * bilinear(level 1)) * max_height

from the uint8 mip levels (vr_terrain_download_mip or the oracle's height_mip).  Rays are clipped to the box
x, z in [-world_size/2, world_size/2], y in [min(0, max_height), max(0, max_height)]; the first hit is found by marching the
clipped segment in steps of 1/16 of a level-0 texel along xz (max_height / 4096 in y for vertical rays) and bisecting the
first sign change of g(t) = y(t) - H64(xz(t)).
"""
import numpy as np

MISS, HIT, INVALID, STEP_LIMIT = 0, 1, 2, 3


def ulp32(x):
    """Spacing of float32 at |x| (of the smallest normal number below it)."""
    return np.spacing(np.maximum(np.abs(np.asarray(x, np.float64)), np.float64(np.finfo(np.float32).tiny)).astype(np.float32)).astype(np.float64)


class Surface64:
    def __init__(self, level0, level1, world_size, max_height):
        """level0 / level1: (h, w) uint8 mip levels 0 and 1 (a one-level chain passes level 0 twice: the sampler clamps the LOD)."""
        self.l0 = np.asarray(level0, np.float64) / 255.0
        self.l1 = np.asarray(level1, np.float64) / 255.0
        self.ws = float(world_size)
        self.mh = float(max_height)
        self.h0, self.w0 = self.l0.shape

    @staticmethod
    def _bilinear(tex, u, v):
        h, w = tex.shape
        X, Y = u * w - 0.5, v * h - 0.5
        x0, y0 = np.floor(X), np.floor(Y)
        fx, fy = X - x0, Y - y0
        xa, xb = np.clip(x0, 0, w - 1).astype(np.int64), np.clip(x0 + 1, 0, w - 1).astype(np.int64)
        ya, yb = np.clip(y0, 0, h - 1).astype(np.int64), np.clip(y0 + 1, 0, h - 1).astype(np.int64)
        t00, t10, t01, t11 = tex[ya, xa], tex[ya, xb], tex[yb, xa], tex[yb, xb]
        top, bot = t00 + (t10 - t00) * fx, t01 + (t11 - t01) * fx
        val = top + (bot - top) * fy
        ddx = ((t10 - t00) + ((t11 - t01) - (t10 - t00)) * fy) * w          # per unit of u; the cell with the larger coordinate on a boundary
        ddy = ((t01 - t00) + ((t11 - t10) - (t01 - t00)) * fx) * h
        return val, ddx, ddy

    def H(self, x, z, grad=False):
        """H64 at world (x, z) (arrays); with grad also dH/dx, dH/dz."""
        x, z = np.asarray(x, np.float64), np.asarray(z, np.float64)
        u, v = (x + 0.5 * self.ws) / self.ws, (z + 0.5 * self.ws) / self.ws
        a, ax, az = self._bilinear(self.l0, u, v)
        b, bx, bz = self._bilinear(self.l1, u, v)
        hv = (0.9 * a + 0.1 * b) * self.mh
        if not grad:
            return hv
        k = self.mh / self.ws
        return hv, (0.9 * ax + 0.1 * bx) * k, (0.9 * az + 0.1 * bz) * k

    def normal(self, x, z):
        _, gx, gz = self.H(x, z, grad=True)
        n = np.stack([-gx, np.ones_like(gx), -gz], -1)
        return n / np.linalg.norm(n, axis=-1, keepdims=True)

    def slope_bound(self, x, z):
        """S: the largest |grad H64| over the point's 3 x 3 level-0 cells.  Each gradient component is linear in the other
        coordinate on every piece between level-0 and level-1 cell boundaries, so the maximum sits at a piece corner: the
        gradient is taken on both sides of every half-texel line of the 3 x 3 block."""
        x, z = np.asarray(x, np.float64), np.asarray(z, np.float64)
        tx, tz = self.ws / self.w0, self.ws / self.h0
        cx = (np.floor((x + 0.5 * self.ws) / tx - 0.5) + 0.5) * tx - 0.5 * self.ws     # world x of the cell's lower texel centre
        cz = (np.floor((z + 0.5 * self.ws) / tz - 0.5) + 0.5) * tz - 0.5 * self.ws
        offs = np.concatenate([np.arange(-1.0, 2.01, 0.5) + e for e in (-1e-6, 1e-6)])
        best = np.zeros(x.shape)
        for ox in offs:
            for oz in offs:
                _, gx, gz = self.H(cx + ox * tx, cz + oz * tz, grad=True)
                best = np.maximum(best, np.hypot(gx, gz))
        return best

    def height_tol(self, x, z):
        """The bound of a height the device evaluates in fp32 at (x, z): 8 (ulp32(world_size) S + ulp32(max_height)) - the
        first-order effect of rounding uv, and the rounding of the result; 8 is the margin."""
        return 8.0 * (ulp32(self.ws) * self.slope_bound(x, z) + ulp32(self.mh))

    # ---- rays ------------------------------------------------------------------------------------------------------
    def clip(self, o, d, t_max):
        """Slab clip of rays (n, 3) to the box: (t0, t1, inside); the segment is [t0, t1] when inside."""
        o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
        n = o.shape[0]
        half = 0.5 * self.ws
        lo = np.array([-half, min(0.0, self.mh), -half])
        hi = np.array([half, max(0.0, self.mh), half])
        t0, t1 = np.zeros(n), np.asarray(np.broadcast_to(t_max, (n,)), np.float64).copy()
        inside = np.ones(n, bool)
        for k in range(3):
            nz = d[:, k] != 0.0
            with np.errstate(divide="ignore", invalid="ignore"):
                a, b = (lo[k] - o[:, k]) / d[:, k], (hi[k] - o[:, k]) / d[:, k]
            t0 = np.where(nz, np.maximum(t0, np.minimum(a, b)), t0)
            t1 = np.where(nz, np.minimum(t1, np.maximum(a, b)), t1)
            inside &= nz | ((o[:, k] >= lo[k]) & (o[:, k] <= hi[k]))
        inside &= t0 <= t1
        return t0, t1, inside

    def g(self, o, d, t):
        return o[..., 1] + t * d[..., 1] - self.H(o[..., 0] + t * d[..., 0], o[..., 2] + t * d[..., 2])

    def march(self, o, d, t0, t1):
        """Samples of g along [t0, t1] of every ray, flattened: (ray index, t, g, first sample of each ray)."""
        o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
        seg = np.maximum(t1 - t0, 0.0)
        step_xz = np.hypot(d[:, 0] * self.w0, d[:, 2] * self.h0) * 16.0 / self.ws        # sixteenths of a texel per unit of t
        step_y = np.abs(d[:, 1]) * 4096.0 / max(abs(self.mh), 1e-30)
        vertical = step_xz * seg < 1.0
        steps = np.where(vertical, step_y, step_xz) * seg
        cnt = np.clip(np.ceil(np.where(np.isfinite(steps), steps, 1.0)), 1, 1 << 18).astype(np.int64) + 1
        first = np.concatenate([[0], np.cumsum(cnt)])
        ridx = np.repeat(np.arange(o.shape[0]), cnt)
        k = np.arange(first[-1]) - first[ridx]
        t = t0[ridx] + seg[ridx] * (k / (cnt[ridx] - 1))
        return ridx, t, self.g(o[ridx], d[ridx], t), first

    def first_hit64(self, o, d, t_max=np.inf):
        """One march of every ray.  Returns a dict of per-ray arrays: status (MISS / HIT / INVALID); t - the first hit; gmin -
        the smallest g over the march before the hit, up to 1/8 texel (two march steps) in front of it (over the whole clipped
        segment for a miss; +inf when nothing precedes the hit) and t_at, where it was found; gall / t_all - the smallest g over
        the whole clipped segment and where; t0, t1 - the clipped segment; plus the march itself (`samples`) for gmin_upto."""
        o, d = np.asarray(o, np.float64).reshape(-1, 3), np.asarray(d, np.float64).reshape(-1, 3)
        n = o.shape[0]
        tm = np.asarray(np.broadcast_to(t_max, (n,)), np.float64)
        valid = np.isfinite(o).all(1) & np.isfinite(d).all(1) & (np.abs(d).max(1) > 0) & (tm >= 0)
        os_, ds_ = np.where(valid[:, None], o, 0.0), np.where(valid[:, None], d, [0.0, -1.0, 0.0])
        t0, t1, inside = self.clip(os_, ds_, np.where(valid, tm, 0.0))
        inside &= valid
        status = np.where(valid, MISS, INVALID)
        t_hit, gmin, t_at = np.full(n, np.nan), np.full(n, np.inf), np.full(n, np.nan)
        gall, t_all = np.full(n, np.inf), np.full(n, np.nan)
        idx = np.nonzero(inside)[0]
        out = dict(status=status, t=t_hit, gmin=gmin, t_at=t_at, gall=gall, t_all=t_all, t0=t0, t1=t1, samples=None)
        if idx.size == 0:
            return out
        ridx, t, g, first = self.march(os_[idx], ds_[idx], t0[idx], t1[idx])
        out["samples"] = (idx, first, t, g)
        eps = 1e-9 * max(1.0, abs(self.mh))                  # float64 rounding of a ray that lies in the surface (flat maps)
        lo, hi, who = [], [], []
        for j, r in enumerate(idx):
            ts, gs = t[first[j]:first[j + 1]], g[first[j]:first[j + 1]]
            k = gs.argmin()
            gall[r], t_all[r] = gs[k], ts[k]
            if gs[k] > eps:
                gmin[r], t_at[r] = gs[k], ts[k]
                continue
            k = int(np.argmax(gs <= eps))
            status[r] = HIT
            if k == 0:
                t_hit[r] = ts[0]
                continue
            if k > 2:
                m = gs[:k - 2].argmin()
                gmin[r], t_at[r] = gs[m], ts[m]
            lo.append(ts[k - 1]); hi.append(ts[k]); who.append(r)
        if who:                                              # bisection of the first sign change, all rays at once
            who, lo, hi = np.asarray(who), np.asarray(lo), np.asarray(hi)
            for _ in range(60):
                mid = 0.5 * (lo + hi)
                below = self.g(os_[who], ds_[who], mid) <= eps
                hi, lo = np.where(below, mid, hi), np.where(below, lo, mid)
            t_hit[who] = hi
        return out

    @staticmethod
    def gmin_upto(model, rays, t_end):
        """Smallest g of the model's march over [t0, t_end] for the given ray indices, and where (+inf, nan where the
        march has no sample there)."""
        gm, at = np.full(len(rays), np.inf), np.full(len(rays), np.nan)
        if model["samples"] is None:
            return gm, at
        idx, first, t, g = model["samples"]
        slot = {int(r): j for j, r in enumerate(idx)}
        for i, (r, te) in enumerate(zip(rays, t_end)):
            j = slot.get(int(r))
            if j is None:
                continue
            ts = t[first[j]:first[j + 1]]
            k = int(np.searchsorted(ts, te, side="right"))
            if k > 0:
                gs = g[first[j]:first[j] + k]
                m = gs.argmin()
                gm[i], at[i] = gs[m], ts[m]
        return gm, at

    def ray_tol(self, o, d, t):
        """Bound of |g| at a point the device reports at parameter t: the height bound there plus the fp32 rounding of
        origin + t dir, 8 ulp32(|t| |dir|) (|dir.y| / |dir| + S)."""
        o, d = np.asarray(o, np.float64).reshape(-1, 3), np.asarray(d, np.float64).reshape(-1, 3)
        x, z = o[:, 0] + t * d[:, 0], o[:, 2] + t * d[:, 2]
        S = self.slope_bound(x, z)
        dl = np.linalg.norm(d, axis=1)
        return 8.0 * (ulp32(self.ws) * S + ulp32(self.mh)) + 8.0 * ulp32(np.abs(t) * dl) * (np.abs(d[:, 1]) / dl + S)
