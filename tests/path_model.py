"""The definition of a path on a map (vr_terrain_path) in numpy float32: vectorised over the map, a Python loop over the segments, the
preparation in Python floats (doubles).  Written from the text of vrenderer_amd/csrc/vr_path.h's comment, not from its functions or
the kernel.  No culling: every texel meets every segment.

  map          w x h texels over the world [-S/2, S/2]^2; texel i has its centre at texel coordinate i
  segments     n points make n - 1 segments (point s, point s + 1); closed: one more, (point n - 1, point 0); n == 1: (point 0, point 0)
  preparation  in double, each result rounded to fp32 once (beyond fp32's range: +-FLT_MAX): per call wx = S / w, wz = S / h,
               inv_r2 = 1 / radius^2, h2 = hardness^2, k = 1 / (1 - h2) (from the unrounded h2), R = 1 / sqrt(inv_r2) from the rounded
               inv_r2; per segment ax = (xa + S/2) / S * w - 0.5, az likewise with h, dx = xb - xa, dz = zb - za,
               inv_len2 = 1 / (dx^2 + dz^2) from the rounded dx, dz - 0 where that is no finite fp32 - ha, dh = hb - ha; the span of
               an axis, from the rounded values: bx = ax + dx / wx, E = 2^-20 * ((|ax| + w) * wx + (|az| + h) * wz + |dx| + |dz|),
               [floor(min(ax, bx) - (R + E) / wx) - 1, ceil(max(ax, bx) + (R + E) / wx) + 2) clipped to the map, an end that is not
               a number clipping to the wide side; a segment with an empty span is dropped, the others keep their order
  a texel      ox = float(i) - ax; px = ox * wx; (z likewise); dot = px * dx + pz * dz; t0 = dot * inv_len2; t = t0 clamped to [0, 1] by
               comparisons (a NaN stays); ex = px - t * dx; ez = pz - t * dz; d2 = ex * ex + ez * ez; q = d2 * inv_r2
  the winner   in list order from q* = 1: a segment wins where q < q* (strict); a texel none wins is not written
  apply        f = 1 where q <= h2, else u = (1 - q) * k, f = (u * u) * (3 - 2 * u); target = ha + t * dh; a = f * opacity;
               LEVEL to = target; CUT to = min(val, target); FILL to = max(val, target); PAINT per channel of the mask to = color[c];
               val = clamp(val + a * (to - val), 0, 255); the byte is floor(val + 0.5)

Every array operation below is one IEEE fp32 operation per element, in the written order, so the result is the device's, bit for
bit."""
import math

import numpy as np

F = np.float32
FLT_MAX = float(np.finfo(np.float32).max)
LEVEL, CUT, FILL, PAINT = 0, 1, 2, 3
CLOSED = 1
MAX_POINTS = 4096
OPS = (("level", LEVEL), ("cut", CUT), ("fill", FILL), ("paint", PAINT))


def params(radius, hardness=0.0, opacity=1.0, op=LEVEL, color=(0.0, 0.0, 0.0, 0.0), channel_mask=1, closed=False):
    """A call's parameters as a dict with fp32-exact values (what the C struct carries)."""
    return dict(radius=float(F(radius)), hardness=float(F(hardness)), opacity=float(F(opacity)), op=int(op), color=tuple(float(F(c)) for c in color),
                channel_mask=int(channel_mask), closed=bool(closed))


def _round(v):
    return F(min(max(v, -FLT_MAX), FLT_MAX))


def _div(a, b):
    """a / b as IEEE doubles divide (Python raises where C gives an infinity or a NaN)."""
    if b == 0.0:
        return math.nan if a == 0.0 or math.isnan(a) else math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def prepare_const(p, world_size, w, h):
    S = float(F(world_size))
    h2 = p["hardness"] * p["hardness"]
    k = dict(wx=_round(S / w), wz=_round(S / h), inv_r2=_round(_div(1.0, p["radius"] * p["radius"])), h2=F(h2), k=F(1.0 / (1.0 - h2)), opacity=F(p["opacity"]))
    k["R"] = _round(_div(1.0, math.sqrt(float(k["inv_r2"]))))
    return k


def _span(lo, hi, r, n):
    a, b = lo - r, hi + r
    if math.isfinite(a):
        a = math.floor(a) - 1.0
    if math.isfinite(b):
        b = math.ceil(b) + 2.0
    s0 = 0 if not a > 0.0 else (int(a) if a < n else n)            # an end that is not a number clips to the map's edge
    s1 = n if not b < n else (int(b) if b > 0.0 else 0)
    return s0, s1


def prepare_segment(a, b, k, world_size, w, h):
    """a, b: (x, z, height) -> dict of the prepared segment."""
    S = float(F(world_size))
    xa, za, ha = (float(F(v)) for v in a[:3])
    xb, zb, hb = (float(F(v)) for v in b[:3])
    s = dict(ax=_round((xa + S / 2) / S * w - 0.5), az=_round((za + S / 2) / S * h - 0.5), dx=_round(xb - xa), dz=_round(zb - za), ha=F(ha), dh=F(hb - ha))
    dx, dz, ax, az, wx, wz = float(s["dx"]), float(s["dz"]), float(s["ax"]), float(s["az"]), float(k["wx"]), float(k["wz"])
    len2 = dx * dx + dz * dz
    inv = 1.0 / len2 if len2 > 0.0 else 0.0
    s["inv_len2"] = F(inv) if inv <= FLT_MAX else F(0)
    bx, bz = ax + _div(dx, wx), az + _div(dz, wz)
    E = 2.0 ** -20 * ((abs(ax) + w) * wx + (abs(az) + h) * wz + abs(dx) + abs(dz))
    reach = float(k["R"]) + E
    s["x0"], s["x1"] = _span(min(ax, bx), max(ax, bx), _div(reach, wx), w)
    s["y0"], s["y1"] = _span(min(az, bz), max(az, bz), _div(reach, wz), h)
    return s


def segments_of(points, closed):
    """The (a, b) index pairs of a path of n points."""
    n = len(points)
    if n == 0:
        return []
    if n == 1:
        return [(0, 0)]
    return [(i, (i + 1) % n) for i in range(n if closed else n - 1)]


def prepare(points, p, world_size, w, h):
    """(k, the segments that meet the map in order, rect {x, y, w, h})."""
    pts = np.asarray(points, F)
    pts = pts.reshape(-1, pts.shape[-1] if pts.ndim == 2 and pts.size else 3)
    k = prepare_const(p, world_size, w, h)
    segs = [prepare_segment(pts[i], pts[j], k, world_size, w, h) for i, j in segments_of(pts, p["closed"])]
    live = [s for s in segs if s["x1"] > s["x0"] and s["y1"] > s["y0"]]
    if not live:
        return k, live, (0, 0, 0, 0)
    x0, y0 = min(s["x0"] for s in live), min(s["y0"] for s in live)
    return k, live, (x0, y0, max(s["x1"] for s in live) - x0, max(s["y1"] for s in live) - y0)


def texel_chain(s, k, w, h):
    """(q, t), float32 (h, w), of every texel of the map against one segment."""
    with np.errstate(invalid="ignore", over="ignore"):
        ox = np.arange(w, dtype=F)[None, :] - s["ax"]
        oz = np.arange(h, dtype=F)[:, None] - s["az"]
        px, pz = ox * k["wx"], oz * k["wz"]
        dot = px * s["dx"] + pz * s["dz"]
        t0 = dot * s["inv_len2"]
        t1 = np.where(t0 < F(0), F(0), t0)
        t = np.where(t1 > F(1), F(1), t1).astype(F)
        ex, ez = px - t * s["dx"], pz - t * s["dz"]
        d2 = ex * ex + ez * ez
        q = (d2 * k["inv_r2"]).astype(F)
    return q, t


def falloff(q, k):
    """f of covered texels (q < 1); means nothing elsewhere."""
    with np.errstate(invalid="ignore", over="ignore"):
        u = (F(1) - q) * k["k"]
        f = (u * u) * (F(3) - F(2) * u)
        return np.where(q <= k["h2"], F(1), f).astype(F)


def path(texels, points, p, world_size, detail=None):
    """One call on a copy of `texels` ((h, w) uint8 for the heightmap, (h, w, 4) uint8 for the albedo) -> (new texels, rect).  `detail`,
    a dict, receives per texel q (1 where uncovered), t, winner (the index among the segments that meet the map, -1: none), f (0 where
    uncovered), covered, and the prepared constants and segments."""
    h, w = texels.shape[:2]
    k, segs, rect = prepare(points, p, world_size, w, h)
    best_q, best_t = np.full((h, w), F(1)), np.zeros((h, w), F)
    winner = np.full((h, w), -1, np.int32)
    ha, dh = np.zeros((h, w), F), np.zeros((h, w), F)
    for i, s in enumerate(segs):
        q, t = texel_chain(s, k, w, h)
        with np.errstate(invalid="ignore"):
            wins = q < best_q
        best_q, best_t = np.where(wins, q, best_q).astype(F), np.where(wins, t, best_t).astype(F)
        winner[wins] = i
        ha[wins], dh[wins] = s["ha"], s["dh"]
    covered = winner >= 0
    f = np.where(covered, falloff(best_q, k), F(0)).astype(F)
    with np.errstate(invalid="ignore"):
        target = ha + best_t * dh
    a = f * k["opacity"]
    val = texels.astype(F).reshape(h, w, -1)
    out = val.copy()
    for c in range(val.shape[2]):
        if not p["channel_mask"] >> c & 1:
            continue
        v = val[..., c]
        if p["op"] == PAINT:
            to = np.full((h, w), F(p["color"][c]))
        elif p["op"] == CUT:
            to = np.minimum(v, target)
        elif p["op"] == FILL:
            to = np.maximum(v, target)
        else:
            to = target
        out[..., c] = np.minimum(np.maximum(v + a * (to - v), F(0)), F(255))
    res = np.where(covered[..., None], np.floor(out + F(0.5)).astype(np.uint8), texels.reshape(h, w, -1)).astype(np.uint8)
    if detail is not None:
        detail.update(q=best_q, t=best_t, winner=winner, f=f, covered=covered, target=target, prepared=k, segments=segs, rect=tuple(rect))
    return res.reshape(texels.shape), tuple(rect)
