"""The definition of a region on a map (vr_terrain_region) in numpy float32: vectorised over the map, a Python loop over the edges, the
preparation in Python floats (doubles).  Written from the text of vrenderer_amd/csrc/vr_region.h's comment, not from its functions or
the kernel.  No culling unless asked for: every texel meets every edge.

  map          w x h texels over the world [-S/2, S/2]^2; texel i has its centre at texel coordinate i
  contours     closed; contour c has counts[c] >= 3 consecutive points, the last joined to its first; no counts: one contour
  preparation  in double, each result rounded to fp32 once (beyond fp32's range: +-FLT_MAX): per call wx = S / w, wz = S / h; soft =
               feather > 0, then inv_r2 = 1 / feather^2, R = 1 / sqrt(inv_r2) from the rounded inv_r2, else both 0; per point
               vx = (x + S/2) / S * w - 0.5, vz likewise with h; per edge a -> b from the ROUNDED vx, vz: ax = vx_a, az = vz_a,
               bz = vz_b, dx = (vx_b - vx_a) * wx, dz = (vz_b - vz_a) * wz, inv_len2 = 1 / (dx^2 + dz^2) from the rounded dx, dz - 0
               where that is no finite fp32; the distance box of an axis: bx' = ax + dx / wx,
               E = 2^-20 * ((|ax| + w) * wx + (|az| + h) * wz + |dx| + |dz|),
               [floor(min(ax, bx') - (R + E) / wx) - 1, ceil(max(ax, bx') + (R + E) / wx) + 2) clipped to the map; the span is the
               box with x1 = w; an edge with an empty span is dropped, the others keep their order; the rectangle is per axis the
               hull of the boxes' clipped ends over all edges, and nothing where that is empty or no edge is left
  a texel      ox = float(i) - ax; px = ox * wx (z likewise); up = az <= float(j); ub = bz <= float(j); m2 = px * dz; m3 = pz * dx;
               left = (up != ub) and (m2 > m3 if up else m2 < m3); soft: the path's chain from px, pz: dot = px * dx + pz * dz,
               t = dot * inv_len2 clamped to [0, 1] by comparisons, ex = px - t * dx, ez = pz - t * dz, q = (ex * ex + ez * ez) * inv_r2
  per texel    inside = XOR of left over the edges; q* = 1, then q* = q where q < q*
  weight       f0 = (t * t) * (3 - 2 * t), t = 1 - q*, where 0 < q* < 1, 1 where q* <= 0.  default: inside f = 1, outside f = f0 where
               q* < 1, else not written; FEATHER_INSIDE: inside f = 1 - f0 where q* < 1 else 1, outside not written; hard: inside f = 1
  apply        a = f * opacity; LEVEL to = target; CUT to = min(val, target); FILL to = max(val, target); PAINT per channel of the
               mask to = color[c]: val = clamp(val + a * (to - val), 0, 255); RAISE: val = clamp(val + a * target, 0, 255); the byte
               is floor(val + 0.5)

Every array operation below is one IEEE fp32 operation per element, in the written order, so the result is the device's, bit for
bit."""
import math

import numpy as np

from tests.path_model import FLT_MAX, _div, _round, _span

F = np.float32
LEVEL, CUT, FILL, RAISE, PAINT = 0, 1, 2, 3, 4
FEATHER_INSIDE = 1
MAX_POINTS = 4096
OP_IDS = {LEVEL: "level", CUT: "cut", FILL: "fill", RAISE: "raise", PAINT: "paint"}
TILE_W, TILE_H = 32, 8


def params(op=LEVEL, target=0.0, feather=0.0, opacity=1.0, color=(0.0, 0.0, 0.0, 0.0), channel_mask=1, feather_inside=False):
    """A call's parameters as a dict with fp32-exact values (what the C struct carries)."""
    return dict(op=int(op), target=float(F(target)), feather=float(F(feather)), opacity=float(F(opacity)), color=tuple(float(F(c)) for c in color),
                channel_mask=int(channel_mask), feather_inside=bool(feather_inside))


def prepare_const(p, world_size, w, h):
    S = float(F(world_size))
    soft = p["feather"] > 0.0
    k = dict(wx=_round(S / w), wz=_round(S / h), opacity=F(p["opacity"]), target=F(p["target"]), soft=soft)
    k["inv_r2"] = _round(_div(1.0, p["feather"] * p["feather"])) if soft else F(0)
    k["R"] = _round(_div(1.0, math.sqrt(float(k["inv_r2"])))) if soft else F(0)
    return k


def prepare_vertex(pt, world_size, w, h):
    S = float(F(world_size))
    x, z = float(F(pt[0])), float(F(pt[1]))
    return _round((x + S / 2) / S * w - 0.5), _round((z + S / 2) / S * h - 0.5)


def allowance(e, k, w, h):
    """E of an edge, world units (a double)."""
    return 2.0 ** -20 * ((abs(float(e["ax"])) + w) * float(k["wx"]) + (abs(float(e["az"])) + h) * float(k["wz"]) + abs(float(e["dx"])) + abs(float(e["dz"])))


def prepare_edge(a, b, k, w, h):
    wx, wz = float(k["wx"]), float(k["wz"])
    e = dict(ax=a[0], az=a[1], bz=b[1], bx=b[0], dx=_round((float(b[0]) - float(a[0])) * wx), dz=_round((float(b[1]) - float(a[1])) * wz))
    dx, dz, ax, az = float(e["dx"]), float(e["dz"]), float(e["ax"]), float(e["az"])
    len2 = dx * dx + dz * dz
    inv = 1.0 / len2 if len2 > 0.0 else 0.0
    e["inv_len2"] = F(inv) if inv <= FLT_MAX else F(0)
    bx, bz = ax + _div(dx, wx), az + _div(dz, wz)
    reach = float(k["R"]) + allowance(e, k, w, h)
    e["x0"], e["dist_x1"] = _span(min(ax, bx), max(ax, bx), _div(reach, wx), w)
    e["y0"], e["y1"] = _span(min(az, bz), max(az, bz), _div(reach, wz), h)
    e["x1"] = w
    return e


def contour_pairs(n, contours):
    """The (a, b) index pairs of the edges, in order."""
    counts = list(contours) if contours is not None and len(contours) else ([n] if n else [])
    assert sum(counts) == n and all(c >= 3 for c in counts)
    out, first = [], 0
    for m in counts:
        out += [(first + i, first + (i + 1) % m) for i in range(m)]
        first += m
    return out


def prepare(points, contours, p, world_size, w, h):
    """(k, every edge in order, the edges that meet the map in order, rect {x, y, w, h})."""
    pts = np.asarray(points, F).reshape(-1, 2)
    k = prepare_const(p, world_size, w, h)
    verts = [prepare_vertex(pt, world_size, w, h) for pt in pts]
    every = [prepare_edge(verts[i], verts[j], k, w, h) for i, j in contour_pairs(len(pts), contours)]
    live = [e for e in every if e["x1"] > e["x0"] and e["y1"] > e["y0"]]
    if not every:
        return k, every, [], (0, 0, 0, 0)
    x0, y0 = min(e["x0"] for e in every), min(e["y0"] for e in every)
    x1, y1 = max(e["dist_x1"] for e in every), max(e["y1"] for e in every)
    if x1 <= x0 or y1 <= y0 or not live:
        return k, every, [], (0, 0, 0, 0)
    return k, every, live, (x0, y0, x1 - x0, y1 - y0)


def edge_chain(e, k, w, h, xs=None, ys=None):
    """(left, q), bool and float32 (len(ys), len(xs)), of the texels xs x ys (default: the whole map) against one edge; q is None for a
    hard edge."""
    xs = np.arange(w) if xs is None else xs
    ys = np.arange(h) if ys is None else ys
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        fj = ys.astype(F)[:, None]
        ox = xs.astype(F)[None, :] - e["ax"]
        oz = fj - e["az"]
        px, pz = ox * k["wx"], oz * k["wz"]
        up, ub = e["az"] <= fj, e["bz"] <= fj
        m2, m3 = px * e["dz"], pz * e["dx"]
        left = (up != ub) & np.where(up, m2 > m3, m2 < m3)
        if not k["soft"]:
            return left, None
        dot = px * e["dx"] + pz * e["dz"]
        t0 = dot * e["inv_len2"]
        t1 = np.where(t0 < F(0), F(0), t0)
        t = np.where(t1 > F(1), F(1), t1).astype(F)
        ex, ez = px - t * e["dx"], pz - t * e["dz"]
        d2 = ex * ex + ez * ez
        q = (d2 * k["inv_r2"]).astype(F)
    return left, q


def classify(edges, k, w, h, cull=False):
    """(inside, q*) of every texel.  cull=True: each 32 x 8 tile of the map meets only the edges whose spans meet it - the device's walk."""
    inside, best = np.zeros((h, w), bool), np.full((h, w), F(1))
    if not cull:
        for e in edges:
            left, q = edge_chain(e, k, w, h)
            inside ^= left
            if q is not None:
                with np.errstate(invalid="ignore"):
                    best = np.where(q < best, q, best).astype(F)
        return inside, best
    for ty in range(0, h, TILE_H):
        for tx in range(0, w, TILE_W):
            xs, ys = np.arange(tx, min(tx + TILE_W, w)), np.arange(ty, min(ty + TILE_H, h))
            sl = (slice(ys[0], ys[-1] + 1), slice(xs[0], xs[-1] + 1))
            for e in edges:
                if not (e["x0"] <= xs[-1] and e["x1"] > xs[0] and e["y0"] <= ys[-1] and e["y1"] > ys[0]):
                    continue
                left, q = edge_chain(e, k, w, h, xs, ys)
                inside[sl] ^= left
                if q is not None:
                    with np.errstate(invalid="ignore"):
                        best[sl] = np.where(q < best[sl], q, best[sl])
    return inside, best


def weight(inside, q, k, p):
    """(covered, f)."""
    if not k["soft"]:
        return inside.copy(), np.where(inside, F(1), F(0)).astype(F)
    near = q < F(1)
    with np.errstate(invalid="ignore", over="ignore"):
        t = F(1) - q
        f0 = np.where(q <= F(0), F(1), (t * t) * (F(3) - F(2) * t)).astype(F)
    if p["feather_inside"]:
        return inside.copy(), np.where(inside, np.where(near, F(1) - f0, F(1)), F(0)).astype(F)
    covered = inside | near
    return covered, np.where(inside, F(1), np.where(near, f0, F(0))).astype(F)


def region(texels, points, p, world_size, contours=None, detail=None, cull=False):
    """One call on a copy of `texels` ((h, w) uint8 for the heightmap, (h, w, 4) uint8 for the albedo) -> (new texels, rect).  `detail`,
    a dict, receives per texel inside, q (1 where no edge is nearer than the feather), f (0 where uncovered), covered, and the prepared
    constants and edges."""
    h, w = texels.shape[:2]
    k, every, edges, rect = prepare(points, contours, p, world_size, w, h)
    inside, q = classify(edges, k, w, h, cull=cull)
    covered, f = weight(inside, q, k, p)
    a = f * k["opacity"]
    val = texels.astype(F).reshape(h, w, -1)
    out = val.copy()
    for c in range(val.shape[2]):
        if not p["channel_mask"] >> c & 1:
            continue
        v = val[..., c]
        if p["op"] == RAISE:
            out[..., c] = np.minimum(np.maximum(v + a * k["target"], F(0)), F(255))
            continue
        if p["op"] == PAINT:
            to = np.full((h, w), F(p["color"][c]))
        elif p["op"] == CUT:
            to = np.minimum(v, k["target"])
        elif p["op"] == FILL:
            to = np.maximum(v, k["target"])
        else:
            to = np.full((h, w), k["target"])
        out[..., c] = np.minimum(np.maximum(v + a * (to - v), F(0)), F(255))
    res = np.where(covered[..., None], np.floor(out + F(0.5)).astype(np.uint8), texels.reshape(h, w, -1)).astype(np.uint8)
    if detail is not None:
        detail.update(inside=inside, q=q, f=f, covered=covered, prepared=k, edges=edges, every_edge=every, rect=tuple(rect))
    return res.reshape(texels.shape), tuple(rect)
