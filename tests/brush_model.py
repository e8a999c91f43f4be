"""The definition of a brush stroke (vr_terrain_brush) in numpy float32: vectorised over the map, a Python loop over the dabs, the
preparation in Python floats (doubles).  Written from the stated definition, not from the kernel:

  map          w0 x h0 texels span the world [-S/2, S/2]^2; texel i has its centre at texel coordinate i
  preparation  in double, each result rounded to fp32 once: cx = (x + S/2) / S * w0 - 0.5, cz likewise with h0,
               sx = S / (w0 * radius), sz = S / (h0 * radius) (the radius is radius * w0 / S texels), h2 = hardness^2, k = 1 / (1 - h2); the span of an axis is
               [floor(cx - 1/sx) - 1, ceil(cx + 1/sx) + 2) from the rounded cx and sx, clipped to the map; a span of at most 5 x 5
               texels none of which the dab covers is empty
  weight       u = (float(i) - cx) * sx, v = (float(j) - cz) * sz, q = u*u + v*v; outside when not q < 1; f = 1 when q <= h2, else
               t = (1 - q) * k, f = (t*t) * (3 - 2*t)
  stroke       val starts as the stored byte; per covering dab, in order, with a = f * strength:
               RAISE val + f * strength; FLATTEN val + a * (target - val); SMOOTH val + a * (m - val) with m = float(sum of the
               3 x 3 clamped neighbourhood before the stroke) * 0.11111111f; PAINT per masked channel val + a * (color[c] - val);
               then min(max(val, 0), 255); after the last dab the byte is floor(val + 0.5)

Every array operation below is one IEEE fp32 operation per element, in the written order, so the result is the device's, bit
for bit."""
import math

import numpy as np

RAISE, FLATTEN, SMOOTH, PAINT = 0, 1, 2, 3
F = np.float32


def _axis_span(c, s, n):
    c, s = float(c), float(s)
    r = 1.0 / s if s != 0.0 else math.inf
    a, b = c - r, c + r
    if math.isfinite(a):
        a = math.floor(a) - 1.0
    if math.isfinite(b):
        b = math.ceil(b) + 2.0
    lo = 0 if not a > 0.0 else (int(a) if a < n else n)         # an end that is not a number clips to the map's edge
    hi = n if not b < n else (int(b) if b > 0.0 else 0)
    return lo, hi


def prepare(dab, world_size, w0, h0):
    """(x, z, radius, hardness, strength) as fp32 values -> dict of the prepared dab."""
    with np.errstate(over="ignore"):
        x, z, radius, hardness, strength = (float(F(v)) for v in dab[:5])
        S = float(F(world_size))
        h2 = hardness * hardness
        d = dict(cx=F((x + S / 2) / S * w0 - 0.5), cz=F((z + S / 2) / S * h0 - 0.5), sx=F(S / (w0 * radius)), sz=F(S / (h0 * radius)),
                 h2=F(h2), k=F(1.0 / (1.0 - h2)), strength=F(strength))
    d["x0"], d["x1"] = _axis_span(d["cx"], d["sx"], w0)
    d["y0"], d["y1"] = _axis_span(d["cz"], d["sz"], h0)
    # a span of at most 5 x 5 texels is tested texel by texel: a small dab between the texel centres covers nothing and misses the map
    if 0 < d["x1"] - d["x0"] <= 5 and 0 < d["y1"] - d["y0"] <= 5 and not weight(d, w0, h0)[0][d["y0"]:d["y1"], d["x0"]:d["x1"]].any():
        d["x1"] = d["x0"]
    return d


def weight(d, w0, h0):
    """(inside, f): boolean (h0, w0) and float32 (h0, w0); f means nothing outside."""
    with np.errstate(invalid="ignore", over="ignore"):
        u = (np.arange(w0, dtype=F)[None, :] - d["cx"]) * d["sx"]
        v = (np.arange(h0, dtype=F)[:, None] - d["cz"]) * d["sz"]
        q = u * u + v * v
        inside = q < F(1)
        t = (F(1) - q) * d["k"]
        f = (t * t) * (F(3) - F(2) * t)
        f = np.where(q <= d["h2"], F(1), f).astype(F)
    return inside, f


def mean9(hm):
    """m of SMOOTH for every texel of the map as it is now."""
    p = np.pad(hm.astype(np.int32), 1, mode="edge")
    h, w = hm.shape
    total = sum(p[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3))
    return total.astype(F) * F(0.11111111)


def rect_of(prepared):
    """{x, y, w, h} of the hull of the non-empty spans, (0, 0, 0, 0) when there is none."""
    live = [d for d in prepared if d["x1"] > d["x0"] and d["y1"] > d["y0"]]
    if not live:
        return (0, 0, 0, 0)
    x0, y0 = min(d["x0"] for d in live), min(d["y0"] for d in live)
    return (x0, y0, max(d["x1"] for d in live) - x0, max(d["y1"] for d in live) - y0)


def stroke(texels, op, dabs, world_size, target=0.0, color=(0, 0, 0, 0), channels=0xF):
    """One stroke on a copy of `texels` ((h, w) uint8 for the heightmap ops, (h, w, 4) uint8 for PAINT) -> (new texels, rect)."""
    h0, w0 = texels.shape[:2]
    rows = np.asarray(dabs, F)
    rows = rows.reshape(-1, 5) if rows.ndim == 1 else rows                 # (n, 5), or (n, 8) as the C struct lays a dab out
    prepared = [prepare(d, world_size, w0, h0) for d in rows]
    val = texels.astype(F)
    m = mean9(texels) if op == SMOOTH else None
    with np.errstate(invalid="ignore", over="ignore"):
        for d in prepared:
            inside, f = weight(d, w0, h0)
            if op == RAISE:
                new = val + f * d["strength"]
            else:
                a = f * d["strength"]
                if op == FLATTEN:
                    new = val + a * (F(target) - val)
                elif op == SMOOTH:
                    new = val + a * (m - val)
                else:
                    new = val.copy()
                    for c in range(4):
                        if channels >> c & 1:
                            new[..., c] = val[..., c] + a * (F(color[c]) - val[..., c])
            new = np.minimum(np.maximum(new, F(0)), F(255))
            val = np.where(inside if op != PAINT else inside[..., None], new, val).astype(F)
    return np.floor(val + F(0.5)).astype(np.uint8), rect_of(prepared)
