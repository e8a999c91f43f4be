"""The definition of thermal erosion under a brush mask (vr_terrain_erode) in numpy float32: vectorised over the map, a Python loop
over the dabs, the sweeps and the eight neighbours.  Written from the stated definition, not from the header or the kernel:

  mask       the dabs are prepared as for a stroke on the heightmap (brush_model.prepare, empty dabs dropped); the mask of texel c is
             m_c = max over the kept dabs that cover it of f * strength (f: brush_model.weight), 0 where none does; the rectangle
             is the hull of the kept spans (brush_model.rect_of)
  state      h_c, fp32, starts as the stored byte
  iteration  every cell from the previous iteration's state only: acc = 0, then for the neighbours inside the map in the order
             (dx, dy) = (-1,-1) (0,-1) (1,-1) (-1,0) (1,0) (-1,1) (0,1) (1,1):
               T = talus on the axes, talus * 1.41421354f (one fp32 product) on the diagonals
               w = min(m_c, m_n); nothing unless w > 0
               h_c >= h_n: e = (h_c - h_n) - T, and if e > 0: acc = acc - (rate * e) * w
               otherwise:  e = (h_n - h_c) - T, and if e > 0: acc = acc + (rate * e) * w
             then h_c' = h_c + acc; nothing is clamped between iterations
  end        a texel with m_c > 0 is stored as floor(min(max(h, 0), 255) + 0.5); one with m_c == 0 is not written

Every array operation below is one IEEE fp32 operation per element, in the written order, so the result is the device's, bit
for bit."""
import numpy as np

from tests.brush_model import prepare, rect_of, weight

F = np.float32
NEIGHBOURS = ((-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1))


def _rows(dabs):
    rows = np.asarray(dabs, F)
    return rows.reshape(-1, 5) if rows.ndim == 1 else rows           # (n, 5), or (n, 8) as the C struct lays a dab out


def mask_of(shape, dabs, world_size):
    """(mask, rect): float32 (h0, w0) and (x, y, w, h)."""
    h0, w0 = shape
    prepared = [prepare(d, world_size, w0, h0) for d in _rows(dabs)]
    m = np.zeros((h0, w0), F)
    with np.errstate(invalid="ignore", over="ignore"):
        for d in prepared:
            if not (d["x1"] > d["x0"] and d["y1"] > d["y0"]):
                continue
            inside, f = weight(d, w0, h0)
            a = (f * d["strength"]).astype(F)
            m = np.where(inside & (a > m), a, m).astype(F)
    return m, rect_of(prepared)


def _shifted(a, dx, dy, fill):
    """a[y + dy, x + dx], `fill` where that lies outside the map."""
    h, w = a.shape
    out = np.full((h, w), fill, a.dtype)
    ys, yd = (slice(dy, h), slice(0, h - dy)) if dy >= 0 else (slice(0, h + dy), slice(-dy, h))
    xs, xd = (slice(dx, w), slice(0, w - dx)) if dx >= 0 else (slice(0, w + dx), slice(-dx, w))
    out[yd, xd] = a[ys, xs]
    return out


def sweep(h, m, talus, rate, neighbours=NEIGHBOURS):
    """One iteration over the whole map: float32 (h0, w0) -> float32 (h0, w0).  (`neighbours`: another order is another operation -
    the sensitivity checks of tests/erosion_state.py pass one to show that a test can tell.)"""
    talus, rate = F(talus), F(rate)
    diagonal = F(talus * F(1.41421354))
    acc = np.zeros_like(h)
    for dx, dy in neighbours:
        T = diagonal if dx and dy else talus
        hn, mn = _shifted(h, dx, dy, F(0)), _shifted(m, dx, dy, F(0))        # outside the map: mask 0, no edge
        w = np.minimum(m, mn)
        live = w > F(0)
        down = h >= hn
        e_down = (h - hn) - T
        e_up = (hn - h) - T
        minus = acc - (rate * e_down) * w
        plus = acc + (rate * e_up) * w
        acc = np.where(live & down & (e_down > F(0)), minus, np.where(live & ~down & (e_up > F(0)), plus, acc)).astype(F)
    return (h + acc).astype(F)


def state(texels, dabs, world_size, iterations, talus, rate, neighbours=NEIGHBOURS):
    """(h, mask, rect) after `iterations` sweeps: the fp32 plane before the final rounding."""
    m, rect = mask_of(texels.shape, dabs, world_size)
    h = texels.astype(F)
    with np.errstate(under="ignore"):
        for _ in range(int(iterations)):
            h = sweep(h, m, talus, rate, neighbours)
    return h, m, rect


def erode(texels, dabs, world_size, iterations, talus, rate):
    """`iterations` sweeps on a copy of `texels` ((h, w) uint8) -> (new texels, rect)."""
    h, m, rect = state(texels, dabs, world_size, iterations, talus, rate)
    stored = np.floor(np.minimum(np.maximum(h, F(0)), F(255)) + F(0.5)).astype(np.uint8)
    return np.where(m > F(0), stored, texels).astype(np.uint8), rect
