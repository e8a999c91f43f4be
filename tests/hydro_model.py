"""The definition of hydraulic erosion under a brush mask (vr_terrain_erode_hydraulic) in numpy float32: vectorised over the map, a
Python loop over the sweeps and the four neighbours.  Written from the stated definition, not from the header or the kernel:

  mask       erode_model.mask_of: m_c = max over the kept dabs that cover c of weight * strength, 0 where none does; the rectangle
             is the hull of the kept spans
  state      h_c the terrain, starts as the stored byte; d_c the water, starts as rain * m_c; s_c the sediment, starts at 0
  per call   keep = 1 - evaporation
  sweep      every cell from the previous sweep's state only: dd = ds = out = 0, then for the neighbours n inside the map in the
             order (dx, dy) = (0,-1) (-1,0) (1,0) (0,1), with w = min(m_c, m_n), nothing unless w > 0, S = h + d:
               S_c >= S_n: phi = min(flow * (S_c - S_n), 0.25) * w; q = phi * d_c; ts = phi * s_c; dd -= q; ds -= ts; out += q
               otherwise:  phi = min(flow * (S_n - S_c), 0.25) * w; q = phi * d_n; ts = phi * s_n; dd += q; ds += ts
             then d1 = max(d_c + dd, 0), s1 = max(s_c + ds, 0), C = capacity * out, and
               s1 < C:     e = (dissolve * (C - s1)) * m_c; h' = h_c - e; s' = s1 + e
               otherwise:  g = deposit * (s1 - C);          h' = h_c + g; s' = s1 - g
             d' = d1 * keep + rain * m_c, each product and the sum rounded
  end        a texel with m_c > 0 is stored as floor(min(max(h + s, 0), 255) + 0.5); one with m_c == 0 is not written

Every array operation below is one IEEE fp32 operation per element, in the written order, so the result is the device's, bit
for bit; numpy keeps subnormals, and so does the device."""
import numpy as np

from tests.erode_model import _shifted, mask_of

F = np.float32
NEIGHBOURS = ((0, -1), (-1, 0), (1, 0), (0, 1))


def sweep(h, d, s, m, rain, flow, capacity, dissolve, deposit, keep, neighbours=NEIGHBOURS):
    """One sweep over the whole map: float32 (h0, w0) planes -> (h', d', s').  (`neighbours`: another order is another operation - the
    sensitivity checks of tests/erosion_state.py pass one to show that a test can tell.)"""
    rain, flow, capacity, dissolve, deposit, keep = F(rain), F(flow), F(capacity), F(dissolve), F(deposit), F(keep)
    zero, quarter = F(0), F(0.25)
    dd, ds, out = np.zeros_like(h), np.zeros_like(h), np.zeros_like(h)
    S = h + d
    for dx, dy in neighbours:
        hn, dn, sn, mn = (_shifted(a, dx, dy, zero) for a in (h, d, s, m))   # outside the map: mask 0, no edge
        w = np.where(m < mn, m, mn)
        live = w > zero
        Sn = hn + dn
        gives = S >= Sn
        f = flow * np.where(gives, S - Sn, Sn - S)
        phi = np.where(f < quarter, f, quarter) * w
        q = phi * np.where(gives, d, dn)
        ts = phi * np.where(gives, s, sn)
        out_ = live & gives
        in_ = live & ~gives
        dd = np.where(out_, dd - q, np.where(in_, dd + q, dd)).astype(F)
        ds = np.where(out_, ds - ts, np.where(in_, ds + ts, ds)).astype(F)
        out = np.where(out_, out + q, out).astype(F)
    dsum, ssum = d + dd, s + ds
    d1 = np.where(dsum > zero, dsum, zero).astype(F)
    s1 = np.where(ssum > zero, ssum, zero).astype(F)
    C = capacity * out
    e = (dissolve * (C - s1)) * m
    g = deposit * (s1 - C)
    takes = s1 < C
    h2 = np.where(takes, h - e, h + g).astype(F)
    s2 = np.where(takes, s1 + e, s1 - g).astype(F)
    d2 = (d1 * keep + rain * m).astype(F)
    return h2, d2, s2


def state(texels, dabs, world_size, iterations, rain, flow, capacity, dissolve, deposit, evaporation, neighbours=NEIGHBOURS, keep=None):
    """(h, d, s, mask, rect) after `iterations` sweeps: the fp32 planes before the final rounding.  (`keep`: another value than
    1 - evaporation, for the sensitivity checks only.)"""
    m, rect = mask_of(texels.shape, dabs, world_size)
    keep = F(F(1.0) - F(evaporation)) if keep is None else F(keep)
    h = texels.astype(F)
    d = (F(rain) * m).astype(F)
    s = np.zeros_like(h)
    with np.errstate(under="ignore"):
        for _ in range(int(iterations)):
            h, d, s = sweep(h, d, s, m, rain, flow, capacity, dissolve, deposit, keep, neighbours)
    return h, d, s, m, rect


def hydro(texels, dabs, world_size, iterations, rain, flow, capacity, dissolve, deposit, evaporation):
    """`iterations` sweeps on a copy of `texels` ((h, w) uint8) -> (new texels, rect)."""
    h, _, s, m, rect = state(texels, dabs, world_size, iterations, rain, flow, capacity, dissolve, deposit, evaporation)
    stored = np.floor(np.minimum(np.maximum(h + s, F(0)), F(255)) + F(0.5)).astype(np.uint8)
    return np.where(m > F(0), stored, texels).astype(np.uint8), rect
