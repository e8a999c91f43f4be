"""Model of the decoded tables of a map (what every tile pass and every height query reads instead of the mip chain), in numpy, written
from the table definitions - the DevTex comments of vrenderer_amd/csrc/vr_internal.h - and, for what an in-place change has to
refresh, from the header text of vrenderer_amd/csrc/vr_dirty.h.  Input: one level of a chain as uint8; output: that level's tables.

    heightmap (h, w) uint8                 t(x, y) = float32(byte) / float32(255) of the clamp-addressed texel (x, y)
      quad   (h + 2, w + 2) uint32         entry (ix, iy): bytes (ix-1, iy-1) | (ix, iy-1) << 8 | (ix-1, iy) << 16 | (ix, iy) << 24
      quadf  (h + 2, w + 2, 4) float32     (t00, t10 - t00, t01, t11 - t01) of the same four texels
      fast   (h + 3, w + 3, 4) float32     the same footprint, one more entry per axis
    albedo (h, w, 4) uint8                 lin(c) = float32(eotf64(c / 255)), the context's 256-entry table
      fast   (h + 3, w + 3, 4) float32     (lin r, lin g, lin b, 0) of the clamp-addressed texel (ix-1, iy-1)
      rgbf   (h, w, 4) float32             (lin r, lin g, lin b, 0) of texel (ix, iy)

Everything is exact and compared as bits (floats viewed as uint32), with no tolerance anywhere: the division is one IEEE division,
correctly rounded, each difference one fp32 subtraction (equal neighbours give +0.0), and an entry of the sRGB table is a float64
value rounded once.  That value comes out of the C library's pow, which need not be correctly rounded: lut_condition() moves each
of the 256 float64 values by up to 4 ulp either way and asks that it still rounds to the same float32; an entry that does not is
listed with both candidates and a texel with that code may hold either.  tests/test_tables_model_cpu.py asserts that no entry pow
computes is listed; the one that is - code 0, an exact 0.0 that the move carries below zero - comes from a division and stays +0.0."""
import numpy as np

TABLES = {"height": ("quad", "quadf", "fast"), "albedo": ("fast", "rgbf")}


# ---- the two decodes -----------------------------------------------------------------------------------------------------------------
def unorm8():
    """float32(b) / float32(255) for the 256 bytes: numpy's float32 division is IEEE's."""
    t = np.arange(256, dtype=np.float32) / np.float32(255.0)
    assert t.dtype == np.float32
    return t


def eotf64(c):
    c = np.asarray(c, np.float64)
    return np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)


def srgb_lut():
    return eotf64(np.arange(256, dtype=np.float64) / 255.0).astype(np.float32)


def lut_condition(ulps=4):
    """{code: (float32 candidates)} for every code whose float64 value, moved by up to `ulps` ulp (float64) either way, does not round
    to one float32."""
    v = eotf64(np.arange(256, dtype=np.float64) / 255.0)
    lo, hi = v.copy(), v.copy()
    for _ in range(ulps):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
    a, b = lo.astype(np.float32), hi.astype(np.float32)
    return {int(i): (a[i], b[i]) for i in np.nonzero(a.view(np.uint32) != b.view(np.uint32))[0]}


def lut_candidates():
    """The sRGB table and its alternative: equal wherever lut_condition() holds.  The codes of the linear segment (c / 255 <= 0.04045:
    0 .. 10) have no alternative whatever the condition says: their value is one IEEE division, which no C library changes.  (Code 0
    is the one entry the condition reports - an exact 0.0 moved below zero rounds to -0.0 - and the table holds +0.0.)"""
    lut, alt = srgb_lut(), srgb_lut()
    for code, (a, b) in lut_condition().items():
        if code / 255.0 > 0.04045:
            alt[code] = b if lut[code].view(np.uint32) == a.view(np.uint32) else a
    return lut, alt


# ---- the tables of one level -----------------------------------------------------------------------------------------------------------
def _clamped(n, entries, shift):
    """Texel index of entries 0 .. entries - 1 of one axis of an n-texel level: clamp(i + shift, 0, n - 1)."""
    return np.clip(np.arange(entries) + shift, 0, n - 1)


def _footprint(level, extra):
    """The four clamp-addressed texels (ix-1, iy-1) (ix, iy-1) (ix-1, iy) (ix, iy) of every entry of a (h + extra, w + extra) table."""
    h, w = level.shape
    x0, x1 = _clamped(w, w + extra, -1), _clamped(w, w + extra, 0)
    y0, y1 = _clamped(h, h + extra, -1), _clamped(h, h + extra, 0)
    return level[y0][:, x0], level[y0][:, x1], level[y1][:, x0], level[y1][:, x1]


def _decoded(level, extra):
    t = unorm8()
    t00, t10, t01, t11 = (t[b] for b in _footprint(level, extra))
    out = np.stack([t00, t10 - t00, t01, t11 - t01], -1)
    assert out.dtype == np.float32
    return out


def height_tables(level):
    """{'quad', 'quadf', 'fast'} of one (h, w) uint8 level of a heightmap's chain."""
    level = np.asarray(level, np.uint8)
    assert level.ndim == 2
    b00, b10, b01, b11 = (b.astype(np.uint32) for b in _footprint(level, 2))
    return {"quad": b00 | (b10 << np.uint32(8)) | (b01 << np.uint32(16)) | (b11 << np.uint32(24)), "quadf": _decoded(level, 2), "fast": _decoded(level, 3)}


def albedo_tables(level, lut=None):
    """{'fast', 'rgbf'} of one (h, w, 4) uint8 level of an albedo's chain."""
    level = np.asarray(level, np.uint8)
    assert level.ndim == 3 and level.shape[2] == 4
    lut = srgb_lut() if lut is None else lut
    h, w = level.shape[:2]
    rgbf = np.zeros((h, w, 4), np.float32)
    rgbf[..., :3] = lut[level[..., :3]]
    return {"fast": rgbf[_clamped(h, h + 3, -1)][:, _clamped(w, w + 3, -1)], "rgbf": rgbf}


def tables(which, level, lut=None):
    return height_tables(level) if which == "height" else albedo_tables(level, lut)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def mismatches(which, got, level):
    """[(table, (iy, ix), device value, model value)] - the first entry of every table of `got` (one level's dict, as TerrainPass.Tables
    returns it) whose bits are not the model's of `level`; a wrong shape or a missing table is reported the same way."""
    want, alt = tables(which, level), None
    if which == "albedo":
        lut, lut2 = lut_candidates()
        if lut.tobytes() != lut2.tobytes():
            alt = tables(which, level, lut2)
    bad = []
    if sorted(got) != sorted(want):
        return [("tables", None, sorted(got), sorted(want))]
    for name in TABLES[which]:
        g, m = got[name], want[name]
        if g.shape != m.shape or g.dtype != m.dtype:
            bad.append((name, None, (g.shape, str(g.dtype)), (m.shape, str(m.dtype))))
            continue
        differ = bits(g) != bits(m)
        if alt is not None:
            differ &= bits(g) != bits(alt[name])
        if differ.ndim == 3:
            differ = differ.any(-1)
        at = np.argwhere(differ)
        if len(at):
            iy, ix = (int(v) for v in at[0])
            bad.append((name, (iy, ix), g[iy, ix].tolist(), m[iy, ix].tolist(), len(at)))
    return bad


# ---- what a change of level 0 has to refresh (vr_dirty.h's header text, one axis at a time; spans are half open) ----------------------
READS = {("height", "quad"): (2, 0, 1), ("height", "quadf"): (2, 0, 1), ("height", "fast"): (3, 0, 1), ("albedo", "fast"): (3, 0, 0)}    # extra entries, k0, k1


def level_size(n0, level):
    return max(1, n0 >> level)


def mip_next(lo, hi, dw):
    """Texel x of a level reads 2x and min(2x + 1, sw - 1) of the level below: [lo, hi) dirties [lo >> 1, min(((hi - 1) >> 1) + 1, dw))."""
    if hi <= lo:
        return 0, 0
    lo, hi = lo >> 1, min(((hi - 1) >> 1) + 1, dw)
    return (lo, hi) if hi > lo else (0, 0)


def dirty_entries(lo, hi, w, tw, k0, k1):
    """Entry ix reads the texels clamp(ix - 1 + k, 0, w - 1), k in [k0, k1]: texels [lo, hi) dirty the entries [lo + 1 - k1, hi + 1 - k0);
    a span that touches texel 0 dirties every entry in front, one that touches texel w - 1 every entry behind."""
    if hi <= lo:
        return 0, 0
    e_lo, e_hi = lo + 1 - k1, hi + 1 - k0
    if lo <= 0:
        e_lo = 0
    if hi >= w:
        e_hi = tw
    return max(e_lo, 0), min(e_hi, tw)


def dirty_table_span(which, table, lo, hi, w):
    """The entries of one axis of `table` that texels [lo, hi) of a w-texel level dirty; rgbf is indexed like the chain."""
    if table == "rgbf":
        return (lo, hi) if hi > lo else (0, 0)
    extra, k0, k1 = READS[(which, table)]
    return dirty_entries(lo, hi, w, w + extra, k0, k1)


def refresh_rectangles(w, h):
    """(name, x, y, ew, eh): pyramid_model.refresh_edits of a w x h map, each moved and cut to lie inside it (that list is written for maps
    of 64 x 19 texels and more), duplicates dropped."""
    from tests import pyramid_model as pm
    seen, out = set(), []
    for name, x, y, ew, eh in pm.refresh_edits(w, h):
        x, y = min(max(x, 0), w - 1), min(max(y, 0), h - 1)
        r = (x, y, min(ew, w - x), min(eh, h - y))
        if r not in seen:
            seen.add(r)
            out.append((name,) + r)
    return out


# ---- a device terrain against the model (tp: a TerrainPass; used by the GPU tests only) ------------------------------------------------
WHICH = ("height", "albedo")


def read_tables(tp):
    return {which: tp.Tables(which) for which in WHICH}


def assert_tables_are_the_model(tp, what):
    """Every table of every level of both maps: the model's shape and bits of the device's own level.  Returns what was read."""
    got = read_tables(tp)
    for which in WHICH:
        assert len(got[which]) == tp.mip_levels(which), (what, which)
        for l, lv in enumerate(got[which]):
            for bad in mismatches(which, lv, tp.download_mip(which, l)):
                raise AssertionError(f"{what}: {which} level {l}, table {bad[0]}: first wrong entry (iy, ix) = {bad[1]}, device {bad[2]}, model {bad[3]}"
                                     + (f" ({bad[4]} entries differ)" if len(bad) > 4 else ""))
    return got


def assert_tables_equal(a, b, what):
    """Two read-backs, bit for bit."""
    for which in WHICH:
        assert len(a[which]) == len(b[which]), (what, which)
        for l, (x, y) in enumerate(zip(a[which], b[which])):
            assert sorted(x) == sorted(y), (what, which, l)
            for name in x:
                d = bits(x[name]) != bits(y[name])
                d = d.any(-1) if d.ndim == 3 else d
                at = np.argwhere(d)
                assert len(at) == 0, (f"{what}: {which} level {l}, table {name}: {len(at)} entries differ, first (iy, ix) = {at[0].tolist()}: "
                                      f"{x[name][tuple(at[0])].tolist()} against {y[name][tuple(at[0])].tolist()}")


def tables_differ(a, b):
    return any(bits(x[n]).tobytes() != bits(y[n]).tobytes() for which in WHICH for x, y in zip(a[which], b[which]) for n in x)
