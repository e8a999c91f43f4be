"""CPU tests of tests/tables_model.py, the model the decoded tables of a terrain are held to on the device
(tests/test_terrain_tables_gpu.py): the vectorised model against a per-entry restatement with explicit clamps, the rectangle
vr_dirty.h's header text predicts against what actually changes in the model's tables, and the condition under which the sRGB table
is decided whatever pow the C library has."""
import math
import struct

import numpy as np
import pytest

from tests import f64_frontend as fe
from tests import frontend_common as fc
from tests import tables_model as tm

DIRTY_SHAPES = [(5, 5), (7, 2), (33, 17)]


def _chain(which, level0):
    """Every level of a chain under the project's box-filter models (an open sRGB code takes the lower candidate: any bytes will do)."""
    out = [level0]
    while max(out[-1].shape[:2]) > 1:
        p = out[-1]
        out.append(fe.mip_r8(p) if which == "height" else np.concatenate([fe.mip_srgb(p)[0], fe.mip_r8(p[..., 3])[..., None]], -1))
    assert len(out) == fe.num_mip_levels(level0.shape[1], level0.shape[0])
    return out


def _f32(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def _scalar_tables(which, level):
    """The tables of one level entry by entry, every index clamped with min(max(.)); floats as their bit patterns."""
    h, w = level.shape[:2]
    cl = lambda v, n: min(max(v, 0), n - 1)
    f = np.float32
    if which == "height":
        t = lambda x, y: f(level[cl(y, h), cl(x, w)]) / f(255.0)
        quad = [[int(level[cl(iy - 1, h), cl(ix - 1, w)]) | int(level[cl(iy - 1, h), cl(ix, w)]) << 8 | int(level[cl(iy, h), cl(ix - 1, w)]) << 16
                 | int(level[cl(iy, h), cl(ix, w)]) << 24 for ix in range(w + 2)] for iy in range(h + 2)]

        def foot(ix, iy):
            t00, t10, t01, t11 = t(ix - 1, iy - 1), t(ix, iy - 1), t(ix - 1, iy), t(ix, iy)
            return [_f32(v) for v in (t00, f(t10 - t00), t01, f(t11 - t01))]
        return {"quad": quad, "quadf": [[foot(ix, iy) for ix in range(w + 2)] for iy in range(h + 2)],
                "fast": [[foot(ix, iy) for ix in range(w + 3)] for iy in range(h + 3)]}
    lin = [_f32(f(c / 12.92 if c <= 0.04045 else math.pow((c + 0.055) / 1.055, 2.4))) for c in (i / 255.0 for i in range(256))]
    texel = lambda x, y: [lin[int(level[cl(y, h), cl(x, w), c])] for c in range(3)] + [0]
    return {"fast": [[texel(ix - 1, iy - 1) for ix in range(w + 3)] for iy in range(h + 3)], "rgbf": [[texel(ix, iy) for ix in range(w)] for iy in range(h)]}


@pytest.mark.parametrize("shape", fc.CREATE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_vectorised_model_is_the_per_entry_restatement(shape):
    """Every level of both chains of the CREATE_SHAPES maps, every table: shape, dtype and every bit.  The restatement decodes sRGB with
    math.pow where the model uses numpy's power: the two agree because the table is decided (the last test)."""
    w, h = shape
    hm, al = fc.random_texture(w, h, fc.CREATE_SEED)
    for which, level0 in (("height", hm), ("albedo", al)):
        for l, level in enumerate(_chain(which, level0)):
            got, want = tm.tables(which, level), _scalar_tables(which, level)
            assert tuple(sorted(got)) == tuple(sorted(tm.TABLES[which]))
            lh, lw = level.shape[:2]
            assert (lw, lh) == (tm.level_size(w, l), tm.level_size(h, l))
            for name, g in got.items():
                extra = {"quad": 2, "quadf": 2, "fast": 3, "rgbf": 0}[name]
                assert g.shape == ((lh + extra, lw + extra) if name == "quad" else (lh + extra, lw + extra, 4)), (which, l, name, g.shape)
                assert g.dtype == (np.uint32 if name == "quad" else np.float32)
                assert tm.bits(g).tolist() == want[name], (which, l, name)
                if name != "quad":
                    assert not np.signbit(g[g == 0.0]).any()         # equal neighbours give + 0.0, and so does the fourth component of a colour


def _changed_box(a, b):
    d = tm.bits(a) != tm.bits(b)
    if d.ndim == 3:
        d = d.any(-1)
    at = np.argwhere(d)
    return None if len(at) == 0 else (int(at[:, 1].min()), int(at[:, 0].min()), int(at[:, 1].max()) + 1, int(at[:, 0].max()) + 1)


def _predicted(which, table, spans, l, w, h):
    (x0, x1), (y0, y1) = spans
    if x1 <= x0 or y1 <= y0:
        return None
    ex, ey = tm.dirty_table_span(which, table, x0, x1, tm.level_size(w, l)), tm.dirty_table_span(which, table, y0, y1, tm.level_size(h, l))
    return ex[0], ey[0], ex[1], ey[1]


def _cases(w, h):
    return [(f"texel ({x}, {y})", x, y, 1, 1) for y in range(h) for x in range(w)] + tm.refresh_rectangles(w, h)


@pytest.mark.parametrize("shape", DIRTY_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_what_changes_lies_inside_what_the_dirty_rule_predicts(shape):
    """Every single texel and every rectangle of pyramid_model.refresh_edits (cut to the map) is inverted (b -> 255 - b, so every texel of
    it changes); the chain is rebuilt in full and so are all tables.  At every level, for every table, the entries whose bits differ
    lie inside the span pair vr_dirty.h's text gives for the dirty texels of that level (the chain rule applied level by level), and at
    level 0 - where every texel of the rectangle did change - the box of the changed entries IS the predicted one for the quad table
    and both albedo tables: the rule is not loose there.  (quadf and fast of the heightmap hold differences, which may stay equal.)"""
    w, h = shape
    hm, al = fc.random_texture(w, h, fc.CREATE_SEED)
    seen_rim = 0
    for which, level0 in (("height", hm), ("albedo", al)):
        before = [tm.tables(which, lv) for lv in _chain(which, level0)]
        for name, x, y, ew, eh in _cases(w, h):
            edited = level0.copy()
            edited[y:y + eh, x:x + ew] = 255 - edited[y:y + eh, x:x + ew]
            spans = ((x, x + ew), (y, y + eh))
            for l, level in enumerate(_chain(which, edited)):
                if l > 0:
                    spans = (tm.mip_next(*spans[0], tm.level_size(w, l)), tm.mip_next(*spans[1], tm.level_size(h, l)))
                after = tm.tables(which, level)
                for table in tm.TABLES[which]:
                    box, want = _changed_box(before[l][table], after[table]), _predicted(which, table, spans, l, w, h)
                    what = (which, name, l, table, box, want)
                    if box is not None:
                        assert want is not None and want[0] <= box[0] and want[1] <= box[1] and box[2] <= want[2] and box[3] <= want[3], what
                    if l == 0 and (which, table) != ("height", "quadf") and (which, table) != ("height", "fast"):
                        assert box == want, what
                    if l == 0 and table == "fast" and x + ew == w:
                        assert want[2] == w + 3
                        seen_rim += 1
    assert seen_rim > 0


@pytest.mark.parametrize("shape", DIRTY_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_a_change_of_a_rim_texel_changes_the_rim_entries(shape):
    """The failure the device tests are for must be visible in the tables: a change of texel (w - 1, h - 1) changes the quad entries
    w, w + 1 of the last rows and the fast entries w, w + 1, w + 2 (the albedo's likewise), a change of texel (0, 0) entry 0 - at level
    0 and, where the chain rule carries the change up, at the clamped rim of every coarser level too.  A change of texel w - 2 leaves
    the last entry column of every table as it was: that column reads texel w - 1 alone."""
    w, h = shape
    hm, al = fc.random_texture(w, h, fc.CREATE_SEED)
    for which, level0 in (("height", hm), ("albedo", al)):
        base = _chain(which, level0)
        for corner in ((w - 1, h - 1), (0, 0)):
            edited = level0.copy()
            edited[corner[1], corner[0]] = 255 - edited[corner[1], corner[0]]
            chain = _chain(which, edited)
            for l, (p, q) in enumerate(zip(base, chain)):
                if np.array_equal(p, q):
                    continue                                              # (an odd last column feeds no coarser level)
                lh, lw = q.shape[:2]
                tp, tq = tm.tables(which, p), tm.tables(which, q)
                for table in tm.TABLES[which]:
                    if table == "rgbf":
                        continue
                    d = tm.bits(tp[table]) != tm.bits(tq[table])
                    d = d.any(-1) if d.ndim == 3 else d
                    extra = tm.READS[(which, table)][0]
                    decoded = (lambda a, y, x: a[y, x]) if which == "height" else (lambda a, y, x: a[y, x, :3])      # (alpha is not in the tables)
                    if (decoded(p, -1, -1) != decoded(q, -1, -1)).any():
                        assert d[lh + extra - 1, lw:lw + extra].all() and d[lh:lh + extra, lw + extra - 1].all(), (which, l, table)
                    if (decoded(p, 0, 0) != decoded(q, 0, 0)).any():
                        assert d[0, 0], (which, l, table)
        edited = level0.copy()
        edited[:, w - 2] = 255 - edited[:, w - 2]
        for table in tm.TABLES[which]:
            a, b = tm.tables(which, level0)[table], tm.tables(which, edited)[table]
            if table != "rgbf":
                assert np.array_equal(tm.bits(a)[:, -1], tm.bits(b)[:, -1]), (which, table)
            assert not np.array_equal(tm.bits(a), tm.bits(b))


def test_the_srgb_table_is_decided_whatever_pow_the_c_library_has():
    """Each of the 256 float64 values eotf(i / 255) is moved by 4 ulp (float64) down and up and must round to the same float32, bit for
    bit.  All 245 entries that pow computes (codes 11 .. 255) do: an error of a few ulp in pow cannot change the table the device holds.
    By the letter one entry does not - code 0: its value is an exact 0.0, and 4 ulp below zero rounds to -0.0.  It is 0 / 12.92, one
    IEEE division that no C library changes, so the model carries +0.0 alone and no second candidate anywhere.  The table is monotone,
    starts at 0 and ends at 1; numpy's power and math.pow give the same float32 entries."""
    open_codes = tm.lut_condition(4)
    print(f"\nsRGB table: {len(open_codes)} of 256 entries open under +- 4 ulp: {open_codes}")
    assert [c for c in open_codes if c / 255.0 > 0.04045] == [], open_codes
    assert sorted(open_codes) == [0] and [tm.bits(np.float32([v]))[0] for v in open_codes[0]] == [0x80000000, 0]
    assert tm.eotf64(0.0) == 0.0 and not np.signbit(tm.eotf64(0.0)) and tm.srgb_lut().view(np.uint32)[0] == 0
    lut, alt = tm.lut_candidates()
    assert lut.tobytes() == alt.tobytes() and lut.dtype == np.float32
    assert lut[0] == 0.0 and lut[255] == 1.0 and (np.diff(lut) > 0).all()
    scalar = np.float32([c / 12.92 if c <= 0.04045 else math.pow((c + 0.055) / 1.055, 2.4) for c in (i / 255.0 for i in range(256))])
    assert scalar.tobytes() == lut.tobytes()
    t = tm.unorm8()
    assert t[0] == 0.0 and t[255] == 1.0 and (np.diff(t) > 0).all()
    # float32(b) / float32(255) is the float64 quotient rounded once (b / 255 has no double-rounding case: 53 >= 2 * 24 + 2)
    assert (np.arange(256) / 255.0).astype(np.float32).tobytes() == t.tobytes()
