// What has to be (re)built of everything derived from a map once a rectangle of its level 0 holds new texels (vr_derive.hip).
// vr_terrain_edit passes the w x h sub-rectangle it replaced; creating a terrain passes the whole map, which dirties the whole of
// every structure (the edge rules below; asserted by tests/host/dirty_check.cpp), so there is one path and no rule of its own for
// "everything".  Plain C++17: no HIP, no library types - a CPU program changes every rectangle of small maps, rebuilds everything
// in full and checks that whatever changed lies inside what this header predicts, and that the prediction stays close to it
// (tests/host/dirty_check.cpp).  vr_derive.hip takes every rectangle from here and computes none itself.
//
// A DirtyRect is half open, [x0, x1) x [y0, y1), in the index space of the array it names; empty once a side is.  The two axes
// never mix, so every rule is a rule on one axis (DirtySpan), applied twice.  Every structure is a pure function of the chain, and
// rebuilding an element that did not change is harmless: the rules may be wide, never narrow.
//
//   mip chain      texel x of level l reads texels 2x and min(2x + 1, sw - 1) of level l - 1 (sw its size): [x0, x1) of a level
//                  dirties [x0 >> 1, min(((x1 - 1) >> 1) + 1, dw)) of the next (dw = max(1, sw >> 1)).  With an odd sw the
//                  last column feeds nothing, and the span may come out empty - then no coarser level changes either.
//   tables         entry ix of a clamp-addressed table reads the texels clamp(ix - 1 + k, 0, w - 1) for k in [k0, k1]:
//                    quad, quadf  (w + 2 entries)  k = 0, 1
//                    fast, R8     (w + 3 entries)  k = 0, 1
//                    fast, SRGBA8 (w + 3 entries)  k = 0
//                    pack, SRGBA8 (w + 3 entries)  k = 0, 1      (a whole footprint per entry: vr_packed.h)
//                  so texels [x0, x1) dirty the entries [x0 + 1 - k1, x1 + 1 - k0); a span that touches texel 0 also dirties
//                  every entry in front (they clamp to it), one that touches texel w - 1 every entry behind.  rgbf is indexed
//                  like the chain.
//   leaf nodes     node ix of a surface's finest level covers the texels [rx0 + ix s, rx0 + (ix + 1) s); n = 2^num_lods of them
//                  per side.  Parents: node ix of a level has the children 2 ix and 2 ix + 1.
//   pyramid cells  leaf cell ix (w0 + 1 of them) reads the level-0 quad entry ix and the level-1 texels jx0(ix) .. jx1(ix) of
//                  vr_pyramid_leaf_cell: floor((ix - 0.5) r - 0.5 - m) .. floor((ix + 0.5) r - 0.5 + m) + 1, clamped, r = w1 / w0,
//                  m = 1 / 64.  Texel j is therefore read by cells with (j - 0.5 - m) / r - 0.5 <= ix < (j + 1.5 + m) / r + 0.5;
//                  in integers, with m < 1 / 2 and room for the kernel's fp32 rounding of r (relative 2^-23, ix <= 2^14):
//                  floor((j - 1) w0 / w1) - 1 <= ix <= ceil((j + 2) w0 / w1) + 1.  The clamps again extend a span that touches
//                  an end of level 1 to the end of the cells.  A one-level chain samples level 0 twice (w1 = w0).
//                  Parents: cell px of a level has the children 2 px and min(2 px + 1, cw - 1).
#pragma once

#include <stdint.h>

struct DirtySpan { int lo = 0, hi = 0; };                        // [lo, hi)
struct DirtyRect { int x0 = 0, y0 = 0, x1 = 0, y1 = 0; };        // [x0, x1) x [y0, y1)

inline bool dirty_empty(DirtySpan s) { return s.hi <= s.lo; }
inline bool dirty_empty(const DirtyRect& r) { return r.x1 <= r.x0 || r.y1 <= r.y0; }
inline DirtyRect dirty_rect(DirtySpan x, DirtySpan y) { DirtyRect r; r.x0 = x.lo; r.x1 = x.hi; r.y0 = y.lo; r.y1 = y.hi; return r; }
inline DirtySpan dirty_x(const DirtyRect& r) { DirtySpan s; s.lo = r.x0; s.hi = r.x1; return s; }
inline DirtySpan dirty_y(const DirtyRect& r) { DirtySpan s; s.lo = r.y0; s.hi = r.y1; return s; }
inline DirtyRect dirty_whole(int w, int h) { DirtyRect r; r.x1 = w; r.y1 = h; return r; }      // all of a w x h level
inline DirtySpan dirty_clip(DirtySpan s, int n)
{
    if (s.lo < 0) s.lo = 0;
    if (s.hi > n) s.hi = n;
    if (s.hi < s.lo) s.hi = s.lo;
    return s;
}
// the smallest span that holds both (an empty one holds nothing)
inline DirtySpan dirty_hull(DirtySpan a, DirtySpan b)
{
    if (dirty_empty(a)) return b;
    if (dirty_empty(b)) return a;
    DirtySpan s; s.lo = a.lo < b.lo ? a.lo : b.lo; s.hi = a.hi > b.hi ? a.hi : b.hi;
    return s;
}
inline int64_t dirty_floor_div(int64_t a, int64_t b) { const int64_t q = a / b; return (a % b != 0 && ((a < 0) != (b < 0))) ? q - 1 : q; }
inline int64_t dirty_ceil_div(int64_t a, int64_t b) { return -dirty_floor_div(-a, b); }

inline int dirty_level_size(int size0, int level) { const int s = size0 >> level; return s > 1 ? s : 1; }

// ---- mip chain ----
// `dw`: size of the next level
inline DirtySpan dirty_mip_next(DirtySpan s, int dw)
{
    if (dirty_empty(s)) return DirtySpan();
    DirtySpan d; d.lo = s.lo >> 1; d.hi = ((s.hi - 1) >> 1) + 1;
    return dirty_clip(d, dw);
}

// ---- tables ----
// `w`: texels of the level, `tw`: entries of the table, [k0, k1]: the texels clamp(ix - 1 + k) entry ix reads
inline DirtySpan dirty_entries(DirtySpan s, int w, int tw, int k0, int k1)
{
    if (dirty_empty(s)) return DirtySpan();
    DirtySpan e; e.lo = s.lo + 1 - k1; e.hi = s.hi + 1 - k0;
    if (s.lo <= 0) e.lo = 0;
    if (s.hi >= w) e.hi = tw;
    return dirty_clip(e, tw);
}
inline DirtySpan dirty_quad_entries(DirtySpan s, int w) { return dirty_entries(s, w, w + 2, 0, 1); }          // quad and quadf
inline DirtySpan dirty_fast_r8_entries(DirtySpan s, int w) { return dirty_entries(s, w, w + 3, 0, 1); }
inline DirtySpan dirty_fast_srgba8_entries(DirtySpan s, int w) { return dirty_entries(s, w, w + 3, 0, 0); }
inline DirtySpan dirty_pack_srgba8_entries(DirtySpan s, int w) { return dirty_entries(s, w, w + 3, 0, 1); }    // holds fast's span: one entry more in front

// ---- node heights (mip-style path) ----
// `origin`: first texel of the surface's root on this axis, `s`: texels per leaf node, `n`: leaf nodes per side
inline DirtySpan dirty_leaf_nodes(DirtySpan t, int origin, int s, int n)
{
    if (dirty_empty(t)) return DirtySpan();
    DirtySpan d;
    d.lo = (int)dirty_floor_div((int64_t)t.lo - origin, s);
    d.hi = (int)dirty_ceil_div((int64_t)t.hi - origin, s);
    return dirty_clip(d, n);
}
inline DirtySpan dirty_node_parents(DirtySpan s)
{
    if (dirty_empty(s)) return DirtySpan();
    DirtySpan d; d.lo = s.lo >> 1; d.hi = ((s.hi - 1) >> 1) + 1;
    return d;
}

// ---- query pyramid ----
// `l0`, `l1`: the dirty texels of levels 0 and 1 (of a one-level chain: l1 = l0, w1 = w0); w0 + 1 cells
inline DirtySpan dirty_pyramid_cells(DirtySpan l0, DirtySpan l1, int w0, int w1)
{
    const int cw = w0 + 1;
    DirtySpan a = dirty_clip(dirty_quad_entries(l0, w0), cw), b;
    if (!dirty_empty(l1)) {
        b.lo = (int)dirty_floor_div((int64_t)(l1.lo - 1) * w0, w1) - 1;
        b.hi = (int)dirty_ceil_div((int64_t)(l1.hi - 1 + 2) * w0, w1) + 2;
        if (l1.lo <= 0) b.lo = 0;
        if (l1.hi >= w1) b.hi = cw;
        b = dirty_clip(b, cw);
    }
    return dirty_hull(a, b);
}
// both axes; a level-1 rectangle that is empty as a whole (an edit inside the odd last row or column of level 0) contributes nothing
inline DirtyRect dirty_pyramid_leaf_cells(const DirtyRect& l0, DirtyRect l1, int w0, int h0, int w1, int h1)
{
    if (dirty_empty(l1)) l1 = DirtyRect();
    return dirty_rect(dirty_pyramid_cells(dirty_x(l0), dirty_x(l1), w0, w1), dirty_pyramid_cells(dirty_y(l0), dirty_y(l1), h0, h1));
}
// `pw`: cells of the parent level, (cw + 1) / 2
inline DirtySpan dirty_pyramid_parents(DirtySpan s, int pw)
{
    if (dirty_empty(s)) return DirtySpan();
    DirtySpan d; d.lo = s.lo >> 1; d.hi = ((s.hi - 1) >> 1) + 1;
    return dirty_clip(d, pw);
}
