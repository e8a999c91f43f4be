// CPU check of vr_dirty.h, the rectangle rules of vr_derive.hip (vr_terrain_edit, and vr_terrain_create as the edit of the whole
// map).  No HIP: g++ -std=c++17 -I vrenderer_amd/csrc.
//
// The program restates, on the CPU, what the library derives from a map - the mip chain, the three table shapes (quad / quadf,
// fast R8, fast SRGBA8; rgbf is indexed like the chain), the dyadic min / max tree of the node heights (one surface and 2 x 2
// surfaces, leaf nodes of one and of two texels) and the query pyramid with vr_pyramid_leaf_cell's level-1 reach - and for every
// rectangle of every map size w, h in 1..9 (a seeded sample of 2000 rectangles for 16 x 16, 17 x 5 and 32 x 32) changes the
// texels inside, rebuilds everything IN FULL and compares with the state before:
//
//   containment  every element that changed lies inside the rectangle vr_dirty.h predicts for its structure and level;
//   tightness    the prediction is not "everything": per axis its span is at most the span of what changed plus K elements.
//
// Each rectangle is run under two algebras.  REAL is the library's arithmetic - (sum + 2) >> 2, packed bytes, min / max bytes,
// (9 mn0 + mn1) / 10 - over a random map whose texels are flipped (^ 0x80): roundings and equal neighbours may hide a change, so
// only containment is asserted.  COUNT makes every dependency visible: the map is 0, the edited texels are 1, and every
// derived element is the SUM of the elements it reads (duplicates of a clamped address included), so an element changes if
// and only if it reads, through any path, an edited texel.  What changes is then exactly the product of one interval per axis,
// and tightness is asserted against it.
//
// K, per axis (both sides together), from the rules:
//   mip chain, rgbf, all tables, node levels: 0.  The rules are exact: a level's span is the image of the span below under
//     x -> x >> 1 (the odd last column, which feeds nothing, is cut by the clip to dw); an entry's span is the preimage of the
//     texel span under ix -> clamp(ix - 1 + k), and the clamp's whole preimage of an edge texel is included.
//   pyramid leaf cells: 8.  Level-1 texel j is read by the cells (j - 0.5 - m) / r - 0.5 <= ix < (j + 1.5 + m) / r + 0.5 with
//     1 / r = w0 / w1 in [2, 3] and m = 1 / 64; vr_dirty.h takes floor((j - 1) / r) - 1 and ceil((j + 2) / r) + 2 instead: on
//     each side that is (0.5 - m) / r <= 1.46 from the constant, 0.5 from the half cell, 1 from the integer rounding and 1
//     of margin for the kernel's fp32 product - under 4 cells per side.  The level-0 part (the quad entry) is exact.
//   pyramid level l >= 1: 2 max(1, ceil(4 / 2^l)).  A child span that is s cells wide of the truth on one side gives a parent
//     span at most ceil(s / 2) wide of it, and one stray child can still name one stray parent.
// Hence area(predicted) <= (a + K)(b + K) = area(changed) + K (a + b) + K^2 for a changed a x b block: factor 1 on the area
// plus a border term, nowhere near "dirty = everything".
//
// Creating a terrain rests on the opposite end: the rectangle {0, 0, w, h} dirties ALL of every structure, at every level
// (check_whole_map: every w, h in 1..20 and 31, 32, 33, 64, 67, the same surfaces and leaf sizes), as equalities.
#include "vr_dirty.h"

#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <vector>

typedef std::vector<uint32_t> Grid;
static long g_failures = 0, g_cases = 0, g_checks = 0;

static int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

struct NodeCfg { int per_side, S, L, s; };          // surfaces per side, texels per surface side, levels below the root, texels per leaf

struct Built {
    int levels = 0;
    std::vector<int> w, h;
    std::vector<Grid> chain, quad, fast_r8, fast_px;
    std::vector<std::vector<std::vector<Grid>>> nodes;    // [config][surface][depth], n x n values (min and max folded into one word)
    std::vector<Grid> pyr; std::vector<int> pw, ph;
};

static uint32_t fold(bool real, uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return real ? (a | b << 8 | c << 16 | d << 24) : a + b + c + d; }

static Built build(const Grid& map, int w0, int h0, bool real, const std::vector<NodeCfg>& cfgs)
{
    Built B;
    int levels = 1; { int m = w0 > h0 ? w0 : h0; while (m > 1) { m >>= 1; levels++; } }
    B.levels = levels;
    B.chain.push_back(map); B.w.push_back(w0); B.h.push_back(h0);
    for (int l = 1; l < levels; l++) {                    // vr_mip_*_texel: 2x, min(2x + 1, sw - 1)
        const int sw = B.w[l - 1], sh = B.h[l - 1], dw = sw > 1 ? sw >> 1 : 1, dh = sh > 1 ? sh >> 1 : 1;
        const Grid& src = B.chain[l - 1];
        Grid dst((size_t)dw * dh);
        for (int y = 0; y < dh; y++) for (int x = 0; x < dw; x++) {
            const int x0 = 2 * x, x1 = std::min(2 * x + 1, sw - 1), y0 = 2 * y, y1 = std::min(2 * y + 1, sh - 1);
            const uint32_t sum = src[y0 * sw + x0] + src[y0 * sw + x1] + src[y1 * sw + x0] + src[y1 * sw + x1];
            dst[y * dw + x] = real ? (sum + 2) >> 2 : sum;
        }
        B.chain.push_back(dst); B.w.push_back(dw); B.h.push_back(dh);
    }
    for (int l = 0; l < levels; l++) {
        const int w = B.w[l], h = B.h[l];
        const Grid& src = B.chain[l];
        Grid q((size_t)(w + 2) * (h + 2)), f((size_t)(w + 3) * (h + 3)), p((size_t)(w + 3) * (h + 3));
        for (int tw = 2; tw <= 3; tw++)                    // vr_quad_entry / vr_footprint_entry: quad, quadf (tw = 2), fast R8 (tw = 3)
            for (int iy = 0; iy < h + tw; iy++) for (int ix = 0; ix < w + tw; ix++) {
                const int x0 = clampi(ix - 1, 0, w - 1), x1 = clampi(ix, 0, w - 1), y0 = clampi(iy - 1, 0, h - 1), y1 = clampi(iy, 0, h - 1);
                (tw == 2 ? q : f)[(size_t)iy * (w + tw) + ix] = fold(real, src[y0 * w + x0], src[y0 * w + x1], src[y1 * w + x0], src[y1 * w + x1]);
            }
        for (int iy = 0; iy < h + 3; iy++) for (int ix = 0; ix < w + 3; ix++)          // vr_fast_srgba8_entry
            p[(size_t)iy * (w + 3) + ix] = src[clampi(iy - 1, 0, h - 1) * w + clampi(ix - 1, 0, w - 1)];
        B.quad.push_back(q); B.fast_r8.push_back(f); B.fast_px.push_back(p);
    }
    for (const NodeCfg& c : cfgs) {                        // vr_minmax_leaf_node / vr_minmax_up_node
        std::vector<std::vector<Grid>> per_surface;
        for (int surf = 0; surf < c.per_side * c.per_side; surf++) {
            const int rx0 = (surf % c.per_side) * c.S, ry0 = (surf / c.per_side) * c.S;
            std::vector<Grid> lv(c.L + 1);
            for (int d = c.L; d >= 0; d--) {
                const int n = 1 << d;
                lv[d].resize((size_t)n * n);
                for (int iz = 0; iz < n; iz++) for (int ix = 0; ix < n; ix++) {
                    uint32_t mn = ~0u, mx = 0, sum = 0;
                    if (d == c.L) {
                        for (int j = 0; j < c.s; j++) for (int i = 0; i < c.s; i++) {
                            const uint32_t v = map[(size_t)(ry0 + iz * c.s + j) * w0 + rx0 + ix * c.s + i];
                            mn = std::min(mn, v); mx = std::max(mx, v); sum += v;
                        }
                    } else {
                        for (int j = 0; j < 2; j++) for (int i = 0; i < 2; i++) {
                            const uint32_t v = lv[d + 1][(size_t)(2 * iz + j) * (2 * n) + 2 * ix + i];
                            mn = std::min(mn, v & 0xffffu); mx = std::max(mx, v >> 16); sum += v;
                        }
                    }
                    lv[d][(size_t)iz * n + ix] = real ? (mn | mx << 16) : sum;
                }
            }
            per_surface.push_back(lv);
        }
        B.nodes.push_back(per_surface);
    }
    {   // vr_pyramid_leaf_cell / vr_pyramid_up_cell
        const int l1 = std::min(1, levels - 1), w1 = B.w[l1], h1 = B.h[l1], cw = w0 + 1, ch = h0 + 1;
        const Grid& lv1 = B.chain[l1];
        Grid leaf((size_t)cw * ch);
        const float m = 1.0f / 64.0f, rx = (float)w1 / (float)w0, rz = (float)h1 / (float)h0;
        for (int iz = 0; iz < ch; iz++) for (int ix = 0; ix < cw; ix++) {
            const uint32_t e = B.quad[0][(size_t)iz * (w0 + 2) + ix];
            int jx0 = (int)floorf(((float)ix - 0.5f) * rx - 0.5f - m), jx1 = (int)floorf(((float)ix + 0.5f) * rx - 0.5f + m) + 1;
            int jz0 = (int)floorf(((float)iz - 0.5f) * rz - 0.5f - m), jz1 = (int)floorf(((float)iz + 0.5f) * rz - 0.5f + m) + 1;
            jx0 = clampi(jx0, 0, w1 - 1); jx1 = clampi(jx1, 0, w1 - 1); jz0 = clampi(jz0, 0, h1 - 1); jz1 = clampi(jz1, 0, h1 - 1);
            uint32_t mn1 = 255, mx1 = 0, sum = 0;
            for (int z = jz0; z <= jz1; z++) for (int x = jx0; x <= jx1; x++) { const uint32_t v = lv1[(size_t)z * w1 + x]; mn1 = std::min(mn1, v); mx1 = std::max(mx1, v); sum += v; }
            if (real) {
                const uint32_t b0 = e & 255u, b1 = (e >> 8) & 255u, b2 = (e >> 16) & 255u, b3 = e >> 24;
                const uint32_t mn0 = std::min(std::min(b0, b1), std::min(b2, b3)), mx0 = std::max(std::max(b0, b1), std::max(b2, b3));
                leaf[(size_t)iz * cw + ix] = (9u * mn0 + mn1) / 10u | std::min((9u * mx0 + mx1 + 9u) / 10u, 255u) << 16;
            } else leaf[(size_t)iz * cw + ix] = e + sum;
        }
        B.pyr.push_back(leaf); B.pw.push_back(cw); B.ph.push_back(ch);
        int w = cw, h = ch;
        while (!(w == 1 && h == 1)) {
            const int pw = (w + 1) / 2, ph = (h + 1) / 2;
            const Grid& c = B.pyr.back();
            Grid p((size_t)pw * ph);
            for (int pz = 0; pz < ph; pz++) for (int px = 0; px < pw; px++) {
                const int x0 = 2 * px, x1 = std::min(2 * px + 1, w - 1), z0 = 2 * pz, z1 = std::min(2 * pz + 1, h - 1);
                const uint32_t a = c[(size_t)z0 * w + x0], b = c[(size_t)z0 * w + x1], cc = c[(size_t)z1 * w + x0], d = c[(size_t)z1 * w + x1];
                if (real) p[(size_t)pz * pw + px] = std::min(std::min(a & 0xffffu, b & 0xffffu), std::min(cc & 0xffffu, d & 0xffffu))
                                                  | std::max(std::max(a >> 16, b >> 16), std::max(cc >> 16, d >> 16)) << 16;
                else p[(size_t)pz * pw + px] = a + b + cc + d;
            }
            B.pyr.push_back(p); B.pw.push_back(pw); B.ph.push_back(ph);
            w = pw; h = ph;
        }
    }
    return B;
}

// what changed between two builds of a gw-wide grid against the predicted rectangle; K < 0: containment only
static void compare(const Grid& a, const Grid& b, int gw, const DirtyRect& pred, int K, const char* what, int level, int w0, int h0, const DirtyRect& edit)
{
    int cx0 = 1 << 30, cx1 = -1, cy0 = 1 << 30, cy1 = -1;
    bool outside = false;
    for (size_t i = 0; i < a.size(); i++) if (a[i] != b[i]) {
        const int x = (int)(i % gw), y = (int)(i / gw);
        cx0 = std::min(cx0, x); cx1 = std::max(cx1, x + 1); cy0 = std::min(cy0, y); cy1 = std::max(cy1, y + 1);
        if (x < pred.x0 || x >= pred.x1 || y < pred.y0 || y >= pred.y1) outside = true;
    }
    g_checks++;
    const int gh = (int)(a.size() / gw);
    bool bad = outside || (!dirty_empty(pred) && (pred.x0 < 0 || pred.y0 < 0 || pred.x1 > gw || pred.y1 > gh));     // (a kernel would write out of bounds)
    if (K >= 0 && !dirty_empty(pred)) {
        const int cw = cx1 > cx0 ? cx1 - cx0 : 0, ch = cy1 > cy0 ? cy1 - cy0 : 0;
        if (pred.x1 - pred.x0 > cw + K || pred.y1 - pred.y0 > ch + K) bad = true;
    }
    if (bad && g_failures++ < 20)
        printf("FAIL %s level %d of %d x %d, edit [%d,%d)x[%d,%d): predicted [%d,%d)x[%d,%d), changed [%d,%d)x[%d,%d)%s\n", what, level, w0, h0,
               edit.x0, edit.x1, edit.y0, edit.y1, pred.x0, pred.x1, pred.y0, pred.y1, cx0, cx1, cy0, cy1, outside ? " - a change OUTSIDE the prediction" : "");
}

static void run_rect(const Grid& base_real, int w0, int h0, const DirtyRect& e, const std::vector<NodeCfg>& cfgs, const Built before[2])
{
    g_cases++;
    for (int mode = 0; mode < 2; mode++) {
        const bool real = mode == 0;
        Grid map = real ? base_real : Grid((size_t)w0 * h0, 0u);
        for (int y = e.y0; y < e.y1; y++) for (int x = e.x0; x < e.x1; x++) map[(size_t)y * w0 + x] = real ? (map[(size_t)y * w0 + x] ^ 0x80u) : 1u;
        const Built after = build(map, w0, h0, real, cfgs);
        const Built& b4 = before[mode];
        const int K0 = real ? -1 : 0;
        // the chain and the tables, exactly as vr_derive_chain walks them
        std::vector<DirtyRect> chain(after.levels);
        chain[0] = e;
        for (int l = 1; l < after.levels; l++)
            chain[l] = dirty_rect(dirty_mip_next(dirty_x(chain[l - 1]), dirty_level_size(w0, l)), dirty_mip_next(dirty_y(chain[l - 1]), dirty_level_size(h0, l)));
        for (int l = 0; l < after.levels; l++) {
            const int w = after.w[l], h = after.h[l];
            if (w != dirty_level_size(w0, l) || h != dirty_level_size(h0, l)) { g_failures++; printf("FAIL dirty_level_size(%d)\n", l); }
            const DirtySpan cx = dirty_x(chain[l]), cy = dirty_y(chain[l]);
            compare(b4.chain[l], after.chain[l], w, chain[l], K0, "chain", l, w0, h0, e);
            compare(b4.quad[l], after.quad[l], w + 2, dirty_rect(dirty_quad_entries(cx, w), dirty_quad_entries(cy, h)), K0, "quad", l, w0, h0, e);
            compare(b4.fast_r8[l], after.fast_r8[l], w + 3, dirty_rect(dirty_fast_r8_entries(cx, w), dirty_fast_r8_entries(cy, h)), K0, "fast R8", l, w0, h0, e);
            compare(b4.fast_px[l], after.fast_px[l], w + 3, dirty_rect(dirty_fast_srgba8_entries(cx, w), dirty_fast_srgba8_entries(cy, h)), K0, "fast SRGBA8", l, w0, h0, e);
        }
        for (size_t c = 0; c < cfgs.size(); c++)
            for (int surf = 0; surf < cfgs[c].per_side * cfgs[c].per_side; surf++) {
                const int rx0 = (surf % cfgs[c].per_side) * cfgs[c].S, ry0 = (surf / cfgs[c].per_side) * cfgs[c].S;
                DirtySpan x = dirty_leaf_nodes(dirty_x(e), rx0, cfgs[c].s, 1 << cfgs[c].L), y = dirty_leaf_nodes(dirty_y(e), ry0, cfgs[c].s, 1 << cfgs[c].L);
                for (int d = cfgs[c].L; d >= 0; d--) {
                    // (vr_derive_node_heights stops at the first empty level: the levels above must then be unchanged - an empty prediction says so)
                    compare(b4.nodes[c][surf][d], after.nodes[c][surf][d], 1 << d, dirty_rect(x, y), K0, "nodes", d, w0, h0, e);
                    x = dirty_node_parents(x); y = dirty_node_parents(y);
                    if (dirty_empty(x) || dirty_empty(y)) { x = DirtySpan(); y = DirtySpan(); }
                }
            }
        {
            const int l1 = after.levels > 1 ? 1 : 0;
            const DirtyRect leaf = dirty_pyramid_leaf_cells(chain[0], chain[l1], w0, h0, dirty_level_size(w0, l1), dirty_level_size(h0, l1));
            DirtySpan x = dirty_x(leaf), y = dirty_y(leaf);
            for (size_t l = 0; l < after.pyr.size(); l++) {
                const int side = l == 0 ? 4 : std::max(1, (4 + (1 << l) - 1) >> l);
                compare(b4.pyr[l], after.pyr[l], after.pw[l], dirty_rect(x, y), real ? -1 : 2 * side, "pyramid", (int)l, w0, h0, e);
                x = dirty_pyramid_parents(x, (after.pw[l] + 1) / 2); y = dirty_pyramid_parents(y, (after.ph[l] + 1) / 2);
            }
        }
    }
}

static uint32_t g_rng = 0x2545F491u;
static uint32_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 17; g_rng ^= g_rng << 5; return g_rng; }

// the surfaces the mip-style path of the node heights applies to: power-of-two surfaces inside the map, leaf nodes of one and of two texels
static std::vector<NodeCfg> node_configs(int w0, int h0)
{
    std::vector<NodeCfg> cfgs;
    if (w0 == h0 && (w0 & (w0 - 1)) == 0) {
        for (int per_side = 1; per_side <= 2; per_side++) {
            const int S = w0 / per_side;
            if (S < 1) continue;
            int lg = 0; while ((1 << lg) < S) lg++;
            for (int s = 1; s <= 2 && s <= S; s++) { NodeCfg c; c.per_side = per_side; c.S = S; c.s = s; c.L = lg - (s - 1); cfgs.push_back(c); }
        }
    }
    return cfgs;
}

static void run_size(int w0, int h0, int sample)
{
    const std::vector<NodeCfg> cfgs = node_configs(w0, h0);
    Grid base((size_t)w0 * h0);
    for (uint32_t& v : base) v = rnd() & 255u;
    const Built before[2] = { build(base, w0, h0, true, cfgs), build(Grid((size_t)w0 * h0, 0u), w0, h0, false, cfgs) };
    if (sample == 0) {
        for (int y0 = 0; y0 < h0; y0++) for (int y1 = y0 + 1; y1 <= h0; y1++)
            for (int x0 = 0; x0 < w0; x0++) for (int x1 = x0 + 1; x1 <= w0; x1++) { DirtyRect e; e.x0 = x0; e.x1 = x1; e.y0 = y0; e.y1 = y1; run_rect(base, w0, h0, e, cfgs, before); }
    } else {
        for (int k = 0; k < sample; k++) {
            DirtyRect e;
            e.x0 = (int)(rnd() % (uint32_t)w0); e.y0 = (int)(rnd() % (uint32_t)h0);
            // a third of the sample: small rectangles; the rest: any extent, so that edges are touched often
            const bool small = k % 3 == 0;
            e.x1 = e.x0 + 1 + (int)(rnd() % (uint32_t)(small ? std::min(3, w0 - e.x0) : w0 - e.x0));
            e.y1 = e.y0 + 1 + (int)(rnd() % (uint32_t)(small ? std::min(3, h0 - e.y0) : h0 - e.y0));
            run_rect(base, w0, h0, e, cfgs, before);
        }
    }
}

static long g_whole = 0;
static void expect_whole(const DirtyRect& r, int w, int h, const char* what, int level, int w0, int h0)
{
    g_checks++;
    if (r.x0 == 0 && r.y0 == 0 && r.x1 == w && r.y1 == h) return;
    if (g_failures++ < 20) printf("FAIL whole map %d x %d: %s level %d is [%d,%d)x[%d,%d), not all %d x %d\n", w0, h0, what, level, r.x0, r.x1, r.y0, r.y1, w, h);
}
// vr_terrain_create: the rectangle {0, 0, w0, h0} is all of every structure, walked as vr_derive.hip walks them
static void check_whole_map(int w0, int h0)
{
    g_whole++;
    int levels = 1; { int m = w0 > h0 ? w0 : h0; while (m > 1) { m >>= 1; levels++; } }
    const DirtyRect whole = dirty_whole(w0, h0);
    DirtyRect chain = whole, chain1 = whole;
    for (int l = 0; l < levels; l++) {
        const int w = dirty_level_size(w0, l), h = dirty_level_size(h0, l);
        if (l) chain = dirty_rect(dirty_mip_next(dirty_x(chain), w), dirty_mip_next(dirty_y(chain), h));
        if (l == 1) chain1 = chain;
        const DirtySpan cx = dirty_x(chain), cy = dirty_y(chain);
        expect_whole(chain, w, h, "chain (rgbf, SRGBA8 inner)", l, w0, h0);
        expect_whole(dirty_rect(dirty_quad_entries(cx, w), dirty_quad_entries(cy, h)), w + 2, h + 2, "quad (R8 inner)", l, w0, h0);
        expect_whole(dirty_rect(dirty_fast_r8_entries(cx, w), dirty_fast_r8_entries(cy, h)), w + 3, h + 3, "fast R8 entries", l, w0, h0);
        expect_whole(dirty_rect(dirty_fast_srgba8_entries(cx, w), dirty_fast_srgba8_entries(cy, h)), w + 3, h + 3, "fast SRGBA8 entries", l, w0, h0);
    }
    for (const NodeCfg& c : node_configs(w0, h0))
        for (int surf = 0; surf < c.per_side * c.per_side; surf++) {
            const int rx0 = (surf % c.per_side) * c.S, ry0 = (surf / c.per_side) * c.S;
            DirtySpan x = dirty_leaf_nodes(dirty_x(whole), rx0, c.s, 1 << c.L), y = dirty_leaf_nodes(dirty_y(whole), ry0, c.s, 1 << c.L);
            for (int d = c.L; d >= 0; d--) {
                expect_whole(dirty_rect(x, y), 1 << d, 1 << d, "nodes", d, w0, h0);
                x = dirty_node_parents(x); y = dirty_node_parents(y);
            }
        }
    {
        const int l1 = levels > 1 ? 1 : 0;
        const DirtyRect leaf = dirty_pyramid_leaf_cells(whole, chain1, w0, h0, dirty_level_size(w0, l1), dirty_level_size(h0, l1));
        DirtySpan x = dirty_x(leaf), y = dirty_y(leaf);
        int cw = w0 + 1, ch = h0 + 1;
        for (int l = 0;; l++) {
            expect_whole(dirty_rect(x, y), cw, ch, "pyramid", l, w0, h0);
            if (cw == 1 && ch == 1) break;
            cw = (cw + 1) / 2; ch = (ch + 1) / 2;
            x = dirty_pyramid_parents(x, cw); y = dirty_pyramid_parents(y, ch);
        }
    }
}

int main()
{
    for (int h = 1; h <= 9; h++) for (int w = 1; w <= 9; w++) run_size(w, h, 0);
    run_size(16, 16, 2000); run_size(17, 5, 2000); run_size(32, 32, 2000);
    {
        std::vector<int> sizes;
        for (int n = 1; n <= 20; n++) sizes.push_back(n);
        for (int n : { 31, 32, 33, 64, 67 }) sizes.push_back(n);
        for (int h : sizes) for (int w : sizes) check_whole_map(w, h);
    }
    // the span helpers on their own
    { DirtySpan s; s.lo = 4; s.hi = 5; if (!dirty_empty(dirty_mip_next(s, 2))) { g_failures++; printf("FAIL the last column of an odd level feeds nothing\n"); } }
    if (dirty_floor_div(-1, 2) != -1 || dirty_ceil_div(-1, 2) != 0 || dirty_floor_div(5, 2) != 2 || dirty_ceil_div(5, 2) != 3) { g_failures++; printf("FAIL floor / ceil division\n"); }
    printf("%ld rectangles, %ld whole maps, %ld comparisons, %ld failures\n", g_cases, g_whole, g_checks, g_failures);
    return g_failures ? 1 : 0;
}
