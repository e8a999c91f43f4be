// A region on level 0 of one of a terrain's maps (vr_terrain_region; its kernel: vr_region.hip): the inside of a polygon - a lake
// bed, a plateau, a building pad, a quarry, a painted zone - levelled, cut, filled, raised or painted, with a feathered outline.
// The definition, for the device and for the host.  Plain C++17, no HIP types: the host compiles this header alone
// (tests/host/region_check.cpp).
//
// As in vr_path.h everything a texel sees is fp32, evaluated in the written order with no contraction, and uses +, -, *, comparisons,
// fminf / fmaxf and int -> float conversions only, so a numpy float32 model (tests/region_model.py) reproduces the device bit for
// bit.  Division and the square root live in the preparation, on the host, in double, each result rounded to fp32 once (path_round:
// beyond fp32's range +-FLT_MAX, never an infinity).  The distance to an edge is the path's chain - path_offset and path_nearest of
// vr_path.h - and the weight's tail is brush_falloff: neither is restated here.  DESIGN.md 4ac.
//
//   map          w x h texels of map `which` span the world [-S/2, S/2]^2; texel i has its centre at texel coordinate i (vr_path.h).
//   contours     n points form closed contours: contour c has counts[c] >= 3 consecutive points and the edges (point s, point s + 1),
//                the last point joined to the contour's first.  No counts: one contour of all n points.  Inside is the even-odd rule
//                over all edges of all contours: a contour inside another is a hole, a bow-tie has two lobes.
//   preparation  region_const, per call:
//                  wx = S / w            wz = S / h                       world units per texel on each axis
//                  soft = feather > 0; then inv_r2 = 1 / feather^2 and cull_r = 1 / sqrt(inv_r2) from the ROUNDED inv_r2 (the
//                  feather the device's q < 1 means); a hard edge has inv_r2 = cull_r = 0 and evaluates no distance at all
//                region_vertex, per point, ONCE:
//                  vx = (x + S/2) / S * w - 0.5      vz = (z + S/2) / S * h - 0.5        (the path's ax, az)
//                region_edge, per edge a -> b, from the two vertices' ROUNDED numbers:
//                  ax = vx_a   az = vz_a   bz = vz_b                       the edge that ends at a vertex and the one that starts
//                                                                          there carry the same two numbers
//                  dx = (vx_b - vx_a) * wx           dz = (vz_b - vz_a) * wz             the edge vector, world units
//                  inv_len2 = 1 / (dx^2 + dz^2) from the ROUNDED dx, dz, or 0 (as path_segment's)
//                The edge vector comes from the texel coordinates, not from the world points as a path's does: a + d is then b to
//                within d's own rounding, so the crossing of a straddled row lies ON the edge (below).  From world differences b
//                would be off by the roundings of vx and vz, an absolute error - and on an edge of less height than that error the
//                crossing could run far past b.
//                The distance box per axis is path_span's with the path's E, [floor(min(ax, bx') - (R + E) / wx) - 1,
//                ceil(max(ax, bx') + (R + E) / wx) + 2) clipped to [0, w] with bx' = ax + dx / wx, R = cull_r and
//                  E = 2^-20 * ((|ax| + w) * wx + (|az| + h) * wz + |dx| + |dz|)         (world units)
//                z likewise.  The SPAN of an edge - what the tile cull tests - is the distance box stretched to the right edge of the
//                map: x1 = w.  The box's own x1 travels in the edge's spare word (dist_x1).  An edge with an empty span - wholly right
//                of the map (x0 = w), above or below it (no rows) - is dropped; an edge left of the map clips to x0 = 0, keeps a
//                non-empty span and still counts.  The call's rectangle is, per axis, the hull of the distance boxes' clipped ends
//                over ALL edges, dropped ones too - the polygon's bounding box plus the reach; where it is empty on either axis the
//                region misses the map and nothing is listed.
//   a texel      (i, j) against edge e, every line one fp32 operation; fi = (float)i, fj = (float)j are exact:
//                  px, pz                            path_offset(ax, az, wx, wz, i, j): p, from a to the texel's centre, world units
//                  up = az <= fj                     ub = bz <= fj                straddles = up != ub      (half-open: exact)
//                  m2 = px * dz                      m3 = pz * dx
//                  left = straddles && (up ? m2 > m3 : m2 < m3)                   the edge crosses the row to the left of the texel
//                  soft only: q = path_nearest(px, pz, dx, dz, inv_len2, inv_r2)
//                A horizontal edge (az == bz) never straddles.  A vertex on a texel row belongs to the rows at and below its number
//                for both of its edges, the same comparison on the same number: it is never counted by one and missed by the other.
//   per texel    over the call's edges in list order: inside = XOR of `left`; q* = 1 at the start, q* = q where q < q* (strict; a
//                NaN never wins).  Neither depends on the order, nor f on which edge won.
//   weight       region_weight: f0 by brush_falloff(q*, 0, 1) where q* < 1 (t = 1 - q*; f0 = (t * t) * (3 - 2 * t)).
//                  default            inside: f = 1                                   outside: covered where q* < 1, f = f0
//                  FEATHER_INSIDE     inside: f = 1 - f0 where q* < 1, else 1         outside: not written
//                  hard edge          inside: f = 1                                   outside: not written
//   apply        region_apply, with vr_brush.h's functions (a = f * opacity, one fp32 product; clamped to [0, 255]):
//                  LEVEL  brush_blend, to = target       CUT  to = fminf(val, target)       FILL  to = fmaxf(val, target)
//                  RAISE  brush_raise(val, a, target): val + a * target, target a signed delta
//                  PAINT  per channel c of channel_mask: brush_blend, to = color[c]
//                and the byte is brush_byte(val).  A texel that is not covered is not written.
//
// The three properties the tile cull and the tests stand on.  Write u = 2^-24 and P = (|ax| + w) * wx + (|az| + h) * wz >= |px| + |pz|.
//
//   error locality   A texel whose `left` differs from the exact answer - the exact crossing of its row by the segment from (ax, az)
//                to (vx_b, vz_b) - lies on a straddled row within 8u' |dx| < E of that crossing, a point of the edge (u' = u (1 + 4u)).
//                Proof.  `straddles` is exact.  Exactly, with D = (vx_b - ax, vz_b - az) and T = (fi - ax, fj - az), the texel is right
//                of the crossing of an upward edge iff C = Tx Dz - Tz Dx > 0.  px carries two roundings, dz one, the product one:
//                m2 = wx wz Tx Dz (1 + e2), m3 = wx wz Tz Dx (1 + e3), |e2|, |e3| <= 4u'.  The comparison of m2 with m3 is exact, so
//                a wrong sign needs |Tx Dz - Tz Dx| <= 4u' (|Tx Dz| + |Tz Dx|).  On a straddled row Tz = s Dz with s in [0, 1) and
//                Dz != 0, so |Tx - s Dx| <= 4u' (|Tx| + s |Dx|), hence |Tx - s Dx| <= 8u' s |Dx| / (1 - 4u') : the texel is that near, along
//                its row, to a + s D - and s = 0 (a vertex on the row) leaves no room at all.  In world units 8u' |dx| (1 + ..) < 16u |dx|
//                <= E.  The downward edge mirrors it.  So a wrong side test is a matter of the texels at the crossing and never flips
//                a run of a row.  (Beyond fp32's range - a product that overflows on both sides, or one below 2^-126 - the bound
//                does not hold: inf > inf is false, the edge then does not count.  Points of the sizes a world has are far from both.)
//   the span     A texel whose row the edge straddles has az <= fj < bz or bz <= fj < az: its row lies in [min(az, bz), max(az, bz)],
//                inside the box's rows, which reach a texel and more beyond both.  A texel left of x0 is at least one texel plus E / wx
//                left of both ends of the edge, so exactly not right of the crossing and, by error locality, not `left` on the
//                device either.  x1 = w: no texel of the map is right of the span.  An edge left of the map (bx' < 0) has x0 = 0.
//   cull invisibility   An edge whose span misses a texel (i, j) neither has `left` there nor q < 1: its rows miss j - then no straddle,
//                and q >= 1 by the path's span proof, whose box this is - or i < x0 - then not `left` (the span), and q >= 1 again.  So
//                evaluating a texel with only the edges whose spans meet its tile changes neither the parity nor q*.  The variant that
//                skips path_nearest where the distance box [x0, dist_x1) misses the tile stands on the path's proof alone.
//
// A texel is a pure function of its own byte, its coordinates and the call: neither the rectangle nor the tile nor the order in
// which the device visits edges can show.
#pragma once
#include "vr_path.h"

#include <vector>

// the ops of vr_region_params::op (include/vrterrain.h: VR_REGION_*)
constexpr int kRegionLevel = 0, kRegionCut = 1, kRegionFill = 2, kRegionRaise = 3, kRegionPaint = 4;
constexpr int kRegionMaxPoints = 4096;           // VR_MAX_REGION_POINTS: a contour has as many edges as points, and they fit the list buffers
static_assert(kRegionMaxPoints <= kPathMaxListed, "a region's edges travel in the brush's list buffers");
constexpr uint32_t kRegionFeatherInside = 1u;    // VR_REGION_FEATHER_INSIDE
constexpr uint32_t kRegionSoft = 0x100u;         // RegionConst::flags only: feather > 0

// A prepared edge, as the kernel reads it.  The span stands where BrushDab's does.
struct RegionEdge {
    float ax, az;               // end a, texel coordinates: the vertex's two numbers
    float dx, dz;               // b - a, world units
    float inv_len2;             // 1 / |b - a|^2, or 0
    float bz;                   // end b's vz: the number the next edge carries as its az
    float pad0;
    int32_t x0, x1, y0, y1;     // the span [x0, x1) x [y0, y1): the distance box with x1 = w; empty: the edge is dropped
    int32_t dist_x1;            // the distance box's own x1
};
static_assert(sizeof(RegionEdge) == sizeof(BrushDab), "RegionEdge travels in the brush's list buffers");

// Everything else a call's kernel needs: wave-uniform, passed by value.
struct RegionConst {
    float wx, wz;               // world units per texel
    float inv_r2;               // 1 / feather^2, 0 for a hard edge
    float opacity, target;
    float cull_r;               // 1 / sqrt(inv_r2): the feather the spans reach out by, 0 for a hard edge
    int32_t op;
    uint32_t flags;             // kRegionFeatherInside, kRegionSoft
    float color[4];
    uint32_t channel_mask;
    uint32_t pad[3];
};
static_assert(sizeof(RegionConst) == 64, "RegionConst layout");

struct RegionPoint { float x, z; };
struct RegionVertex { float vx, vz; };

inline bool region_edge_empty(const RegionEdge& e) { return e.x1 <= e.x0 || e.y1 <= e.y0; }

// ---- preparation (host, double) ----------------------------------------------------------------------------------------------
// the caller has checked the ranges (feather >= 0, opacity in [0, 1], everything finite)
inline RegionConst region_const(float feather, float opacity, float target, int op, uint32_t user_flags, const float color[4], uint32_t channel_mask, float world_size,
                                int w, int h)
{
    RegionConst k;
    const double S = (double)world_size;
    const bool soft = feather > 0.0f;
    k.wx = path_round(S / (double)w);
    k.wz = path_round(S / (double)h);
    k.inv_r2 = soft ? path_round(1.0 / ((double)feather * (double)feather)) : 0.0f;
    k.opacity = opacity;
    k.target = target;
    k.cull_r = soft ? path_round(1.0 / sqrt((double)k.inv_r2)) : 0.0f;
    k.op = op;
    k.flags = (user_flags & kRegionFeatherInside) | (soft ? kRegionSoft : 0u);
    for (int c = 0; c < 4; c++) k.color[c] = color[c];
    k.channel_mask = channel_mask;
    k.pad[0] = k.pad[1] = k.pad[2] = 0;
    return k;
}

inline RegionVertex region_vertex(const RegionPoint& p, float world_size, int w, int h)
{
    const double S = (double)world_size;
    RegionVertex v;
    v.vx = path_round(((double)p.x + S / 2) / S * w - 0.5);
    v.vz = path_round(((double)p.z + S / 2) / S * h - 0.5);
    return v;
}

inline RegionEdge region_edge(const RegionVertex& a, const RegionVertex& b, const RegionConst& k, int w, int h)
{
    RegionEdge e;
    const double wx = (double)k.wx, wz = (double)k.wz;
    e.ax = a.vx; e.az = a.vz; e.bz = b.vz;
    e.dx = path_round(((double)b.vx - (double)a.vx) * wx);
    e.dz = path_round(((double)b.vz - (double)a.vz) * wz);
    const double len2 = (double)e.dx * (double)e.dx + (double)e.dz * (double)e.dz;
    const double inv = len2 > 0.0 ? 1.0 / len2 : 0.0;
    e.inv_len2 = inv <= (double)kPathMaxFloat ? (float)inv : 0.0f;
    e.pad0 = 0.0f;
    const double ax = (double)e.ax, az = (double)e.az, dx = (double)e.dx, dz = (double)e.dz;
    const double bx = ax + dx / wx, bz = az + dz / wz;
    const double E = 9.5367431640625e-07 * ((fabs(ax) + w) * wx + (fabs(az) + h) * wz + fabs(dx) + fabs(dz));
    const double reach = (double)k.cull_r + E;
    path_span(ax < bx ? ax : bx, ax < bx ? bx : ax, reach / wx, w, &e.x0, &e.dist_x1);
    path_span(az < bz ? az : bz, az < bz ? bz : az, reach / wz, h, &e.y0, &e.y1);
    e.x1 = w;
    return e;
}

// false: the counts do not describe n points (a contour of fewer than 3, a sum that is not n, counts missing)
inline bool region_contours_ok(uint32_t n, const uint32_t* counts, uint32_t num_contours)
{
    if (num_contours == 0) return n == 0 || n >= 3;                 // one contour of all n points
    if (counts == nullptr) return false;
    uint64_t sum = 0;
    for (uint32_t c = 0; c < num_contours; c++) {
        if (counts[c] < 3) return false;
        sum += counts[c];
        if (sum > n) return false;
    }
    return sum == n;
}

// The edges of a region that meet the w x h map, in order, into `out`, the vertices into `verts` (both cleared first), and the call's
// rectangle into rect = {x0, y0, x1, y1} (all zero, and no edges, where the region misses the map).  The caller has checked the contours.
inline void region_prepare(const RegionPoint* pts, uint32_t n, const uint32_t* counts, uint32_t num_contours, const RegionConst& k, float world_size, int w, int h,
                           std::vector<RegionVertex>& verts, std::vector<RegionEdge>& out, int32_t rect[4])
{
    out.clear();
    verts.resize(n);
    rect[0] = rect[1] = rect[2] = rect[3] = 0;
    for (uint32_t i = 0; i < n; i++) verts[i] = region_vertex(pts[i], world_size, w, h);
    const uint32_t whole = n;
    const uint32_t nc = num_contours ? num_contours : (n ? 1u : 0u);
    bool any = false;
    uint32_t first = 0;
    for (uint32_t c = 0; c < nc; c++) {
        const uint32_t m = num_contours ? counts[c] : whole;
        for (uint32_t i = 0; i < m; i++) {
            const RegionEdge e = region_edge(verts[first + i], verts[first + (i + 1u) % m], k, w, h);
            if (!any) { rect[0] = e.x0; rect[1] = e.y0; rect[2] = e.dist_x1; rect[3] = e.y1; any = true; }
            else {
                rect[0] = e.x0 < rect[0] ? e.x0 : rect[0]; rect[1] = e.y0 < rect[1] ? e.y0 : rect[1];
                rect[2] = e.dist_x1 > rect[2] ? e.dist_x1 : rect[2]; rect[3] = e.y1 > rect[3] ? e.y1 : rect[3];
            }
            if (!region_edge_empty(e)) out.push_back(e);
        }
        first += m;
    }
    if (rect[2] <= rect[0] || rect[3] <= rect[1] || out.empty()) {
        out.clear();
        rect[0] = rect[1] = rect[2] = rect[3] = 0;
    }
}

// ---- per texel -----------------------------------------------------------------------------------------------------------
// 1 where edge e crosses row fj to the left of the texel whose offset from a is (px, pz) - path_offset's - else 0
VR_PATH_FN uint32_t region_left(const RegionEdge& e, float px, float pz, float fj)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const bool up = e.az <= fj, ub = e.bz <= fj;
    const float m2 = px * e.dz, m3 = pz * e.dx;
    const bool right_of = up ? m2 > m3 : m2 < m3;
    return (up != ub) && right_of ? 1u : 0u;
}

// false: the texel is not written; true: *f is its weight
VR_PATH_FN bool region_weight(uint32_t flags, bool inside, float q, float* f)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (!(flags & kRegionSoft)) { *f = 1.0f; return inside; }
    float f0 = 0.0f;
    const bool near = brush_falloff(q, 0.0f, 1.0f, &f0);
    if (flags & kRegionFeatherInside) { *f = near ? 1.0f - f0 : 1.0f; return inside; }
    *f = inside ? 1.0f : f0;
    return inside || near;
}

// LEVEL, CUT, FILL, RAISE: the heightmap's value under weight f
VR_PATH_FN float region_apply(int op, float opacity, float val, float f, float target)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (op == kRegionRaise) {
        const float a = f * opacity;
        return brush_raise(val, a, target);
    }
    const float to = op == kRegionCut ? fminf(val, target) : (op == kRegionFill ? fmaxf(val, target) : target);
    return brush_blend(val, f, opacity, to);
}

// ---- the whole operation over host arrays (the host check drives it, the library does not) -------------------------------------
// texels: w x h x channels bytes (channels 1 or 4), changed in place; inside (w x h bytes), q and f (w x h floats; f is 0 where the
// texel is not written) may be null.  No cull: every texel meets every edge.
inline void region_serial(uint8_t* texels, int w, int h, int channels, const RegionEdge* edges, uint32_t n, const RegionConst& k, uint8_t* inside_out, float* q_out,
                          float* f_out)
{
    const bool soft = (k.flags & kRegionSoft) != 0;
    for (int j = 0; j < h; j++)
        for (int i = 0; i < w; i++) {
            float best_q = 1.0f;
            uint32_t par = 0;
            for (uint32_t s = 0; s < n; s++) {
                const RegionEdge& e = edges[s];
                float px, pz;
                path_offset(e.ax, e.az, k.wx, k.wz, i, j, &px, &pz);
                par ^= region_left(e, px, pz, (float)j);
                if (soft) {
                    float q, t;
                    path_nearest(px, pz, e.dx, e.dz, e.inv_len2, k.inv_r2, &q, &t);
                    if (q < best_q) best_q = q;
                }
            }
            const size_t at = (size_t)j * w + i;
            float f = 0.0f;
            const bool covered = region_weight(k.flags, par != 0, best_q, &f);
            if (inside_out) inside_out[at] = (uint8_t)par;
            if (q_out) q_out[at] = best_q;
            if (f_out) f_out[at] = covered ? f : 0.0f;
            if (!covered) continue;
            uint8_t* px = texels + at * channels;
            if (k.op == kRegionPaint) {
                for (int c = 0; c < channels; c++)
                    if (k.channel_mask & (1u << c)) px[c] = brush_byte(brush_blend((float)px[c], f, k.opacity, k.color[c]));
            } else px[0] = brush_byte(region_apply(k.op, k.opacity, (float)px[0], f, k.target));
        }
}
