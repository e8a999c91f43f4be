// A path on level 0 of one of a terrain's maps (vr_terrain_path; its kernel: vr_path.hip): a corridor of constant half-width along a
// polyline, whose target height ramps from control point to control point - a road, an embankment, a river bed, a painted track.
// The definition, for the device and for the host.  Plain C++17, no HIP types: the host compiles this header alone
// (tests/host/path_check.cpp).
//
// As in vr_brush.h everything a texel sees is fp32, evaluated in the written order with no contraction, and uses +, -, *,
// comparisons, fminf / fmaxf and int -> float conversions only, so a numpy float32 model (tests/path_model.py) reproduces the device
// bit for bit.  Division and the square root live in the preparation, on the host, in double, each result rounded to fp32 once
// (beyond fp32's range: +-FLT_MAX, never an infinity).  DESIGN.md 4ab.
//
//   map          w x h texels of map `which` span the world [-S/2, S/2]^2; texel i has its centre at texel coordinate i.  The two maps
//                of a terrain may differ in size and need not be square: a path is prepared for the map it addresses.
//   segments     n points make n - 1 segments (a_s, b_s) = (point s, point s + 1); closed: one more, (point n - 1, point 0); n == 1:
//                the one segment (point 0, point 0).  A segment whose ends coincide is a disc.
//   preparation  path_const, per call:
//                  wx = S / w            wz = S / h                       world units per texel on each axis
//                  inv_r2 = 1 / radius^2                                  (q is a squared distance times this)
//                  h2 = hardness^2       k = 1 / (1 - h2)                 (k from the unrounded h2, as brush_prepare's)
//                  cull_r = 1 / sqrt(inv_r2), from the ROUNDED inv_r2      (the radius the device's q < 1 means; the span's)
//                path_segment, per segment, from the fp32 points:
//                  ax = (xa + S/2) / S * w - 0.5     az = (za + S/2) / S * h - 0.5       a in texel coordinates
//                  dx = xb - xa                      dz = zb - za                        the segment vector, world units
//                  inv_len2 = 1 / (dx^2 + dz^2) from the ROUNDED dx, dz; 0 where that is not a finite fp32 (a zero-length
//                             segment, or one so short that the inverse overflows): t is then 0 and the segment is a disc about a
//                  ha = height of a                  dh = hb - ha
//                and a conservative span per axis, in double from the ROUNDED values (what the device computes with), after
//                brush_span's pattern: with bx = ax + dx / wx (b as the device sees it), R = cull_r and the rounding allowance
//                  E = 2^-20 * ((|ax| + w) * wx + (|az| + h) * wz + |dx| + |dz|)         (world units; below)
//                [floor(min(ax, bx) - (R + E) / wx) - 1, ceil(max(ax, bx) + (R + E) / wx) + 2), clipped to [0, w]; z likewise.
//                An end that is not a number clips to the map's edge, the wide side.  A segment with an empty span misses the map
//                and is dropped; the others keep their order.
//   the proof    of the span.  Write u = 2^-24.  For a texel of the map |p| <= P = (|ax| + w) * wx + (|az| + h) * wz.  (float)i is
//                exact; px and pz carry 2 roundings each, the products t * dx, t * dz one, the differences ex, ez one: the
//                computed e differs from p - t * d, for the computed t - which lies in [0, 1], so p - t * d is the offset to A
//                point of the segment - by at most sqrt(2) * (3 |p| + 2 |d|) u < 5 u (P + |d|) in length.  q has 3 more roundings
//                and inv_r2 is exact by R's definition: a computed q < 1 means |e| < R (1 + 2u).  So a covered texel lies within
//                R (1 + 2u) + 5 u (P + |d|) < R + E of the segment in world units (E = 16 u (P + |dx| + |dz|); R * 2u is far below
//                the one texel of margin on either side, which also takes the roundings of the double arithmetic), hence within
//                that over wx texels of [min(ax, bx), max(ax, bx)] on the x axis.  Where the fp32 chain overflows q is an infinity
//                or a NaN and the texel is not covered.  tests/host/path_check.cpp tests it on seeded segments.
//   a texel      path_texel, texel (i, j) against segment s, every line one fp32 operation:
//                  ox = (float)i - ax          oz = (float)j - az
//                  px = ox * wx                pz = oz * wz                  p: from a to the texel's centre, world units
//                  m0 = px * dx                m1 = pz * dz                  dot = m0 + m1
//                  t0 = dot * inv_len2         t1 = t0 < 0 ? 0 : t0          t = t1 > 1 ? 1 : t1     (comparisons: a NaN stays one)
//                  gx = t * dx                 gz = t * dz
//                  ex = px - gx                ez = pz - gz                  e: from the nearest point to the texel's centre
//                  xx = ex * ex                zz = ez * ez                  d2 = xx + zz
//                  q = d2 * inv_r2
//   the winner   over the call's segments in list order, starting from q* = 1: segment s wins where q_s < q* (strict: of equal q
//                the lowest index keeps the texel; a q that is not below 1, a NaN included, never wins).  A texel no segment wins
//                is not written.  Because a winner has q < 1, leaving out any segments whose q is not below 1 on the texel - the
//                tile cull by the spans - cannot change it.
//   apply        with the winner's q and t: f by brush_falloff(q, h2, k) - the dab's profile, vr_brush.h's own function - and
//                th = t * dh; target = ha + th.  Per op, with vr_brush.h's brush_blend (a = f * opacity; val + a * (to - val);
//                clamped to [0, 255]):
//                  LEVEL  to = target            CUT  to = fminf(val, target)            FILL  to = fmaxf(val, target)
//                  PAINT  per channel c of channel_mask: to = color[c]
//                and the byte is brush_byte(val).  Applied once: a path never meets a texel twice, however it bends.
//
// A texel is a pure function of its own byte, its coordinates and the call: neither the rectangle nor the tile nor the order in
// which the device visits segments can show.
#pragma once
#include "vr_brush.h"

#include <vector>

#if defined(__HIPCC__)
#define VR_PATH_FN __host__ __device__ __forceinline__
#else
#define VR_PATH_FN inline
#endif

// the ops of vr_path_params::op (include/vrterrain.h: VR_PATH_*)
constexpr int kPathLevel = 0, kPathCut = 1, kPathFill = 2, kPathPaint = 3;
constexpr int kPathMaxPoints = 4096;             // VR_MAX_PATH_POINTS
constexpr int kPathMaxListed = 4096;             // VR_MAX_BRUSH_DABS: the list buffers the segments travel in
static_assert(kPathMaxPoints <= kPathMaxListed, "a closed path of kPathMaxPoints points has as many segments: they fit the brush's list buffers");
constexpr float kPathMaxFloat = 3.402823466e38f;

// A prepared segment, as the kernel reads it.  The span stands where BrushDab's does.
struct PathSeg {
    float ax, az;               // end a, texel coordinates
    float dx, dz;               // b - a, world units
    float inv_len2;             // 1 / |b - a|^2, or 0
    float ha, dh;               // the target at a, and hb - ha
    int32_t x0, x1, y0, y1;     // the span [x0, x1) x [y0, y1), clipped to the map; empty: the segment misses the map
    uint32_t pad;
};
static_assert(sizeof(PathSeg) == sizeof(BrushDab), "PathSeg travels in the brush's list buffers");

// Everything else a call's kernel needs: wave-uniform, passed by value.
struct PathConst {
    float wx, wz;               // world units per texel
    float inv_r2, h2, k, opacity;
    float cull_r;               // 1 / sqrt(inv_r2): the radius the spans reach out by
    int32_t op;
    float color[4];
    uint32_t channel_mask;
    uint32_t pad[3];
};
static_assert(sizeof(PathConst) == 64, "PathConst layout");

struct PathPoint { float x, z, height; };

inline bool path_seg_empty(const PathSeg& s) { return s.x1 <= s.x0 || s.y1 <= s.y0; }

// ---- preparation (host, double) ----------------------------------------------------------------------------------------------
inline float path_round(double v)               // to fp32 once; beyond its range: +-FLT_MAX, never an infinity
{
    if (v > (double)kPathMaxFloat) return kPathMaxFloat;
    if (v < -(double)kPathMaxFloat) return -kPathMaxFloat;
    return (float)v;
}

// the caller has checked the ranges (radius > 0, hardness in [0, 1), opacity in [0, 1], everything finite)
inline PathConst path_const(float radius, float hardness, float opacity, int op, const float color[4], uint32_t channel_mask, float world_size, int w, int h)
{
    PathConst k;
    const double S = (double)world_size, h2 = (double)hardness * (double)hardness;
    k.wx = path_round(S / (double)w);
    k.wz = path_round(S / (double)h);
    k.inv_r2 = path_round(1.0 / ((double)radius * (double)radius));
    k.h2 = (float)h2;
    k.k = (float)(1.0 / (1.0 - h2));
    k.opacity = opacity;
    k.cull_r = path_round(1.0 / sqrt((double)k.inv_r2));
    k.op = op;
    for (int c = 0; c < 4; c++) k.color[c] = color[c];
    k.channel_mask = channel_mask;
    k.pad[0] = k.pad[1] = k.pad[2] = 0;
    return k;
}

// One axis of the span, [floor(lo - r) - 1, ceil(hi + r) + 2) clipped to [0, n]; an end that is not a number clips to the wide side.
inline void path_span(double lo, double hi, double r, int n, int32_t* s0, int32_t* s1)
{
    const double a = floor(lo - r) - 1.0, b = ceil(hi + r) + 2.0;
    *s0 = !(a > 0.0) ? 0 : (a < (double)n ? (int32_t)a : n);
    *s1 = !(b < (double)n) ? n : (b > 0.0 ? (int32_t)b : 0);
}

inline PathSeg path_segment(const PathPoint& a, const PathPoint& b, const PathConst& k, float world_size, int w, int h)
{
    const double S = (double)world_size;
    PathSeg s;
    s.ax = path_round(((double)a.x + S / 2) / S * w - 0.5);
    s.az = path_round(((double)a.z + S / 2) / S * h - 0.5);
    s.dx = path_round((double)b.x - (double)a.x);
    s.dz = path_round((double)b.z - (double)a.z);
    const double len2 = (double)s.dx * (double)s.dx + (double)s.dz * (double)s.dz;
    const double inv = len2 > 0.0 ? 1.0 / len2 : 0.0;
    s.inv_len2 = inv <= (double)kPathMaxFloat ? (float)inv : 0.0f;
    s.ha = a.height;
    s.dh = (float)((double)b.height - (double)a.height);
    const double wx = (double)k.wx, wz = (double)k.wz, ax = (double)s.ax, az = (double)s.az, dx = (double)s.dx, dz = (double)s.dz;
    const double bx = ax + dx / wx, bz = az + dz / wz;
    const double E = 9.5367431640625e-07 * ((fabs(ax) + w) * wx + (fabs(az) + h) * wz + fabs(dx) + fabs(dz));
    const double reach = (double)k.cull_r + E;
    path_span(ax < bx ? ax : bx, ax < bx ? bx : ax, reach / wx, w, &s.x0, &s.x1);
    path_span(az < bz ? az : bz, az < bz ? bz : az, reach / wz, h, &s.y0, &s.y1);
    s.pad = 0;
    return s;
}

// how many segments n points make (0 for n == 0; the caller has refused closed with n < 3)
inline uint32_t path_segment_count(uint32_t n, bool closed) { return n == 0 ? 0u : (n == 1 ? 1u : (closed ? n : n - 1u)); }

// The segments of a path that meet the w x h map, in order, into `out` (cleared first), and the hull of their spans into
// rect = {x0, y0, x1, y1} (all zero where none meets the map).
inline void path_prepare(const PathPoint* pts, uint32_t n, bool closed, const PathConst& k, float world_size, int w, int h, std::vector<PathSeg>& out, int32_t rect[4])
{
    out.clear();
    rect[0] = rect[1] = rect[2] = rect[3] = 0;
    const uint32_t ns = path_segment_count(n, closed);
    for (uint32_t i = 0; i < ns; i++) {
        const PathSeg s = path_segment(pts[i], pts[(i + 1u) % n], k, world_size, w, h);
        if (path_seg_empty(s)) continue;
        if (out.empty()) { rect[0] = s.x0; rect[1] = s.y0; rect[2] = s.x1; rect[3] = s.y1; }
        else {
            rect[0] = s.x0 < rect[0] ? s.x0 : rect[0]; rect[1] = s.y0 < rect[1] ? s.y0 : rect[1];
            rect[2] = s.x1 > rect[2] ? s.x1 : rect[2]; rect[3] = s.y1 > rect[3] ? s.y1 : rect[3];
        }
        out.push_back(s);
    }
}

// ---- per texel -----------------------------------------------------------------------------------------------------------
// The chain in its two halves, on plain numbers, so that a region's edge (vr_region.h) runs the same operations: the head gives p,
// from a to the centre of texel (i, j) in world units; the tail q and t of the point of a + t * d nearest to p.
VR_PATH_FN void path_offset(float ax, float az, float wx, float wz, int i, int j, float* px, float* pz)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float ox = (float)i - ax, oz = (float)j - az;
    *px = ox * wx;
    *pz = oz * wz;
}
VR_PATH_FN void path_nearest(float px, float pz, float dx, float dz, float inv_len2, float inv_r2, float* q, float* t)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float m0 = px * dx, m1 = pz * dz;
    const float dot = m0 + m1;
    const float t0 = dot * inv_len2;
    const float t1 = t0 < 0.0f ? 0.0f : t0;
    const float tc = t1 > 1.0f ? 1.0f : t1;
    const float gx = tc * dx, gz = tc * dz;
    const float ex = px - gx, ez = pz - gz;
    const float xx = ex * ex, zz = ez * ez;
    const float d2 = xx + zz;
    *q = d2 * inv_r2;
    *t = tc;
}

// texel (i, j) against segment s: q = (distance / radius)^2 and the parameter t of the nearest point, clamped to [0, 1]
VR_PATH_FN void path_texel(const PathSeg& s, const PathConst& k, int i, int j, float* q, float* t)
{
    float px, pz;
    path_offset(s.ax, s.az, k.wx, k.wz, i, j, &px, &pz);
    path_nearest(px, pz, s.dx, s.dz, s.inv_len2, k.inv_r2, q, t);
}

// the target of the winner
VR_PATH_FN float path_target(const PathSeg& s, float t)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float th = t * s.dh;
    return s.ha + th;
}

// LEVEL, CUT, FILL: the heightmap's value under weight f and the target
VR_PATH_FN float path_apply(int op, float opacity, float val, float f, float target)
{
    const float to = op == kPathCut ? fminf(val, target) : (op == kPathFill ? fmaxf(val, target) : target);
    return brush_blend(val, f, opacity, to);
}

// ---- the whole operation over host arrays (the host check drives it, the library does not) -------------------------------------
// texels: w x h x channels bytes (channels 1 or 4), changed in place; q, t, f (w x h floats) and winner (w x h int32, -1: none) may
// be null.  No cull: every texel meets every segment.
inline void path_serial(uint8_t* texels, int w, int h, int channels, const PathSeg* segs, uint32_t n, const PathConst& k, float* q_out, float* t_out,
                        float* f_out, int32_t* winner)
{
    for (int j = 0; j < h; j++)
        for (int i = 0; i < w; i++) {
            float best_q = 1.0f, best_t = 0.0f;
            int32_t best = -1;
            for (uint32_t s = 0; s < n; s++) {
                float q, t;
                path_texel(segs[s], k, i, j, &q, &t);
                if (q < best_q) { best_q = q; best_t = t; best = (int32_t)s; }
            }
            const size_t at = (size_t)j * w + i;
            float f = 0.0f;
            const bool covered = best >= 0 && brush_falloff(best_q, k.h2, k.k, &f);
            if (q_out) q_out[at] = best_q;
            if (t_out) t_out[at] = best_t;
            if (f_out) f_out[at] = covered ? f : 0.0f;
            if (winner) winner[at] = best;
            if (!covered) continue;
            uint8_t* px = texels + at * channels;
            if (k.op == kPathPaint) {
                for (int c = 0; c < channels; c++)
                    if (k.channel_mask & (1u << c)) px[c] = brush_byte(brush_blend((float)px[c], f, k.opacity, k.color[c]));
            } else px[0] = brush_byte(path_apply(k.op, k.opacity, (float)px[0], f, path_target(segs[best], best_t)));
        }
}
