// A brush stroke on level 0 of one of a terrain's maps (vr_terrain_brush, vr_brush.hip): the definition, for the device and for
// the host.  Plain C++17, no HIP types: the host compiles this header alone (tests/host/brush_check.cpp).
//
// Everything a texel sees is fp32, evaluated in the written order with no contraction, and uses +, -, *, comparisons, floorf and
// int -> float conversions only - the operations IEEE 754 rounds the same way everywhere - so a numpy float32 model
// (tests/brush_model.py) reproduces the device bit for bit.  That is the contract; DESIGN.md 4s.
//
//   map          w0 x h0 texels span the world [-S/2, S/2]^2 (S = world_size; the queries' uv = ((x, z) + S/2) / S); texel i has its
//                centre at texel coordinate i.  The two maps of a terrain may differ in size: a dab is prepared for the map the
//                stroke addresses, and is an ellipse in texel space where that map is not square.
//   preparation  brush_prepare, on the host, in double, each result rounded to fp32 once:
//                  cx = (x + S/2) / S * w0 - 0.5      cz = (z + S/2) / S * h0 - 0.5
//                  sx = S / (w0 * radius)             sz = S / (h0 * radius)    (a texel is S / w0 world units wide: the
//                                                                              radius is radius * w0 / S texels, and 1 / sx is that)
//                  h2 = hardness^2                    k = 1 / (1 - h2)          (k from the unrounded h2)
//                and a conservative span per axis, from the ROUNDED centre and scale (the values the device computes with):
//                [floor(cx - 1/sx) - 1, ceil(cx + 1/sx) + 2), clipped to the map.  Every texel with q < 1 lies inside it
//                (tests/host/brush_check.cpp); a centre or scale beyond fp32's range clips to "nothing" or to "the whole axis".
//                A span of at most 5 x 5 texels is tested texel by texel, with brush_weight, and is empty if the dab covers none
//                (a small dab between the texel centres): such a dab misses the map like one that lies beside it.
//   weight       brush_weight: u = (float(i) - cx) * sx, v = (float(j) - cz) * sz, q = u*u + v*v; outside when !(q < 1);
//                f = 1 when q <= h2, else t = (1 - q) * k and f = (t*t) * (3 - 2*t).
//   stroke       one op and up to VR_MAX_BRUSH_DABS dabs in order.  A texel's fp32 value (four for the albedo) starts as its stored
//                byte; the dabs that cover it are applied in list order (brush_apply, a = f * strength), each followed by
//                min(max(val, 0), 255); after the last the byte is (uint8)floorf(val + 0.5f) (brush_byte).
//                  RAISE    val + f * strength              FLATTEN  val + a * (target - val)
//                  SMOOTH   val + a * (m - val), m = float(sum of the 3 x 3 clamped neighbourhood BEFORE the stroke) * 0.11111111f
//                  PAINT    per channel of channel_mask: val + a * (color[c] - val)
//
// Two consequences.  A texel no dab covers keeps its byte exactly (it is not written at all).  Sub-step strengths accumulate
// inside one stroke and are quantised once at its end: a stroke split over two calls is two quantisations - not the same stroke.
// SMOOTH's mean comes from a snapshot of the map as it was before the stroke, so the result does not depend on the order in
// which the device visits texels.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define VR_BRUSH_FN __host__ __device__ __forceinline__
#else
#define VR_BRUSH_FN inline
#endif

// the ops of vr_brush_stroke::op (include/vrterrain.h: VR_BRUSH_*)
constexpr int kBrushRaise = 0, kBrushFlatten = 1, kBrushSmooth = 2, kBrushPaint = 3;

// A prepared dab, as the kernel reads it.
struct BrushDab {
    float cx, cz;               // centre, texel coordinates
    float sx, sz;               // texels -> unit disc
    float h2, k;                // hardness^2, 1 / (1 - hardness^2)
    float strength;
    int32_t x0, x1, y0, y1;     // the span [x0, x1) x [y0, y1), clipped to the map; empty: the dab misses the map
    uint32_t pad;
};
static_assert(sizeof(BrushDab) == 48, "BrushDab layout");

inline bool brush_dab_empty(const BrushDab& d) { return d.x1 <= d.x0 || d.y1 <= d.y0; }
constexpr int kBrushSmallSpan = 5;          // spans up to this size on both axes are tested texel by texel on the host (brush_prepare)

// One axis of the span: [floor(c - 1/s) - 1, ceil(c + 1/s) + 2) clipped to [0, n].  c - 1/s may be an infinity or (inf - inf) a
// NaN: an end that is not a number clips to the map's edge, the wide side.
inline void brush_span(float c, float s, int n, int32_t* lo, int32_t* hi)
{
    const double r = 1.0 / (double)s;
    const double a = floor((double)c - r) - 1.0, b = ceil((double)c + r) + 2.0;
    *lo = !(a > 0.0) ? 0 : (a < (double)n ? (int32_t)a : n);
    *hi = !(b < (double)n) ? n : (b > 0.0 ? (int32_t)b : 0);
}

VR_BRUSH_FN bool brush_weight(const BrushDab& d, int i, int j, float* f);

// The weight's tail, on q = (distance / radius)^2 however it was measured (a dab's disc here, a path's corridor in vr_path.h).
// false: outside, !(q < 1); true: *f is 1 out to q <= h2, then the smoothstep of (1 - q) * k.
VR_BRUSH_FN bool brush_falloff(float q, float h2, float k, float* f)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (!(q < 1.0f)) return false;
    if (q <= h2) { *f = 1.0f; return true; }
    const float t = (1.0f - q) * k;
    const float tt = t * t, s = 3.0f - 2.0f * t;
    *f = tt * s;
    return true;
}

// (x, z, radius, hardness, strength) of a w0 x h0 map that spans `world_size`; the caller has checked the ranges
inline BrushDab brush_prepare(float x, float z, float radius, float hardness, float strength, float world_size, int w0, int h0)
{
    const double S = (double)world_size, h2 = (double)hardness * (double)hardness;
    BrushDab d;
    d.cx = (float)(((double)x + S / 2) / S * w0 - 0.5);
    d.cz = (float)(((double)z + S / 2) / S * h0 - 0.5);
    d.sx = (float)(S / (w0 * (double)radius));
    d.sz = (float)(S / (h0 * (double)radius));
    d.h2 = (float)h2;
    d.k = (float)(1.0 / (1.0 - h2));
    d.strength = strength;
    brush_span(d.cx, d.sx, w0, &d.x0, &d.x1);
    brush_span(d.cz, d.sz, h0, &d.y0, &d.y1);
    d.pad = 0;
    // a small dab may lie between the texel centres and cover none (a radius under half a texel has a span of at most 5): the
    // span of one that covers no texel - by the function the device runs - is empty, so a stroke of such dabs touches nothing
    if (!brush_dab_empty(d) && d.x1 - d.x0 <= kBrushSmallSpan && d.y1 - d.y0 <= kBrushSmallSpan) {
        bool any = false;
        float f;
        for (int j = d.y0; j < d.y1 && !any; j++)
            for (int i = d.x0; i < d.x1 && !any; i++) any = brush_weight(d, i, j, &f);
        if (!any) d.x1 = d.x0;
    }
    return d;
}

// false: texel (i, j) is outside the dab; true: *f is its weight
VR_BRUSH_FN bool brush_weight(const BrushDab& d, int i, int j, float* f)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float u = ((float)i - d.cx) * d.sx;
    const float v = ((float)j - d.cz) * d.sz;
    const float uu = u * u, vv = v * v;
    const float q = uu + vv;
    return brush_falloff(q, d.h2, d.k, f);
}

VR_BRUSH_FN float brush_clamp(float val) { return fminf(fmaxf(val, 0.0f), 255.0f); }

// RAISE: one dab of weight f on `val`
VR_BRUSH_FN float brush_raise(float val, float f, float strength)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float a = f * strength;
    return brush_clamp(val + a);
}
// FLATTEN, SMOOTH, PAINT: towards `to` (the target, the snapshot's mean, the channel's colour)
VR_BRUSH_FN float brush_blend(float val, float f, float strength, float to)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float a = f * strength;
    const float d = to - val;
    const float ad = a * d;
    return brush_clamp(val + ad);
}
// SMOOTH's mean from the sum of the nine bytes
VR_BRUSH_FN float brush_mean9(int sum) { return (float)sum * 0.11111111f; }
// the byte a value ends as
VR_BRUSH_FN uint8_t brush_byte(float val) { return (uint8_t)floorf(val + 0.5f); }
