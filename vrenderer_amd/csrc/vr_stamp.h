// A stamp - a prepared patch of R8 or SRGBA8 texels - set into level 0 of a map at a position, size and angle, with a blend rule
// (vr_terrain_stamp; its kernel: vr_stamp.hip).  The definition, for the device and for the host.  Plain C++17, no HIP types: the
// host compiles this header alone (tests/host/stamp_check.cpp).
//
// As in vr_texture.h everything a texel sees is fp32, evaluated in the written order with no contraction, and uses +, -, *,
// comparisons, floorf, fminf / fmaxf and int <-> float conversions only, so a numpy float32 model (tests/stamp_model.py)
// reproduces the device bit for bit.  Division and trigonometry live in the preparation, on the host, in double, each result
// rounded to fp32 once (texture_round: never an infinity).  DESIGN.md 4y.
//
//   map          w0 x h0 texels span the world [-S/2, S/2]^2; texel i has its centre at texel coordinate i, world
//                x = (i + 0.5) * S / w0 - S/2 (vr_brush.h's convention).  The stamp is sw x sh texels; stamp texel k covers the
//                stamp coordinates [k, k + 1), its centre is at k + 0.5, and the stamp spans u in [0, sw], v in [0, sh].
//   placement    the stamp's centre is at world (x, z); its own u axis points along (cos r, sin r) in world (x, z), its v axis
//                along (-sin r, cos r), r = rotation; it is size_x world units long on u and size_z on v.
//   preparation  stamp_prepare, per call, in double with c = cos(r), s = sin(r) (each expression evaluated left to right):
//                  tx = S / w0                    tz = S / h0                       world units per map texel
//                  dx = (0.5 * tx - S / 2) - x    dz = (0.5 * tz - S / 2) - z       texel (0, 0)'s centre relative to the stamp's
//                  gu = sw / size_x               gv = sh / size_z                  stamp texels per world unit
//                  A00 = c * tx * gu      A01 = s * tz * gu      B0 = (c * dx + s * dz) * gu + 0.5 * sw
//                  A10 = -s * tx * gv     A11 = c * tz * gv      B1 = (c * dz - s * dx) * gv + 0.5 * sh
//                the two feather ramps, by texture_ramp's rule (vr_texture.h) on the rise from 0 to wd:
//                  wd_u = feather * (0.5 * sw)    wd_v = feather * (0.5 * sh)
//                  SOFT where wd > 0 and 1 / wd is a normal fp32 number: inv = 1 / wd;  HARD otherwise (a feather of 0): inv = 0
//                and the rectangle: the four corners (a, b) in {-0.5, 0.5}^2 lie at
//                  lx = a * size_x, lz = b * size_z;  wx = x + (lx * c - lz * s), wz = z + (lx * s + lz * c)
//                  px = (wx + S / 2) / S * w0 - 0.5,  pz = (wz + S / 2) / S * h0 - 0.5      map texel coordinates
//                [floor(min px) - 1, ceil(max px) + 2) x [floor(min pz) - 1, ceil(max pz) + 2) - the hull of the corners in
//                texel indices grown by one texel on each side, half open - clipped to the map.  Empty: the stamp misses the map.
//   texel (i, j) u = ((float)i * A00 + (float)j * A01) + B0, v = ((float)i * A10 + (float)j * A11) + B1.
//                COVERED when 0 <= u <= sw and 0 <= v <= sh; a texel that is not covered is not written.
//   weight       wu = 1 where inv_u == 0, else smooth(fminf(u, sw - u) * inv_u) with smooth(p) = (r * r) * (3 - 2 * r),
//                r = fminf(fmaxf(p, 0), 1) (texture_smooth); wv likewise; wf = wu * wv.
//   sample       per axis f = fminf(fmaxf(u - 0.5f, 0), sw - 1), i0 = (int)floorf(f), t = f - (float)i0, i1 = min(i0 + 1, sw - 1)
//                (texture_axis's form: clamp addressing); per channel s = texture_lerp2 of the four texels' bytes as floats.
//   value        s' = s * gain + offset (two operations);  a = wf * opacity, and under VR_STAMP_USE_ALPHA
//                a = a * (s_alpha * k255) with k255 = (float)(1.0 / 255.0) and s_alpha the stamp's sampled alpha (before gain).
//                val_c starts as the map's stored byte; per channel c of channel_mask:
//                  BLEND  brush_blend(val, a, 1, s')                     = clamp(val + a * (s' - val))
//                  ADD    clamp(val + a * s')                            SUB    clamp(val - a * s')
//                  MAX    brush_blend(val, a, 1, fmaxf(val, s'))         MIN    brush_blend(val, a, 1, fminf(val, s'))
//                (clamp: to [0, 255], brush_clamp); the byte is brush_byte(val_c), one rounding.
//
// A covered texel with a == 0 keeps its byte: every op then adds a product with 0 to an integer in [0, 255].  A texel reads only its
// own map texel and the stamp, which the call does not write, so the result does not depend on how the device divides the work or
// the order in which it visits the texels.  Every texel the fp32 expressions above find covered lies inside the rectangle:
// the expressions' rounding moves u by far less than one map texel's worth (i, j <= 16384: a few hundredths of a texel at most), which the
// rectangle's one texel of growth absorbs (tests/host/stamp_check.cpp).
//
// Sampling is bilinear and nothing else.  A stamp minified by more than about 2 - more than two stamp texels per map texel - skips
// texels and aliases; filtering it down first is the caller's business.
#pragma once
#include "vr_dirty.h"
#include "vr_texture.h"

#if defined(__HIPCC__)
#define VR_STAMP_FN __host__ __device__ __forceinline__
#else
#define VR_STAMP_FN inline
#endif

// vr_stamp's formats and vr_stamp_params' ops and flags (include/vrterrain.h: VR_STAMP_*)
constexpr int kStampR8 = 0, kStampSrgba8 = 1;
constexpr int kStampBlend = 0, kStampAdd = 1, kStampSub = 2, kStampMax = 3, kStampMin = 4;
constexpr uint32_t kStampUseAlpha = 1u;
constexpr int kStampMaxSide = 4096;
constexpr float kStampInv255 = (float)(1.0 / 255.0);

// Everything a call's kernel needs beside the map and the stamp: wave-uniform, passed by value.
struct StampConst {
    float A00, A01, B0, A10, A11, B1;
    float inv_u, inv_v;             // 0: a hard edge, weight 1
    float opacity, gain, offset;
    int32_t sw, sh;
    int32_t op;
    uint32_t channel_mask, flags;
};
static_assert(sizeof(StampConst) == 64, "StampConst layout");

// a placement as the caller states it (vr_stamp_params without its reserved words)
struct StampDesc {
    float x, z, size_x, size_z, rotation, opacity, feather, gain, offset;
    int32_t op;
    uint32_t channel_mask, flags;
};

// ---- preparation (host, double) ----------------------------------------------------------------------------------------------
// one axis of the rectangle: [floor(lo) - 1, ceil(hi) + 2) clipped to [0, n]; an end that is not a number clips to the wide side
inline void stamp_span(double lo, double hi, int n, int* x0, int* x1)
{
    const double a = floor(lo) - 1.0, b = ceil(hi) + 2.0;
    *x0 = !(a > 0.0) ? 0 : (a < (double)n ? (int)a : n);
    *x1 = !(b < (double)n) ? n : (b > 0.0 ? (int)b : 0);
}

// the caller has checked the ranges (finite fields, sizes > 0, 1 <= sw, sh <= kStampMaxSide); *rect may come out empty
inline StampConst stamp_prepare(const StampDesc& d, float world_size, int w0, int h0, int sw, int sh, DirtyRect* rect)
{
    StampConst k;
    const double S = (double)world_size, x = (double)d.x, z = (double)d.z, sx = (double)d.size_x, sz = (double)d.size_z;
    const double c = cos((double)d.rotation), s = sin((double)d.rotation);
    const double tx = S / w0, tz = S / h0;
    const double dx = (0.5 * tx - S / 2) - x, dz = (0.5 * tz - S / 2) - z;
    const double gu = sw / sx, gv = sh / sz;
    k.A00 = texture_round(c * tx * gu); k.A01 = texture_round(s * tz * gu); k.B0 = texture_round((c * dx + s * dz) * gu + 0.5 * sw);
    k.A10 = texture_round(-s * tx * gv); k.A11 = texture_round(c * tz * gv); k.B1 = texture_round((c * dz - s * dx) * gv + 0.5 * sh);
    float edge;
    texture_ramp(0.0, (double)d.feather * (0.5 * sw), true, &edge, &k.inv_u);
    texture_ramp(0.0, (double)d.feather * (0.5 * sh), true, &edge, &k.inv_v);
    k.opacity = d.opacity; k.gain = d.gain; k.offset = d.offset;
    k.sw = sw; k.sh = sh; k.op = d.op; k.channel_mask = d.channel_mask; k.flags = d.flags;
    double lo_x = 0.0, hi_x = 0.0, lo_z = 0.0, hi_z = 0.0;
    for (int q = 0; q < 4; q++) {
        const double lx = ((q & 1) ? 0.5 : -0.5) * sx, lz = ((q & 2) ? 0.5 : -0.5) * sz;
        const double wx = x + (lx * c - lz * s), wz = z + (lx * s + lz * c);
        const double px = (wx + S / 2) / S * w0 - 0.5, pz = (wz + S / 2) / S * h0 - 0.5;
        if (q == 0 || px < lo_x) lo_x = px;
        if (q == 0 || px > hi_x) hi_x = px;
        if (q == 0 || pz < lo_z) lo_z = pz;
        if (q == 0 || pz > hi_z) hi_z = pz;
    }
    stamp_span(lo_x, hi_x, w0, &rect->x0, &rect->x1);
    stamp_span(lo_z, hi_z, h0, &rect->y0, &rect->y1);
    return k;
}

// ---- per texel -----------------------------------------------------------------------------------------------------------
VR_STAMP_FN float stamp_coord(int i, int j, float a0, float a1, float b)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float p0 = (float)i * a0, p1 = (float)j * a1;
    const float p = p0 + p1;
    return p + b;
}
VR_STAMP_FN bool stamp_covered(float u, float v, float fsw, float fsh) { return u >= 0.0f && u <= fsw && v >= 0.0f && v <= fsh; }

// the feather's weight along one axis
VR_STAMP_FN float stamp_edge(float u, float fsw, float inv)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (inv == 0.0f) return 1.0f;
    const float rest = fsw - u;
    const float d = fminf(u, rest);
    return texture_smooth(d * inv);
}

// the bilinear tap of one axis: stamp coordinate u -> (i0, i1, t) on an axis of n texels, clamp addressing
VR_STAMP_FN void stamp_axis(float u, int n, int* i0, int* i1, float* t)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    float f = u - 0.5f;
    f = fminf(fmaxf(f, 0.0f), (float)(n - 1));
    const int a = (int)floorf(f);
    *i0 = a;
    *t = f - (float)a;
    *i1 = a + 1 < n - 1 ? a + 1 : n - 1;
}

VR_STAMP_FN float stamp_apply(int op, float val, float a, float sp)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (op == kStampAdd) { const float t = a * sp; return brush_clamp(val + t); }
    if (op == kStampSub) { const float t = a * sp; return brush_clamp(val - t); }
    const float to = op == kStampMax ? fmaxf(val, sp) : (op == kStampMin ? fminf(val, sp) : sp);
    return brush_blend(val, a, 1.0f, to);
}

// Map texel (i, j), whose NC values `val` start as its stored bytes.  `b(x, y)`: stamp texel (x, y), inside the stamp, as a dword
// (channel c in bits 8c .. 8c + 7; an R8 stamp's byte in the low eight).  false: not covered, `val` is untouched.
template <int NC, class Fetch>
VR_STAMP_FN bool stamp_texel(const StampConst& k, const Fetch& b, int i, int j, float (&val)[NC])
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float u = stamp_coord(i, j, k.A00, k.A01, k.B0), v = stamp_coord(i, j, k.A10, k.A11, k.B1);
    const float fsw = (float)k.sw, fsh = (float)k.sh;
    if (!stamp_covered(u, v, fsw, fsh)) return false;
    const float wu = stamp_edge(u, fsw, k.inv_u), wv = stamp_edge(v, fsh, k.inv_v);
    const float wf = wu * wv;
    int i0, i1, j0, j1;
    float tu, tv;
    stamp_axis(u, k.sw, &i0, &i1, &tu);
    stamp_axis(v, k.sh, &j0, &j1, &tv);
    const uint32_t t00 = b(i0, j0), t10 = b(i1, j0), t01 = b(i0, j1), t11 = b(i1, j1);
    float s[NC];
    for (int c = 0; c < NC; c++)
        s[c] = texture_lerp2((float)((t00 >> (8 * c)) & 255u), (float)((t10 >> (8 * c)) & 255u), (float)((t01 >> (8 * c)) & 255u),
                             (float)((t11 >> (8 * c)) & 255u), tu, tv);
    float a = wf * k.opacity;
    if (NC == 4 && (k.flags & kStampUseAlpha)) { const float al = s[NC - 1] * kStampInv255; a = a * al; }
    for (int c = 0; c < NC; c++) {
        if (!(k.channel_mask & (1u << c))) continue;
        const float g = s[c] * k.gain;
        const float sp = g + k.offset;
        val[c] = stamp_apply(k.op, val[c], a, sp);
    }
    return true;
}

// ---- the whole operation over host arrays (the host check drives it, the library does not) -------------------------------------
// map: w0 x h0 texels of NC bytes, changed in place inside `r`; stamp: k.sw x k.sh texels of NC bytes
template <int NC>
inline void stamp_serial(uint8_t* map, int w0, int h0, const uint8_t* stamp, const StampConst& k, const DirtyRect& r)
{
    const auto fetch = [=](int x, int y) -> uint32_t {
        const uint8_t* p = stamp + ((size_t)y * k.sw + x) * NC;
        uint32_t t = 0;
        for (int c = 0; c < NC; c++) t |= (uint32_t)p[c] << (8 * c);
        return t;
    };
    (void)h0;
    for (int j = r.y0; j < r.y1; j++)
        for (int i = r.x0; i < r.x1; i++) {
            uint8_t* px = map + ((size_t)j * w0 + i) * NC;
            float val[NC];
            for (int c = 0; c < NC; c++) val[c] = (float)px[c];
            if (!stamp_texel<NC>(k, fetch, i, j, val)) continue;
            for (int c = 0; c < NC; c++) px[c] = brush_byte(val[c]);
        }
}
