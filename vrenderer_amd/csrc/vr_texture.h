// Rule-based painting of level 0 of the albedo from the heightmap's shape (vr_terrain_texture; its kernel: vr_texture.hip): altitude
// and slope layers under a brush mask or over the whole map.  The definition, for the device and for the host.  Plain C++17, no HIP
// types: the host compiles this header alone (tests/host/texture_check.cpp).
//
// As in vr_brush.h everything a texel sees is fp32, evaluated in the written order with no contraction, and uses +, -, *,
// comparisons, floorf, fminf / fmaxf and int <-> float conversions only, so a numpy float32 model (tests/texture_model.py)
// reproduces the device bit for bit.  Division, square root and trigonometry live in the preparation, on the host, in double, each
// result rounded to fp32 once.  DESIGN.md 4x.
//
//   maps         the heightmap is w0 x h0 bytes, the albedo wa x ha SRGBA8 texels; both span the world [-S/2, S/2]^2.
//   preparation  texture_prepare, per call (in double, rounded once):
//                  rx = w0 / wa                       rz = h0 / ha               height texels per albedo texel
//                  kx = max_height / 255 * w0 / S     kz = max_height / 255 * h0 / S
//                                                                              heightmap steps per height texel -> the tangent
//                per layer, with A(v) = v * 255 / max_height (world units of height -> heightmap steps) and
//                T(d) = tan(d * pi / 180)^2 (degrees -> SQUARED tangent), four ramps as (edge, inv):
//                  altitude rise   from A(alt_lo - alt_fade) to A(alt_lo)       altitude fall   from A(alt_hi) to A(alt_hi + alt_fade)
//                  slope rise      from T(max(slope_lo - slope_fade, 0)) to T(slope_lo)
//                  slope fall      from T(slope_hi) to T(min(slope_hi + slope_fade, 89.5))
//                A ramp of width wd = to - from > 0 (in double) whose 1 / wd is a normal fp32 number is SOFT: edge = the outer end - `from`
//                of a rise, `to` of a fall - and inv = 1 / wd.  Every other ramp - a fade of 0, a slope fade clamped away, a width
//                whose reciprocal overflows - is HARD: edge = the band's own end (`to` of a rise, `from` of a fall) and inv = 0.
//                No infinity is ever carried: an edge beyond fp32's range is stored as +-FLT_MAX (no height or slope reaches it).
//   sample       albedo texel (i, j) looks at the height coordinate
//                  fx = ((float)i + 0.5f) * rx - 0.5f, then fx = fminf(fmaxf(fx, 0.0f), (float)(w0 - 1));
//                  i0 = (int)floorf(fx), tx = fx - (float)i0, i1 = min(i0 + 1, w0 - 1);      z likewise with j, rz, h0: j0, tz, j1
//   height texel (x, y) of the heightmap's level-0 bytes b gives (texture_corner)
//                  h = (float)b[y][x]
//                  gx = (float)(b[y][min(x + 1, w0 - 1)] - b[y][max(x - 1, 0)]) * 0.5f      (the integer difference first: exact)
//                  gz = (float)(b[min(y + 1, h0 - 1)][x] - b[max(y - 1, 0)][x]) * 0.5f
//   albedo texel each of h, gx, gz at the corners q00 = (i0, j0), q10 = (i1, j0), q01 = (i0, j1), q11 = (i1, j1) (texture_lerp2):
//                  top = q00 + tx * (q10 - q00);  bot = q01 + tx * (q11 - q01);  q = top + tz * (bot - top)
//                then ax = gx * kx, az = gz * kz, s2 = ax * ax + az * az                     (the squared tangent of the slope)
//   band         a SOFT ramp is r = fminf(fmaxf(p, 0), 1) with p = (v - edge) * inv for a rise and (edge - v) * inv for a fall,
//                smoothed as (r * r) * (3 - 2 * r); a HARD rise is v >= edge ? 1 : 0, a HARD fall v <= edge ? 1 : 0
//                (texture_rise, texture_fall; v = h for the altitude ramps, s2 for the slope ramps).  The layer's weight is
//                  wl = ((ra_lo * ra_hi) * (rs_lo * rs_hi)) * opacity                         (texture_layer_weight)
//   composite    val_c starts as the stored byte; the layers are applied in list order: for each channel c of the layer's mask
//                val_c = brush_blend(val_c, m, wl, color[c]) - vr_brush.h's own function, a = m * wl, its clamp included; after the
//                last layer the byte is brush_byte(val_c).  m is the erosions' mask of the texel (erode_mask_max over the dabs
//                prepared FOR THE ALBEDO MAP, vr_erode.h), or 1 on every texel with VR_TEXTURE_WHOLE_MAP.
//
// A texel with mask 0 is not written.  A texel whose layers all weigh 0 keeps its byte: every blend then adds a * d = 0 to an
// integer in [0, 255], and brush_byte of an untouched byte is that byte.  A texel is a pure function of the two maps as they were
// before the call and reads no albedo texel but its own, so the result does not depend on how the device divides the work or on
// where it reads the height bytes from (LDS or memory).
#pragma once
#include "vr_brush.h"
#include "vr_erode.h"

#if defined(__HIPCC__)
#define VR_TEXTURE_FN __host__ __device__ __forceinline__
#else
#define VR_TEXTURE_FN inline
#endif

constexpr int kTextureMaxLayers = 8;             // VR_TEXTURE_MAX_LAYERS (include/vrterrain.h)
constexpr int kRampAltLo = 0, kRampAltHi = 1, kRampSlopeLo = 2, kRampSlopeHi = 3;
constexpr float kTextureMaxFloat = 3.402823466e38f;

// A prepared layer, as the kernel reads it.
struct TextureLayer {
    float color[4];             // stored encoding, [0, 255]
    float opacity;
    float edge[4], inv[4];      // the four ramps (kRamp*); inv == 0: a hard edge
    uint32_t channel_mask;
    uint32_t pad[2];
};
static_assert(sizeof(TextureLayer) == 64, "TextureLayer layout");

// Everything a call's kernel needs beside the maps and the mask: wave-uniform, passed by value.
struct TextureConst {
    float rx, rz, kx, kz;
    int32_t num_layers, pad[3];
    TextureLayer layer[kTextureMaxLayers];
};
static_assert(sizeof(TextureConst) == 32 + 64 * kTextureMaxLayers, "TextureConst layout");

// one layer as the caller states it (vr_texture_layer without its reserved words)
struct TextureLayerDesc {
    float color[4], opacity, alt_lo, alt_hi, alt_fade, slope_lo, slope_hi, slope_fade;
    uint32_t channel_mask;
};

// ---- preparation (host, double) ----------------------------------------------------------------------------------------------
inline float texture_round(double v)            // to fp32 once; beyond its range: +-FLT_MAX, never an infinity
{
    if (v > (double)kTextureMaxFloat) return kTextureMaxFloat;
    if (v < -(double)kTextureMaxFloat) return -kTextureMaxFloat;
    return (float)v;
}
// the ramp from `from` to `to` (from <= to); rise: 0 at `from`, 1 at `to`; fall: 1 at `from`, 0 at `to`
inline void texture_ramp(double from, double to, bool rise, float* edge, float* inv)
{
    const double wd = to - from;
    if (wd > 0.0) {
        const double r = 1.0 / wd;
        if (r <= (double)kTextureMaxFloat && (float)r >= 1.17549435e-38f) { *edge = texture_round(rise ? from : to); *inv = (float)r; return; }      // a normal fp32 number
    }
    *edge = texture_round(rise ? to : from); *inv = 0.0f;
}
inline double texture_tan2(double deg) { const double t = tan(deg * 3.14159265358979323846 / 180.0); return t * t; }

inline TextureLayer texture_prepare_layer(const TextureLayerDesc& d, float max_height)
{
    TextureLayer l;
    for (int c = 0; c < 4; c++) l.color[c] = d.color[c];
    l.opacity = d.opacity;
    const double A = 255.0 / (double)max_height;
    const double alo = (double)d.alt_lo, ahi = (double)d.alt_hi, af = (double)d.alt_fade;
    texture_ramp((alo - af) * A, alo * A, true, &l.edge[kRampAltLo], &l.inv[kRampAltLo]);
    texture_ramp(ahi * A, (ahi + af) * A, false, &l.edge[kRampAltHi], &l.inv[kRampAltHi]);
    const double slo = (double)d.slope_lo, shi = (double)d.slope_hi, sf = (double)d.slope_fade;
    const double below = slo - sf > 0.0 ? slo - sf : 0.0, above = shi + sf < 89.5 ? shi + sf : 89.5;
    texture_ramp(texture_tan2(below), texture_tan2(slo), true, &l.edge[kRampSlopeLo], &l.inv[kRampSlopeLo]);
    texture_ramp(texture_tan2(shi), texture_tan2(above), false, &l.edge[kRampSlopeHi], &l.inv[kRampSlopeHi]);
    l.channel_mask = d.channel_mask;
    l.pad[0] = l.pad[1] = 0;
    return l;
}

// the caller has checked the ranges (1 <= n <= kTextureMaxLayers, max_height finite and > 0, the layers' own)
inline TextureConst texture_prepare(const TextureLayerDesc* layers, int n, float max_height, float world_size, int w0, int h0, int wa, int ha)
{
    TextureConst k;
    const double S = (double)world_size, step = (double)max_height / 255.0;
    k.rx = texture_round((double)w0 / (double)wa);
    k.rz = texture_round((double)h0 / (double)ha);
    k.kx = texture_round(step * (double)w0 / S);
    k.kz = texture_round(step * (double)h0 / S);
    k.num_layers = n; k.pad[0] = k.pad[1] = k.pad[2] = 0;
    for (int i = 0; i < kTextureMaxLayers; i++) {
        if (i < n) { k.layer[i] = texture_prepare_layer(layers[i], max_height); continue; }
        TextureLayer& l = k.layer[i];
        for (int c = 0; c < 4; c++) { l.color[c] = 0.0f; l.edge[c] = 0.0f; l.inv[c] = 0.0f; }
        l.opacity = 0.0f; l.channel_mask = 0; l.pad[0] = l.pad[1] = 0;
    }
    return k;
}

// ---- per texel -----------------------------------------------------------------------------------------------------------
// the sample point of one axis: albedo index i -> (i0, i1, t) on a height axis of n texels
VR_TEXTURE_FN void texture_axis(int i, float r, int n, int* i0, int* i1, float* t)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float c = (float)i + 0.5f;
    const float p = c * r;
    float f = p - 0.5f;
    f = fminf(fmaxf(f, 0.0f), (float)(n - 1));
    const int a = (int)floorf(f);
    *i0 = a;
    *t = f - (float)a;
    *i1 = a + 1 < n - 1 ? a + 1 : n - 1;
}

VR_TEXTURE_FN int texture_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// h, gx, gz of height texel (x, y), inside the map; `b(x, y)`: the byte of a texel inside the map, as an int
template <class Fetch>
VR_TEXTURE_FN void texture_corner(const Fetch& b, int w0, int h0, int x, int y, float* h, float* gx, float* gz)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    *h = (float)b(x, y);
    const int dx = b(texture_clampi(x + 1, 0, w0 - 1), y) - b(texture_clampi(x - 1, 0, w0 - 1), y);
    const int dz = b(x, texture_clampi(y + 1, 0, h0 - 1)) - b(x, texture_clampi(y - 1, 0, h0 - 1));
    *gx = (float)dx * 0.5f;
    *gz = (float)dz * 0.5f;
}

VR_TEXTURE_FN float texture_lerp2(float q00, float q10, float q01, float q11, float tx, float tz)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float d0 = q10 - q00, p0 = tx * d0, top = q00 + p0;
    const float d1 = q11 - q01, p1 = tx * d1, bot = q01 + p1;
    const float dv = bot - top, pv = tz * dv;
    return top + pv;
}

// the height h (heightmap steps) and the squared tangent s2 under albedo texel (i, j)
template <class Fetch>
VR_TEXTURE_FN void texture_sample(const TextureConst& k, const Fetch& b, int w0, int h0, int i, int j, float* h, float* s2)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    int i0, i1, j0, j1;
    float tx, tz;
    texture_axis(i, k.rx, w0, &i0, &i1, &tx);
    texture_axis(j, k.rz, h0, &j0, &j1, &tz);
    float h00, h10, h01, h11, x00, x10, x01, x11, z00, z10, z01, z11;
    texture_corner(b, w0, h0, i0, j0, &h00, &x00, &z00);
    texture_corner(b, w0, h0, i1, j0, &h10, &x10, &z10);
    texture_corner(b, w0, h0, i0, j1, &h01, &x01, &z01);
    texture_corner(b, w0, h0, i1, j1, &h11, &x11, &z11);
    *h = texture_lerp2(h00, h10, h01, h11, tx, tz);
    const float gx = texture_lerp2(x00, x10, x01, x11, tx, tz);
    const float gz = texture_lerp2(z00, z10, z01, z11, tx, tz);
    const float ax = gx * k.kx, az = gz * k.kz;
    const float xx = ax * ax, zz = az * az;
    *s2 = xx + zz;
}

VR_TEXTURE_FN float texture_smooth(float p)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float r = fminf(fmaxf(p, 0.0f), 1.0f);
    const float rr = r * r, two = 2.0f * r, s = 3.0f - two;
    return rr * s;
}
VR_TEXTURE_FN float texture_rise(float v, float edge, float inv)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (inv == 0.0f) return v >= edge ? 1.0f : 0.0f;
    const float d = v - edge;
    return texture_smooth(d * inv);
}
VR_TEXTURE_FN float texture_fall(float v, float edge, float inv)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (inv == 0.0f) return v <= edge ? 1.0f : 0.0f;
    const float d = edge - v;
    return texture_smooth(d * inv);
}

VR_TEXTURE_FN float texture_layer_weight(const TextureLayer& l, float h, float s2)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float ra_lo = texture_rise(h, l.edge[kRampAltLo], l.inv[kRampAltLo]);
    const float ra_hi = texture_fall(h, l.edge[kRampAltHi], l.inv[kRampAltHi]);
    const float rs_lo = texture_rise(s2, l.edge[kRampSlopeLo], l.inv[kRampSlopeLo]);
    const float rs_hi = texture_fall(s2, l.edge[kRampSlopeHi], l.inv[kRampSlopeHi]);
    const float ra = ra_lo * ra_hi, rs = rs_lo * rs_hi;
    const float w = ra * rs;
    return w * l.opacity;
}

// the layers, in list order, on the four values of a texel whose mask is m
VR_TEXTURE_FN void texture_composite(const TextureConst& k, float h, float s2, float m, float (&val)[4])
{
    for (int l = 0; l < kTextureMaxLayers; l++) {
        if (l >= k.num_layers) break;
        const TextureLayer& L = k.layer[l];
        const float wl = texture_layer_weight(L, h, s2);
        for (int c = 0; c < 4; c++)
            if (L.channel_mask & (1u << c)) val[c] = brush_blend(val[c], m, wl, L.color[c]);
    }
}

// ---- the whole operation over host arrays (the host check drives it, the library does not) -------------------------------------
// height: w0 x h0 bytes; albedo: wa x ha x 4 bytes, changed in place; mask: wa x ha floats (1 everywhere for the whole map)
inline void texture_serial(const uint8_t* height, int w0, int h0, uint8_t* albedo, int wa, int ha, const TextureConst& k, const float* mask)
{
    const auto fetch = [=](int x, int y) -> int { return (int)height[(size_t)y * w0 + x]; };
    for (int j = 0; j < ha; j++)
        for (int i = 0; i < wa; i++) {
            const float m = mask[(size_t)j * wa + i];
            if (!(m > 0.0f)) continue;
            float h, s2, val[4];
            texture_sample(k, fetch, w0, h0, i, j, &h, &s2);
            uint8_t* px = albedo + ((size_t)j * wa + i) * 4;
            for (int c = 0; c < 4; c++) val[c] = (float)px[c];
            texture_composite(k, h, s2, m, val);
            for (int c = 0; c < 4; c++) px[c] = brush_byte(val[c]);
        }
}
