// Procedural noise on level 0 of one of a terrain's maps (vr_terrain_noise; its kernel: vr_noise.hip): fractal value or gradient
// noise in world space, added to or blended into the stored bytes under a brush mask or over the whole map.  The definition, for the
// device and for the host.  Plain C++17, no HIP types: the host compiles this header alone (tests/host/noise_check.cpp).
//
// As in vr_brush.h everything a texel sees is fp32, evaluated in the written order with no contraction, and uses +, -, *,
// comparisons, floorf, fabsf, fminf / fmaxf, int <-> float conversions and uint32 arithmetic only, so a numpy float32 / uint32 model
// (tests/noise_model.py) reproduces the device bit for bit.  Division and powers live in the preparation, on the host, in double,
// each result rounded to fp32 once.  DESIGN.md 4z.
//
//   map          w x h texels of map `which` span the world [-S/2, S/2]^2; the noise is a function of the world position of a texel's
//                centre, so the same parameters give the same landscape on maps of different resolution.
//   preparation  noise_prepare, per call (in double, rounded once; beyond fp32's range: +-FLT_MAX, never an infinity).  With
//                L_0 = 1, L_(o+1) = L_o * lacunarity and G_0 = 1, G_(o+1) = G_o * gain (running products: "lacunarity^o", "gain^o"),
//                F_o = frequency * L_o, for octave o < octaves:
//                  sx[o] = S / w * F_o                 sz[o] = S / h * F_o                  lattice cells per texel
//                  ox[o] = (offset_x - S / 2) * F_o    oz[o] = (offset_z - S / 2) * F_o     the lattice coordinate of the map's edge
//                  a[o]  = G_o / (G_0 + ... + G_(octaves-1))                                the weights: they sum to 1
//                The octaves from `octaves` to 11 hold zeros.
//   range        noise_in_range, per call, in double from the ROUNDED constants: for every octave the lattice coordinates of the
//                map's four corner texels, (0.5 | w - 0.5) * sx[o] + ox[o] and (0.5 | h - 0.5) * sz[o] + oz[o], are below 2^22 in
//                magnitude.  u is linear in the texel index, so that bounds it on the whole map.  It is what keeps
//                (int32_t)floorf(u) defined and tx = u - floorf(u) meaningful (at 2^22 an fp32 is a multiple of 0.5); the entry point
//                refuses a call that fails it.
//   lattice      texel (i, j), octave o (noise_axis):
//                  c = (float)i + 0.5f;  p = c * sx[o];  u = p + ox[o];  cx = floorf(u);  tx = u - cx  (in [0, 1]: 1 where u is a
//                  tiny negative number);  the cell is (uint32_t)(int32_t)cx - a negative cell wraps, in unsigned arithmetic;
//                  z likewise with j, sz, oz: cz, tz.
//   hash         noise_hash(x, y, s) = the project's avalanche (vr_tex.hip's vr_hash32): h = (x * 0x9E3779B1) ^ (y * 0x85EBCA77) ^
//                (s * 0xC2B2AE3D); h ^= h >> 16; h *= 0x7FEB352D; h ^= h >> 15; h *= 0x846CA68B; h ^= h >> 16 - all uint32.
//                Octave o hashes its corners (cx + dx, cz + dz), dx, dz in {0, 1} (uint32, wrapping), with s = seed + o.
//   fade         noise_fade(t): a = t * 6; b = a - 15; c = t * b; d = c + 10; t2 = t * t; t3 = t2 * t; fminf(t3 * d, 1) - the quintic
//                t^3 (t (6 t - 15) + 10).  In fp32 the product exceeds 1 by up to 1.1e-6 on some 22000 values of t just below 1,
//                hence the fminf; it is never negative (t3 >= 0, d >= 1).
//   basis        with fx = fade(tx), fz = fade(tz) and the corners q00 = (0, 0), q10 = (1, 0), q01 = (0, 1), q11 = (1, 1):
//                VALUE     q = (float)(int32_t)(hash >> 8) * 1.1920929e-07f - 1.0f: the top 24 bits as a multiple of 2^-23 in
//                          [-1, 1), exact.  n = lerp2(q00, q10, q01, q11, fx, fz), vr_texture.h's order:
//                          top = q00 + fx * (q10 - q00); bot = q01 + fx * (q11 - q01); n = top + fz * (bot - top).
//                          RANGE [-1, 1], proven: the corner differences are exact, fx and fz lie in [0, 1], so top and bot are
//                          rounded between two corners; bot - top is rounded by at most 2^-24 and the last sum lands within
//                          2^-24 of [-1, 1 - 2^-23], which rounds into [-1, 1].
//                GRADIENT  the corner's gradient is one of eight unit vectors, chosen by k = hash >> 29:
//                          0 (1, 0)  1 (-1, 0)  2 (0, 1)  3 (0, -1)  4 (r, r)  5 (-r, r)  6 (r, -r)  7 (-r, -r),  r = 0.70710678f;
//                          with the offset to the corner dx = tx - (0 | 1), dz = tz - (0 | 1):  p0 = gx * dx; p1 = gz * dz;
//                          q = p0 + p1.  e = lerp2(q00, q10, q01, q11, fx, fz); n = fminf(fmaxf(e * 1.41421354f, -1), 1).
//                          RANGE [-1, 1]: in real arithmetic |e| <= sqrt(2) / 2, reached at a cell's centre when its four diagonal
//                          gradients point at it, and the two constants multiply to 0.99999997 - less than one fp32 step below 1,
//                          which the roundings of the chain can use up.  The clamp is what makes the bound hold in fp32; it binds
//                          by ulps, if ever.  At a lattice point (tx = tz = 0) n is 0 exactly.
//   fractal      f = 0; for o = 0 .. octaves - 1, ascending:  f = f + a[o] * x_o  (t = a[o] * x_o; f = f + t)  with
//                FBM     x_o = n_o
//                BILLOW  x_o = 2 * |n_o| - 1          (two = 2 * fabsf(n_o); two - 1)
//                RIDGED  x_o = 1 - 2 * |n_o|          (1 - two)
//                and last f = fminf(fmaxf(f, -1), 1): |x_o| <= 1 and the weights sum to 1 before their rounding, so the clamp binds
//                by ulps, if ever.  f lies in [-1, 1].
//   apply        t = amplitude * f; per channel c of channel_mask (the heightmap has the one channel, mask 1; every selected
//                channel of an albedo texel receives the same f), the fp32 value starting as the stored byte, with the mask m:
//                ADD    val_c = brush_raise(val_c, m, t)                       val_c + m * t
//                BLEND  to = base + t; val_c = brush_blend(val_c, m, 1.0f, to)   val_c + m * (to - val_c)
//                - vr_brush.h's own functions, their clamp to [0, 255] included - and the byte is brush_byte(val_c).  m is the
//                erosions' mask of the texel (erode_mask_max over the dabs prepared for the map, vr_erode.h), or 1 on every texel
//                with VR_NOISE_WHOLE_MAP.
//
// A texel with mask 0 is not written.  A texel is a pure function of its own byte, its coordinates, the parameters and its mask, so
// the result cannot depend on the rectangle, the tile or how the device divides the work.
#pragma once
#include "vr_brush.h"
#include "vr_erode.h"

#if defined(__HIPCC__)
#define VR_NOISE_FN __host__ __device__ __forceinline__
#else
#define VR_NOISE_FN inline
#endif

constexpr int kNoiseMaxOctaves = 12;             // VR_NOISE_MAX_OCTAVES (include/vrterrain.h)
constexpr int kNoiseValue = 0, kNoiseGradient = 1;                  // VR_NOISE_VALUE, _GRADIENT
constexpr int kNoiseFbm = 0, kNoiseBillow = 1, kNoiseRidged = 2;    // VR_NOISE_FBM, _BILLOW, _RIDGED
constexpr int kNoiseAdd = 0, kNoiseBlend = 1;                       // VR_NOISE_ADD, _BLEND
constexpr float kNoiseMaxFloat = 3.402823466e38f;
constexpr double kNoiseCoordLimit = 4194304.0;   // 2^22

// Everything a call's kernel needs beside the map and the mask: wave-uniform, passed by value.
struct NoiseConst {
    float sx[kNoiseMaxOctaves], sz[kNoiseMaxOctaves], ox[kNoiseMaxOctaves], oz[kNoiseMaxOctaves], a[kNoiseMaxOctaves];
    float amplitude, base;
    uint32_t seed;
    int32_t octaves, basis, fractal, op;
    uint32_t channel_mask;
};
static_assert(sizeof(NoiseConst) == 20 * kNoiseMaxOctaves + 32, "NoiseConst layout");

// a call as the caller states it (vr_noise_params without its reserved words and flags)
struct NoiseDesc {
    float frequency, offset_x, offset_z, lacunarity, gain, amplitude, base;
    uint32_t seed;
    int32_t octaves, basis, fractal, op;
    uint32_t channel_mask;
};

// ---- preparation (host, double) ----------------------------------------------------------------------------------------------
inline float noise_round(double v)              // to fp32 once; beyond its range: +-FLT_MAX, never an infinity
{
    if (v > (double)kNoiseMaxFloat) return kNoiseMaxFloat;
    if (v < -(double)kNoiseMaxFloat) return -kNoiseMaxFloat;
    return (float)v;
}

// the caller has checked the ranges (1 <= octaves <= kNoiseMaxOctaves, frequency > 0, everything finite, the enums)
inline NoiseConst noise_prepare(const NoiseDesc& d, float world_size, int w, int h)
{
    NoiseConst k;
    const double S = (double)world_size;
    double total = 0.0, G = 1.0;
    for (int o = 0; o < d.octaves; o++) { total += G; G *= (double)d.gain; }
    double L = 1.0;
    G = 1.0;
    for (int o = 0; o < kNoiseMaxOctaves; o++) {
        if (o >= d.octaves) { k.sx[o] = k.sz[o] = k.ox[o] = k.oz[o] = k.a[o] = 0.0f; continue; }
        const double F = (double)d.frequency * L;
        k.sx[o] = noise_round(S / (double)w * F);
        k.sz[o] = noise_round(S / (double)h * F);
        k.ox[o] = noise_round(((double)d.offset_x - S / 2) * F);
        k.oz[o] = noise_round(((double)d.offset_z - S / 2) * F);
        k.a[o] = noise_round(G / total);
        L *= (double)d.lacunarity;
        G *= (double)d.gain;
    }
    k.amplitude = d.amplitude; k.base = d.base; k.seed = d.seed;
    k.octaves = d.octaves; k.basis = d.basis; k.fractal = d.fractal; k.op = d.op; k.channel_mask = d.channel_mask;
    return k;
}

// every lattice coordinate of every octave stays below 2^22 in magnitude on a w x h map (the comment's `range`)
inline bool noise_in_range(const NoiseConst& k, int w, int h)
{
    for (int o = 0; o < k.octaves; o++) {
        const double u0 = 0.5 * (double)k.sx[o] + (double)k.ox[o], u1 = ((double)w - 0.5) * (double)k.sx[o] + (double)k.ox[o];
        const double v0 = 0.5 * (double)k.sz[o] + (double)k.oz[o], v1 = ((double)h - 0.5) * (double)k.sz[o] + (double)k.oz[o];
        if (!(fabs(u0) < kNoiseCoordLimit && fabs(u1) < kNoiseCoordLimit && fabs(v0) < kNoiseCoordLimit && fabs(v1) < kNoiseCoordLimit)) return false;
    }
    return true;
}

// ---- per texel -----------------------------------------------------------------------------------------------------------
VR_NOISE_FN uint32_t noise_hash(uint32_t x, uint32_t y, uint32_t s)
{
    uint32_t h = (x * 0x9E3779B1u) ^ (y * 0x85EBCA77u) ^ (s * 0xC2B2AE3Du);
    h ^= h >> 16; h *= 0x7FEB352Du; h ^= h >> 15; h *= 0x846CA68Bu; h ^= h >> 16;
    return h;
}

// one axis of the lattice: texel index i -> the cell and the position inside it
VR_NOISE_FN void noise_axis(int i, float s, float o, uint32_t* cell, float* t)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float c = (float)i + 0.5f;
    const float p = c * s;
    const float u = p + o;
    const float cx = floorf(u);
    *t = u - cx;
    *cell = (uint32_t)(int32_t)cx;
}

VR_NOISE_FN float noise_fade(float t)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float a = t * 6.0f, b = a - 15.0f, c = t * b, d = c + 10.0f;
    const float t2 = t * t, t3 = t2 * t;
    return fminf(t3 * d, 1.0f);
}

VR_NOISE_FN float noise_lerp2(float q00, float q10, float q01, float q11, float tx, float tz)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float d0 = q10 - q00, p0 = tx * d0, top = q00 + p0;
    const float d1 = q11 - q01, p1 = tx * d1, bot = q01 + p1;
    const float dv = bot - top, pv = tz * dv;
    return top + pv;
}

// VALUE's corner: the hash's top 24 bits in [-1, 1)
VR_NOISE_FN float noise_corner_value(uint32_t hash)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float q = (float)(int32_t)(hash >> 8) * 1.1920929e-07f;
    return q - 1.0f;
}

// GRADIENT's corner: the gradient of `hash` against the offset (dx, dz) to that corner
VR_NOISE_FN float noise_corner_gradient(uint32_t hash, float dx, float dz)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const uint32_t k = hash >> 29;
    const float r = 0.70710678f;
    float gx, gz;
    if (k < 4u) {
        const float one = (k & 1u) ? -1.0f : 1.0f;
        gx = k < 2u ? one : 0.0f;
        gz = k < 2u ? 0.0f : one;
    } else {
        gx = (k & 1u) ? -r : r;
        gz = (k & 2u) ? -r : r;
    }
    const float p0 = gx * dx, p1 = gz * dz;
    return p0 + p1;
}

// n of one octave at the cell (cx, cz), position (tx, tz), hashed with `s`
VR_NOISE_FN float noise_basis(int basis, uint32_t cx, uint32_t cz, float tx, float tz, uint32_t s)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const uint32_t h00 = noise_hash(cx, cz, s), h10 = noise_hash(cx + 1u, cz, s), h01 = noise_hash(cx, cz + 1u, s), h11 = noise_hash(cx + 1u, cz + 1u, s);
    const float fx = noise_fade(tx), fz = noise_fade(tz);
    if (basis == kNoiseValue)
        return noise_lerp2(noise_corner_value(h00), noise_corner_value(h10), noise_corner_value(h01), noise_corner_value(h11), fx, fz);
    const float x1 = tx - 1.0f, z1 = tz - 1.0f;
    const float e = noise_lerp2(noise_corner_gradient(h00, tx, tz), noise_corner_gradient(h10, x1, tz), noise_corner_gradient(h01, tx, z1),
                                noise_corner_gradient(h11, x1, z1), fx, fz);
    return fminf(fmaxf(e * 1.41421354f, -1.0f), 1.0f);
}

// an octave's term from its n
VR_NOISE_FN float noise_term(int fractal, float n)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (fractal == kNoiseFbm) return n;
    const float two = 2.0f * fabsf(n);
    return fractal == kNoiseBillow ? two - 1.0f : 1.0f - two;
}

// f of texel (i, j); `n_out` (host only, may be null): the kNoiseMaxOctaves values n_o, zeros behind `octaves`
VR_NOISE_FN float noise_fractal(const NoiseConst& k, int i, int j, float* n_out = nullptr)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    float f = 0.0f;
    if (n_out) for (int o = 0; o < kNoiseMaxOctaves; o++) n_out[o] = 0.0f;
    for (int o = 0; o < kNoiseMaxOctaves; o++) {                   // a constant bound, left at the call's own count
        if (o >= k.octaves) break;
        uint32_t cx, cz;
        float tx, tz;
        noise_axis(i, k.sx[o], k.ox[o], &cx, &tx);
        noise_axis(j, k.sz[o], k.oz[o], &cz, &tz);
        const float n = noise_basis(k.basis, cx, cz, tx, tz, k.seed + (uint32_t)o);
        if (n_out) n_out[o] = n;
        const float t = k.a[o] * noise_term(k.fractal, n);
        f = f + t;
    }
    return fminf(fmaxf(f, -1.0f), 1.0f);
}

// one channel's value under the mask m
VR_NOISE_FN float noise_apply(const NoiseConst& k, float val, float m, float f)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float t = k.amplitude * f;
    if (k.op == kNoiseAdd) return brush_raise(val, m, t);
    const float to = k.base + t;
    return brush_blend(val, m, 1.0f, to);
}

// ---- the whole operation over host arrays (the host check drives it, the library does not) -------------------------------------
// texels: w x h x channels bytes (channels 1 or 4), changed in place; mask: w x h floats (1 everywhere for the whole map)
inline void noise_serial(uint8_t* texels, int w, int h, int channels, const NoiseConst& k, const float* mask)
{
    for (int j = 0; j < h; j++)
        for (int i = 0; i < w; i++) {
            const float m = mask[(size_t)j * w + i];
            if (!(m > 0.0f)) continue;
            const float f = noise_fractal(k, i, j);
            uint8_t* px = texels + ((size_t)j * w + i) * channels;
            for (int c = 0; c < channels; c++)
                if (k.channel_mask & (1u << c)) px[c] = brush_byte(noise_apply(k, (float)px[c], m, f));
        }
}
