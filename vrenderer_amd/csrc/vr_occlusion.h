// Sky visibility baked into level 0 of the albedo by horizon marching over the heightmap (vr_terrain_occlusion; its kernel:
// vr_occlusion.hip): every albedo texel under a brush mask, or of the whole map, marches the level-0 height bytes along 4, 8 or 16
// fixed directions out to a world-space radius, keeps the steepest horizon of each, and either tints the albedo towards a shadow
// colour by the occlusion that leaves (TINT) or stores the visibility as a byte (STORE).  The definition, for the device and for the
// host.  Plain C++17, no HIP types: the host compiles this header alone (tests/host/occlusion_check.cpp).
//
// As in vr_texture.h everything a texel sees is fp32, evaluated in the written order with no contraction, and uses +, -, *,
// comparisons, floorf, fminf / fmaxf, int <-> float conversions and integer arithmetic only, so a numpy float32 model
// (tests/occlusion_model.py) reproduces the device bit for bit.  Division, square root and trigonometry live in the preparation, on
// the host, in double, each result rounded to fp32 once; no infinity is carried.  DESIGN.md 4ad.
//
//   maps         the heightmap is w0 x h0 bytes b, the albedo wa x ha SRGBA8 texels; both span the world [-S/2, S/2]^2.
//   preparation  occlusion_prepare, per call (in double, rounded once):
//                  directions   DIR16 = (1,0) (2,1) (1,1) (1,2) (0,1) (-1,2) (-1,1) (-2,1) (-1,0) (-2,-1) (-1,-1) (-1,-2) (0,-1) (1,-2)
//                               (1,-1) (2,-1), as (dx, dz) in height texels; with D = directions (4, 8 or 16) direction d of the
//                               call is DIR16[d * (16 / D)], d = 0 .. D - 1
//                  per d        L_d = sqrt((dx * S / w0)^2 + (dz * S / h0)^2)          the world length of one step
//                               n_d = floor(radius / L_d)                               the number of steps; may be 0
//                               g_d = fp32(max_height / 255 / L_d)                      heightmap steps per march step -> the tangent
//                  rk[k]        fp32(1 / k), k = 1 .. 64
//                  V[q]         fp32(1 - sin(atan(q * TMAX / Q))), q = 0 .. Q, Q = 64, TMAX = 8: the cosine-weighted visibility of a
//                               direction whose horizon has tangent q / 8.  The definition is the piecewise-linear interpolant of
//                               this table, not the smooth function.
//                A call whose march reaches more than kOcclusionMaxReach = 64 height texels on an axis in some direction - n_d *
//                max(|dx|, |dz|) > 64 - is refused by the entry point, not clamped (occlusion_prepare returns false).
//   centre       albedo texel (i, j) stands on height texel x0 = ((2 i + 1) * w0) / (2 * wa), y0 = ((2 j + 1) * h0) / (2 * ha) - integer
//                division in 64 bits, no floating point; c = b[y0][x0]
//   march        per direction d: num = 0, den = 1; for k = 1 .. n_d in that order the sample (x0 + k dx, y0 + k dz); one outside the
//                map is skipped, not clamped; otherwise dh = b[..] - c, and if dh * den > num * k then num = dh, den = k (exact
//                integers; the comparison is strict: the first of several equal ratios wins)
//   direction    t = ((float)num * rk[den]) * g_d;  t = fmaxf(t - bias, 0);  u = fminf(t, TMAX) * 8.0f;
//                q = min((int)floorf(u), Q - 1);  f = u - (float)q;  v_d = V[q] + f * (V[q + 1] - V[q])
//   texel        vis = (((v_0 + v_1) + v_2) + ...) * (1.0f / D)   (left to right; 1 / D is a power of two)
//                o = fminf(fmaxf((1.0f - vis) * gain, 0.0f), 1.0f)
//   composite    the texture's (vr_texture.h): val_c starts as the stored byte, m is the erosions' mask of the texel over the dabs
//                prepared FOR THE ALBEDO, or 1 everywhere with VR_OCCLUSION_WHOLE_MAP; for each channel c of channel_mask
//                  TINT    val_c = brush_blend(val_c, m, o * opacity, color[c])           (the product o * opacity first)
//                  STORE   val_c = brush_blend(val_c, m, opacity, 255.0f * (1.0f - o))
//                and the byte is brush_byte(val_c).  A texel with m = 0 is not written.
//
// Locality.  A texel reads the height bytes (x0 + k dx, y0 + k dz) for 0 <= k <= n_d alone: none further than n_d |dx| by n_d |dz|
// from its centre, |k dx| <= n_d |dx| <= reach_x and |k dz| <= reach_z, where reach_x and reach_z are the largest n_d |dx| and n_d |dz|
// of the call's directions.  It reads no albedo texel but its own, and nothing the call writes (the heightmap is not written).  So the
// result does not depend on how the device divides the work, on the order of the texels, or on where the height bytes come from.
//
// The staged footprint's bound.  x0(i) = floor((i + 1/2) * w0 / wa) does not fall as i grows, and floor(a + b) - floor(a) <= ceil(b):
// over the 32 columns i .. i + 31 of a tile the centres lie in x0(i) .. x0(i) + ceil(31 w0 / wa), at most ceil(32 w0 / wa) + 1
// columns; the 8 rows likewise, ceil(8 h0 / ha) + 1.  The footprint of the tile whose first texel is (i, j) has its origin at
// (x0(i) - reach_x, y0(j) - reach_z) and is fw = ceil(32 w0 / wa) + 1 + 2 reach_x by fh = ceil(8 h0 / ha) + 1 + 2 reach_z bytes
// (occlusion_footprint), so a sample x = x0(i') + k dx of a texel i' of the tile has the local column x - (x0(i) - reach_x) =
// (x0(i') - x0(i)) + (k dx + reach_x), in [0, ceil(32 w0 / wa)] + [0, 2 reach_x] = [0, fw - 1]; rows likewise.  Every sample inside the
// map is therefore inside the footprint: OcclusionFoot's clamp is for memory safety alone and never binds
// (tests/host/occlusion_check.cpp counts the binds over 300 seeded maps and radii: 0).  A footprint cell beyond the map's edge holds
// the edge's byte and is never read - such a sample is skipped.
#pragma once
#include "vr_brush.h"
#include "vr_erode.h"

#include <math.h>
#include <stdlib.h>

#if defined(__HIPCC__)
#define VR_OCCLUSION_FN __host__ __device__ __forceinline__
#else
#define VR_OCCLUSION_FN inline
#endif

constexpr int kOcclusionMaxReach = 64;           // VR_OCCLUSION_MAX_REACH (include/vrterrain.h)
constexpr int kOcclusionMaxDirs = 16;
constexpr int kOcclusionQ = 64;                  // the visibility table's intervals
constexpr float kOcclusionTMax = 8.0f;           // ... over tangents 0 .. 8: Q / TMAX = 8, exact
constexpr int kOcclusionTint = 0, kOcclusionStore = 1;           // VR_OCCLUSION_TINT / _STORE
constexpr int kOcclusionFootBytes = 32768;       // the largest footprint the kernel stages in LDS
constexpr float kOcclusionMaxFloat = 3.402823466e38f;

constexpr int kOcclusionDir16[16][2] = { { 1, 0 }, { 2, 1 }, { 1, 1 }, { 1, 2 }, { 0, 1 }, { -1, 2 }, { -1, 1 }, { -2, 1 },
                                         { -1, 0 }, { -2, -1 }, { -1, -1 }, { -1, -2 }, { 0, -1 }, { 1, -2 }, { 1, -1 }, { 2, -1 } };

// Everything a call's kernel needs beside the maps and the mask: wave-uniform, passed by value.
struct OcclusionConst {
    float V[kOcclusionQ + 1];                    // the visibility table
    float rk[kOcclusionMaxReach + 1];            // rk[k] = 1 / k; rk[0] = 0, never read (den >= 1)
    int32_t dx[kOcclusionMaxDirs], dz[kOcclusionMaxDirs], n[kOcclusionMaxDirs];
    float g[kOcclusionMaxDirs];
    float bias, gain, opacity, inv_d;            // inv_d = 1 / directions
    float color[4];
    uint32_t channel_mask, mode;
    int32_t directions, reach_x, reach_z, pad;
};
static_assert(sizeof(OcclusionConst) == 4 * (65 + 65 + 4 * 16 + 8 + 6), "OcclusionConst layout");

// the call as the caller states it (vr_occlusion_params without its flags and reserved words)
struct OcclusionDesc {
    float radius, max_height, gain, bias, opacity, color[4];
    uint32_t channel_mask;
    int32_t directions;
    uint32_t mode;
};

// ---- preparation (host, double) ----------------------------------------------------------------------------------------------
inline float occlusion_round(double v)          // to fp32 once; beyond its range: FLT_MAX, never an infinity
{
    return v > (double)kOcclusionMaxFloat ? kOcclusionMaxFloat : (float)v;
}

// The caller has checked the ranges (radius, max_height finite and > 0, directions 4, 8 or 16, the others').  false: the march of some
// direction reaches more than kOcclusionMaxReach height texels on an axis (or the maps' sizes give no step length at all); then *k
// is not to be used.
inline bool occlusion_prepare(const OcclusionDesc& p, float world_size, int w0, int h0, OcclusionConst* k)
{
    const double S = (double)world_size;
    const int D = p.directions, stride = kOcclusionMaxDirs / D;
    bool ok = true;
    k->reach_x = k->reach_z = 0;
    for (int d = 0; d < kOcclusionMaxDirs; d++) {
        k->dx[d] = k->dz[d] = k->n[d] = 0; k->g[d] = 0.0f;
        if (d >= D) continue;
        const int dx = kOcclusionDir16[d * stride][0], dz = kOcclusionDir16[d * stride][1];
        const double ax = (double)dx * S / (double)w0, az = (double)dz * S / (double)h0;
        const double L = sqrt(ax * ax + az * az);
        const double steps = floor((double)p.radius / L);
        const int far = abs(dx) > abs(dz) ? abs(dx) : abs(dz);
        if (!(steps * (double)far <= (double)kOcclusionMaxReach)) { ok = false; continue; }       // (a NaN is refused too)
        const int n = (int)steps;
        k->dx[d] = dx; k->dz[d] = dz; k->n[d] = n;
        k->g[d] = occlusion_round((double)p.max_height / 255.0 / L);
        if (n * abs(dx) > k->reach_x) k->reach_x = n * abs(dx);
        if (n * abs(dz) > k->reach_z) k->reach_z = n * abs(dz);
    }
    k->rk[0] = 0.0f;
    for (int i = 1; i <= kOcclusionMaxReach; i++) k->rk[i] = (float)(1.0 / (double)i);
    for (int q = 0; q <= kOcclusionQ; q++) k->V[q] = (float)(1.0 - sin(atan((double)q * (double)kOcclusionTMax / (double)kOcclusionQ)));
    k->bias = p.bias; k->gain = p.gain; k->opacity = p.opacity; k->inv_d = 1.0f / (float)D;        // (a power of two: exact)
    for (int c = 0; c < 4; c++) k->color[c] = p.color[c];
    k->channel_mask = p.channel_mask; k->mode = p.mode;
    k->directions = D; k->pad = 0;
    return ok;
}

// the staged footprint of a 32 x 8 tile (the comment's bound), in bytes each way
inline void occlusion_footprint(const OcclusionConst& k, int w0, int h0, int wa, int ha, int tile_w, int tile_h, int64_t* fw, int64_t* fh)
{
    *fw = ((int64_t)tile_w * w0 + wa - 1) / wa + 1 + 2 * (int64_t)k.reach_x;
    *fh = ((int64_t)tile_h * h0 + ha - 1) / ha + 1 + 2 * (int64_t)k.reach_z;
}

// ---- per texel -----------------------------------------------------------------------------------------------------------
// the height texel albedo texel i stands on, on an axis of n0 height texels under na albedo texels
VR_OCCLUSION_FN int occlusion_centre(int i, int n0, int na) { return (int)(((2 * (int64_t)i + 1) * (int64_t)n0) / (2 * (int64_t)na)); }

VR_OCCLUSION_FN int occlusion_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// 24-bit integer products: |dh| <= 255, den and k <= 64, so every product of the march fits, and the device has them at full rate
VR_OCCLUSION_FN int occlusion_mul(int a, int b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __mul24(a, b);
#else
    return a * b;
#endif
}

// How the march reads a height byte: at(x, y) is the address of a texel inside the map, step(dx, dz) what one march step adds to it,
// load(a) the byte.  From the map itself: every address the march forms belongs to a sample inside the map.
struct OcclusionDirect {
    const uint8_t* height; int w0;
    VR_OCCLUSION_FN int at(int x, int y) const { return y * w0 + x; }                  // (a map has at most 2^26 texels)
    VR_OCCLUSION_FN int step(int dx, int dz) const { return dz * w0 + dx; }
    VR_OCCLUSION_FN int load(int a) const { return (int)height[a]; }
};
// ... and from a tile's staged footprint: texel (ox + lx, oy + ly), clamped to the map, at [ly * fw + lx].  The clamps - of the centre
// into the footprint, of an address into its fw * fh bytes - never bind (the comment's bound); were the tile size or the origin changed
// without fw and fh they would give wrong bytes, not a fault, and the byte-exact tests are the check.
struct OcclusionFoot {
    const uint8_t* foot; int ox, oy, fw, fh;
    VR_OCCLUSION_FN int at(int x, int y) const { return occlusion_clampi(y - oy, 0, fh - 1) * fw + occlusion_clampi(x - ox, 0, fw - 1); }
    VR_OCCLUSION_FN int step(int dx, int dz) const { return dz * fw + dx; }
    VR_OCCLUSION_FN int load(int a) const
    {
        const unsigned last = (unsigned)(fw * fh - 1), u = (unsigned)a;
        return (int)foot[u < last ? u : last];
    }
};

// how many steps of d from p stay on an axis of n0 texels (d: 0, +-1 or +-2); kOcclusionMaxReach: all of them
VR_OCCLUSION_FN int occlusion_room(int p, int d, int n0)
{
    if (d == 0) return kOcclusionMaxReach;
    const int r = d > 0 ? n0 - 1 - p : p;
    return d == 1 || d == -1 ? r : r >> 1;
}

// The steepest horizon of direction (dx, dz) seen from height texel (x0, y0), whose byte is c: *num / *den, the rise in heightmap
// steps over the step count.  The march runs along a straight line out of a convex map: its samples are inside the map for k <= lim
// and outside it from then on.  A skipped sample reads the centre's byte instead - dh = 0, which never wins: num starts at 0 and only
// grows, so 0 * den > num * k is false.  Returns how many samples were skipped (the host's checks count them; the device drops the
// value).
template <class Fetch>
VR_OCCLUSION_FN int occlusion_march(const Fetch& b, int w0, int h0, int x0, int y0, int c, int dx, int dz, int n, int* num, int* den)
{
    const int rx = occlusion_room(x0, dx, w0), rz = occlusion_room(y0, dz, h0);
    const int room = rx < rz ? rx : rz, lim = n < room ? n : room;
    const int home = b.at(x0, y0), da = b.step(dx, dz);
    int best = 0, at = 1, a = home;
    for (int k = 1; k <= n; k++) {
        a += da;
        const int dh = b.load(k <= lim ? a : home) - c;
        if (occlusion_mul(dh, at) > occlusion_mul(best, k)) { best = dh; at = k; }
    }
    *num = best; *den = at;
    return n - lim;
}

// the visibility of a direction whose horizon is num / den march steps; V, rk: the call's tables, wherever they are kept
VR_OCCLUSION_FN float occlusion_direction(const float* V, const float* rk, float g, float bias, int num, int den)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float r = (float)num * rk[den];
    float t = r * g;
    t = fmaxf(t - bias, 0.0f);
    const float u = fminf(t, kOcclusionTMax) * 8.0f;
    int q = (int)floorf(u);
    q = q < kOcclusionQ - 1 ? q : kOcclusionQ - 1;
    const float f = u - (float)q;
    const float lo = V[q], d = V[q + 1] - lo;
    const float fd = f * d;
    return lo + fd;
}

// the occlusion o of the albedo texel that stands on height texel (x0, y0)
template <class Fetch>
VR_OCCLUSION_FN float occlusion_texel(const OcclusionConst& k, const float* V, const float* rk, const Fetch& b, int w0, int h0, int x0, int y0)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const int c = b.load(b.at(x0, y0));
    float sum = 0.0f;                            // (0 + v_0 is v_0)
    for (int d = 0; d < kOcclusionMaxDirs; d++) {
        if (d >= k.directions) break;
        int num, den;
        occlusion_march(b, w0, h0, x0, y0, c, k.dx[d], k.dz[d], k.n[d], &num, &den);
        sum = sum + occlusion_direction(V, rk, k.g[d], k.bias, num, den);
    }
    const float vis = sum * k.inv_d;
    const float s = 1.0f - vis;
    return fminf(fmaxf(s * k.gain, 0.0f), 1.0f);
}

// the call on the four values of a texel whose mask is m and whose occlusion is o
VR_OCCLUSION_FN void occlusion_composite(const OcclusionConst& k, float o, float m, float (&val)[4])
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const bool store = k.mode == (uint32_t)kOcclusionStore;
    const float w = store ? k.opacity : o * k.opacity;
    const float vb = 1.0f - o;
    const float stored = 255.0f * vb;
    for (int c = 0; c < 4; c++)
        if (k.channel_mask & (1u << c)) val[c] = brush_blend(val[c], m, w, store ? stored : k.color[c]);
}

// ---- the whole operation over host arrays (the host check drives it, the library does not) -------------------------------------
// height: w0 x h0 bytes; albedo: wa x ha x 4 bytes, changed in place; mask: wa x ha floats (1 everywhere for the whole map);
// fetch_of(i, j): the fetch albedo texel (i, j) reads its height bytes through
template <class FetchOf>
inline void occlusion_serial(int w0, int h0, uint8_t* albedo, int wa, int ha, const OcclusionConst& k, const float* mask, const FetchOf& fetch_of)
{
    for (int j = 0; j < ha; j++)
        for (int i = 0; i < wa; i++) {
            const float m = mask[(size_t)j * wa + i];
            if (!(m > 0.0f)) continue;
            const float o = occlusion_texel(k, k.V, k.rk, fetch_of(i, j), w0, h0, occlusion_centre(i, w0, wa), occlusion_centre(j, h0, ha));
            uint8_t* px = albedo + ((size_t)j * wa + i) * 4;
            float val[4];
            for (int c = 0; c < 4; c++) val[c] = (float)px[c];
            occlusion_composite(k, o, m, val);
            for (int c = 0; c < 4; c++) px[c] = brush_byte(val[c]);
        }
}
