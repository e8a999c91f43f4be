// Thermal (talus) erosion of level 0 of the heightmap under a brush mask (vr_terrain_erode; its kernels: vr_erode.hip): the definition, for the
// device and for the host.  Plain C++17, no HIP types: the host compiles this header alone (tests/host/erode_check.cpp).
//
// As in vr_brush.h everything a texel sees is fp32, evaluated in the written order with no contraction, and uses +, -, *,
// comparisons, floorf and int -> float conversions only, so a numpy float32 model (tests/erode_model.py) reproduces the device
// bit for bit.  DESIGN.md 4u.
//
//   mask        the dabs are prepared as for a stroke on the heightmap (brush_prepare, empty dabs dropped); the mask of texel c is
//               m_c = max over the kept dabs that cover it of f * strength (f: brush_weight, strength in [0, 1]), 0 where none
//               does.  A maximum has no order.  The rectangle is the hull of the kept spans; every texel outside it has mask 0.
//   state       h_c, fp32, starts as the stored byte.
//   iteration   every cell from the previous iteration's state only: acc = 0.0f, then for the eight neighbours n in the order
//               (dx, dy) = (-1,-1) (0,-1) (1,-1) (-1,0) (1,0) (-1,1) (0,1) (1,1) that lie inside the MAP (erode_edge):
//                 T = talus for the four axis neighbours, talus * 1.41421354f (one fp32 product per call) for the diagonals
//                 w = min(m_c, m_n); the edge is skipped unless w > 0
//                 h_c >= h_n:  e = (h_c - h_n) - T;  e > 0:  acc = acc - (rate * e) * w
//                 otherwise:   e = (h_n - h_c) - T;  e > 0:  acc = acc + (rate * e) * w
//               so both ends of an edge compute the same magnitude; then h_c' = h_c + acc.  Nothing is clamped in between.
//   end         after `iterations` sweeps a texel with m_c > 0 is stored as (uint8)floorf(min(max(h, 0), 255) + 0.5f)
//               (erode_byte); one with m_c == 0 is not written.
//
// A texel outside the rectangle has mask 0, so no edge reaches it: the whole computation lives inside the rectangle, and a cell
// is a pure function of the previous sweep - the result cannot depend on how the device cuts the rectangle into tiles or on how
// many sweeps one launch advances.  erode_serial is the definition in executable form (two buffers, swapped per iteration); the
// host check drives it, the library does not.
#pragma once
#include "vr_brush.h"

#if defined(__HIPCC__)
#define VR_ERODE_FN __host__ __device__ __forceinline__
#else
#define VR_ERODE_FN inline
#endif

constexpr int kErodeMaxIterations = 1024;        // VR_ERODE_MAX_ITERATIONS (include/vrterrain.h)

// the diagonal neighbours' talus, formed once per call
inline float erode_diagonal_talus(float talus)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return talus * 1.41421354f;
}

// one more covering dab of weight f in a texel's mask (the mask starts at 0.0f)
VR_ERODE_FN float erode_mask_max(float m, float f, float strength)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float a = f * strength;
    return a > m ? a : m;
}

// one neighbour's share of acc; T: the talus of this direction
VR_ERODE_FN float erode_edge(float acc, float hc, float hn, float mc, float mn, float T, float rate)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float w = mc < mn ? mc : mn;
    if (!(w > 0.0f)) return acc;
    if (hc >= hn) {
        const float d = hc - hn;
        const float e = d - T;
        if (e > 0.0f) { const float re = rate * e; const float p = re * w; acc = acc - p; }
    } else {
        const float d = hn - hc;
        const float e = d - T;
        if (e > 0.0f) { const float re = rate * e; const float p = re * w; acc = acc + p; }
    }
    return acc;
}

// the byte a masked texel ends as
VR_ERODE_FN uint8_t erode_byte(float h)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float c = h < 0.0f ? 0.0f : (h > 255.0f ? 255.0f : h);
    return (uint8_t)floorf(c + 0.5f);
}

// The mask of every texel of rect = {x0, y0, x1, y1} under the prepared dabs (none empty), into a plane of the rectangle's size: the
// serial evaluators' first step, vr_hydro.h's as well.
inline void erode_serial_mask(const BrushDab* dabs, size_t n, const int rect[4], float* mask)
{
    const int rw = rect[2] - rect[0];
    for (int y = rect[1]; y < rect[3]; y++)
        for (int x = rect[0]; x < rect[2]; x++) {
            float m = 0.0f;
            for (size_t d = 0; d < n; d++) {
                float f;
                if (x < dabs[d].x0 || x >= dabs[d].x1 || y < dabs[d].y0 || y >= dabs[d].y1 || !brush_weight(dabs[d], x, y, &f)) continue;
                m = erode_mask_max(m, f, dabs[d].strength);
            }
            mask[(size_t)(y - rect[1]) * rw + (x - rect[0])] = m;
        }
}

// The whole operation over a host array.  map: w0 x h0 bytes, changed in place; dabs: the prepared dabs that met the map (none
// empty); rect = {x0, y0, x1, y1}: the hull of their spans; mask, a, b: room for (x1 - x0) * (y1 - y0) floats each.
inline void erode_serial(uint8_t* map, int w0, int h0, const BrushDab* dabs, size_t n, const int rect[4], int iterations, float talus,
                         float rate, float* mask, float* a, float* b)
{
    const int x0 = rect[0], y0 = rect[1], rw = rect[2] - rect[0], rh = rect[3] - rect[1];
    if (rw <= 0 || rh <= 0) return;
    erode_serial_mask(dabs, n, rect, mask);
    for (int j = 0; j < rh; j++)
        for (int i = 0; i < rw; i++) a[(size_t)j * rw + i] = (float)map[(size_t)(y0 + j) * w0 + (x0 + i)];
    static const int ndx[8] = { -1, 0, 1, -1, 1, -1, 0, 1 }, ndy[8] = { -1, -1, -1, 0, 0, 1, 1, 1 };
    const float T[2] = { talus, erode_diagonal_talus(talus) };
    float* cur = a; float* nxt = b;
    for (int it = 0; it < iterations; it++) {
        for (int j = 0; j < rh; j++)
            for (int i = 0; i < rw; i++) {
                const float hc = cur[(size_t)j * rw + i], mc = mask[(size_t)j * rw + i];
                float acc = 0.0f;
                for (int k = 0; k < 8; k++) {
                    const int x = x0 + i + ndx[k], y = y0 + j + ndy[k];
                    if (x < 0 || x >= w0 || y < 0 || y >= h0) continue;                           // outside the map: no edge
                    const bool in_rect = i + ndx[k] >= 0 && i + ndx[k] < rw && j + ndy[k] >= 0 && j + ndy[k] < rh;
                    if (!in_rect) continue;                                                       // mask 0: w > 0 fails
                    const size_t at = (size_t)(j + ndy[k]) * rw + (size_t)(i + ndx[k]);
                    acc = erode_edge(acc, hc, cur[at], mc, mask[at], T[(ndx[k] != 0 && ndy[k] != 0) ? 1 : 0], rate);
                }
                nxt[(size_t)j * rw + i] = hc + acc;
            }
        float* t = cur; cur = nxt; nxt = t;
    }
    for (int j = 0; j < rh; j++)
        for (int i = 0; i < rw; i++)
            if (mask[(size_t)j * rw + i] > 0.0f) map[(size_t)(y0 + j) * w0 + (x0 + i)] = erode_byte(cur[(size_t)j * rw + i]);
}
