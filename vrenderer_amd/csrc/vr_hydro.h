// Hydraulic erosion of level 0 of the heightmap under a brush mask (vr_terrain_erode_hydraulic; its kernels: vr_erode.hip): the definition, for
// the device and for the host.  Plain C++17, no HIP types: the host compiles this header alone (tests/host/hydro_check.cpp).
//
// As in vr_erode.h everything a texel sees is fp32, evaluated in the written order with no contraction, and uses +, -, *,
// comparisons (min and max are comparisons), floorf and int -> float conversions only - no division, no square root - so a numpy
// float32 model (tests/hydro_model.py) reproduces the device bit for bit.  DESIGN.md 4v.
//
//   mask        vr_erode.h's: m_c = max over the kept dabs that cover c of f * strength, 0 where none does; the rectangle is the
//               hull of the kept spans; every texel outside it has mask 0.
//   state       h_c the terrain in heightmap steps, starts as the stored byte; d_c the water depth, starts as rain * m_c; s_c the
//               suspended sediment, starts at 0.  All fp32.
//   per call    keep = 1.0f - evaporation (hydro_keep), on the host.
//   sweep       every cell from the previous sweep's h, d, s of itself and its four axis neighbours: dd = ds = out = 0.0f, then
//               for the neighbours n inside the MAP in the order (dx, dy) = (0,-1) (-1,0) (1,0) (0,1) (hydro_edge):
//                 w = min(m_c, m_n); the edge is skipped unless w > 0
//                 S_c = h_c + d_c, S_n = h_n + d_n
//                 S_c >= S_n (c gives):  phi = min(flow * (S_c - S_n), 0.25f) * w;  q = phi * d_c;  ts = phi * s_c
//                                        dd = dd - q;  ds = ds - ts;  out = out + q
//                 otherwise (n gives):   phi = min(flow * (S_n - S_c), 0.25f) * w;  q = phi * d_n;  ts = phi * s_n
//                                        dd = dd + q;  ds = ds + ts
//               so both ends of an edge compute the same q and ts, bit for bit.  phi is the share of the giver's water that crosses
//               the edge; four edges take at most all of it, which is why nothing is divided.  Then (hydro_cell):
//                 d1 = max(d_c + dd, 0.0f);  s1 = max(s_c + ds, 0.0f);  C = capacity * out
//                 s1 < C:     e = (dissolve * (C - s1)) * m_c;  h' = h_c - e;  s' = s1 + e
//                 otherwise:  g = deposit * (s1 - C);           h' = h_c + g;  s' = s1 - g
//                 d' = d1 * keep + rain * m_c  (three roundings: the two products, then the sum)
//   end         after `iterations` sweeps a texel with m_c > 0 is stored as erode_byte(h + s): what is still suspended settles
//               where it is.  One with m_c == 0 is not written.
//
// A texel outside the rectangle has mask 0, d = 0 and s = 0, and no edge reaches it: the whole computation lives inside the
// rectangle, and a cell is a pure function of the previous sweep - the bytes depend neither on how the device cuts the rectangle
// into tiles nor on how many sweeps one launch advances.  hydro_serial is the definition in executable form (two sets of planes,
// swapped per sweep); the host check drives it, the library does not.
//
// Ranges (anything else is refused): iterations 1 .. 1024, rain [0, 16], flow (0, 1], capacity [0, 64], dissolve, deposit and
// evaporation [0, 1], all finite.  Within them no infinity and no NaN arises in 1024 sweeps.  Water: an edge moves q out of one
// cell and the same q into the other, and q <= 0.25 * d of the giver on each of at most four edges, so d + dd >= 0 up to rounding
// (the max restores it) and a sweep changes the rectangle's total water only by evaporation (keep <= 1) and by rain, at most 16 per
// cell: after k sweeps the total, and with it every d, is at most (k + 1) * 16 * cells, times (1 + 2^-23)^(8k) < 1.002 for the
// roundings - below 1.2e12 for 1024 sweeps of the largest map (2^26 texels).  Sediment: a cell dissolves at most capacity * out
// <= 64 * d per sweep and otherwise only passes s along or drops it, so the total s, and every |h - byte|, stays below
// 1024 * 2^26 * 64 * 1.2e12 < 6e24.  Every S, difference and product formed from these is below 1e27, far inside fp32: growth is
// linear in the water present, never geometric.
#pragma once
#include "vr_erode.h"

#if defined(__HIPCC__)
#define VR_HYDRO_FN __host__ __device__ __forceinline__
#else
#define VR_HYDRO_FN inline
#endif

constexpr int kHydroMaxIterations = 1024;        // VR_HYDRO_MAX_ITERATIONS (include/vrterrain.h)

// the call's constants, as the kernels and the serial evaluator take them
struct HydroConst { float rain, flow, capacity, dissolve, deposit, keep; };
// what a cell gathers over its edges
struct HydroAcc { float dd, ds, out; };

// the share of the water that stays after a sweep's evaporation, formed once per call
inline float hydro_keep(float evaporation)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return 1.0f - evaporation;
}

// the water a texel of mask m starts with, and receives per sweep
VR_HYDRO_FN float hydro_rain(float rain, float m)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return rain * m;
}

// what crossed one edge (for the host check): the water, the sediment, and whether c was the giver
struct HydroFlux { float q, ts; bool gives; };

// One neighbour's share of the cell's sums; *x (may be NULL) receives what crossed the edge.
VR_HYDRO_FN void hydro_edge(HydroAcc& a, float hc, float dc, float sc, float mc, float hn, float dn, float sn, float mn, float flow, HydroFlux* x = nullptr)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float w = mc < mn ? mc : mn;
    if (x) *x = HydroFlux{ 0.0f, 0.0f, false };
    if (!(w > 0.0f)) return;
    const float Sc = hc + dc, Sn = hn + dn;
    if (Sc >= Sn) {
        const float diff = Sc - Sn;
        const float f = flow * diff;
        const float fm = f < 0.25f ? f : 0.25f;
        const float phi = fm * w;
        const float q = phi * dc;
        const float ts = phi * sc;
        a.dd = a.dd - q; a.ds = a.ds - ts; a.out = a.out + q;
        if (x) *x = HydroFlux{ q, ts, true };
    } else {
        const float diff = Sn - Sc;
        const float f = flow * diff;
        const float fm = f < 0.25f ? f : 0.25f;
        const float phi = fm * w;
        const float q = phi * dn;
        const float ts = phi * sn;
        a.dd = a.dd + q; a.ds = a.ds + ts;
        if (x) *x = HydroFlux{ q, ts, false };
    }
}

// the cell after the sweep, from its state before and its sums
VR_HYDRO_FN void hydro_cell(float hc, float dc, float sc, float mc, const HydroAcc& a, const HydroConst& k, float* h1, float* d1, float* s1)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float dsum = dc + a.dd, ssum = sc + a.ds;
    const float dn = dsum > 0.0f ? dsum : 0.0f;
    const float sn = ssum > 0.0f ? ssum : 0.0f;
    const float C = k.capacity * a.out;
    if (sn < C) {
        const float room = C - sn;
        const float er = k.dissolve * room;
        const float e = er * mc;
        *h1 = hc - e; *s1 = sn + e;
    } else {
        const float over = sn - C;
        const float g = k.deposit * over;
        *h1 = hc + g; *s1 = sn - g;
    }
    const float kept = dn * k.keep;
    const float rained = hydro_rain(k.rain, mc);
    *d1 = kept + rained;
}

// the byte a masked texel ends as: the terrain and what is still suspended above it
VR_HYDRO_FN uint8_t hydro_byte(float h, float s)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float settled = h + s;
    return erode_byte(settled);
}

// The whole operation over a host array.  map: w0 x h0 bytes, changed in place; dabs: the prepared dabs that met the map (none
// empty); rect = {x0, y0, x1, y1}: the hull of their spans; mask: room for (x1 - x0) * (y1 - y0) floats, a and b for three times
// that (h, d, s planes one after the other).  Returns false if a d or an s was ever negative (it never is).
inline bool hydro_serial(uint8_t* map, int w0, int h0, const BrushDab* dabs, size_t n, const int rect[4], int iterations, const HydroConst& k,
                         float* mask, float* a, float* b)
{
    const int x0 = rect[0], y0 = rect[1], rw = rect[2] - rect[0], rh = rect[3] - rect[1];
    if (rw <= 0 || rh <= 0) return true;
    const size_t cells = (size_t)rw * (size_t)rh;
    erode_serial_mask(dabs, n, rect, mask);
    for (int j = 0; j < rh; j++)
        for (int i = 0; i < rw; i++) {
            const size_t at = (size_t)j * rw + i;
            a[at] = (float)map[(size_t)(y0 + j) * w0 + (x0 + i)];
            a[cells + at] = hydro_rain(k.rain, mask[at]);
            a[2 * cells + at] = 0.0f;
        }
    static const int ndx[4] = { 0, -1, 1, 0 }, ndy[4] = { -1, 0, 0, 1 };
    bool non_negative = true;
    float* cur = a; float* nxt = b;
    for (int it = 0; it < iterations; it++) {
        for (int j = 0; j < rh; j++)
            for (int i = 0; i < rw; i++) {
                const size_t c = (size_t)j * rw + i;
                HydroAcc acc = { 0.0f, 0.0f, 0.0f };
                for (int e = 0; e < 4; e++) {
                    const int x = x0 + i + ndx[e], y = y0 + j + ndy[e];
                    if (x < 0 || x >= w0 || y < 0 || y >= h0) continue;                           // outside the map: no edge
                    const bool in_rect = i + ndx[e] >= 0 && i + ndx[e] < rw && j + ndy[e] >= 0 && j + ndy[e] < rh;
                    if (!in_rect) continue;                                                       // mask 0: w > 0 fails
                    const size_t at = (size_t)(j + ndy[e]) * rw + (size_t)(i + ndx[e]);
                    hydro_edge(acc, cur[c], cur[cells + c], cur[2 * cells + c], mask[c], cur[at], cur[cells + at], cur[2 * cells + at], mask[at], k.flow);
                }
                hydro_cell(cur[c], cur[cells + c], cur[2 * cells + c], mask[c], acc, k, &nxt[c], &nxt[cells + c], &nxt[2 * cells + c]);
                if (!(nxt[cells + c] >= 0.0f) || !(nxt[2 * cells + c] >= 0.0f)) non_negative = false;
            }
        float* t = cur; cur = nxt; nxt = t;
    }
    for (int j = 0; j < rh; j++)
        for (int i = 0; i < rw; i++) {
            const size_t c = (size_t)j * rw + i;
            if (mask[c] > 0.0f) map[(size_t)(y0 + j) * w0 + (x0 + i)] = hydro_byte(cur[c], cur[2 * cells + c]);
        }
    return non_negative;
}
