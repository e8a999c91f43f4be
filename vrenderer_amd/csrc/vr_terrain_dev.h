// Everything the library derives from a terrain's two maps, one element at a time: a texel of the next mip level, an entry
// of each decoded table, a node's (min, max), a cell of the query pyramid.  The kernels of vr_derive.hip call these for the
// elements of a rectangle - the whole map when a terrain is created, the dirty rectangle of an in-place edit - and no other
// kernel does.  There is no second copy of any of these expressions, nor of the kernels around them.
#pragma once
#include "vr_internal.h"
#include "vr_tex_dev.h"

// ---- mip chain -------------------------------------------------------------------------------------
// 2x2 box downsample of an R8_UNORM level: round(avg * 255) == (sum + 2) >> 2.
__device__ __forceinline__ void vr_mip_r8_texel(const uint8_t* __restrict__ src, int sw, int sh, uint8_t* __restrict__ dst, int dw, int x, int y)
{
    int x0 = 2 * x, x1 = min(2 * x + 1, sw - 1), y0 = 2 * y, y1 = min(2 * y + 1, sh - 1);
    int sum = src[y0 * sw + x0] + src[y0 * sw + x1] + src[y1 * sw + x0] + src[y1 * sw + x1];
    dst[y * dw + x] = (uint8_t)((sum + 2) >> 2);
}
// SRGBA8 level: decode to linear, average, re-encode (what a blit into an SRGBA8 render target does); alpha is linear.
// lut / thr: the context's tables (256 entries each; the kernels keep them in LDS).
__device__ __forceinline__ void vr_mip_srgba8_texel(const uint32_t* __restrict__ src, int sw, int sh, uint32_t* __restrict__ dst, int dw, int x, int y,
                                                    const float* lut, const float* thr)
{
    int x0 = 2 * x, x1 = min(2 * x + 1, sw - 1), y0 = 2 * y, y1 = min(2 * y + 1, sh - 1);
    uint32_t p00 = src[(size_t)y0 * sw + x0], p10 = src[(size_t)y0 * sw + x1];
    uint32_t p01 = src[(size_t)y1 * sw + x0], p11 = src[(size_t)y1 * sw + x1];
    uint32_t o = 0;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        int sh8 = 8 * c;
        float a = (lut[(p00 >> sh8) & 255u] + lut[(p10 >> sh8) & 255u]) + (lut[(p01 >> sh8) & 255u] + lut[(p11 >> sh8) & 255u]);
        o |= vr_srgb_encode(a * 0.25f, thr) << sh8;
    }
    uint32_t al = ((p00 >> 24) + (p10 >> 24) + (p01 >> 24) + (p11 >> 24) + 2u) >> 2;
    dst[(size_t)y * dw + x] = o | (al << 24);
}

// ---- decoded tables (DevTex) -------------------------------------------------------------------------
// quad: entry (ix, iy) of the (w+2) x (h+2) table packs the clamp-addressed texels (ix-1, iy-1) (ix, iy-1) (ix-1, iy) (ix, iy)
__device__ __forceinline__ void vr_quad_entry(const uint8_t* __restrict__ src, int w, int h, uint32_t* __restrict__ dst, int ix, int iy)
{
    const int x0 = min(max(ix - 1, 0), w - 1), x1 = min(max(ix, 0), w - 1);
    const int y0 = min(max(iy - 1, 0), h - 1), y1 = min(max(iy, 0), h - 1);
    dst[(size_t)iy * (w + 2) + ix] = (uint32_t)src[y0 * w + x0] | ((uint32_t)src[y0 * w + x1] << 8)
                                   | ((uint32_t)src[y1 * w + x0] << 16) | ((uint32_t)src[y1 * w + x1] << 24);
}
// the same footprint decoded, in a table `tw` entries wide: quadf (tw = w + 2) and the R8 flavour of fast (tw = w + 3)
__device__ __forceinline__ void vr_footprint_entry(const uint8_t* __restrict__ src, int w, int h, float4* __restrict__ dst, int tw, int ix, int iy)
{
    const int x0 = min(max(ix - 1, 0), w - 1), x1 = min(max(ix, 0), w - 1);
    const int y0 = min(max(iy - 1, 0), h - 1), y1 = min(max(iy, 0), h - 1);
    // UNORM8 -> float, correctly rounded, and the differences the bilinear filter forms first
    const float t00 = (float)src[y0 * w + x0] / 255.0f, t10 = (float)src[y0 * w + x1] / 255.0f;
    const float t01 = (float)src[y1 * w + x0] / 255.0f, t11 = (float)src[y1 * w + x1] / 255.0f;
    dst[(size_t)iy * tw + ix] = make_float4(t00, t10 - t00, t01, t11 - t01);
}
// fast, SRGBA8 flavour: entry (ix, iy) of the (w+3) x (h+3) table is the decoded clamp-addressed texel (ix-1, iy-1)
__device__ __forceinline__ void vr_fast_srgba8_entry(const uint32_t* __restrict__ src, int w, int h, const float* __restrict__ lut,
                                                     float4* __restrict__ dst, int ix, int iy)
{
    const uint32_t p = src[(size_t)min(max(iy - 1, 0), h - 1) * w + min(max(ix - 1, 0), w - 1)];
    dst[(size_t)iy * (w + 3) + ix] = make_float4(lut[p & 255u], lut[(p >> 8) & 255u], lut[(p >> 16) & 255u], 0.0f);
}
// rgbf: dword i of the chain decoded
__device__ __forceinline__ void vr_rgbf_texel(const uint32_t* __restrict__ src, size_t i, const float* __restrict__ lut, float* __restrict__ dst)
{
    const uint32_t p = src[i];
    reinterpret_cast<float4*>(dst)[i] = make_float4(lut[p & 255u], lut[(p >> 8) & 255u], lut[(p >> 16) & 255u], 0.0f);
}

// ---- node heights, mip-style path -----------------------------------------------------------------------
__device__ __forceinline__ float2 vr_finish_minmax(int mnb, int mxb)
{
    float mn = mnb <= 255 ? (float)mnb / 255.0f : INFINITY, mx = mxb >= 0 ? (float)mxb / 255.0f : -INFINITY;
    mn = (mx - mn) == 0.0f ? 0.0f : mn;
    const float extent = (mx - mn) / 2.0f;
    return make_float2(mn + extent, extent);          // m_Position.y, m_Extents.y (QuadTree.cpp:197-198)
}
// leaf node (ix, iz) of an n x n level: the s x s texels at (rx0 + ix s, ry0 + iz s); mm / out are the level's own arrays
__device__ __forceinline__ void vr_minmax_leaf_node(const uint8_t* __restrict__ tex, int tex_w, int rx0, int ry0, uint32_t n, int s,
                                                    uchar2* __restrict__ mm, float2* __restrict__ out, uint32_t ix, uint32_t iz)
{
    const uint64_t node = (uint64_t)iz * n + ix;
    const uint8_t* p = tex + (size_t)(ry0 + (int)iz * s) * tex_w + (rx0 + (int)ix * s);
    int mn = 256, mx = -1;
    for (int j = 0; j < s; j++) for (int i = 0; i < s; i++) { const int b = p[(size_t)j * tex_w + i]; mn = min(mn, b); mx = max(mx, b); }
    mm[node] = make_uchar2((unsigned char)mn, (unsigned char)mx);
    out[node] = vr_finish_minmax(mn, mx);
}
// node (ix, iz) of an n x n level from its four children in the 2n x 2n level below
__device__ __forceinline__ void vr_minmax_up_node(const uchar2* __restrict__ child, uint32_t n, uchar2* __restrict__ mm, float2* __restrict__ out,
                                                  uint32_t ix, uint32_t iz)
{
    const uint64_t node = (uint64_t)iz * n + ix;
    const uchar2* c = child + (size_t)(2u * iz) * (2u * n) + 2u * ix;
    const uchar2 a0 = c[0], a1 = c[1], a2 = c[2u * n], a3 = c[2u * n + 1];
    const int mn = min(min((int)a0.x, (int)a1.x), min((int)a2.x, (int)a3.x)), mx = max(max((int)a0.y, (int)a1.y), max((int)a2.y, (int)a3.y));
    mm[node] = make_uchar2((unsigned char)mn, (unsigned char)mx);
    out[node] = vr_finish_minmax(mn, mx);
}

// ---- query pyramid ---------------------------------------------------------------------------------------
// Level 0.  Cell (ix, iz) is the quad table's entry (ix, iz): texel-centre coordinates X0 in [ix - 1, ix].  Its level-0 part is
// bounded by the entry's four texels (a bilinear interpolant lies between its corners); its level-1 part by every level-1 texel
// a bilinear tap at a point of the cell can touch: X1 = (X0 + 0.5) w1 / w0 - 0.5 over the cell, floor(X1) .. floor(X1) + 1,
// widened by 1/64 texel for the sampler's fp32 rounding of uv.  The two combine at 0.9 : 0.1 in integers (units of 1/2550) and
// round outwards to the 1/255 grid.
__device__ __forceinline__ void vr_pyramid_leaf_cell(const DevTex& hm, int cw, uchar2* __restrict__ out, int ix, int iz)
{
    const int w0 = hm.w0, h0 = hm.h0;
    const int l1 = min(1, hm.levels - 1);
    const int w1 = max(1, w0 >> l1), h1 = max(1, h0 >> l1);
    const uint32_t e = hm.quad[hm.qoff[0] + (uint32_t)iz * (uint32_t)(w0 + 2) + (uint32_t)ix];
    const uint32_t b0 = e & 255u, b1 = (e >> 8) & 255u, b2 = (e >> 16) & 255u, b3 = e >> 24;
    const uint32_t mn0 = min(min(b0, b1), min(b2, b3)), mx0 = max(max(b0, b1), max(b2, b3));
    const float m = 1.0f / 64.0f;
    const float rx = (float)w1 / (float)w0, rz = (float)h1 / (float)h0;
    int jx0 = (int)floorf(((float)ix - 0.5f) * rx - 0.5f - m), jx1 = (int)floorf(((float)ix + 0.5f) * rx - 0.5f + m) + 1;
    int jz0 = (int)floorf(((float)iz - 0.5f) * rz - 0.5f - m), jz1 = (int)floorf(((float)iz + 0.5f) * rz - 0.5f + m) + 1;
    jx0 = vr_clampi(jx0, 0, w1 - 1); jx1 = vr_clampi(jx1, 0, w1 - 1);
    jz0 = vr_clampi(jz0, 0, h1 - 1); jz1 = vr_clampi(jz1, 0, h1 - 1);
    const uint8_t* __restrict__ lv1 = hm.base + hm.off[l1];
    uint32_t mn1 = 255u, mx1 = 0u;
    for (int z = jz0; z <= jz1; z++)
        for (int x = jx0; x <= jx1; x++) {
            const uint32_t v = lv1[(size_t)z * w1 + x];
            mn1 = min(mn1, v); mx1 = max(mx1, v);
        }
    const uint32_t lo = (9u * mn0 + mn1) / 10u, hi = (9u * mx0 + mx1 + 9u) / 10u;
    out[(size_t)iz * cw + ix] = make_uchar2((unsigned char)lo, (unsigned char)min(hi, 255u));
}
// cell (px, pz) of a pw-wide level from its 2 x 2 children in the cw x ch level below, ragged edges included
__device__ __forceinline__ void vr_pyramid_up_cell(const uchar2* __restrict__ child, int cw, int ch, uchar2* __restrict__ parent, int pw, int px, int pz)
{
    const int x0 = 2 * px, x1 = min(2 * px + 1, cw - 1), z0 = 2 * pz, z1 = min(2 * pz + 1, ch - 1);
    const uchar2 a = child[(size_t)z0 * cw + x0], b = child[(size_t)z0 * cw + x1], c = child[(size_t)z1 * cw + x0], d = child[(size_t)z1 * cw + x1];
    parent[(size_t)pz * pw + px] = make_uchar2(min(min(a.x, b.x), min(c.x, d.x)), max(max(a.y, b.y), max(c.y, d.y)));
}
