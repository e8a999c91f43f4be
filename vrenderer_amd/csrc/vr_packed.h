// The packed albedo footprint table of the fused tile pass (DevTex-style table `pack` of an SRGBA8 map; vr_derive.hip builds it,
// k_raster's LIT flavours read it).  Plain C++17 with the HIP qualifiers only where hipcc compiles it: a CPU program packs a random
// map and holds the decode to the float table (tests/host/packed_check.cpp).
//
// Same indexing as DevTex::fast: per level (w + 3) x (h + 3) entries of 16 bytes, clamp-addressed, entry (ix, iy) at
// fast_lv[l].x + (iy - 1) * row + (ix - 1) * 16 - one set of byte offsets still serves the height taps and the albedo.  Where the
// float table holds ONE decoded texel, (ix-1, iy-1), an entry here holds the sRGB8 CODES of the whole bilinear footprint whose floor
// that texel is:
//
//     dword 0: t00 = texel (ix-1, iy-1)    dword 1: t10 = (ix, iy-1)    dword 2: t01 = (ix-1, iy)    dword 3: t11 = (ix, iy)
//     a dword: r << 2 | g << 12 | b << 22  - three 10-bit fields, each the code times four
//
// so a pixel fetches its albedo footprint with one 16-byte load instead of four, and a field, extracted with one v_bfe_u32, IS the
// byte offset of the code's float in the 256-entry sRGB8 -> linear table the fused flavours hold in LDS.  That table is the context's
// own (vr_context::d_srgb_lut), the one vr_fast_srgba8_entry decodes with: the twelve floats are bit for bit the float table's.
// Alpha is not kept (the float table stores 0 there and the filter never reads it).
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define VR_PACKED_FN __host__ __device__ __forceinline__
#else
#define VR_PACKED_FN inline
#endif

// one SRGBA8 texel (r in the low byte) as a dword of an entry
VR_PACKED_FN uint32_t vr_pack_texel(uint32_t p) { return ((p & 255u) << 2) | (((p >> 8) & 255u) << 12) | (((p >> 16) & 255u) << 22); }
// channel c (0 r, 1 g, 2 b) of such a dword: the byte offset of its float in a 256-float table (the low two bits are zero)
VR_PACKED_FN uint32_t vr_packed_lut_offset(uint32_t word, int c) { return (word >> (10 * c)) & 0x3ffu; }

// entry (ix, iy) of the (w + 3) x (h + 3) table of a w x h level at `src`; out: the entry's four dwords
VR_PACKED_FN void vr_packed_entry(const uint32_t* src, int w, int h, int ix, int iy, uint32_t out[4])
{
    const int xa = ix - 1 < 0 ? 0 : (ix - 1 > w - 1 ? w - 1 : ix - 1), xb = ix < 0 ? 0 : (ix > w - 1 ? w - 1 : ix);
    const int ya = iy - 1 < 0 ? 0 : (iy - 1 > h - 1 ? h - 1 : iy - 1), yb = iy < 0 ? 0 : (iy > h - 1 ? h - 1 : iy);
    out[0] = vr_pack_texel(src[(size_t)ya * w + xa]); out[1] = vr_pack_texel(src[(size_t)ya * w + xb]);
    out[2] = vr_pack_texel(src[(size_t)yb * w + xa]); out[3] = vr_pack_texel(src[(size_t)yb * w + xb]);
}
