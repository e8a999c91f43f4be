// vr_terrain_region: the inside of a polygon, with a feathered outline - one parity bit and one distance per texel, over the region's
// edges - written into level 0 of a map by one kernel, through vr_list_call (vr_level0.h).  The definition, texel by texel, is
// vr_region.h; this file holds nothing of it but the order in which the header's functions are called.
//
//   k_region<OP>   the tile frame and the chunk walk of vr_brush_dev.h over RegionEdge: lane d tests edge base + d's span - its
//                distance box stretched to the right edge of the map - against the tile, the survivors are listed in list order, and
//                every lane runs them in that order: path_offset once, region_left into the parity bit, and - where the call has a
//                feather, a wave-uniform flag - path_nearest into q*, a min-reduction with a strict <.  The edge read in the inner loop
//                is wave-uniform (brush_chunk_entry's readfirstlane): scalar loads.  Behind the last barrier region_weight, one load
//                and one store.  A texel with no coverage is not written.
//                Most edges reach a tile right of them through the stretch alone, with their distance box far away: for those
//                path_nearest is skipped by a wave-uniform test of the box's own x1 (RegionEdge::dist_x1) against the tile - by the
//                path's span proof no texel of such a tile has q < 1.  Measured against the plain loop and kept: 35 to 40 us
//                ahead on a 4096-edge coastline, level elsewhere (profiles/terrain_region_variants.txt).
//
// The kernel is untimed, like the brush kernel.
#include "vr_level0.h"
#include "vr_region.h"

// `map`: level 0 (R8: bytes, SRGBA8: dwords), w0 x h0; `r`: the call's rectangle, inside the map; `edges`: n of them, none empty
template <int OP>
__global__ __launch_bounds__(kBrushThreads) void k_region(void* __restrict__ map, int w0, int h0, DirtyRect r, const RegionEdge* __restrict__ edges, uint32_t n, RegionConst k)
{
    constexpr int NC = OP == kRegionPaint ? 4 : 1;
    __shared__ uint16_t list[kBrushChunk];  // the chunk's edges that meet this tile, in list order
    __shared__ uint32_t wave_total[4];
    const BrushTile tile = brush_tile(r);
    const int cx = tile.cx(w0), cy = tile.cy(h0);
    const float fj = (float)cy;
    const bool soft = (k.flags & kRegionSoft) != 0;                // a kernel argument: uniform
    float best_q = 1.0f;
    uint32_t par = 0;
    for (uint32_t base = 0; base < n; base += kBrushChunk) {       // (n is a kernel argument: the trip count is uniform)
        const uint32_t total = brush_chunk_list(edges, n, base, tile, list, wave_total);
        for (uint32_t i = 0; i < total; i++) {
            const RegionEdge e = edges[brush_chunk_entry(list, i, n)];
            float px, pz;
            path_offset(e.ax, e.az, k.wx, k.wz, cx, cy, &px, &pz);
            par ^= region_left(e, px, pz, fj);
            if (soft && e.dist_x1 > tile.tx0) {                    // uniform: the distance box meets the tile
                float q, t;
                path_nearest(px, pz, e.dx, e.dz, e.inv_len2, k.inv_r2, &q, &t);
                if (q < best_q) best_q = q;
            }
        }
        __syncthreads();                                           // the next chunk overwrites list and wave_total
    }
    float f;
    if (!(tile.inside && region_weight(k.flags, par != 0, best_q, &f))) return;       // behind the last barrier
    const size_t at = (size_t)cy * (size_t)w0 + (size_t)cx;
    if (OP == kRegionPaint) {
        const uint32_t stored = ((const uint32_t*)map)[at];
        uint32_t out = 0;
#pragma unroll
        for (int c = 0; c < NC; c++) {
            float val = (float)((stored >> (8 * c)) & 255u);
            if (k.channel_mask & (1u << c)) val = brush_blend(val, f, k.opacity, k.color[c]);
            out |= (uint32_t)brush_byte(val) << (8 * c);
        }
        ((uint32_t*)map)[at] = out;
    } else {
        const float val = (float)((const uint8_t*)map)[at];
        ((uint8_t*)map)[at] = brush_byte(region_apply(OP, k.opacity, val, f, k.target));
    }
}

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
extern "C" VR_API int vr_terrain_region(vr_terrain* t, int which, const vr_region_params* p, const vr_region_point* points, uint32_t n, const uint32_t* contour_counts,
                                        uint32_t num_contours, int32_t out_rect[4])
{
    static_assert(sizeof(vr_region_point) == 8 && sizeof(vr_region_params) == 64, "vr_region_point / vr_region_params layout");
    static_assert(sizeof(vr_region_point) == sizeof(RegionPoint), "RegionPoint is vr_region_point");
    static_assert(VR_REGION_LEVEL == kRegionLevel && VR_REGION_CUT == kRegionCut && VR_REGION_FILL == kRegionFill && VR_REGION_RAISE == kRegionRaise &&
                  VR_REGION_PAINT == kRegionPaint && VR_REGION_FEATHER_INSIDE == kRegionFeatherInside, "vr_region.h's ops and flags");
    static_assert(VR_MAX_REGION_POINTS == kRegionMaxPoints && VR_MAX_BRUSH_DABS == kPathMaxListed, "vr_region.h's limits");
    // the argument checks come before any use of the device (and leave the terrain alone)
    VR_REQUIRE(t != nullptr, "terrain is NULL");
    VR_REQUIRE(p != nullptr, "params is NULL");
    VR_REQUIRE(points != nullptr || n == 0, "points is NULL with n > 0");
    VR_REQUIRE(n <= VR_MAX_REGION_POINTS, "more than VR_MAX_REGION_POINTS points");
    VR_REQUIRE(which == 0 || which == 1, "which must be 0 (heightmap) or 1 (albedo)");
    const int op = p->op;
    VR_REQUIRE(op == VR_REGION_LEVEL || op == VR_REGION_CUT || op == VR_REGION_FILL || op == VR_REGION_RAISE || op == VR_REGION_PAINT, "unknown op");
    VR_REQUIRE((op == VR_REGION_PAINT) == (which == 1), "LEVEL, CUT, FILL and RAISE work on the heightmap, PAINT on the albedo");
    VR_REQUIRE((p->flags & ~(uint32_t)VR_REGION_FEATHER_INSIDE) == 0, "unknown flag bits");
    VR_REQUIRE(region_contours_ok(n, contour_counts, num_contours), "every contour needs at least 3 points, and contour_counts must sum to n");
    VR_REQUIRE(host_finite(p->target) && host_finite(p->feather) && host_finite(p->opacity), "params holds a NaN or an infinity");
    for (int c = 0; c < 4; c++) VR_REQUIRE(host_finite(p->color[c]), "color is NaN or infinite");
    VR_REQUIRE(p->feather >= 0.0f, "feather must not be negative");
    VR_REQUIRE(p->opacity >= 0.0f && p->opacity <= 1.0f, "opacity outside [0, 1]");
    if (op == VR_REGION_RAISE) VR_REQUIRE(p->target >= -255.0f && p->target <= 255.0f, "RAISE's target outside [-255, 255]");
    else VR_REQUIRE(p->target >= 0.0f && p->target <= 255.0f, "target outside [0, 255]");
    for (int c = 0; c < 4; c++) VR_REQUIRE(p->color[c] >= 0.0f && p->color[c] <= 255.0f, "color outside [0, 255]");
    VR_REQUIRE(p->channel_mask >= 1u && p->channel_mask <= 15u, "channel_mask must be 1 .. 15");
    VR_REQUIRE(which == 1 || p->channel_mask == 1u, "the heightmap has channel_mask 1");
    for (int i = 0; i < 6; i++) VR_REQUIRE(p->reserved[i] == 0, "reserved must be zero");
    for (uint32_t i = 0; i < n; i++) VR_REQUIRE(host_finite(points[i].x) && host_finite(points[i].z), "a point holds a NaN or an infinity");
    // the handle is looked into from here on
    const DevTex& tex = vr_terrain_map(t, which);
    const RegionConst k = region_const(p->feather, p->opacity, p->target, op, p->flags, p->color, p->channel_mask, t->p.world_size, tex.w0, tex.h0);
    int32_t hull[4];
    region_prepare((const RegionPoint*)points, n, contour_counts, num_contours, k, t->p.world_size, tex.w0, tex.h0, t->region_verts, t->region_prepared, hull);
    DirtyRect dirty;
    if (!t->region_prepared.empty()) { dirty.x0 = hull[0]; dirty.y0 = hull[1]; dirty.x1 = hull[2]; dirty.y1 = hull[3]; }
    return vr_list_call(t, which, dirty, t->region_prepared.data(), (uint32_t)t->region_prepared.size(), out_rect,
        [&](const DirtyRect&) -> int { return vr_brush_reserve(t, 0); },                            // nothing beyond the list
        [&](hipStream_t s, const DirtyRect& r, uint32_t ne) -> int {
            void* mem = const_cast<uint8_t*>(tex.base);
            const RegionEdge* edges = (const RegionEdge*)t->d_brush_dabs;
            const dim3 grid = tiles_32x8(r), block(kBrushThreads);
            switch (op) {
            case VR_REGION_LEVEL: hipLaunchKernelGGL(k_region<kRegionLevel>, grid, block, 0, s, mem, tex.w0, tex.h0, r, edges, ne, k); break;
            case VR_REGION_CUT: hipLaunchKernelGGL(k_region<kRegionCut>, grid, block, 0, s, mem, tex.w0, tex.h0, r, edges, ne, k); break;
            case VR_REGION_FILL: hipLaunchKernelGGL(k_region<kRegionFill>, grid, block, 0, s, mem, tex.w0, tex.h0, r, edges, ne, k); break;
            case VR_REGION_RAISE: hipLaunchKernelGGL(k_region<kRegionRaise>, grid, block, 0, s, mem, tex.w0, tex.h0, r, edges, ne, k); break;
            default: hipLaunchKernelGGL(k_region<kRegionPaint>, grid, block, 0, s, mem, tex.w0, tex.h0, r, edges, ne, k); break;
            }
            return VR_OK;
        });
}
