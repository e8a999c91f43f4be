// vr_terrain_path: a corridor along a polyline - one weight and one target per texel, from the nearest of the path's segments -
// written into level 0 of a map by one kernel, through vr_list_call (vr_level0.h).  The definition, texel by texel, is vr_path.h; this
// file holds nothing of it but the order in which the header's functions are called.
//
//   k_path<OP>   the tile frame and the chunk walk of vr_brush_dev.h over PathSeg: lane d tests segment base + d against the tile,
//                the survivors are listed in list order, and every lane runs them in that order and keeps (q, t, index) of the
//                smallest q below 1 - a min-reduction with a strict <, so of equal q the lowest index stays.  The segment read in
//                the inner loop is wave-uniform (brush_chunk_entry's readfirstlane): scalar loads.  The winner's heights are read
//                once, behind the last barrier, by the lane's own index.  A texel no segment covers is not written.
//                The tile cull is the span's box alone: a second test of the tile against the segment's capsule was measured
//                against it and not kept (profiles/terrain_path_variants.txt).
//
// The kernel is untimed, like the brush kernel.
#include "vr_level0.h"
#include "vr_path.h"

// `map`: level 0 (R8: bytes, SRGBA8: dwords), w0 x h0; `r`: the call's rectangle, inside the map; `segs`: n of them, none empty
template <int OP>
__global__ __launch_bounds__(kBrushThreads) void k_path(void* __restrict__ map, int w0, int h0, DirtyRect r, const PathSeg* __restrict__ segs, uint32_t n, PathConst k)
{
    constexpr int NC = OP == kPathPaint ? 4 : 1;
    __shared__ uint16_t list[kBrushChunk];  // the chunk's segments that meet this tile, in list order
    __shared__ uint32_t wave_total[4];
    const BrushTile tile = brush_tile(r);
    const int cx = tile.cx(w0), cy = tile.cy(h0);
    float best_q = 1.0f, best_t = 0.0f;
    uint32_t best = 0;
    for (uint32_t base = 0; base < n; base += kBrushChunk) {       // (n is a kernel argument: the trip count is uniform)
        const uint32_t total = brush_chunk_list(segs, n, base, tile, list, wave_total);
        for (uint32_t e = 0; e < total; e++) {
            const uint32_t si = brush_chunk_entry(list, e, n);
            const PathSeg s = segs[si];
            float q, t;
            path_texel(s, k, cx, cy, &q, &t);
            if (q < best_q) { best_q = q; best_t = t; best = si; }
        }
        __syncthreads();                                           // the next chunk overwrites list and wave_total
    }
    float f;
    if (!(tile.inside && brush_falloff(best_q, k.h2, k.k, &f))) return;      // behind the last barrier
    const size_t at = (size_t)cy * (size_t)w0 + (size_t)cx;
    if (OP == kPathPaint) {
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
        const PathSeg& s = segs[best < n ? best : n - 1];
        const float val = (float)((const uint8_t*)map)[at];
        ((uint8_t*)map)[at] = brush_byte(path_apply(OP, k.opacity, val, f, path_target(s, best_t)));
    }
}

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
extern "C" VR_API int vr_terrain_path(vr_terrain* t, int which, const vr_path_params* p, const vr_path_point* points, uint32_t n, int32_t out_rect[4])
{
    static_assert(sizeof(vr_path_point) == 16 && sizeof(vr_path_params) == 64, "vr_path_point / vr_path_params layout");
    static_assert(VR_PATH_LEVEL == kPathLevel && VR_PATH_CUT == kPathCut && VR_PATH_FILL == kPathFill && VR_PATH_PAINT == kPathPaint, "vr_path.h's ops");
    static_assert(VR_MAX_PATH_POINTS == kPathMaxPoints && VR_MAX_BRUSH_DABS == kPathMaxListed, "vr_path.h's limits");
    // the argument checks come before any use of the device (and leave the terrain alone)
    VR_REQUIRE(t != nullptr, "terrain is NULL");
    VR_REQUIRE(p != nullptr, "params is NULL");
    VR_REQUIRE(points != nullptr || n == 0, "points is NULL with n > 0");
    VR_REQUIRE(n <= VR_MAX_PATH_POINTS, "more than VR_MAX_PATH_POINTS points");
    VR_REQUIRE(which == 0 || which == 1, "which must be 0 (heightmap) or 1 (albedo)");
    const int op = p->op;
    VR_REQUIRE(op == VR_PATH_LEVEL || op == VR_PATH_CUT || op == VR_PATH_FILL || op == VR_PATH_PAINT, "unknown op");
    VR_REQUIRE((op == VR_PATH_PAINT) == (which == 1), "LEVEL, CUT and FILL work on the heightmap, PAINT on the albedo");
    VR_REQUIRE((p->flags & ~(uint32_t)VR_PATH_CLOSED) == 0, "unknown flag bits");
    const bool closed = (p->flags & VR_PATH_CLOSED) != 0;
    VR_REQUIRE(!closed || n >= 3, "VR_PATH_CLOSED needs at least 3 points");
    VR_REQUIRE(host_finite(p->radius) && host_finite(p->hardness) && host_finite(p->opacity), "params holds a NaN or an infinity");
    for (int c = 0; c < 4; c++) VR_REQUIRE(host_finite(p->color[c]), "color is NaN or infinite");
    VR_REQUIRE(p->radius > 0.0f, "radius must be positive");
    VR_REQUIRE(p->hardness >= 0.0f && p->hardness < 1.0f, "hardness outside [0, 1)");
    VR_REQUIRE(p->opacity >= 0.0f && p->opacity <= 1.0f, "opacity outside [0, 1]");
    for (int c = 0; c < 4; c++) VR_REQUIRE(p->color[c] >= 0.0f && p->color[c] <= 255.0f, "color outside [0, 255]");
    VR_REQUIRE(p->channel_mask >= 1u && p->channel_mask <= 15u, "channel_mask must be 1 .. 15");
    VR_REQUIRE(which == 1 || p->channel_mask == 1u, "the heightmap has channel_mask 1");
    for (int i = 0; i < 6; i++) VR_REQUIRE(p->reserved[i] == 0, "reserved must be zero");
    for (uint32_t i = 0; i < n; i++) {
        const vr_path_point& q = points[i];
        VR_REQUIRE(host_finite(q.x) && host_finite(q.z) && host_finite(q.height) && host_finite(q.reserved), "a point holds a NaN or an infinity");
        VR_REQUIRE(q.height >= 0.0f && q.height <= 255.0f, "height outside [0, 255]");
        VR_REQUIRE(q.reserved == 0.0f, "a point's reserved word must be zero");
    }
    // the handle is looked into from here on
    const DevTex& tex = vr_terrain_map(t, which);
    const PathConst k = path_const(p->radius, p->hardness, p->opacity, op, p->color, p->channel_mask, t->p.world_size, tex.w0, tex.h0);
    static_assert(sizeof(vr_path_point) == sizeof(PathPoint) + sizeof(float), "PathPoint is vr_path_point without its reserved word");
    std::vector<PathPoint>& pts = t->path_points;
    pts.resize(n);
    for (uint32_t i = 0; i < n; i++) pts[i] = PathPoint{ points[i].x, points[i].z, points[i].height };
    int32_t hull[4];
    path_prepare(pts.data(), n, closed, k, t->p.world_size, tex.w0, tex.h0, t->path_prepared, hull);
    DirtyRect dirty;
    if (!t->path_prepared.empty()) { dirty.x0 = hull[0]; dirty.y0 = hull[1]; dirty.x1 = hull[2]; dirty.y1 = hull[3]; }
    return vr_list_call(t, which, dirty, t->path_prepared.data(), (uint32_t)t->path_prepared.size(), out_rect,
        [&](const DirtyRect&) -> int { return vr_brush_reserve(t, 0); },                            // nothing beyond the list
        [&](hipStream_t s, const DirtyRect& r, uint32_t ns) -> int {
            void* mem = const_cast<uint8_t*>(tex.base);
            const PathSeg* segs = (const PathSeg*)t->d_brush_dabs;
            const dim3 grid = tiles_32x8(r), block(kBrushThreads);
            switch (op) {
            case VR_PATH_LEVEL: hipLaunchKernelGGL(k_path<kPathLevel>, grid, block, 0, s, mem, tex.w0, tex.h0, r, segs, ns, k); break;
            case VR_PATH_CUT: hipLaunchKernelGGL(k_path<kPathCut>, grid, block, 0, s, mem, tex.w0, tex.h0, r, segs, ns, k); break;
            case VR_PATH_FILL: hipLaunchKernelGGL(k_path<kPathFill>, grid, block, 0, s, mem, tex.w0, tex.h0, r, segs, ns, k); break;
            default: hipLaunchKernelGGL(k_path<kPathPaint>, grid, block, 0, s, mem, tex.w0, tex.h0, r, segs, ns, k); break;
            }
            return VR_OK;
        });
}
