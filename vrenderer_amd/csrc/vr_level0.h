// The host's call frame of every entry point that writes level 0 of a terrain map on the device (edit, brush, both erosions, texture,
// occlusion, stamp, noise, path, region), behind the entry point's own argument checks.  The ordering rules live here and nowhere else: a refusal comes before
// any effect, the history capture is first on the stream, hipGetLastError follows the launches, out_rect is zeroed past the last
// argument refusal and filled on success only.  The kernels' side of it is vr_brush_dev.h; DESIGN.md 4aa.
#pragma once
#include "vr_brush_dev.h"

#include <string.h>

inline dim3 tiles_32x8(const DirtyRect& r) { return dim3((unsigned)((r.x1 - r.x0 + kBrushTileW - 1) / kBrushTileW), (unsigned)((r.y1 - r.y0 + kBrushTileH - 1) / kBrushTileH)); }
inline void level0_out_rect(int32_t out_rect[4], const DirtyRect& r)
{
    if (out_rect) { out_rect[0] = r.x0; out_rect[1] = r.y0; out_rect[2] = r.x1 - r.x0; out_rect[3] = r.y1 - r.y0; }
}

// One write of the rectangle `dirty` of map `which`: nothing at all for an empty rectangle; else vr_derive_level0_write, whose write
// step is the history capture, then write(stream) - the caller's copies and launches, and order_side_end of a side resource of its
// own - then hipGetLastError.
template <class Write>
int vr_level0_call(vr_terrain* t, int which, const DirtyRect& dirty, int32_t out_rect[4], Write&& write)
{
    level0_out_rect(out_rect, DirtyRect());
    if (dirty_empty(dirty)) return VR_OK;                          // nothing is launched
    VR_HIP(hipSetDevice(t->ctx->device));
    const int rc = vr_derive_level0_write(t, which, dirty, [&](hipStream_t s) -> int {
        { const int hrc = vr_history_capture(t, which, dirty, s); if (hrc) return hrc; }       // history on: the rectangle as it is, first
        { const int wrc = write(s); if (wrc) return wrc; }
        VR_HIP(hipGetLastError());
        return VR_OK;
    });
    if (rc == VR_OK) level0_out_rect(out_rect, dirty);
    return rc;
}

// A call whose kernel walks a prepared list - dabs, a path's segments (vr_path.h) or a region's edges (vr_region.h) - that travels in the terrain's brush list buffers:
// `count` elements at `prepared`, of BrushDab's size, prepared on the host for map `which`, and the hull `dirty` of their spans.
// Nothing at all where the list is empty; then reserve(rectangle) - everything the launches need, before anything is launched - the
// one wait on the host, the pinned list, and as the write the upload, launch(stream, rectangle, count) and order_side_end of the
// brush's buffers, whose order_side_idle the next call takes.
template <class Elem, class Reserve, class Launch>
int vr_list_call(vr_terrain* t, int which, const DirtyRect& dirty, const Elem* prepared, uint32_t count, int32_t out_rect[4], Reserve&& reserve, Launch&& launch)
{
    static_assert(sizeof(Elem) == sizeof(BrushDab), "the list travels in h_brush_dabs / d_brush_dabs");
    level0_out_rect(out_rect, DirtyRect());
    if (count == 0) return VR_OK;                                  // n == 0, or every element misses the map: nothing is launched

    VR_HIP(hipSetDevice(t->ctx->device));
    { const int rc = reserve(dirty); if (rc) return rc; }
    // the one wait on the host: only where the previous stroke, erosion or path has not been consumed yet
    { const int rc = vr_brush_consumed(t); if (rc) return rc; }
    memcpy(t->h_brush_dabs, prepared, (size_t)count * sizeof(BrushDab));
    return vr_level0_call(t, which, dirty, out_rect, [&](hipStream_t s) -> int {
        VR_HIP(hipMemcpyAsync(t->d_brush_dabs, t->h_brush_dabs, (size_t)count * sizeof(BrushDab), hipMemcpyHostToDevice, s));
        { const int lrc = launch(s, dirty, count); if (lrc) return lrc; }
        VR_HIP(hipGetLastError());
        return order_side_end(t->ord_brush, VrOrderOps(), s);
    });
}

// A stroke's or an erosion's call: the dabs checked (as a stroke of `op`) and prepared for map `which`, then vr_list_call.
template <class Reserve, class Launch>
int vr_brush_call(vr_terrain* t, int which, const vr_brush_dab* dabs, uint32_t n, int op, int32_t out_rect[4], Reserve&& reserve, Launch&& launch)
{
    { const int rc = vr_brush_check_dabs(dabs, n, op); if (rc) return rc; }
    const DirtyRect dirty = vr_brush_prepare_dabs(t, vr_terrain_map(t, which), dabs, n);
    const std::vector<BrushDab>& prepared = t->brush_prepared;
    return vr_list_call(t, which, dirty, prepared.data(), (uint32_t)prepared.size(), out_rect, reserve, launch);
}

// An operation under the erosions' mask of a dab list (strength is an opacity), or - `whole` - over the whole map with no list, when
// none of ord_brush's buffers is touched.  launch(stream, rectangle, dabs on the device or nullptr, count).
template <class Launch>
int vr_mask_call(vr_terrain* t, int which, bool whole, const vr_brush_dab* dabs, uint32_t n, int32_t out_rect[4], Launch&& launch)
{
    if (whole) {
        const DevTex& tex = vr_terrain_map(t, which);
        const DirtyRect dirty = dirty_whole(tex.w0, tex.h0);
        return vr_level0_call(t, which, dirty, out_rect, [&](hipStream_t s) -> int { return launch(s, dirty, (const BrushDab*)nullptr, 0u); });
    }
    return vr_brush_call(t, which, dabs, n, VR_BRUSH_FLATTEN, out_rect,
        [&](const DirtyRect&) -> int { return vr_brush_reserve(t, 0); },                         // nothing beyond the dab list
        [&](hipStream_t s, const DirtyRect& dirty, uint32_t nd) -> int { return launch(s, dirty, (const BrushDab*)t->d_brush_dabs, nd); });
}
