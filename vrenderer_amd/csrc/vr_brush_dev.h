// Device code the kernels that walk a dab list share (k_brush in vr_brush.hip, k_sweep_begin in vr_erode.hip): a 256-thread
// workgroup per 32 x 8 tile of the rectangle, one texel per lane, the list walked in chunks of 256 dabs.
#pragma once
#include "vr_internal.h"
#include "vr_dirty.h"
#include "vr_brush.h"
#include "vr_erode.h"

#include <string.h>

constexpr int kBrushTileW = 32, kBrushTileH = 8, kBrushChunk = 256;

__device__ __forceinline__ int brush_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
inline dim3 tiles_32x8(const DirtyRect& r) { return dim3((unsigned)((r.x1 - r.x0 + kBrushTileW - 1) / kBrushTileW), (unsigned)((r.y1 - r.y0 + kBrushTileH - 1) / kBrushTileH)); }

// One chunk of the list: lane d tests dab base + d's span against the tile [tx0, tx1) x [ty0, ty1), and the survivors are
// compacted IN LIST ORDER into `list` (ballot + popcount prefix inside a wave, the four waves' totals through `wave_total`).
// Returns how many there are, the same in every lane (a scalar loop bound).  Every lane of the workgroup calls it (two barriers
// inside); the caller puts one more barrier behind its use of `list`, in front of the next chunk.
__device__ __forceinline__ uint32_t brush_chunk_list(const BrushDab* __restrict__ dabs, uint32_t n, uint32_t base, int tx0, int ty0, int tx1, int ty1,
                                                     uint16_t (&list)[kBrushChunk], uint32_t (&wave_total)[4])
{
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t d = base + (uint32_t)tid;
    bool hit = false;
    if (d < n) {
        const BrushDab& b = dabs[d];
        hit = b.x0 < tx1 && b.x1 > tx0 && b.y0 < ty1 && b.y1 > ty0;
    }
    const unsigned long long m = __ballot(hit);
    const uint32_t before = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wave_total[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t first = 0, total = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) { const uint32_t c = wave_total[k]; first += k < wave ? c : 0u; total += c; }
    if (hit) list[first + before] = (uint16_t)d;               // first + before < total <= 256
    __syncthreads();
    return __builtin_amdgcn_readfirstlane(total);
}

// entry e of the chunk's list: the dab's index, wave-uniform and inside the list whatever LDS held
__device__ __forceinline__ uint32_t brush_chunk_entry(const uint16_t (&list)[kBrushChunk], uint32_t e, uint32_t n)
{
    const uint32_t di = __builtin_amdgcn_readfirstlane((uint32_t)list[e]);
    return di < n ? di : n - 1;
}

// The erosions' mask (vr_erode.h) of the lane's texel (x, y) under the whole list, for the tile [tx0, tx1) x [ty0, ty1).  Every lane
// of the workgroup calls it and stays to the end (barriers inside); a lane whose texel is not `inside` the tile gets 0.
__device__ __forceinline__ float brush_tile_mask(const BrushDab* __restrict__ dabs, uint32_t n, int tx0, int ty0, int tx1, int ty1, int x, int y, bool inside,
                                                 uint16_t (&list)[kBrushChunk], uint32_t (&wave_total)[4])
{
    float m = 0.0f;
    for (uint32_t base = 0; base < n; base += kBrushChunk) {       // (n is a kernel argument: the trip count is uniform)
        const uint32_t total = brush_chunk_list(dabs, n, base, tx0, ty0, tx1, ty1, list, wave_total);
        for (uint32_t e = 0; e < total; e++) {
            const BrushDab b = dabs[brush_chunk_entry(list, e, n)];
            float f;
            if (inside && brush_weight(b, x, y, &f)) m = erode_mask_max(m, f, b.strength);
        }
        __syncthreads();                                           // the next chunk overwrites list and wave_total
    }
    return m;
}

// ---- host side ----------------------------------------------------------------------------------------------------------
// A stroke's or an erosion's path behind its entry point's own argument checks: the dabs checked (as a stroke of `op`) and prepared
// for map `which`; nothing at all for an empty list; then reserve(rectangle) - everything the launches need, before anything is
// launched - the one wait on the host, the pinned list, and inside vr_derive_level0_write the history capture, the upload,
// launch(stream, rectangle, dabs) and order_side_end of the brush's buffers, whose order_side_idle the next call takes.
template <class Reserve, class Launch>
int vr_brush_call(vr_terrain* t, int which, const vr_brush_dab* dabs, uint32_t n, int op, int32_t out_rect[4], Reserve&& reserve, Launch&& launch)
{
    { const int rc = vr_brush_check_dabs(dabs, n, op); if (rc) return rc; }
    const DirtyRect dirty = vr_brush_prepare_dabs(t, which == 0 ? t->height : t->albedo, dabs, n);
    const std::vector<BrushDab>& prepared = t->brush_prepared;
    if (out_rect) { out_rect[0] = out_rect[1] = out_rect[2] = out_rect[3] = 0; }
    if (prepared.empty()) return VR_OK;                            // n == 0, or every dab misses the map: nothing is launched

    VR_HIP(hipSetDevice(t->ctx->device));
    { const int rc = reserve(dirty); if (rc) return rc; }
    // the one wait on the host: only where the previous stroke or erosion has not been consumed yet
    { const int rc = vr_brush_consumed(t); if (rc) return rc; }
    const uint32_t nd = (uint32_t)prepared.size();
    memcpy(t->h_brush_dabs, prepared.data(), (size_t)nd * sizeof(BrushDab));
    const int rc = vr_derive_level0_write(t, which, dirty, [&](hipStream_t s) -> int {
        { const int hrc = vr_history_capture(t, which, dirty, s); if (hrc) return hrc; }       // history on: the rectangle as it is, first
        VR_HIP(hipMemcpyAsync(t->d_brush_dabs, t->h_brush_dabs, (size_t)nd * sizeof(BrushDab), hipMemcpyHostToDevice, s));
        { const int lrc = launch(s, dirty, nd); if (lrc) return lrc; }
        VR_HIP(hipGetLastError());
        return order_side_end(t->ord_brush, VrOrderOps(), s);
    });
    if (rc) return rc;
    if (out_rect) { out_rect[0] = dirty.x0; out_rect[1] = dirty.y0; out_rect[2] = dirty.x1 - dirty.x0; out_rect[3] = dirty.y1 - dirty.y0; }
    return VR_OK;
}
