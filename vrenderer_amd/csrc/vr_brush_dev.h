// Device code the kernels that write level 0 of a map share - and nothing of the host's (that is vr_level0.h): the tile frame (a
// 256-thread workgroup per 32 x 8 tile of the call's rectangle, one texel per lane) and the dab list walked in chunks of 256.
#pragma once
#include "vr_internal.h"
#include "vr_dirty.h"
#include "vr_brush.h"
// (kept: brush_tile_mask is the chunk walk round erode_mask_max.  It cannot move next to it - vr_erode.h is the definition the host
// checks compile alone, and the walk is barriers and LDS - so the device frame includes the definition, not the other way round.)
#include "vr_erode.h"

constexpr int kBrushTileShift = 5, kBrushTileW = 1 << kBrushTileShift, kBrushTileH = 8, kBrushThreads = 256, kBrushChunk = 256;
static_assert(kBrushTileW * kBrushTileH == kBrushThreads && kBrushChunk == kBrushThreads, "one texel per lane; a chunk is one dab per lane");

__device__ __forceinline__ int brush_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// The tile mapping, once.  Of a grid of tiles_32x8(r) (vr_level0.h) workgroup (bx, by) has the tile whose first texel is
// (brush_tile_x(r.x0), brush_tile_y(r.y0)), and lane l has texel (brush_lane_x(), brush_lane_y()) = (l % 32, l / 32) of it.  A
// barrier-free kernel adds the two, and a lane at or beyond the rectangle's x1 or y1 leaves at once.
__device__ __forceinline__ int brush_tile_x(int x0) { return x0 + (int)blockIdx.x * kBrushTileW; }
__device__ __forceinline__ int brush_tile_y(int y0) { return y0 + (int)blockIdx.y * kBrushTileH; }
__device__ __forceinline__ int brush_lane_x(int tid = (int)threadIdx.x) { return tid & (kBrushTileW - 1); }
__device__ __forceinline__ int brush_lane_y(int tid = (int)threadIdx.x) { return tid >> kBrushTileShift; }

// The frame of a kernel with barriers, over the rectangle `r` of a map: the tile [tx0, tx1) x [ty0, ty1) clipped to r, the lane's
// texel (x, y) and whether it is `inside` the tile.  Every lane stays to the last barrier (the ballots and barriers want whole waves);
// one that is not inside works on the texel clamped into the w x h map, (cx(w), cy(h)), and writes nothing.
struct BrushTile {
    int tx0, ty0, tx1, ty1, x, y; bool inside;
    __device__ __forceinline__ int cx(int w) const { return brush_clampi(x, 0, w - 1); }
    __device__ __forceinline__ int cy(int h) const { return brush_clampi(y, 0, h - 1); }
};
__device__ __forceinline__ BrushTile brush_tile(const DirtyRect& r)
{
    BrushTile t;
    const int tid = (int)threadIdx.x;                              // (read first: the kernels' code objects are those of the frame written out in each)
    t.tx0 = brush_tile_x(r.x0); t.ty0 = brush_tile_y(r.y0);
    t.tx1 = t.tx0 + kBrushTileW < r.x1 ? t.tx0 + kBrushTileW : r.x1; t.ty1 = t.ty0 + kBrushTileH < r.y1 ? t.ty0 + kBrushTileH : r.y1;
    t.x = t.tx0 + brush_lane_x(tid); t.y = t.ty0 + brush_lane_y(tid);
    t.inside = t.x < t.tx1 && t.y < t.ty1;
    return t;
}

// (No shared texel codec: a level0_load / level0_store pair - a byte, or a dword unpacked by shifts and packed through brush_byte - was
// tried in k_brush, k_stamp, k_noise and k_texture, and the compiler told it from each kernel's own spelling - shifts in the first two,
// uchar4 in the others - in every SRGBA8 instance and in k_noise's whole-map R8 one.  The spellings stay where they were.)

// One chunk of the list: lane d tests dab base + d's span against the tile, and the survivors are compacted IN LIST ORDER into `list`
// (ballot + popcount prefix inside a wave, the four waves' totals through `wave_total`).  Returns how many there are, the same in
// every lane (a scalar loop bound).  Every lane of the workgroup calls it (two barriers inside); the caller puts one more barrier
// behind its use of `list`, in front of the next chunk.  The element is a BrushDab or anything else that carries a span [x0, x1) x
// [y0, y1) (vr_path.h's PathSeg): there is the one walk.
template <class Elem>
__device__ __forceinline__ uint32_t brush_chunk_list(const Elem* __restrict__ dabs, uint32_t n, uint32_t base, const BrushTile& t,
                                                     uint16_t (&list)[kBrushChunk], uint32_t (&wave_total)[4])
{
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t d = base + (uint32_t)tid;
    bool hit = false;
    if (d < n) {
        const Elem& b = dabs[d];
        hit = b.x0 < t.tx1 && b.x1 > t.tx0 && b.y0 < t.ty1 && b.y1 > t.ty0;
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

// The erosions' mask (vr_erode.h) of the lane's texel under the whole list.  Every lane of the workgroup calls it and stays to the
// end (barriers inside); a lane whose texel is not inside the tile gets 0.
__device__ __forceinline__ float brush_tile_mask(const BrushDab* __restrict__ dabs, uint32_t n, const BrushTile& t, uint16_t (&list)[kBrushChunk], uint32_t (&wave_total)[4])
{
    float m = 0.0f;
    for (uint32_t base = 0; base < n; base += kBrushChunk) {       // (n is a kernel argument: the trip count is uniform)
        const uint32_t total = brush_chunk_list(dabs, n, base, t, list, wave_total);
        for (uint32_t e = 0; e < total; e++) {
            const BrushDab b = dabs[brush_chunk_entry(list, e, n)];
            float f;
            if (t.inside && brush_weight(b, t.x, t.y, &f)) m = erode_mask_max(m, f, b.strength);
        }
        __syncthreads();                                           // the next chunk overwrites list and wave_total
    }
    return m;
}
