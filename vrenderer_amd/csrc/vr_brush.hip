// vr_terrain_brush: a stroke - an ordered list of dabs - applied to level 0 of a map on the device by one kernel, through
// vr_brush_call (vr_level0.h).  The definition of a stroke, texel by texel, is vr_brush.h; this file holds nothing of it but the
// order in which the header's functions are called.
//
//   k_brush_snapshot   SMOOTH only: the stroke's rectangle grown by one texel (clamped) out of the map, so that the 3 x 3 means
//                      are those of the map before the stroke whatever order the tiles run in
//   k_brush<op>        the tile frame and the chunk walk of vr_brush_dev.h; every lane applies the chunk's listed dabs in list
//                      order.  A texel no dab covers is not written.
//
// The kernel is untimed, like the mip and table kernels; the node-height and pyramid work counts where the edit's does.
#include "vr_level0.h"

struct BrushArgs {
    float target;               // FLATTEN
    float color[4];             // PAINT, stored encoding
    uint32_t channel_mask;      // PAINT
};

__global__ __launch_bounds__(kBrushThreads) void k_brush_snapshot(const uint8_t* __restrict__ map, int w0, uint8_t* __restrict__ snap, DirtyRect sr)
{
    const int x = brush_tile_x(sr.x0) + brush_lane_x(), y = brush_tile_y(sr.y0) + brush_lane_y();
    if (x >= sr.x1 || y >= sr.y1) return;
    snap[(size_t)(y - sr.y0) * (size_t)(sr.x1 - sr.x0) + (size_t)(x - sr.x0)] = map[(size_t)y * w0 + x];
}

// `map`: level 0 (R8: bytes, SRGBA8: dwords), w0 x h0; `r`: the stroke's rectangle, inside the map; `dabs`: n of them, none empty;
// `snap`: SMOOTH's snapshot of the rectangle `sr`
template <int OP>
__global__ __launch_bounds__(kBrushThreads) void k_brush(void* __restrict__ map, int w0, int h0, DirtyRect r, const BrushDab* __restrict__ dabs, uint32_t n,
                                                         BrushArgs a, const uint8_t* __restrict__ snap, DirtyRect sr)
{
    constexpr int NC = OP == kBrushPaint ? 4 : 1;
    __shared__ uint16_t list[kBrushChunk];  // the chunk's dabs that meet this tile, in list order
    __shared__ uint32_t wave_total[4];
    const BrushTile tile = brush_tile(r);
    const int x = tile.x, y = tile.y;
    const size_t at = (size_t)tile.cy(h0) * (size_t)w0 + (size_t)tile.cx(w0);
    float val[NC];
    uint32_t stored;
    if (OP == kBrushPaint) {
        stored = ((const uint32_t*)map)[at];
#pragma unroll
        for (int c = 0; c < NC; c++) val[c] = (float)((stored >> (8 * c)) & 255u);
    } else {
        stored = ((const uint8_t*)map)[at];
        val[0] = (float)stored;
    }
    float mean = 0.0f;
    if (OP == kBrushSmooth) {
        const int sw = sr.x1 - sr.x0;
        int sum = 0;
#pragma unroll
        for (int dy = -1; dy <= 1; dy++)
#pragma unroll
            for (int dx = -1; dx <= 1; dx++) {
                const int nx = brush_clampi(brush_clampi(x + dx, 0, w0 - 1), sr.x0, sr.x1 - 1), ny = brush_clampi(brush_clampi(y + dy, 0, h0 - 1), sr.y0, sr.y1 - 1);
                sum += (int)snap[(size_t)(ny - sr.y0) * (size_t)sw + (size_t)(nx - sr.x0)];
            }
        mean = brush_mean9(sum);
    }
    bool touched = false;
    for (uint32_t base = 0; base < n; base += kBrushChunk) {       // (n is a kernel argument: the trip count is uniform)
        const uint32_t total = brush_chunk_list(dabs, n, base, tile, list, wave_total);
        for (uint32_t e = 0; e < total; e++) {
            const BrushDab b = dabs[brush_chunk_entry(list, e, n)];
            float f;
            if (tile.inside && brush_weight(b, x, y, &f)) {
                touched = true;
                if (OP == kBrushRaise) val[0] = brush_raise(val[0], f, b.strength);
                else if (OP == kBrushFlatten) val[0] = brush_blend(val[0], f, b.strength, a.target);
                else if (OP == kBrushSmooth) val[0] = brush_blend(val[0], f, b.strength, mean);
                else {
#pragma unroll
                    for (int c = 0; c < NC; c++)
                        if (a.channel_mask & (1u << c)) val[c] = brush_blend(val[c], f, b.strength, a.color[c]);
                }
            }
        }
        __syncthreads();                                           // the next chunk overwrites list and wave_total
    }
    if (!touched) return;                                          // (touched implies inside)
    if (OP == kBrushPaint) {
        uint32_t out = 0;
#pragma unroll
        for (int c = 0; c < NC; c++) out |= (uint32_t)brush_byte(val[c]) << (8 * c);
        ((uint32_t*)map)[at] = out;
    } else ((uint8_t*)map)[at] = brush_byte(val[0]);
}

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
void vr_brush_release(vr_terrain* t)
{
    (void)vr_brush_consumed(t);
    if (t->ord_brush.ev) (void)hipEventDestroy(t->ord_brush.ev);
    t->ord_brush = VrOrderSide();
    if (t->h_brush_dabs) { (void)hipHostFree(t->h_brush_dabs); t->h_brush_dabs = nullptr; }
    (void)hipFree(t->d_brush_dabs); t->d_brush_dabs = nullptr;
    (void)hipFree(t->d_brush_snap); t->d_brush_snap = nullptr; t->brush_snap_bytes = 0;
    (void)hipFree(t->d_erode); t->d_erode = nullptr; t->erode_bytes = 0; t->erode_last = {};
}

// the previous stroke's kernel has passed: the pinned dabs, their device copy and the snapshot are free again
int vr_brush_consumed(vr_terrain* t) { return order_side_idle(t->ord_brush, VrOrderOps()); }

// Everything a stroke needs, before anything is launched: a refusal leaves the terrain as it was.
int vr_brush_reserve(vr_terrain* t, size_t snap_bytes)
{
    constexpr size_t dab_bytes = (size_t)VR_MAX_BRUSH_DABS * sizeof(BrushDab);
    if (!t->ord_brush.ev) VR_HIP(hipEventCreateWithFlags(&t->ord_brush.ev, hipEventDisableTiming));
    if (!t->h_brush_dabs) {
        const hipError_t e = hipHostMalloc((void**)&t->h_brush_dabs, dab_bytes, hipHostMallocDefault);
        if (e != hipSuccess) { (void)hipGetLastError(); t->h_brush_dabs = nullptr; vr_set_error("terrain brush: %zu bytes of pinned memory: %s", dab_bytes, hipGetErrorString(e)); return VR_ERR_OUT_OF_MEMORY; }
    }
    if (!t->d_brush_dabs) {
        void* p = nullptr;
        if (!vr_dev_alloc(&p, dab_bytes)) { vr_set_error("terrain brush: %zu bytes for the dab list", dab_bytes); return VR_ERR_OUT_OF_MEMORY; }
        t->d_brush_dabs = (BrushDab*)p;
    }
    const int rc = vr_brush_grow(t, &t->d_brush_snap, &t->brush_snap_bytes, snap_bytes);
    if (rc == VR_ERR_OUT_OF_MEMORY) vr_set_error("terrain brush: %zu bytes for the snapshot", snap_bytes);
    return rc;
}

// A buffer whose one reader runs in front of ord_brush's event holds `bytes` (vr_reserve), the old block freed behind
// vr_brush_consumed.  A refusal leaves the terrain as it was; the caller words VR_ERR_OUT_OF_MEMORY's message.
int vr_brush_grow(vr_terrain* t, void** ptr, size_t* capacity, size_t bytes)
{
    return vr_reserve(ptr, capacity, bytes, [t]() -> int { return vr_brush_consumed(t); });
}

// the dab checks of a stroke of `op` (erosion's strengths are opacities: it passes VR_BRUSH_FLATTEN)
int vr_brush_check_dabs(const vr_brush_dab* dabs, uint32_t n, int op)
{
    for (uint32_t i = 0; i < n; i++) {
        const vr_brush_dab& d = dabs[i];
        VR_REQUIRE(host_finite(d.x) && host_finite(d.z) && host_finite(d.radius) && host_finite(d.hardness) && host_finite(d.strength), "a dab holds a NaN or an infinity");
        VR_REQUIRE(d.radius > 0.0f, "radius must be positive");
        VR_REQUIRE(d.hardness >= 0.0f && d.hardness < 1.0f, "hardness outside [0, 1)");
        if (op == VR_BRUSH_RAISE) VR_REQUIRE(fabsf(d.strength) <= 255.0f, "RAISE: |strength| above 255");
        else VR_REQUIRE(d.strength >= 0.0f && d.strength <= 1.0f, "opacity outside [0, 1]");
    }
    return VR_OK;
}

// The dabs that meet the map, in order, prepared for the map `tex`, into t->brush_prepared, and the hull of their spans - on the
// host alone (the vector keeps its room from stroke to stroke).
DirtyRect vr_brush_prepare_dabs(vr_terrain* t, const DevTex& tex, const vr_brush_dab* dabs, uint32_t n)
{
    std::vector<BrushDab>& prepared = t->brush_prepared;
    prepared.clear();
    prepared.reserve(VR_MAX_BRUSH_DABS);
    DirtySpan hx, hy;
    for (uint32_t i = 0; i < n; i++) {
        const vr_brush_dab& d = dabs[i];
        const BrushDab b = brush_prepare(d.x, d.z, d.radius, d.hardness, d.strength, t->p.world_size, tex.w0, tex.h0);
        if (brush_dab_empty(b)) continue;
        DirtySpan sx, sy; sx.lo = b.x0; sx.hi = b.x1; sy.lo = b.y0; sy.hi = b.y1;
        hx = dirty_hull(hx, sx); hy = dirty_hull(hy, sy);
        prepared.push_back(b);
    }
    return dirty_rect(hx, hy);
}

extern "C" VR_API int vr_terrain_brush(vr_terrain* t, const vr_brush_stroke* stroke, const vr_brush_dab* dabs, uint32_t n, int32_t out_rect[4])
{
    static_assert(sizeof(vr_brush_dab) == 32 && sizeof(vr_brush_stroke) == 32, "vr_brush_dab / vr_brush_stroke layout");
    static_assert(VR_BRUSH_RAISE == kBrushRaise && VR_BRUSH_FLATTEN == kBrushFlatten && VR_BRUSH_SMOOTH == kBrushSmooth && VR_BRUSH_PAINT == kBrushPaint, "vr_brush.h's ops");
    static_assert(VR_MAX_BRUSH_DABS <= 65536, "k_brush's index list holds 16-bit indices");
    // the argument checks come before any use of the device (and leave the terrain alone)
    VR_REQUIRE(t != nullptr, "terrain is NULL");
    VR_REQUIRE(stroke != nullptr, "stroke is NULL");
    VR_REQUIRE(dabs != nullptr || n == 0, "dabs is NULL with n > 0");
    VR_REQUIRE(n <= VR_MAX_BRUSH_DABS, "more than VR_MAX_BRUSH_DABS dabs");
    const int op = stroke->op;
    VR_REQUIRE(op == VR_BRUSH_RAISE || op == VR_BRUSH_FLATTEN || op == VR_BRUSH_SMOOTH || op == VR_BRUSH_PAINT, "unknown op");
    VR_REQUIRE(host_finite(stroke->target), "target is NaN or infinite");
    for (int c = 0; c < 4; c++) VR_REQUIRE(host_finite(stroke->color[c]), "color is NaN or infinite");
    if (op == VR_BRUSH_FLATTEN) VR_REQUIRE(stroke->target >= 0.0f && stroke->target <= 255.0f, "target outside [0, 255]");
    if (op == VR_BRUSH_PAINT) {
        VR_REQUIRE(stroke->channel_mask >= 1u && stroke->channel_mask <= 15u, "channel_mask must be 1 .. 15");
        for (int c = 0; c < 4; c++) VR_REQUIRE(stroke->color[c] >= 0.0f && stroke->color[c] <= 255.0f, "color outside [0, 255]");
    }
    const int which = op == VR_BRUSH_PAINT ? 1 : 0;
    const DevTex& tex = vr_terrain_map(t, which);
    BrushArgs a; memset(&a, 0, sizeof(a));
    a.target = stroke->target; a.channel_mask = stroke->channel_mask;
    for (int c = 0; c < 4; c++) a.color[c] = stroke->color[c];
    DirtyRect sr;                                                  // SMOOTH reads the rectangle grown by one texel, clamped to the map
    return vr_brush_call(t, which, dabs, n, op, out_rect,
        [&](const DirtyRect& dirty) -> int {
            sr = dirty;
            if (op == VR_BRUSH_SMOOTH) sr = dirty_rect(dirty_clip(DirtySpan{ dirty.x0 - 1, dirty.x1 + 1 }, tex.w0), dirty_clip(DirtySpan{ dirty.y0 - 1, dirty.y1 + 1 }, tex.h0));
            return vr_brush_reserve(t, op == VR_BRUSH_SMOOTH ? (size_t)(sr.x1 - sr.x0) * (size_t)(sr.y1 - sr.y0) : 0);
        },
        [&](hipStream_t s, const DirtyRect& dirty, uint32_t nd) -> int {
            void* mem = const_cast<uint8_t*>(tex.base);
            const uint8_t* snap = (const uint8_t*)t->d_brush_snap;
            const dim3 grid = tiles_32x8(dirty), block(kBrushThreads);
            switch (op) {
            case VR_BRUSH_RAISE: hipLaunchKernelGGL(k_brush<kBrushRaise>, grid, block, 0, s, mem, tex.w0, tex.h0, dirty, t->d_brush_dabs, nd, a, snap, sr); break;
            case VR_BRUSH_FLATTEN: hipLaunchKernelGGL(k_brush<kBrushFlatten>, grid, block, 0, s, mem, tex.w0, tex.h0, dirty, t->d_brush_dabs, nd, a, snap, sr); break;
            case VR_BRUSH_SMOOTH:
                hipLaunchKernelGGL(k_brush_snapshot, tiles_32x8(sr), block, 0, s, (const uint8_t*)mem, tex.w0, (uint8_t*)t->d_brush_snap, sr);
                hipLaunchKernelGGL(k_brush<kBrushSmooth>, grid, block, 0, s, mem, tex.w0, tex.h0, dirty, t->d_brush_dabs, nd, a, snap, sr); break;
            default: hipLaunchKernelGGL(k_brush<kBrushPaint>, grid, block, 0, s, mem, tex.w0, tex.h0, dirty, t->d_brush_dabs, nd, a, snap, sr); break;
            }
            return VR_OK;
        });
}
