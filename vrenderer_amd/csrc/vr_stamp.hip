// Stamps: a patch of R8 or SRGBA8 texels kept in device memory (vr_stamp_create, vr_stamp_from_terrain) and set into level 0 of a
// map at a position, size and angle with a blend rule (vr_terrain_stamp) by one kernel, through vr_level0_call (vr_level0.h).  The
// definition, texel by texel, is vr_stamp.h; this file holds nothing of it.
//
//   k_stamp_copy<T>            the pitched copies: the caller's device memory into a new stamp, a rectangle of a map's level 0 into one
//   k_stamp<FORMAT>            the barrier-free tile frame of vr_brush_dev.h over the call's rectangle.  The prepared
//                              constants are one kernel argument: wave-uniform, read by scalar loads.  A texel reads a 2 x 2
//                              footprint of the stamp straight from memory, through the caches.  A variant that first loaded the
//                              tile's footprint in stamp space into LDS was built and measured against this one: it beat it at no
//                              shape by more than the run-to-run spread and lost by up to 19 % on the large ones (presumably neighbouring
//                              lanes' taps share cache lines anyway and the staging loop costs more than it saves), so the direct
//                              kernel is the only one (profiles/terrain_stamp_variants.txt).  There is no barrier;
//                              every index is clamped before it addresses memory; a lane outside the rectangle or not covered
//                              stores nothing; there is no loop.
//
// A stamp is a side resource (vr_order.h): one OrderSide, order_side_begin / _end round every kernel and copy that reads or writes
// it, order_side_idle in front of its free.  The kernels are untimed, like the brush kernel.
#include "vr_level0.h"
#include "vr_stamp.h"

#include <new>

struct vr_stamp {
    vr_context* ctx;            // first, like vr_terrain's: the refusals compare the two
    int32_t format, w, h;
    uint8_t* d_texels;          // w x h texels, tightly packed
    VrOrderSide ord;
};

template <class T>
__global__ __launch_bounds__(256) void k_stamp_copy(const uint8_t* __restrict__ src, size_t src_pitch, T* __restrict__ dst, int w, int h)
{
    const int x = brush_tile_x(0) + brush_lane_x(), y = brush_tile_y(0) + brush_lane_y();
    if (x >= w || y >= h) return;
    dst[(size_t)y * (size_t)w + (size_t)x] = ((const T*)(src + (size_t)y * src_pitch))[x];
}

// stamp texel (x, y), inside the stamp, as a dword
template <int FORMAT> struct StampTexel { using type = uint8_t; };
template <> struct StampTexel<kStampSrgba8> { using type = uint32_t; };
template <int FORMAT> struct StampFetch {
    using T = typename StampTexel<FORMAT>::type;
    const T* __restrict__ texels; int sw;
    __host__ __device__ __forceinline__ uint32_t operator()(int x, int y) const { return (uint32_t)texels[(size_t)y * (size_t)sw + (size_t)x]; }
};

// `map`: level 0 (R8: bytes, SRGBA8: dwords), w0 x h0; `r`: the call's rectangle, inside the map; `stamp`: k.sw x k.sh texels
template <int FORMAT>
__global__ __launch_bounds__(256) void k_stamp(void* __restrict__ map, int w0, int h0, DirtyRect r, const void* __restrict__ stamp, StampConst k)
{
    using T = typename StampTexel<FORMAT>::type;
    constexpr int NC = FORMAT == kStampSrgba8 ? 4 : 1;
    const int x = brush_tile_x(r.x0) + brush_lane_x(), y = brush_tile_y(r.y0) + brush_lane_y();
    if (x >= r.x1 || y >= r.y1) return;                            // (no barrier anywhere below)
    const int cx = brush_clampi(x, 0, w0 - 1), cy = brush_clampi(y, 0, h0 - 1);
    StampFetch<FORMAT> fetch;
    fetch.texels = (const T*)stamp; fetch.sw = k.sw;
    const size_t at = (size_t)cy * (size_t)w0 + (size_t)cx;
    float val[NC];
    if constexpr (NC == 4) {
        const uint32_t px = ((const uint32_t*)map)[at];
#pragma unroll
        for (int c = 0; c < NC; c++) val[c] = (float)((px >> (8 * c)) & 255u);
    } else val[0] = (float)((const uint8_t*)map)[at];
    if (!stamp_texel<NC>(k, fetch, cx, cy, val)) return;
    if constexpr (NC == 4) {
        uint32_t out = 0;
#pragma unroll
        for (int c = 0; c < NC; c++) out |= (uint32_t)brush_byte(val[c]) << (8 * c);
        ((uint32_t*)map)[at] = out;
    } else ((uint8_t*)map)[at] = brush_byte(val[0]);
}

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
static size_t stamp_texel_bytes(int format) { return format == VR_STAMP_SRGBA8 ? 4 : 1; }
static dim3 stamp_tiles(int w, int h) { return tiles_32x8(dirty_whole(w, h)); }

// a stamp of `format`, w x h, its memory and its event; everything or nothing
static int stamp_new(vr_context* ctx, int format, int w, int h, vr_stamp** out)
{
    vr_stamp* st = new (std::nothrow) vr_stamp();
    if (!st) { vr_set_error("stamp: host memory"); return VR_ERR_OUT_OF_MEMORY; }
    st->ctx = ctx; st->format = format; st->w = w; st->h = h; st->d_texels = nullptr;
    const size_t bytes = (size_t)w * (size_t)h * stamp_texel_bytes(format);
    void* p = nullptr;
    if (!vr_dev_alloc(&p, bytes)) { delete st; vr_set_error("stamp: %zu bytes of device memory", bytes); return VR_ERR_OUT_OF_MEMORY; }
    st->d_texels = (uint8_t*)p;
    const hipError_t e = hipEventCreateWithFlags(&st->ord.ev, hipEventDisableTiming);
    if (e != hipSuccess) { (void)hipGetLastError(); vr_dev_free(p); delete st; vr_set_error("stamp: hipEventCreateWithFlags -> %s", hipGetErrorString(e)); return VR_ERR_HIP; }
    *out = st;
    return VR_OK;
}

static void stamp_free(vr_stamp* st)
{
    if (st->ord.ev) (void)hipEventDestroy(st->ord.ev);
    vr_dev_free(st->d_texels);
    delete st;
}

// `src` (device memory, rows src_pitch bytes apart) into the stamp, on `s`, between the stamp's order_side_begin and _end
static int stamp_fill(vr_stamp* st, const uint8_t* src, size_t src_pitch, hipStream_t s)
{
    { const int rc = order_side_begin(st->ord, VrOrderOps(), s); if (rc) return rc; }
    if (st->format == VR_STAMP_R8) hipLaunchKernelGGL(k_stamp_copy<uint8_t>, stamp_tiles(st->w, st->h), dim3(256), 0, s, src, src_pitch, st->d_texels, st->w, st->h);
    else hipLaunchKernelGGL(k_stamp_copy<uint32_t>, stamp_tiles(st->w, st->h), dim3(256), 0, s, src, src_pitch, (uint32_t*)st->d_texels, st->w, st->h);
    VR_HIP(hipGetLastError());
    return order_side_end(st->ord, VrOrderOps(), s);
}

extern "C" VR_API int vr_stamp_create(vr_context* ctx, int format, int32_t w, int32_t h, const void* texels, size_t row_pitch_bytes, int device_pointer, vr_stamp** out)
{
    static_assert(VR_STAMP_R8 == kStampR8 && VR_STAMP_SRGBA8 == kStampSrgba8, "vr_stamp.h's formats");
    // the argument checks come before any use of the device
    VR_REQUIRE(out != nullptr, "out is NULL");
    *out = nullptr;
    VR_REQUIRE(ctx != nullptr, "context is NULL");
    VR_REQUIRE(format == VR_STAMP_R8 || format == VR_STAMP_SRGBA8, "format must be VR_STAMP_R8 or VR_STAMP_SRGBA8");
    VR_REQUIRE(w >= 1 && w <= kStampMaxSide && h >= 1 && h <= kStampMaxSide, "a stamp has 1 .. 4096 texels per side");
    VR_REQUIRE(texels != nullptr, "texels is NULL");
    const size_t tb = stamp_texel_bytes(format), row = (size_t)w * tb;
    VR_REQUIRE(row_pitch_bytes == 0 || row_pitch_bytes >= row, "row pitch smaller than a row");
    VR_REQUIRE(!device_pointer || (((uintptr_t)texels | row_pitch_bytes) & (tb - 1)) == 0, "device pointer and pitch must be aligned to the texel size");
    const size_t pitch = row_pitch_bytes ? row_pitch_bytes : row;
    VR_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    vr_stamp* st = nullptr;
    { const int rc = stamp_new(ctx, format, w, h, &st); if (rc) return rc; }
    struct Guard { vr_stamp*& st; ~Guard() { if (st) { (void)hipStreamSynchronize(st->ctx->stream); stamp_free(st); } } } guard{ st };      // an early return frees it
    if (device_pointer) {
        const int rc = stamp_fill(st, (const uint8_t*)texels, pitch, s);
        if (rc) return rc;
    } else {
        // the caller's host memory straight into the stamp; the call returns once it has been consumed
        VR_HIP(hipMemcpy2DAsync(st->d_texels, row, texels, pitch, row, (size_t)h, hipMemcpyHostToDevice, s));
        { const int rc = order_side_end(st->ord, VrOrderOps(), s); if (rc) return rc; }
        VR_HIP(hipStreamSynchronize(s));
    }
    *out = st; st = nullptr;
    return VR_OK;
}

extern "C" VR_API int vr_stamp_from_terrain(vr_terrain* t, int which, int32_t x, int32_t y, int32_t w, int32_t h, vr_stamp** out)
{
    VR_REQUIRE(out != nullptr, "out is NULL");
    *out = nullptr;
    VR_REQUIRE(t != nullptr, "terrain is NULL");
    VR_REQUIRE(which == 0 || which == 1, "which must be 0 (heightmap) or 1 (albedo)");
    VR_REQUIRE(w >= 1 && w <= kStampMaxSide && h >= 1 && h <= kStampMaxSide, "a stamp has 1 .. 4096 texels per side");
    VR_REQUIRE(x >= 0 && y >= 0, "negative coordinate");
    const DevTex& tex = vr_terrain_map(t, which);
    VR_REQUIRE((int64_t)x + w <= tex.w0 && (int64_t)y + h <= tex.h0, "the rectangle is not inside level 0");
    vr_context* ctx = t->ctx;
    VR_HIP(hipSetDevice(ctx->device));
    vr_stamp* st = nullptr;
    { const int rc = stamp_new(ctx, which, w, h, &st); if (rc) return rc; }
    // level 0 as it is on the device: every writer of the maps runs on the context's stream, so the copy, queued there, is behind the last
    const size_t tb = stamp_texel_bytes(which), map_pitch = (size_t)tex.w0 * tb;
    const int rc = stamp_fill(st, tex.base + (size_t)y * map_pitch + (size_t)x * tb, map_pitch, ctx->stream);
    if (rc) { (void)hipStreamSynchronize(ctx->stream); stamp_free(st); return rc; }
    *out = st;
    return VR_OK;
}

extern "C" VR_API void vr_stamp_destroy(vr_stamp* st)
{
    if (!st) return;
    (void)hipSetDevice(st->ctx->device);
    (void)order_side_idle(st->ord, VrOrderOps());
    stamp_free(st);
}

extern "C" VR_API int vr_stamp_info(const vr_stamp* st, int32_t* format, int32_t* w, int32_t* h)
{
    VR_REQUIRE(st != nullptr, "stamp is NULL");
    if (format) *format = st->format;
    if (w) *w = st->w;
    if (h) *h = st->h;
    return VR_OK;
}

extern "C" VR_API int vr_stamp_download(vr_stamp* st, void* host, size_t bytes)
{
    VR_REQUIRE(st != nullptr, "stamp is NULL");
    VR_REQUIRE(host != nullptr, "host is NULL");
    const size_t need = (size_t)st->w * (size_t)st->h * stamp_texel_bytes(st->format);
    VR_REQUIRE(bytes >= need, "capacity below the stamp's texels");
    VR_HIP(hipSetDevice(st->ctx->device));
    hipStream_t s = st->ctx->stream;
    { const int rc = order_side_begin(st->ord, VrOrderOps(), s); if (rc) return rc; }
    VR_HIP(hipMemcpyAsync(host, st->d_texels, need, hipMemcpyDeviceToHost, s));
    VR_HIP(hipStreamSynchronize(s));
    return VR_OK;
}

// k_stamp over the rectangle `r` on `s`
static void stamp_launch(vr_terrain* t, int which, hipStream_t s, const DirtyRect& r, const vr_stamp* st, const StampConst& k)
{
    const DevTex& tex = vr_terrain_map(t, which);
    void* mem = const_cast<uint8_t*>(tex.base);
    if (which == 0) hipLaunchKernelGGL(k_stamp<kStampR8>, tiles_32x8(r), dim3(256), 0, s, mem, tex.w0, tex.h0, r, (const void*)st->d_texels, k);
    else hipLaunchKernelGGL(k_stamp<kStampSrgba8>, tiles_32x8(r), dim3(256), 0, s, mem, tex.w0, tex.h0, r, (const void*)st->d_texels, k);
}

extern "C" VR_API int vr_terrain_stamp(vr_terrain* t, int which, vr_stamp* st, const vr_stamp_params* p, int32_t out_rect[4])
{
    static_assert(sizeof(vr_stamp_params) == 64, "vr_stamp_params layout");
    static_assert(VR_STAMP_BLEND == kStampBlend && VR_STAMP_ADD == kStampAdd && VR_STAMP_SUB == kStampSub && VR_STAMP_MAX == kStampMax && VR_STAMP_MIN == kStampMin,
                  "vr_stamp.h's ops");
    static_assert(VR_STAMP_USE_ALPHA == (int)kStampUseAlpha, "vr_stamp.h's flag");
    // the argument checks come before any use of the device (and leave the terrain and the stamp alone)
    VR_REQUIRE(t != nullptr, "terrain is NULL");
    VR_REQUIRE(st != nullptr, "stamp is NULL");
    VR_REQUIRE(p != nullptr, "params is NULL");
    VR_REQUIRE(which == 0 || which == 1, "which must be 0 (heightmap) or 1 (albedo)");
    VR_REQUIRE(st->format == which, "the stamp's format is not the map's");
    VR_REQUIRE(st->ctx == t->ctx, "the stamp belongs to another context");
    const float f[9] = { p->x, p->z, p->size_x, p->size_z, p->rotation, p->opacity, p->feather, p->gain, p->offset };
    for (float v : f) VR_REQUIRE(host_finite(v), "params holds a NaN or an infinity");
    VR_REQUIRE(p->size_x > 0.0f && p->size_z > 0.0f, "size must be positive");
    VR_REQUIRE(p->opacity >= 0.0f && p->opacity <= 1.0f, "opacity outside [0, 1]");
    VR_REQUIRE(p->feather >= 0.0f && p->feather <= 1.0f, "feather outside [0, 1]");
    VR_REQUIRE(fabsf(p->gain) <= 256.0f, "|gain| above 256");
    VR_REQUIRE(fabsf(p->offset) <= 255.0f, "|offset| above 255");
    VR_REQUIRE(p->op >= VR_STAMP_BLEND && p->op <= VR_STAMP_MIN, "unknown op");
    VR_REQUIRE((p->flags & ~(uint32_t)VR_STAMP_USE_ALPHA) == 0, "unknown flag bits");
    VR_REQUIRE(which == 1 || (p->flags & VR_STAMP_USE_ALPHA) == 0, "VR_STAMP_USE_ALPHA needs an SRGBA8 stamp");
    VR_REQUIRE(p->channel_mask >= 1u && p->channel_mask <= 15u, "channel_mask must be 1 .. 15");
    VR_REQUIRE(which == 1 || p->channel_mask == 1u, "an R8 map has channel_mask 1");
    for (int i = 0; i < 4; i++) VR_REQUIRE(p->reserved[i] == 0, "reserved must be zero");
    const DevTex& tex = vr_terrain_map(t, which);
    StampDesc d;
    d.x = p->x; d.z = p->z; d.size_x = p->size_x; d.size_z = p->size_z; d.rotation = p->rotation; d.opacity = p->opacity; d.feather = p->feather;
    d.gain = p->gain; d.offset = p->offset; d.op = p->op; d.channel_mask = p->channel_mask; d.flags = p->flags;
    DirtyRect dirty;
    const StampConst k = stamp_prepare(d, t->p.world_size, tex.w0, tex.h0, st->w, st->h, &dirty);
    // a stamp that misses the map launches nothing; the call needs no memory beyond the history's own record
    return vr_level0_call(t, which, dirty, out_rect, [&](hipStream_t s) -> int {
        { const int orc = order_side_begin(st->ord, VrOrderOps(), s); if (orc) return orc; }
        stamp_launch(t, which, s, dirty, st, k);
        VR_HIP(hipGetLastError());
        return order_side_end(st->ord, VrOrderOps(), s);
    });
}
