// Everything the library derives from a terrain's two maps - the mip chain, the decoded tables, the node heights, the query
// pyramid - is built HERE, inside a rectangle of level 0, and nowhere else.  Two callers:
//
//   create   vr_tex_upload_and_mip, vr_node_heights_surface, the first ray cast's pyramid: the rectangle is the whole map
//   edit     vr_terrain_edit (below): a sub-rectangle of level 0 is replaced in place and everything is brought up to date inside
//            the dirty rectangle of each structure, so that the terrain is the one vr_terrain_create builds from the edited arrays
//   write    every other writer of level 0 (brush, erosion, texture, stamp, noise: vr_level0.h; undo and redo: vr_history.hip): a
//            kernel rewrites texels inside a rectangle; the same refresh follows.  They share vr_derive_level0_write: the waits
//            in front of the write, the write itself (the caller's), the chain and the tables, the node heights, the pyramid, the
//            order mark behind.
//
// Every rectangle comes from vr_dirty.h (the whole map dirties the whole of every structure: tests/host/dirty_check.cpp); every
// element is computed by the expressions of vr_terrain_dev.h.  Grids are sized from the rectangle, never from the map.
//
//   level 0           k_derive_copy        edit only: one strided copy out of the caller's device memory (or the staging copy of its host memory)
//   levels 1 ..       k_derive_mip_*       one launch per level (a level reads the one below)                             vr_derive_chain
//   tables            k_derive_tables_*    ONE launch per texture: the per-level descriptors travel by value, a workgroup    "
//                                          finds its level by its index
//   node heights      k_derive_minmax_*    leaf nodes that meet the rectangle, then their ancestors, per surface           vr_derive_node_heights
//                                          (timed as VR_K_NODE_HEIGHTS); a surface off the mip-style path runs its whole
//                                          reduction (vr_select.hip), on an edit again
//   query pyramid     k_derive_pyramid_*   once a ray cast asks for it (timed as VR_K_QUERY_PYRAMID)                       vr_derive_pyramid
#include "vr_level0.h"
#include "vr_terrain_dev.h"
#include "vr_packed.h"

template <class T>
__global__ __launch_bounds__(256) void k_derive_copy(const uint8_t* __restrict__ src, size_t src_pitch, T* __restrict__ dst, int dst_w, DirtyRect r)
{
    const int x = brush_tile_x(r.x0) + brush_lane_x(), y = brush_tile_y(r.y0) + brush_lane_y();
    if (x >= r.x1 || y >= r.y1) return;
    dst[(size_t)y * dst_w + x] = reinterpret_cast<const T*>(src + (size_t)(y - r.y0) * src_pitch)[x - r.x0];
}

__global__ __launch_bounds__(256) void k_derive_mip_r8(const uint8_t* __restrict__ src, int sw, int sh, uint8_t* __restrict__ dst, int dw, DirtyRect r)
{
    const int x = brush_tile_x(r.x0) + brush_lane_x(), y = brush_tile_y(r.y0) + brush_lane_y();
    if (x >= r.x1 || y >= r.y1) return;
    vr_mip_r8_texel(src, sw, sh, dst, dw, x, y);
}
__global__ __launch_bounds__(256) void k_derive_mip_srgba8(const uint32_t* __restrict__ src, int sw, int sh, uint32_t* __restrict__ dst, int dw, DirtyRect r,
                                                            const float* __restrict__ lut_g, const float* __restrict__ thr_g)
{
    __shared__ float lut[256];
    __shared__ float thr[256];
    lut[threadIdx.x] = lut_g[threadIdx.x]; thr[threadIdx.x] = thr_g[threadIdx.x];
    __syncthreads();
    const int x = brush_tile_x(r.x0) + brush_lane_x(), y = brush_tile_y(r.y0) + brush_lane_y();
    if (x >= r.x1 || y >= r.y1) return;
    vr_mip_srgba8_texel(src, sw, sh, dst, dw, x, y, lut, thr);
}

// One level's share of the tables launch.  `entries`: the dirty entries of the level's fast table - of an SRGBA8 map: of its pack
// table, which has the same indexing and whose span holds fast's (one entry more in front; that one is rewritten with what it held)
// - which the workgroups tile (32 x 8 each, `blocks_x` per row, the level's first is `first_block`).  `inner`: R8 - the dirty entries of quad / quadf (same
// indexing, one entry less per side); SRGBA8 - the dirty texels of the chain, for rgbf (entry (ix, iy) is texel (ix-1, iy-1)).
struct DeriveLevel {
    uint32_t chain_off;        // bytes into the chain
    uint32_t quad_off;         // entries into quad / quadf
    uint32_t fast_off;         // entries into fast
    int w, h;
    DirtyRect entries, inner;
    uint32_t first_block; int blocks_x;
};
struct DeriveTables { DeriveLevel lv[kMaxLevels]; int levels; };

__device__ __forceinline__ bool derive_tables_entry(const DeriveTables& d, int& l, int& ix, int& iy)
{
    l = 0;
    while (l + 1 < d.levels && blockIdx.x >= d.lv[l + 1].first_block) l++;
    const uint32_t b = blockIdx.x - d.lv[l].first_block;
    // (tiles_32x8's tiles of the level's entries, the workgroups of all levels numbered in one row: not blockIdx's tile)
    ix = d.lv[l].entries.x0 + (int)(b % (uint32_t)d.lv[l].blocks_x) * kBrushTileW + (int)(threadIdx.x % kBrushTileW);
    iy = d.lv[l].entries.y0 + (int)(b / (uint32_t)d.lv[l].blocks_x) * kBrushTileH + (int)(threadIdx.x / kBrushTileW);
    return ix < d.lv[l].entries.x1 && iy < d.lv[l].entries.y1;
}
__global__ __launch_bounds__(256) void k_derive_tables_r8(DeriveTables d, const uint8_t* __restrict__ chain, uint32_t* __restrict__ quad,
                                                           float4* __restrict__ quadf, float4* __restrict__ fast)
{
    int l, ix, iy;
    if (!derive_tables_entry(d, l, ix, iy)) return;
    const DeriveLevel& e = d.lv[l];
    const uint8_t* src = chain + e.chain_off;
    vr_footprint_entry(src, e.w, e.h, fast + e.fast_off, e.w + 3, ix, iy);
    if (ix >= e.inner.x0 && ix < e.inner.x1 && iy >= e.inner.y0 && iy < e.inner.y1) {
        vr_quad_entry(src, e.w, e.h, quad + e.quad_off, ix, iy);
        vr_footprint_entry(src, e.w, e.h, quadf + e.quad_off, e.w + 2, ix, iy);
    }
}
// (rgbf holds a float4 per dword of the chain, the padding between two 256-byte-aligned levels included; only texels are ever
// decoded, and the tile pass - its one reader - clamps every index into its level)
__global__ __launch_bounds__(256) void k_derive_tables_srgba8(DeriveTables d, const uint8_t* __restrict__ chain, const float* __restrict__ lut,
                                                               float4* __restrict__ fast, float* __restrict__ rgbf, uint4* __restrict__ pack)
{
    int l, ix, iy;
    if (!derive_tables_entry(d, l, ix, iy)) return;
    const DeriveLevel& e = d.lv[l];
    vr_fast_srgba8_entry((const uint32_t*)(chain + e.chain_off), e.w, e.h, lut, fast + e.fast_off, ix, iy);
    uint32_t pk[4];
    vr_packed_entry((const uint32_t*)(chain + e.chain_off), e.w, e.h, ix, iy, pk);
    pack[(size_t)e.fast_off + (size_t)iy * (e.w + 3) + ix] = make_uint4(pk[0], pk[1], pk[2], pk[3]);
    const int x = ix - 1, y = iy - 1;
    if (x >= e.inner.x0 && x < e.inner.x1 && y >= e.inner.y0 && y < e.inner.y1)
        vr_rgbf_texel((const uint32_t*)chain, (size_t)(e.chain_off / 4) + (size_t)y * e.w + x, lut, rgbf);
}

// nodes / cells of the rectangle `r` of one level, one lane each
__global__ __launch_bounds__(256) void k_derive_minmax_leaf(const uint8_t* __restrict__ tex, int tex_w, int rx0, int ry0, uint32_t n, int s,
                                                             uchar2* __restrict__ mm, float2* __restrict__ out, DirtyRect r)
{
    const uint32_t rw = (uint32_t)(r.x1 - r.x0), i = blockIdx.x * 256 + threadIdx.x;
    if (i >= rw * (uint32_t)(r.y1 - r.y0)) return;
    vr_minmax_leaf_node(tex, tex_w, rx0, ry0, n, s, mm, out, (uint32_t)r.x0 + i % rw, (uint32_t)r.y0 + i / rw);
}
__global__ __launch_bounds__(256) void k_derive_minmax_up(const uchar2* __restrict__ child, uint32_t n, uchar2* __restrict__ mm, float2* __restrict__ out, DirtyRect r)
{
    const uint32_t rw = (uint32_t)(r.x1 - r.x0), i = blockIdx.x * 256 + threadIdx.x;
    if (i >= rw * (uint32_t)(r.y1 - r.y0)) return;
    vr_minmax_up_node(child, n, mm, out, (uint32_t)r.x0 + i % rw, (uint32_t)r.y0 + i / rw);
}
__global__ __launch_bounds__(256) void k_derive_pyramid_leaf(DevTex hm, int cw, uchar2* __restrict__ out, DirtyRect r)
{
    const int ix = r.x0 + blockIdx.x * 64 + (threadIdx.x & 63), iz = r.y0 + blockIdx.y * 4 + (threadIdx.x >> 6);
    if (ix >= r.x1 || iz >= r.y1) return;
    vr_pyramid_leaf_cell(hm, cw, out, ix, iz);
}
__global__ __launch_bounds__(256) void k_derive_pyramid_up(const uchar2* __restrict__ child, int cw, int ch, uchar2* __restrict__ parent, int pw, DirtyRect r)
{
    const int px = r.x0 + blockIdx.x * 64 + (threadIdx.x & 63), pz = r.y0 + blockIdx.y * 4 + (threadIdx.x >> 6);
    if (px >= r.x1 || pz >= r.y1) return;
    vr_pyramid_up_cell(child, cw, ch, parent, pw, px, pz);
}

// ---------------------------------------------------------------------------------------
// host side: the three functions queue launches on the context's stream and report nothing; whoever calls them asks
// hipGetLastError afterwards
// ---------------------------------------------------------------------------------------
static dim3 tiles_64x4(const DirtyRect& r) { return dim3((unsigned)((r.x1 - r.x0 + 63) / 64), (unsigned)((r.y1 - r.y0 + 3) / 4)); }
// one lane per node: at most 4^num_lods / 256 workgroups, 65536 at VR_MAX_LODS - far below the 2^31 - 1 a grid's x may hold
static unsigned blocks_of(const DirtyRect& r) { return (unsigned)(((uint64_t)(r.x1 - r.x0) * (uint64_t)(r.y1 - r.y0) + 255) / 256); }

void vr_derive_chain(vr_context* ctx, uint8_t* mem, const TexLayout& lay, int w0, int h0, int levels, int texel_bytes, const DirtyRect& dirty)
{
    hipStream_t s = ctx->stream;
    const bool r8 = texel_bytes == 1;
    DirtyRect chain[kMaxLevels];
    chain[0] = dirty;
    for (int l = 1; l < levels; l++)
        chain[l] = dirty_rect(dirty_mip_next(dirty_x(chain[l - 1]), dirty_level_size(w0, l)), dirty_mip_next(dirty_y(chain[l - 1]), dirty_level_size(h0, l)));
    DeriveTables dt; memset(&dt, 0, sizeof(dt));
    dt.levels = levels;
    uint32_t blocks = 0;
    for (int l = 0; l < levels; l++) {
        DeriveLevel& e = dt.lv[l];
        const int lw = dirty_level_size(w0, l), lh = dirty_level_size(h0, l);
        e.chain_off = lay.off[l]; e.quad_off = lay.qoff[l]; e.fast_off = lay.fast_entry[l]; e.w = lw; e.h = lh;
        const DirtySpan cx = dirty_x(chain[l]), cy = dirty_y(chain[l]);
        if (r8) {
            e.entries = dirty_rect(dirty_fast_r8_entries(cx, lw), dirty_fast_r8_entries(cy, lh));
            e.inner = dirty_rect(dirty_quad_entries(cx, lw), dirty_quad_entries(cy, lh));
        } else {
            e.entries = dirty_rect(dirty_pack_srgba8_entries(cx, lw), dirty_pack_srgba8_entries(cy, lh));
            e.inner = chain[l];
        }
        e.first_block = blocks;
        if (dirty_empty(chain[l])) { e.entries = DirtyRect(); e.inner = DirtyRect(); e.blocks_x = 1; continue; }
        const dim3 g = tiles_32x8(e.entries);
        e.blocks_x = (int)g.x;
        blocks += g.x * g.y;
    }
    for (int l = 1; l < levels && !dirty_empty(chain[l]); l++) {
        const int sw = dirty_level_size(w0, l - 1), sh = dirty_level_size(h0, l - 1), dw = dirty_level_size(w0, l);
        if (r8) hipLaunchKernelGGL(k_derive_mip_r8, tiles_32x8(chain[l]), dim3(256), 0, s, mem + lay.off[l - 1], sw, sh, mem + lay.off[l], dw, chain[l]);
        else hipLaunchKernelGGL(k_derive_mip_srgba8, tiles_32x8(chain[l]), dim3(256), 0, s, (const uint32_t*)(mem + lay.off[l - 1]), sw, sh,
                                (uint32_t*)(mem + lay.off[l]), dw, chain[l], ctx->d_srgb_lut, ctx->d_srgb_thr);
    }
    if (r8) hipLaunchKernelGGL(k_derive_tables_r8, dim3(blocks), dim3(256), 0, s, dt, mem, (uint32_t*)(mem + lay.quad_at), (float4*)(mem + lay.quadf_at),
                               (float4*)(mem + lay.fast_at));
    else hipLaunchKernelGGL(k_derive_tables_srgba8, dim3(blocks), dim3(256), 0, s, dt, mem, ctx->d_srgb_lut, (float4*)(mem + lay.fast_at), (float*)(mem + lay.rgbf_at),
                            (uint4*)(mem + lay.pack_at));
}

void vr_derive_node_heights(vr_terrain* t, int surf, const NodeSurface& ns, const DirtyRect& dirty)
{
    hipStream_t s = t->ctx->stream;
    const uint64_t nodes = ((((uint64_t)1 << (2 * (t->num_lods + 1))) - 1) / 3);
    float2* out = t->d_node_heights + (size_t)surf * nodes;
    uchar2* mm = t->d_minmax + (size_t)surf * nodes;
    DirtySpan x = dirty_leaf_nodes(dirty_x(dirty), ns.rx0, ns.leaf, 1 << t->num_lods), y = dirty_leaf_nodes(dirty_y(dirty), ns.ry0, ns.leaf, 1 << t->num_lods);
    for (int d = t->num_lods; d >= 0 && !dirty_empty(x) && !dirty_empty(y); d--) {
        const uint32_t n = 1u << d;
        const uint64_t base = ((((uint64_t)1 << (2 * d)) - 1) / 3);
        const DirtyRect r = dirty_rect(x, y);
        if (d == t->num_lods)
            hipLaunchKernelGGL(k_derive_minmax_leaf, dim3(blocks_of(r)), dim3(256), 0, s, (const uint8_t*)t->d_height, t->height.w0, ns.rx0, ns.ry0, n, ns.leaf,
                               mm + base, out + base, r);
        else
            hipLaunchKernelGGL(k_derive_minmax_up, dim3(blocks_of(r)), dim3(256), 0, s, (const uchar2*)(mm + ((((uint64_t)1 << (2 * (d + 1))) - 1) / 3)), n,
                               mm + base, out + base, r);
        x = dirty_node_parents(x); y = dirty_node_parents(y);
    }
}

void vr_derive_pyramid(const DevTex& hm, const PyrDesc& pd, uchar2* pyramid, const DirtyRect& l0, const DirtyRect& l1, hipStream_t s)
{
    const int lv1 = hm.levels > 1 ? 1 : 0;
    const DirtyRect leaf = dirty_pyramid_leaf_cells(l0, l1, hm.w0, hm.h0, dirty_level_size(hm.w0, lv1), dirty_level_size(hm.h0, lv1));
    DirtySpan x = dirty_x(leaf), y = dirty_y(leaf);
    int cw = pd.cw, ch = pd.ch;                  // cells of the level being written
    for (int l = 0; l < pd.levels && !dirty_empty(x) && !dirty_empty(y); l++) {
        const DirtyRect r = dirty_rect(x, y);
        if (l == 0) hipLaunchKernelGGL(k_derive_pyramid_leaf, tiles_64x4(r), dim3(256), 0, s, hm, cw, pyramid, r);
        else {
            const int pw = (cw + 1) / 2, ph = (ch + 1) / 2;
            hipLaunchKernelGGL(k_derive_pyramid_up, tiles_64x4(r), dim3(256), 0, s, (const uchar2*)(pyramid + pd.off[l - 1]), cw, ch, pyramid + pd.off[l], pw, r);
            cw = pw; ch = ph;
        }
        x = dirty_pyramid_parents(x, (cw + 1) / 2); y = dirty_pyramid_parents(y, (ch + 1) / 2);
    }
}

int vr_derive_level0_write(vr_terrain* t, int which, const DirtyRect& dirty, const std::function<int(hipStream_t)>& write_level0)
{
    vr_context* ctx = t->ctx;
    hipStream_t s = ctx->stream;
    const DevTex& tex = vr_terrain_map(t, which);
    const TexLayout& lay = vr_terrain_layout(t, which);
    // a frame recorded for a target's pending colour planes draws the map as it is now
    { const int rc = vr_terrain_materialise_pending(t); if (rc) return rc; }
    // before the first write: behind every chain queued so far (its vertex stage reads the heightmap) and behind every tile pass
    // (it reads the tables, and the host may have changed the context's stream since it was queued)
    static_assert(kGeoSets == 3, "the list below");
    VrOrderSet* const ord_sets[kGeoSets] = { &t->sets[0].ord, &t->sets[1].ord, &t->sets[2].ord };
    { const int rc = order_terrain_changing(ord_sets, VrOrderOps(), s); if (rc) return rc; }
    { const int rc = order_terrain_tables_changing(ord_sets, VrOrderOps(), s, ctx->events); if (rc) return rc; }
    // geometry built from the old map is stale, whichever map it was (one rule); selections and lock_view stay as they are
    geoslots_invalidate(t->slots);

    { const int rc = write_level0(s); if (rc) return rc; }
    vr_derive_chain(ctx, const_cast<uint8_t*>(tex.base), lay, tex.w0, tex.h0, tex.levels, which == 0 ? 1 : 4, dirty);
    VR_HIP(hipGetLastError());
    if (which == 0 && t->height_loaded && t->d_node_heights) {
        VrKernelScope ks(ctx, VR_K_NODE_HEIGHTS, ctx->stream);
        for (int surf = 0; surf < t->surfaces_per_side * t->surfaces_per_side; surf++) {
            const NodeSurface ns = vr_node_surface(t, surf);
            if (ns.dyadic) vr_derive_node_heights(t, surf, ns, dirty);
            else vr_node_heights_surface(t, surf, ns);     // rare; its rectangles come from float arithmetic not worth inverting
        }
        VR_HIP(hipGetLastError());
    }
    if (which == 0 && t->d_pyramid) {                       // a ray cast has built it
        { const int rc = order_side_begin(t->ord_pyramid, VrOrderOps(), s); if (rc) return rc; }
        const DirtyRect l1 = tex.levels > 1 ? dirty_rect(dirty_mip_next(dirty_x(dirty), dirty_level_size(tex.w0, 1)), dirty_mip_next(dirty_y(dirty), dirty_level_size(tex.h0, 1)))
                                            : dirty;
        {
            VrKernelScope ks(ctx, VR_K_QUERY_PYRAMID, ctx->stream);
            vr_derive_pyramid(tex, vr_pyramid_desc(t, nullptr), t->d_pyramid, dirty, l1, s);
        }
        VR_HIP(hipGetLastError());
        { const int rc = order_side_end(t->ord_pyramid, VrOrderOps(), s); if (rc) return rc; }
    }
    // every set's next chain runs behind the write
    { const int rc = order_terrain_changed(t->ord, ord_sets, VrOrderOps(), s); if (rc) return rc; }
    return VR_OK;
}

extern "C" VR_API int vr_terrain_edit(vr_terrain* t, int which, int32_t x, int32_t y, int32_t w, int32_t h,
                                       const void* texels, size_t row_pitch_bytes, int device_pointer)
{
    // the argument checks come before any use of the device (and leave the terrain alone)
    VR_REQUIRE(t != nullptr, "terrain is NULL");
    VR_REQUIRE(which == 0 || which == 1, "which must be 0 (heightmap) or 1 (albedo)");
    VR_REQUIRE(x >= 0 && y >= 0 && w >= 0 && h >= 0, "negative coordinate or extent");
    const DevTex& tex = vr_terrain_map(t, which);
    const size_t tb = which == 0 ? 1 : 4;
    VR_REQUIRE((int64_t)x + w <= tex.w0 && (int64_t)y + h <= tex.h0, "the rectangle is not inside level 0");
    if (w == 0 || h == 0) return VR_OK;
    VR_REQUIRE(texels != nullptr, "texels is NULL");
    VR_REQUIRE(row_pitch_bytes == 0 || row_pitch_bytes >= (size_t)w * tb, "row pitch smaller than a row");
    VR_REQUIRE(!device_pointer || (((uintptr_t)texels | row_pitch_bytes) & (tb - 1)) == 0, "device pointer and pitch must be aligned to the texel size");
    const size_t row = (size_t)w * tb, pitch = row_pitch_bytes ? row_pitch_bytes : row;
    VR_HIP(hipSetDevice(t->ctx->device));
    // staging of the host-pointer mode: reserved before anything is launched (a refusal leaves the terrain as it was)
    const uint8_t* src = (const uint8_t*)texels; size_t src_pitch = pitch;
    if (!device_pointer) {
        const int rc = vr_query_reserve_stage(t, row * (size_t)h);
        if (rc) return rc;
        src = (const uint8_t*)t->d_query_stage; src_pitch = row;
    }
    DirtyRect dirty; dirty.x0 = x; dirty.y0 = y; dirty.x1 = x + w; dirty.y1 = y + h;
    uint8_t* mem = const_cast<uint8_t*>(tex.base);
    // the host's texels into the staging memory, then one strided copy into level 0; everything else is the shared path
    const int rc = vr_level0_call(t, which, dirty, nullptr, [&](hipStream_t st) -> int {
        if (!device_pointer) {
            if (pitch == row) VR_HIP(hipMemcpyAsync(t->d_query_stage, texels, row * (size_t)h, hipMemcpyHostToDevice, st));
            else VR_HIP(hipMemcpy2DAsync(t->d_query_stage, row, texels, pitch, row, (size_t)h, hipMemcpyHostToDevice, st));
        }
        if (which == 0) hipLaunchKernelGGL(k_derive_copy<uint8_t>, tiles_32x8(dirty), dim3(256), 0, st, src, src_pitch, mem, tex.w0, dirty);
        else hipLaunchKernelGGL(k_derive_copy<uint32_t>, tiles_32x8(dirty), dim3(256), 0, st, src, src_pitch, (uint32_t*)mem, tex.w0, dirty);
        return VR_OK;
    });
    if (rc) return rc;
    if (!device_pointer) VR_HIP(hipStreamSynchronize(t->ctx->stream));      // the caller's host memory has been consumed
    return VR_OK;
}

// One level of one decoded table as it is on the device, densely packed as the kernels above lay it out: `cols` entries per row,
// `rows` rows, from the offsets of the terrain's own TexLayout (rgbf: level l begins at float4 off[l] / 4; the 256-byte padding
// between two levels is never decoded and never shown).  No kernel, and nothing is built.  The copy is a reader of the map's tables
// on the context's stream with no wait of its own, as a tile pass's and a height query's reads of them are (vr_order.h orders the
// maps' writers against the geometry chains and the tile passes of other streams; on the context's stream the stream orders a
// reader behind the writer, and across vr_context_set_stream the host's obligation does), and the entry returns when it has completed.
extern "C" VR_API int vr_debug_terrain_tables(vr_terrain* t, int which, int table, int32_t level, int32_t out_dims[2], void* out, size_t capacity_bytes)
{
    VR_REQUIRE(t != nullptr, "terrain is NULL");
    VR_REQUIRE(which == 0 || which == 1, "which must be 0 (heightmap) or 1 (albedo)");
    VR_REQUIRE(table == VR_DEBUG_TABLE_QUAD || table == VR_DEBUG_TABLE_QUADF || table == VR_DEBUG_TABLE_FAST || table == VR_DEBUG_TABLE_RGBF
               || table == VR_DEBUG_TABLE_PACK, "unknown table");
    VR_REQUIRE(level >= 0, "negative level");
    VR_REQUIRE(out_dims != nullptr, "out_dims is NULL");
    const DevTex& tex = vr_terrain_map(t, which);
    const TexLayout& lay = vr_terrain_layout(t, which);
    const bool has = table == VR_DEBUG_TABLE_FAST || (table == VR_DEBUG_TABLE_RGBF || table == VR_DEBUG_TABLE_PACK ? which == 1 : which == 0);
    int cols = 0, rows = 0;
    size_t at = 0, entry = 16;
    if (has && tex.base != nullptr && level < tex.levels) {
        const int lw = dirty_level_size(tex.w0, level), lh = dirty_level_size(tex.h0, level);
        if (table == VR_DEBUG_TABLE_QUAD) { cols = lw + 2; rows = lh + 2; entry = 4; at = lay.quad_at + (size_t)lay.qoff[level] * 4; }
        else if (table == VR_DEBUG_TABLE_QUADF) { cols = lw + 2; rows = lh + 2; at = lay.quadf_at + (size_t)lay.qoff[level] * 16; }
        else if (table == VR_DEBUG_TABLE_FAST) { cols = lw + 3; rows = lh + 3; at = lay.fast_at + (size_t)lay.fast_entry[level] * 16; }
        else if (table == VR_DEBUG_TABLE_PACK) { cols = lw + 3; rows = lh + 3; at = lay.pack_at + (size_t)lay.fast_entry[level] * 16; }
        else { cols = lw; rows = lh; at = lay.rgbf_at + (size_t)(lay.off[level] / 4) * 16; }
    }
    const size_t bytes = (size_t)cols * (size_t)rows * entry;
    if (!(out == nullptr && capacity_bytes == 0)) {
        VR_REQUIRE(out != nullptr, "out is NULL with a capacity");
        VR_REQUIRE(capacity_bytes >= bytes, "capacity below the level's entries");
    }
    out_dims[0] = cols; out_dims[1] = rows;
    if (out == nullptr || bytes == 0) return VR_OK;
    VR_HIP(hipSetDevice(t->ctx->device));
    hipStream_t s = t->ctx->stream;
    VR_HIP(hipMemcpyAsync(out, tex.base + at, bytes, hipMemcpyDeviceToHost, s));
    VR_HIP(hipStreamSynchronize(s));
    return VR_OK;
}
