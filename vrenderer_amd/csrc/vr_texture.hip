// vr_terrain_texture: level 0 of the albedo painted by rule from the heightmap's shape - altitude and slope layers under a brush mask
// or over the whole map - by one kernel, through vr_mask_call (vr_level0.h).  The definition, texel by texel, is vr_texture.h; this
// file holds nothing of it but where the height bytes come from.
//
//   k_texture<STAGED, WHOLE>   the tile frame of vr_brush_dev.h over the albedo rectangle; the mask is its brush_tile_mask's, and WHOLE
//                              has mask 1 on every texel, walks no list and takes no dab buffer.  The prepared layers (at most 8)
//                              and the call's four constants are one kernel argument: wave-uniform, read by scalar loads.
//                              A texel reads a 4 x 4 footprint of height bytes through HeightFetch.  STAGED: the tile's footprint
//                              - at most (ceil(32 rx) + 4) x (ceil(8 rz) + 4) bytes, origin one texel left of and above the first
//                              texel's sample point, clamped at the map's edge - is loaded into LDS once, row by row by consecutive
//                              lanes; the host chooses it where that is at most 4 KiB.  Otherwise (a heightmap much finer than the
//                              albedo: the lanes' footprints hardly overlap) the lanes read memory directly.  The arithmetic is one
//                              body and the bytes are the same.  Every index is clamped before it addresses memory; a lane with
//                              mask 0 stores nothing.
//
// The kernel is untimed, like the brush kernel.
#include "vr_level0.h"
#include "vr_texture.h"

constexpr int kTextureFootBytes = 4096;

// the byte of height texel (x, y), inside the map
template <bool STAGED> struct HeightFetch;
template <> struct HeightFetch<false> {
    const uint8_t* __restrict__ height; int w0;
    __host__ __device__ __forceinline__ int operator()(int x, int y) const { return (int)height[(size_t)y * (size_t)w0 + (size_t)x]; }
};
template <> struct HeightFetch<true> {
    const uint8_t* foot; int ox, oy, fw, fh;         // LDS: texel (ox + lx, oy + ly), clamped to the map, at [ly * fw + lx]
    // The clamp into the footprint is for memory safety alone and never binds: a tile's sample columns span i0(tx0) ..
    // i0(tx0 + 31) <= i0(tx0) + floor(31 rx) + 1 (clamping fx only contracts), a texel reads one column either side of i0 and
    // i1 = i0 + 1, and floor(31 rx) + 1 <= ceil(32 rx) for every rx > 0 - so lx <= ceil(32 rx) + 3 = fw - 1; rows likewise with 7
    // and 8.  Were the tile size or the origin changed without fw and fh, it would give wrong bytes, not a fault: the byte-exact
    // tests are the check.
    __host__ __device__ __forceinline__ int operator()(int x, int y) const
    {
        const int lx = texture_clampi(x - ox, 0, fw - 1), ly = texture_clampi(y - oy, 0, fh - 1);
        return (int)foot[ly * fw + lx];
    }
};

// `albedo`: level 0, wa x ha; `height`: level 0, w0 x h0; `r`: the call's rectangle, inside the albedo; `dabs`: n of them, prepared for
// the albedo, none empty (WHOLE: none at all); fw x fh: the staged footprint, fw * fh <= kTextureFootBytes
template <bool STAGED, bool WHOLE>
__global__ __launch_bounds__(256) void k_texture(uchar4* __restrict__ albedo, int wa, int ha, const uint8_t* __restrict__ height, int w0, int h0, DirtyRect r,
                                                 const BrushDab* __restrict__ dabs, uint32_t n, TextureConst k, int fw, int fh)
{
    __shared__ uint8_t foot[STAGED ? kTextureFootBytes : 4];
    __shared__ uint16_t list[kBrushChunk];  // the chunk's dabs that meet this tile
    __shared__ uint32_t wave_total[4];
    const BrushTile tile = brush_tile(r);
    const int cx = tile.cx(wa), cy = tile.cy(ha);
    HeightFetch<STAGED> fetch;
    if constexpr (STAGED) {
        // the sample points grow with the texel index: the tile's first texel has the smallest i0 and j0
        int a0, a1, b0, b1; float ta, tb;
        texture_axis(brush_clampi(tile.tx0, 0, wa - 1), k.rx, w0, &a0, &a1, &ta);
        texture_axis(brush_clampi(tile.ty0, 0, ha - 1), k.rz, h0, &b0, &b1, &tb);
        const int ox = a0 - 1, oy = b0 - 1;
        const int cells = fw * fh < kTextureFootBytes ? fw * fh : kTextureFootBytes;
        for (int at = (int)threadIdx.x; at < cells; at += kBrushThreads) {
            const int ly = at / fw, lx = at - ly * fw;
            foot[at] = height[(size_t)brush_clampi(oy + ly, 0, h0 - 1) * (size_t)w0 + (size_t)brush_clampi(ox + lx, 0, w0 - 1)];
        }
        __syncthreads();
        fetch.foot = foot; fetch.ox = ox; fetch.oy = oy; fetch.fw = fw; fetch.fh = fh;
    } else {
        fetch.height = height; fetch.w0 = w0;
    }
    float m;
    if constexpr (WHOLE) m = tile.inside ? 1.0f : 0.0f;
    else m = brush_tile_mask(dabs, n, tile, list, wave_total);
    if (!(tile.inside && m > 0.0f)) return;                        // behind the last barrier
    float h, s2;
    texture_sample(k, fetch, w0, h0, cx, cy, &h, &s2);
    const size_t at = (size_t)cy * (size_t)wa + (size_t)cx;
    const uchar4 px = albedo[at];
    float val[4] = { (float)px.x, (float)px.y, (float)px.z, (float)px.w };
    texture_composite(k, h, s2, m, val);
    albedo[at] = make_uchar4(brush_byte(val[0]), brush_byte(val[1]), brush_byte(val[2]), brush_byte(val[3]));
}

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
static int texture_check_layer(const vr_texture_layer& l)
{
    const float f[11] = { l.color[0], l.color[1], l.color[2], l.color[3], l.opacity, l.alt_lo, l.alt_hi, l.alt_fade, l.slope_lo, l.slope_hi, l.slope_fade };
    for (float v : f) VR_REQUIRE(host_finite(v), "a layer holds a NaN or an infinity");
    for (int c = 0; c < 4; c++) VR_REQUIRE(l.color[c] >= 0.0f && l.color[c] <= 255.0f, "color outside [0, 255]");
    VR_REQUIRE(l.opacity >= 0.0f && l.opacity <= 1.0f, "opacity outside [0, 1]");
    VR_REQUIRE(l.alt_lo <= l.alt_hi, "alt_lo above alt_hi");
    VR_REQUIRE(l.alt_fade >= 0.0f && l.slope_fade >= 0.0f, "a negative fade");
    VR_REQUIRE(l.slope_lo >= 0.0f && l.slope_lo <= l.slope_hi && l.slope_hi <= 89.0f, "slope bounds outside 0 <= lo <= hi <= 89");
    VR_REQUIRE(l.channel_mask >= 1u && l.channel_mask <= 15u, "channel_mask must be 1 .. 15");
    for (int i = 0; i < 4; i++) VR_REQUIRE(l.reserved[i] == 0, "reserved must be zero");
    return VR_OK;
}

// k_texture over the rectangle `r` on `s`; dabs == nullptr: the whole-map variant
static void texture_launch(vr_terrain* t, hipStream_t s, const DirtyRect& r, const BrushDab* dabs, uint32_t nd, const TextureConst& k)
{
    const DevTex& hm = t->height; const DevTex& al = t->albedo;
    const int fw = (int)ceil((double)kBrushTileW * (double)k.rx) + 4, fh = (int)ceil((double)kBrushTileH * (double)k.rz) + 4;
    const bool staged = (int64_t)fw * (int64_t)fh <= kTextureFootBytes;
    uchar4* mem = (uchar4*)const_cast<uint8_t*>(al.base);
    const dim3 grid = tiles_32x8(r);
    if (dabs) {
        if (staged) hipLaunchKernelGGL((k_texture<true, false>), grid, dim3(256), 0, s, mem, al.w0, al.h0, hm.base, hm.w0, hm.h0, r, dabs, nd, k, fw, fh);
        else hipLaunchKernelGGL((k_texture<false, false>), grid, dim3(256), 0, s, mem, al.w0, al.h0, hm.base, hm.w0, hm.h0, r, dabs, nd, k, 0, 0);
    } else {
        if (staged) hipLaunchKernelGGL((k_texture<true, true>), grid, dim3(256), 0, s, mem, al.w0, al.h0, hm.base, hm.w0, hm.h0, r, dabs, 0u, k, fw, fh);
        else hipLaunchKernelGGL((k_texture<false, true>), grid, dim3(256), 0, s, mem, al.w0, al.h0, hm.base, hm.w0, hm.h0, r, dabs, 0u, k, 0, 0);
    }
}

extern "C" VR_API int vr_terrain_texture(vr_terrain* t, const vr_texture_params* p, const vr_texture_layer* layers, const vr_brush_dab* dabs, uint32_t n, int32_t out_rect[4])
{
    static_assert(sizeof(vr_texture_layer) == 64 && sizeof(vr_texture_params) == 32, "vr_texture_layer / vr_texture_params layout");
    static_assert(VR_TEXTURE_MAX_LAYERS == kTextureMaxLayers, "vr_texture.h's limit");
    // the argument checks come before any use of the device (and leave the terrain alone)
    VR_REQUIRE(t != nullptr, "terrain is NULL");
    VR_REQUIRE(p != nullptr, "params is NULL");
    VR_REQUIRE(layers != nullptr, "layers is NULL");
    VR_REQUIRE(p->num_layers >= 1 && p->num_layers <= VR_TEXTURE_MAX_LAYERS, "num_layers outside 1 .. VR_TEXTURE_MAX_LAYERS");
    VR_REQUIRE((p->flags & ~(uint32_t)VR_TEXTURE_WHOLE_MAP) == 0, "unknown flag bits");
    const bool whole = (p->flags & VR_TEXTURE_WHOLE_MAP) != 0;
    VR_REQUIRE(!whole || (dabs == nullptr && n == 0), "VR_TEXTURE_WHOLE_MAP takes no dabs");
    VR_REQUIRE(dabs != nullptr || n == 0, "dabs is NULL with n > 0");
    VR_REQUIRE(n <= VR_MAX_BRUSH_DABS, "more than VR_MAX_BRUSH_DABS dabs");
    for (int i = 0; i < 5; i++) VR_REQUIRE(p->reserved[i] == 0, "reserved must be zero");
    VR_REQUIRE(host_finite(p->max_height) && p->max_height > 0.0f, "max_height must be finite and positive");
    TextureLayerDesc desc[kTextureMaxLayers];
    for (int i = 0; i < p->num_layers; i++) {
        const vr_texture_layer& l = layers[i];
        { const int rc = texture_check_layer(l); if (rc) return rc; }
        TextureLayerDesc& d = desc[i];
        for (int c = 0; c < 4; c++) d.color[c] = l.color[c];
        d.opacity = l.opacity; d.alt_lo = l.alt_lo; d.alt_hi = l.alt_hi; d.alt_fade = l.alt_fade;
        d.slope_lo = l.slope_lo; d.slope_hi = l.slope_hi; d.slope_fade = l.slope_fade; d.channel_mask = l.channel_mask;
    }
    if (!whole) { const int rc = vr_brush_check_dabs(dabs, n, VR_BRUSH_FLATTEN); if (rc) return rc; }       // strength is an opacity
    // the layer list is consumed here, on the host: the kernel takes the prepared layers by value
    const TextureConst k = texture_prepare(desc, p->num_layers, p->max_height, t->p.world_size, t->height.w0, t->height.h0, t->albedo.w0, t->albedo.h0);
    return vr_mask_call(t, 1, whole, dabs, n, out_rect, [&](hipStream_t s, const DirtyRect& dirty, const BrushDab* d_dabs, uint32_t nd) -> int {
        texture_launch(t, s, dirty, d_dabs, nd, k);
        return VR_OK;
    });
}
