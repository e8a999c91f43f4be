// vr_terrain_noise: fractal value or gradient noise added to or blended into level 0 of a map - under a brush mask or over the whole
// map - by one kernel, through vr_mask_call (vr_level0.h).  The definition, texel by texel, is vr_noise.h; this file holds nothing of it.
//
//   k_noise<T, WHOLE>   T = uint8_t (the heightmap) or uchar4 (the albedo).  The tile frame of vr_brush_dev.h; the mask is its
//                       brush_tile_mask's, and WHOLE has mask 1 on every texel, walks no list and takes no dab buffer.  The
//                       prepared per-octave constants are one kernel argument: wave-uniform, read by scalar loads.  The octave
//                       loop is bounded by the constant 12 and left at the call's count; basis and fractal are uniform branches.
//                       A lane with mask 0 stores nothing.  The cost is arithmetic - octaves x four lattice hashes per
//                       texel - and no texel reads any memory but its own byte.
//                       A variant for the whole R8 map with four texels per lane, one dword load and store, was measured against
//                       this kernel and not kept (profiles/terrain_noise_variants.txt).
//
// The kernel is untimed, like the brush kernel.
#include "vr_level0.h"
#include "vr_noise.h"

// `map`: level 0 of the map, w0 x h0; `r`: the call's rectangle, inside the map; `dabs`: n of them, prepared for the map, none empty
// (WHOLE: none at all)
template <class T, bool WHOLE>
__global__ __launch_bounds__(256) void k_noise(T* __restrict__ map, int w0, int h0, DirtyRect r, const BrushDab* __restrict__ dabs, uint32_t n, NoiseConst k)
{
    __shared__ uint16_t list[kBrushChunk];  // the chunk's dabs that meet this tile
    __shared__ uint32_t wave_total[4];
    const BrushTile tile = brush_tile(r);
    const int cx = tile.cx(w0), cy = tile.cy(h0);
    float m;
    if constexpr (WHOLE) m = tile.inside ? 1.0f : 0.0f;
    else m = brush_tile_mask(dabs, n, tile, list, wave_total);
    if (!(tile.inside && m > 0.0f)) return;                        // behind the last barrier
    const float f = noise_fractal(k, cx, cy);
    const size_t at = (size_t)cy * (size_t)w0 + (size_t)cx;
    if constexpr (sizeof(T) == 4) {
        const uchar4 px = map[at];
        float val[4] = { (float)px.x, (float)px.y, (float)px.z, (float)px.w };
#pragma unroll
        for (int c = 0; c < 4; c++)
            if (k.channel_mask & (1u << c)) val[c] = noise_apply(k, val[c], m, f);
        map[at] = make_uchar4(brush_byte(val[0]), brush_byte(val[1]), brush_byte(val[2]), brush_byte(val[3]));
    } else {
        map[at] = brush_byte(noise_apply(k, (float)map[at], m, f));
    }
}

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
// k_noise over the rectangle `r` on `s`; dabs == nullptr: the whole-map variant
static void noise_launch(vr_terrain* t, int which, hipStream_t s, const DirtyRect& r, const BrushDab* dabs, uint32_t nd, const NoiseConst& k)
{
    const DevTex& tex = vr_terrain_map(t, which);
    uint8_t* mem = const_cast<uint8_t*>(tex.base);
    const dim3 grid = tiles_32x8(r);
    if (which == 0) {
        if (dabs) { hipLaunchKernelGGL((k_noise<uint8_t, false>), grid, dim3(256), 0, s, mem, tex.w0, tex.h0, r, dabs, nd, k); return; }
        hipLaunchKernelGGL((k_noise<uint8_t, true>), grid, dim3(256), 0, s, mem, tex.w0, tex.h0, r, dabs, 0u, k);
    } else {
        if (dabs) hipLaunchKernelGGL((k_noise<uchar4, false>), grid, dim3(256), 0, s, (uchar4*)mem, tex.w0, tex.h0, r, dabs, nd, k);
        else hipLaunchKernelGGL((k_noise<uchar4, true>), grid, dim3(256), 0, s, (uchar4*)mem, tex.w0, tex.h0, r, dabs, 0u, k);
    }
}

extern "C" VR_API int vr_terrain_noise(vr_terrain* t, int which, const vr_noise_params* p, const vr_brush_dab* dabs, uint32_t n, int32_t out_rect[4])
{
    static_assert(sizeof(vr_noise_params) == 64, "vr_noise_params layout");
    static_assert(VR_NOISE_MAX_OCTAVES == kNoiseMaxOctaves, "vr_noise.h's limit");
    static_assert(VR_NOISE_VALUE == kNoiseValue && VR_NOISE_GRADIENT == kNoiseGradient, "vr_noise.h's bases");
    static_assert(VR_NOISE_FBM == kNoiseFbm && VR_NOISE_BILLOW == kNoiseBillow && VR_NOISE_RIDGED == kNoiseRidged, "vr_noise.h's fractals");
    static_assert(VR_NOISE_ADD == kNoiseAdd && VR_NOISE_BLEND == kNoiseBlend, "vr_noise.h's ops");
    // the argument checks come before any use of the device (and leave the terrain alone)
    VR_REQUIRE(t != nullptr, "terrain is NULL");
    VR_REQUIRE(p != nullptr, "params is NULL");
    VR_REQUIRE(which == 0 || which == 1, "which must be 0 (heightmap) or 1 (albedo)");
    VR_REQUIRE(p->octaves >= 1 && p->octaves <= VR_NOISE_MAX_OCTAVES, "octaves outside 1 .. VR_NOISE_MAX_OCTAVES");
    VR_REQUIRE(p->basis == VR_NOISE_VALUE || p->basis == VR_NOISE_GRADIENT, "unknown basis");
    VR_REQUIRE(p->fractal >= VR_NOISE_FBM && p->fractal <= VR_NOISE_RIDGED, "unknown fractal");
    VR_REQUIRE(p->op == VR_NOISE_ADD || p->op == VR_NOISE_BLEND, "unknown op");
    VR_REQUIRE((p->flags & ~(uint32_t)VR_NOISE_WHOLE_MAP) == 0, "unknown flag bits");
    const bool whole = (p->flags & VR_NOISE_WHOLE_MAP) != 0;
    VR_REQUIRE(!whole || (dabs == nullptr && n == 0), "VR_NOISE_WHOLE_MAP takes no dabs");
    VR_REQUIRE(dabs != nullptr || n == 0, "dabs is NULL with n > 0");
    VR_REQUIRE(n <= VR_MAX_BRUSH_DABS, "more than VR_MAX_BRUSH_DABS dabs");
    const float fl[7] = { p->frequency, p->offset_x, p->offset_z, p->lacunarity, p->gain, p->amplitude, p->base };
    for (float v : fl) VR_REQUIRE(host_finite(v), "params holds a NaN or an infinity");
    VR_REQUIRE(p->frequency > 0.0f, "frequency must be positive");
    VR_REQUIRE(p->lacunarity >= 1.0f && p->lacunarity <= 4.0f, "lacunarity outside [1, 4]");
    VR_REQUIRE(p->gain >= 0.0f && p->gain <= 1.0f, "gain outside [0, 1]");
    VR_REQUIRE(fabsf(p->amplitude) <= 255.0f, "|amplitude| above 255");
    VR_REQUIRE(p->base >= 0.0f && p->base <= 255.0f, "base outside [0, 255]");
    VR_REQUIRE(p->channel_mask >= 1u && p->channel_mask <= 15u, "channel_mask must be 1 .. 15");
    VR_REQUIRE(which == 1 || p->channel_mask == 1u, "the heightmap has channel_mask 1");
    for (int i = 0; i < 2; i++) VR_REQUIRE(p->reserved[i] == 0, "reserved must be zero");
    if (!whole) { const int rc = vr_brush_check_dabs(dabs, n, VR_BRUSH_FLATTEN); if (rc) return rc; }       // strength is an opacity
    // the handle is looked into from here on
    const DevTex& tex = vr_terrain_map(t, which);
    NoiseDesc d;
    d.frequency = p->frequency; d.offset_x = p->offset_x; d.offset_z = p->offset_z; d.lacunarity = p->lacunarity; d.gain = p->gain;
    d.amplitude = p->amplitude; d.base = p->base; d.seed = p->seed; d.octaves = p->octaves; d.basis = p->basis; d.fractal = p->fractal; d.op = p->op;
    d.channel_mask = p->channel_mask;
    const NoiseConst k = noise_prepare(d, t->p.world_size, tex.w0, tex.h0);
    // the one refusal that needs the map's size: what keeps (int32_t)floorf(u) defined and u - floorf(u) meaningful (vr_noise.h)
    VR_REQUIRE(noise_in_range(k, tex.w0, tex.h0), "a lattice coordinate reaches 2^22 on this map: lower frequency, lacunarity, octaves or the offset");
    return vr_mask_call(t, which, whole, dabs, n, out_rect, [&](hipStream_t s, const DirtyRect& dirty, const BrushDab* d_dabs, uint32_t nd) -> int {
        noise_launch(t, which, s, dirty, d_dabs, nd, k);
        return VR_OK;
    });
}
