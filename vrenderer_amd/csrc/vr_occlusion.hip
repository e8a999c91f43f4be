// vr_terrain_occlusion: sky visibility baked into level 0 of the albedo - every texel under a brush mask or of the whole map marches
// the heightmap along 4, 8 or 16 directions for its horizons - by one kernel, through vr_mask_call (vr_level0.h).  The definition,
// texel by texel, is vr_occlusion.h; this file holds nothing of it but where the height bytes and the two tables come from.
//
//   k_occlusion<STAGED, WHOLE>   the tile frame of vr_brush_dev.h over the albedo rectangle; the mask is its brush_tile_mask's, and
//                                WHOLE has mask 1 on every texel, walks no list and takes no dab buffer.  The call's constants are
//                                one kernel argument (OcclusionConst): a direction's dx, dz, n_d and g_d are wave-uniform, read by
//                                scalar loads; the two tables a lane indexes by its own horizon (V, rk) are copied to LDS.
//                                The mask comes first: a tile none of whose texels has m > 0 stages nothing and marches nothing.
//                                That is one word of LDS, written behind a barrier and read by all 256 lanes behind the next, so
//                                every lane takes the same side and no barrier sits inside a branch lanes can disagree on.  A lane
//                                with m = 0 in a live tile skips the march and still reaches every barrier.
//                                STAGED: the tile's height footprint - the centres' span plus the call's reach on each side,
//                                (ceil(32 w0 / wa) + 1 + 2 reach_x) x (ceil(8 h0 / ha) + 1 + 2 reach_z) bytes, 161 x 137 at reach 64 with
//                                one height texel per albedo texel - is loaded into LDS once, wave w the rows w, w + 4, ..., consecutive
//                                lanes consecutive bytes, every index clamped before it addresses memory; the host chooses it where
//                                the footprint is at most 32 KiB.  Otherwise (a heightmap much finer than the albedo) the lanes read
//                                memory directly.  The arithmetic is one body and the bytes are the same.
//                                The march is the hot loop: per step one LDS byte read, one subtract, two integer multiplies and a
//                                compare, under a wave-uniform trip count.
//                                The footprint's row pitch is fw, unpadded.  A byte read is banked by its dword, (a / 4) mod 32, within
//                                each 32-lane half of the wave; a half is one row of the tile, whose lanes read one footprint row at
//                                columns x0(i) + k dx - the same k dx for all, so a run of at most ceil(32 w0 / wa) + 1 bytes.  Up to
//                                four height texels per albedo texel that is at most 33 consecutive dwords, one bank each but the
//                                last, whatever the pitch and the direction; the two halves never conflict.  Padding the rows could
//                                change nothing.
//
// The kernel is untimed, like the brush kernel.  Registers, LDS and scratch: profiles/terrain_occlusion_isa.txt.
#include "vr_level0.h"
#include "vr_occlusion.h"

static_assert(kOcclusionMaxReach == VR_OCCLUSION_MAX_REACH && kOcclusionTint == VR_OCCLUSION_TINT && kOcclusionStore == VR_OCCLUSION_STORE,
              "vr_occlusion.h's constants");

// `albedo`: level 0, wa x ha; `height`: level 0, w0 x h0; `r`: the call's rectangle, inside the albedo; `dabs`: n of them, prepared for
// the albedo, none empty (WHOLE: none at all); fw x fh: the staged footprint, fw * fh <= kOcclusionFootBytes
template <bool STAGED, bool WHOLE>
__global__ __launch_bounds__(256) void k_occlusion(uchar4* __restrict__ albedo, int wa, int ha, const uint8_t* __restrict__ height, int w0, int h0, DirtyRect r,
                                                   const BrushDab* __restrict__ dabs, uint32_t n, OcclusionConst k, int fw, int fh)
{
    __shared__ uint8_t foot[STAGED ? kOcclusionFootBytes : 4];
    __shared__ float tab_v[kOcclusionQ + 1], tab_rk[kOcclusionMaxReach + 1];
    __shared__ uint16_t list[kBrushChunk];  // the chunk's dabs that meet this tile
    __shared__ uint32_t wave_total[4];
    __shared__ uint32_t live;               // some texel of the tile has m > 0
    const int tid = (int)threadIdx.x;
    const BrushTile tile = brush_tile(r);
    float m;
    if constexpr (WHOLE) m = tile.inside ? 1.0f : 0.0f;            // (every tile of the grid holds a texel of the rectangle: live)
    else {
        m = brush_tile_mask(dabs, n, tile, list, wave_total);
        if (tid == 0) live = 0u;
        __syncthreads();
        if (tile.inside && m > 0.0f) live = 1u;                    // (every writer writes the same word)
        __syncthreads();
        if (live == 0u) return;                                    // the same answer in all 256 lanes: no barrier is left behind
    }
    if (tid <= kOcclusionQ) tab_v[tid] = k.V[tid];
    else if (tid - (kOcclusionQ + 1) <= kOcclusionMaxReach) tab_rk[tid - (kOcclusionQ + 1)] = k.rk[tid - (kOcclusionQ + 1)];
    const int cx = tile.cx(wa), cy = tile.cy(ha);
    const int x0 = occlusion_centre(cx, w0, wa), y0 = occlusion_centre(cy, h0, ha);
    float o = 0.0f;
    if constexpr (STAGED) {
        // the centres grow with the texel index: the tile's first texel has the smallest x0 and y0
        const int ox = occlusion_centre(brush_clampi(tile.tx0, 0, wa - 1), w0, wa) - k.reach_x;
        const int oy = occlusion_centre(brush_clampi(tile.ty0, 0, ha - 1), h0, ha) - k.reach_z;
        const int sw = brush_clampi(fw, 1, kOcclusionFootBytes), sh = brush_clampi(fh, 1, kOcclusionFootBytes / sw);      // sw * sh <= kOcclusionFootBytes, whatever the host passed
        const int lane = tid & 63, wave = tid >> 6;
        for (int ly = wave; ly < sh; ly += kBrushThreads / 64) {
            const uint8_t* __restrict__ row = height + (size_t)brush_clampi(oy + ly, 0, h0 - 1) * (size_t)w0;
            for (int lx = lane; lx < sw; lx += 64) foot[ly * sw + lx] = row[brush_clampi(ox + lx, 0, w0 - 1)];
        }
        __syncthreads();
        if (tile.inside && m > 0.0f) {
            const OcclusionFoot fetch = { foot, ox, oy, sw, sh };
            o = occlusion_texel(k, tab_v, tab_rk, fetch, w0, h0, x0, y0);
        }
    } else {
        __syncthreads();                                           // the tables
        if (tile.inside && m > 0.0f) {
            const OcclusionDirect fetch = { height, w0 };
            o = occlusion_texel(k, tab_v, tab_rk, fetch, w0, h0, x0, y0);
        }
    }
    if (!(tile.inside && m > 0.0f)) return;                        // behind the last barrier
    const size_t at = (size_t)cy * (size_t)wa + (size_t)cx;
    const uchar4 px = albedo[at];
    float val[4] = { (float)px.x, (float)px.y, (float)px.z, (float)px.w };
    occlusion_composite(k, o, m, val);
    albedo[at] = make_uchar4(brush_byte(val[0]), brush_byte(val[1]), brush_byte(val[2]), brush_byte(val[3]));
}

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
#define OCC_REQUIRE(cond, msg) VR_REQUIRE(cond, "vr_terrain_occlusion: " msg)

// k_occlusion over the rectangle `r` on `s`; dabs == nullptr: the whole-map variant
static void occlusion_launch(vr_terrain* t, hipStream_t s, const DirtyRect& r, const BrushDab* dabs, uint32_t nd, const OcclusionConst& k)
{
    const DevTex& hm = t->height; const DevTex& al = t->albedo;
    int64_t fw, fh;
    occlusion_footprint(k, hm.w0, hm.h0, al.w0, al.h0, kBrushTileW, kBrushTileH, &fw, &fh);
    const bool staged = fw * fh <= kOcclusionFootBytes;
    uchar4* mem = (uchar4*)const_cast<uint8_t*>(al.base);
    const dim3 grid = tiles_32x8(r);
    if (dabs) {
        if (staged) hipLaunchKernelGGL((k_occlusion<true, false>), grid, dim3(256), 0, s, mem, al.w0, al.h0, hm.base, hm.w0, hm.h0, r, dabs, nd, k, (int)fw, (int)fh);
        else hipLaunchKernelGGL((k_occlusion<false, false>), grid, dim3(256), 0, s, mem, al.w0, al.h0, hm.base, hm.w0, hm.h0, r, dabs, nd, k, 0, 0);
    } else {
        if (staged) hipLaunchKernelGGL((k_occlusion<true, true>), grid, dim3(256), 0, s, mem, al.w0, al.h0, hm.base, hm.w0, hm.h0, r, dabs, 0u, k, (int)fw, (int)fh);
        else hipLaunchKernelGGL((k_occlusion<false, true>), grid, dim3(256), 0, s, mem, al.w0, al.h0, hm.base, hm.w0, hm.h0, r, dabs, 0u, k, 0, 0);
    }
}

extern "C" VR_API int vr_terrain_occlusion(vr_terrain* t, const vr_occlusion_params* p, const vr_brush_dab* dabs, uint32_t n, int32_t out_rect[4])
{
    static_assert(sizeof(vr_occlusion_params) == 64, "vr_occlusion_params layout");
    // the argument checks come before any use of the device (and leave the terrain alone)
    OCC_REQUIRE(t != nullptr, "terrain is NULL");
    OCC_REQUIRE(p != nullptr, "params is NULL");
    OCC_REQUIRE((p->flags & ~(uint32_t)VR_OCCLUSION_WHOLE_MAP) == 0, "unknown flag bits");
    const bool whole = (p->flags & VR_OCCLUSION_WHOLE_MAP) != 0;
    OCC_REQUIRE(!whole || (dabs == nullptr && n == 0), "VR_OCCLUSION_WHOLE_MAP takes no dabs");
    OCC_REQUIRE(dabs != nullptr || n == 0, "dabs is NULL with n > 0");
    OCC_REQUIRE(n <= VR_MAX_BRUSH_DABS, "more than VR_MAX_BRUSH_DABS dabs");
    for (int i = 0; i < 3; i++) OCC_REQUIRE(p->reserved[i] == 0, "reserved must be zero");
    OCC_REQUIRE(p->mode == VR_OCCLUSION_TINT || p->mode == VR_OCCLUSION_STORE, "unknown mode");
    OCC_REQUIRE(p->directions == 4 || p->directions == 8 || p->directions == 16, "directions must be 4, 8 or 16");
    const float f[9] = { p->radius, p->max_height, p->gain, p->bias, p->opacity, p->color[0], p->color[1], p->color[2], p->color[3] };
    for (float v : f) OCC_REQUIRE(host_finite(v), "params holds a NaN or an infinity");
    OCC_REQUIRE(p->radius > 0.0f, "radius must be positive");
    OCC_REQUIRE(p->max_height > 0.0f, "max_height must be finite and positive");
    OCC_REQUIRE(p->gain >= 0.0f && p->gain <= 16.0f, "gain outside [0, 16]");
    OCC_REQUIRE(p->bias >= 0.0f && p->bias < 8.0f, "bias outside [0, 8)");
    OCC_REQUIRE(p->opacity >= 0.0f && p->opacity <= 1.0f, "opacity outside [0, 1]");
    for (int c = 0; c < 4; c++) OCC_REQUIRE(p->color[c] >= 0.0f && p->color[c] <= 255.0f, "color outside [0, 255]");
    OCC_REQUIRE(p->channel_mask >= 1u && p->channel_mask <= 15u, "channel_mask must be 1 .. 15");
    if (!whole) { const int rc = vr_brush_check_dabs(dabs, n, VR_BRUSH_FLATTEN); if (rc) return rc; }       // strength is an opacity
    // the last refusal reads the maps' sizes from the terrain and nothing else of it
    OcclusionDesc d;
    d.radius = p->radius; d.max_height = p->max_height; d.gain = p->gain; d.bias = p->bias; d.opacity = p->opacity;
    for (int c = 0; c < 4; c++) d.color[c] = p->color[c];
    d.channel_mask = p->channel_mask; d.directions = p->directions; d.mode = p->mode;
    OcclusionConst k;
    OCC_REQUIRE(occlusion_prepare(d, t->p.world_size, t->height.w0, t->height.h0, &k),
                "the radius reaches more than VR_OCCLUSION_MAX_REACH height texels in some direction");
    return vr_mask_call(t, 1, whole, dabs, n, out_rect, [&](hipStream_t s, const DirtyRect& dirty, const BrushDab* d_dabs, uint32_t nd) -> int {
        occlusion_launch(t, s, dirty, d_dabs, nd, k);
        return VR_OK;
    });
}
