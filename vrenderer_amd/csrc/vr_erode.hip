// vr_terrain_erode: thermal (talus) erosion of level 0 of the heightmap under a brush mask, on the device, followed by the refresh
// vr_terrain_edit does (vr_derive_level0_write).  The definition, texel by texel, is vr_erode.h; this file holds nothing of it but
// the order in which the header's functions are called.  DESIGN.md 4u.
//
//   k_erode_begin   one 256-thread workgroup per 32 x 8 tile of the rectangle, one texel per lane, the dab list walked the way
//                   k_brush walks it (vr_brush_dev.h): the mask (fp32) and the state (byte -> fp32) into planes of the rectangle's size
//   k_erode_steps   the hot path, temporally blocked: a workgroup of 768 lanes loads an 80 x 40 tile of state and mask plus a halo of kErodeK = 8
//                   texels into LDS (96 x 56 cells), runs up to kErodeK sweeps there - ping-pong in LDS, one barrier per sweep, the
//                   valid region one ring smaller after each - and stores the tile to the other state plane.  One launch advances
//                   kErodeK iterations: a call of N iterations is ceil(N / kErodeK) launches, the last with the remainder.  Cells
//                   beyond the rectangle load as mask 0 / state 0 and are never stored.
//   k_erode_end     clamp, round and store the byte where the mask is positive
//
// Every cell of a sweep is erode_edge over the previous sweep's values in the header's order, so the bits depend neither on the tile
// nor on kErodeK.  The kernels are untimed, like the brush's.
#include "vr_internal.h"
#include "vr_dirty.h"
#include "vr_erode.h"
#include "vr_brush_dev.h"

#include <string.h>

constexpr int kErodeTileW = 80, kErodeTileH = 40, kErodeK = 8;
constexpr int kErodeThreads = 768;                               // of k_erode_steps: one strip per lane (672 strips); 256 and 1024 were slower
constexpr int kErodeStrip = 8;                                   // a lane sweeps a column of this many cells, its 3 x 3 window in registers
constexpr int kErodeRW = kErodeTileW + 2 * kErodeK, kErodeRH = kErodeTileH + 2 * kErodeK;
constexpr int kErodeCells = kErodeRW * kErodeRH, kErodeStrips = kErodeRW * (kErodeRH / kErodeStrip);
// A wave's 64 lanes take 64 consecutive strips: consecutive columns, and - the row length being a multiple of the 32 banks a
// 4-byte access sees - consecutive banks across the end of a row of strips as well, so every row access is conflict-free.
static_assert(kErodeRW % 32 == 0 && kErodeRH % kErodeStrip == 0, "k_erode_steps' LDS layout");
static_assert(kErodeCells * 12 <= 65536 && 2 * kErodeCells * 12 <= 160 * 1024, "state x 2 + mask: two workgroups per CU");
static_assert(kErodeK >= 4, "a launch advances at least four iterations");

// `map`: level 0 of the heightmap; `r`: the rectangle, inside the map; `dabs`: n of them, none empty; mask, state: planes of r's size
__global__ __launch_bounds__(256) void k_erode_begin(const uint8_t* __restrict__ map, int w0, int h0, DirtyRect r, const BrushDab* __restrict__ dabs, uint32_t n,
                                                     float* __restrict__ mask, float* __restrict__ state)
{
    __shared__ uint16_t list[kBrushChunk];
    __shared__ uint32_t wave_total[4];
    const int tid = (int)threadIdx.x;
    const int tx0 = r.x0 + (int)blockIdx.x * kBrushTileW, ty0 = r.y0 + (int)blockIdx.y * kBrushTileH;
    const int tx1 = tx0 + kBrushTileW < r.x1 ? tx0 + kBrushTileW : r.x1, ty1 = ty0 + kBrushTileH < r.y1 ? ty0 + kBrushTileH : r.y1;
    const int x = tx0 + (tid & 31), y = ty0 + (tid >> 5);
    const bool inside = x < tx1 && y < ty1;
    // every lane stays to the end; one outside the rectangle works on the clamped texel and writes nothing
    const int cx = brush_clampi(x, r.x0, r.x1 - 1), cy = brush_clampi(y, r.y0, r.y1 - 1);
    const float h = (float)map[(size_t)brush_clampi(cy, 0, h0 - 1) * (size_t)w0 + (size_t)brush_clampi(cx, 0, w0 - 1)];
    const float m = brush_tile_mask(dabs, n, tx0, ty0, tx1, ty1, x, y, inside, list, wave_total);
    if (!inside) return;
    const size_t at = (size_t)(y - r.y0) * (size_t)(r.x1 - r.x0) + (size_t)(x - r.x0);
    mask[at] = m;
    state[at] = h;
}

// src, dst, mask: rw x rh planes; steps: 1 .. kErodeK sweeps; talus_d: the diagonals' talus
__global__ __launch_bounds__(kErodeThreads) void k_erode_steps(const float* __restrict__ src, float* __restrict__ dst, const float* __restrict__ mask, int rw, int rh,
                                                     int steps, float talus, float talus_d, float rate)
{
    __shared__ float s_m[kErodeCells];
    __shared__ float s_h[2][kErodeCells];
    const int tid = (int)threadIdx.x;
    const int ox = (int)blockIdx.x * kErodeTileW - kErodeK, oy = (int)blockIdx.y * kErodeTileH - kErodeK;     // the LDS image's origin in the plane
    for (int i = tid; i < kErodeCells; i += kErodeThreads) {
        const int ly = i / kErodeRW, lx = i - ly * kErodeRW;
        const int x = ox + lx, y = oy + ly;
        const bool in = x >= 0 && x < rw && y >= 0 && y < rh;
        const size_t at = (size_t)brush_clampi(y, 0, rh - 1) * (size_t)rw + (size_t)brush_clampi(x, 0, rw - 1);
        const float h = src[at], m = mask[at];
        s_h[0][i] = in ? h : 0.0f;
        s_m[i] = in ? m : 0.0f;
    }
    steps = brush_clampi(steps, 0, kErodeK);                       // (a kernel argument: uniform) more sweeps than the halo holds would read stale rings
    __syncthreads();
    int cur = 0;
    // Sweep s leaves the cells at least s rings inside the image valid; it reads ring s - 1 and inwards of the sweep before.
    for (int s = 1; s <= steps; s++) {
        const float* __restrict__ hin = s_h[cur];
        float* __restrict__ hout = s_h[cur ^ 1];
        for (int idx = tid; idx < kErodeStrips; idx += kErodeThreads) {
            const int sy = idx / kErodeRW, lx = idx - sy * kErodeRW, y0 = sy * kErodeStrip;
            if (lx < s || lx >= kErodeRW - s || y0 + kErodeStrip <= s || y0 >= kErodeRH - s) continue;      // nothing of this strip is valid after the sweep
            const int xl = lx - 1, xr = lx + 1;                    // 1 <= s <= lx < kErodeRW - s: both inside the row
            // rows a (above), c (the cell's) and b (below), three columns each; a row index is clamped before it addresses LDS
            const int ra = brush_clampi(y0 - 1, 0, kErodeRH - 1) * kErodeRW, rc = y0 * kErodeRW;
            float ha0 = hin[ra + xl], ha1 = hin[ra + lx], ha2 = hin[ra + xr], ma0 = s_m[ra + xl], ma1 = s_m[ra + lx], ma2 = s_m[ra + xr];
            float hc0 = hin[rc + xl], hc1 = hin[rc + lx], hc2 = hin[rc + xr], mc0 = s_m[rc + xl], mc1 = s_m[rc + lx], mc2 = s_m[rc + xr];
#pragma unroll
            for (int r = 0; r < kErodeStrip; r++) {
                const int ly = y0 + r;
                const int rb = brush_clampi(ly + 1, 0, kErodeRH - 1) * kErodeRW;
                const float hb0 = hin[rb + xl], hb1 = hin[rb + lx], hb2 = hin[rb + xr], mb0 = s_m[rb + xl], mb1 = s_m[rb + lx], mb2 = s_m[rb + xr];
                if (ly >= s && ly < kErodeRH - s) {
                    float acc = 0.0f;
                    acc = erode_edge(acc, hc1, ha0, mc1, ma0, talus_d, rate);
                    acc = erode_edge(acc, hc1, ha1, mc1, ma1, talus, rate);
                    acc = erode_edge(acc, hc1, ha2, mc1, ma2, talus_d, rate);
                    acc = erode_edge(acc, hc1, hc0, mc1, mc0, talus, rate);
                    acc = erode_edge(acc, hc1, hc2, mc1, mc2, talus, rate);
                    acc = erode_edge(acc, hc1, hb0, mc1, mb0, talus_d, rate);
                    acc = erode_edge(acc, hc1, hb1, mc1, mb1, talus, rate);
                    acc = erode_edge(acc, hc1, hb2, mc1, mb2, talus_d, rate);
                    hout[ly * kErodeRW + lx] = hc1 + acc;
                }
                ha0 = hc0; ha1 = hc1; ha2 = hc2; ma0 = mc0; ma1 = mc1; ma2 = mc2;
                hc0 = hb0; hc1 = hb1; hc2 = hb2; mc0 = mb0; mc1 = mb1; mc2 = mb2;
            }
        }
        __syncthreads();                                           // every lane arrives: the loop bounds are uniform
        cur ^= 1;
    }
    const float* __restrict__ hfin = s_h[cur];
    for (int i = tid; i < kErodeTileW * kErodeTileH; i += kErodeThreads) {
        const int ty = i / kErodeTileW, tx = i - ty * kErodeTileW;
        const int x = (int)blockIdx.x * kErodeTileW + tx, y = (int)blockIdx.y * kErodeTileH + ty;
        if (x < rw && y < rh) dst[(size_t)y * (size_t)rw + (size_t)x] = hfin[(ty + kErodeK) * kErodeRW + (tx + kErodeK)];
    }
}

__global__ __launch_bounds__(256) void k_erode_end(uint8_t* __restrict__ map, int w0, DirtyRect r, const float* __restrict__ mask, const float* __restrict__ state)
{
    const int x = r.x0 + (int)blockIdx.x * kBrushTileW + ((int)threadIdx.x & 31), y = r.y0 + (int)blockIdx.y * kBrushTileH + ((int)threadIdx.x >> 5);
    if (x >= r.x1 || y >= r.y1) return;
    const size_t at = (size_t)(y - r.y0) * (size_t)(r.x1 - r.x0) + (size_t)(x - r.x0);
    if (mask[at] > 0.0f) map[(size_t)y * (size_t)w0 + (size_t)x] = erode_byte(state[at]);
}

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
static bool host_finite(float x) { return x == x && fabsf(x) <= 3.402823466e38f; }

extern "C" VR_API int vr_debug_erode_config(int32_t out[4])
{
    VR_REQUIRE(out != nullptr, "out is NULL");
    out[0] = kErodeTileW; out[1] = kErodeTileH; out[2] = kErodeK; out[3] = 0;
    return VR_OK;
}

// The three planes hold `plane_bytes` each, before anything is launched: all three or none (a refusal leaves the terrain as it was).
static int erode_reserve(vr_terrain* t, size_t plane_bytes)
{
    if (plane_bytes <= t->erode_plane_bytes) return VR_OK;
    size_t want = t->erode_plane_bytes ? t->erode_plane_bytes * 2 : (size_t)1 << 16;
    while (want < plane_bytes) want *= 2;
    const auto idle = [t]() -> int { return vr_brush_consumed(t); };
    void** const slots[3] = { (void**)&t->d_erode_mask, (void**)&t->d_erode_state[0], (void**)&t->d_erode_state[1] };
    const auto grow = [&](size_t bytes) -> int {
        const size_t sizes[3] = { bytes, bytes, bytes };
        const int rc = vr_grow_group(slots, sizes, idle);
        if (!rc) t->erode_plane_bytes = bytes;
        return rc;
    };
    int rc = grow(want);
    if (rc == VR_ERR_OUT_OF_MEMORY && want > plane_bytes) rc = grow(plane_bytes);
    if (rc == VR_ERR_OUT_OF_MEMORY) vr_set_error("terrain erode: 3 x %zu bytes for the mask and state planes", plane_bytes);
    return rc;
}

extern "C" VR_API int vr_terrain_erode(vr_terrain* t, const vr_erode_params* p, const vr_brush_dab* dabs, uint32_t n, int32_t out_rect[4])
{
    static_assert(sizeof(vr_erode_params) == 32, "vr_erode_params layout");
    static_assert(VR_ERODE_MAX_ITERATIONS == kErodeMaxIterations, "vr_erode.h's limit");
    // the argument checks come before any use of the device (and leave the terrain alone)
    VR_REQUIRE(t != nullptr, "terrain is NULL");
    VR_REQUIRE(p != nullptr, "params is NULL");
    VR_REQUIRE(dabs != nullptr || n == 0, "dabs is NULL with n > 0");
    VR_REQUIRE(n <= VR_MAX_BRUSH_DABS, "more than VR_MAX_BRUSH_DABS dabs");
    VR_REQUIRE(p->iterations >= 1 && p->iterations <= VR_ERODE_MAX_ITERATIONS, "iterations outside 1 .. VR_ERODE_MAX_ITERATIONS");
    VR_REQUIRE(host_finite(p->talus) && host_finite(p->rate), "talus or rate is NaN or infinite");
    VR_REQUIRE(p->talus >= 0.0f && p->talus <= 255.0f, "talus outside [0, 255]");
    VR_REQUIRE(p->rate > 0.0f && p->rate <= 0.125f, "rate outside (0, 0.125]");
    for (int i = 0; i < 5; i++) VR_REQUIRE(p->reserved[i] == 0, "reserved must be zero");
    { const int rc = vr_brush_check_dabs(dabs, n, VR_BRUSH_FLATTEN); if (rc) return rc; }        // strength is an opacity
    const DevTex& tex = t->height;
    const DirtyRect dirty = vr_brush_prepare_dabs(t, tex, dabs, n);
    const std::vector<BrushDab>& prepared = t->brush_prepared;
    if (out_rect) { out_rect[0] = out_rect[1] = out_rect[2] = out_rect[3] = 0; }
    if (prepared.empty()) return VR_OK;                            // n == 0, or every dab misses the map: nothing is launched

    vr_context* ctx = t->ctx;
    VR_HIP(hipSetDevice(ctx->device));
    const int rw = dirty.x1 - dirty.x0, rh = dirty.y1 - dirty.y0;
    // everything is reserved before anything is launched
    { const int rc = vr_brush_reserve(t, 0); if (rc) return rc; }
    { const int rc = erode_reserve(t, (size_t)rw * (size_t)rh * sizeof(float)); if (rc) return rc; }
    // the one wait on the host: only where the previous stroke or erode has not been consumed yet
    { const int rc = vr_brush_consumed(t); if (rc) return rc; }
    const uint32_t nd = (uint32_t)prepared.size();
    memcpy(t->h_brush_dabs, prepared.data(), (size_t)nd * sizeof(BrushDab));

    const int iterations = p->iterations;
    const float talus = p->talus, talus_d = erode_diagonal_talus(p->talus), rate = p->rate;
    uint8_t* mem = const_cast<uint8_t*>(tex.base);
    const int rc = vr_derive_level0_write(t, 0, dirty, [&](hipStream_t s) -> int {
        { const int hrc = vr_history_capture(t, 0, dirty, s); if (hrc) return hrc; }           // history on: the rectangle as it is, first
        VR_HIP(hipMemcpyAsync(t->d_brush_dabs, t->h_brush_dabs, (size_t)nd * sizeof(BrushDab), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_erode_begin, tiles_32x8(dirty), dim3(256), 0, s, (const uint8_t*)mem, tex.w0, tex.h0, dirty, t->d_brush_dabs, nd, t->d_erode_mask, t->d_erode_state[0]);
        const dim3 grid((unsigned)((rw + kErodeTileW - 1) / kErodeTileW), (unsigned)((rh + kErodeTileH - 1) / kErodeTileH));
        int cur = 0;
        for (int done = 0; done < iterations; done += kErodeK, cur ^= 1) {
            const int steps = iterations - done < kErodeK ? iterations - done : kErodeK;
            hipLaunchKernelGGL(k_erode_steps, grid, dim3(kErodeThreads), 0, s, (const float*)t->d_erode_state[cur], t->d_erode_state[cur ^ 1], (const float*)t->d_erode_mask, rw, rh,
                               steps, talus, talus_d, rate);
        }
        hipLaunchKernelGGL(k_erode_end, tiles_32x8(dirty), dim3(256), 0, s, mem, tex.w0, dirty, (const float*)t->d_erode_mask, (const float*)t->d_erode_state[cur]);
        VR_HIP(hipGetLastError());
        VR_HIP(hipEventRecord(t->ev_brush, s));
        t->brush_pending = true;
        return VR_OK;
    });
    if (rc) return rc;
    if (out_rect) { out_rect[0] = dirty.x0; out_rect[1] = dirty.y0; out_rect[2] = dirty.x1 - dirty.x0; out_rect[3] = dirty.y1 - dirty.y0; }
    return VR_OK;
}
