// vr_terrain_erode_hydraulic: hydraulic erosion of level 0 of the heightmap under a brush mask, on the device, followed by the
// refresh vr_terrain_edit does (vr_derive_level0_write).  The definition, texel by texel, is vr_hydro.h; this file holds nothing of
// it but the order in which the header's functions are called.  DESIGN.md 4v.
//
//   k_hydro_begin   k_erode_begin's shape and dab walk (vr_brush_dev.h): the mask, the terrain (byte -> fp32), the water
//                   (rain * mask) and the sediment (0) into planes of the rectangle's size
//   k_hydro_steps   the hot path, temporally blocked like k_erode_steps: a workgroup of 704 lanes loads a 56 x 36 tile of h, d, s
//                   and the mask plus a halo of kHydroK = 4 texels into LDS (64 x 44 cells, seven planes: h, d, s twice, the mask
//                   once), runs up to kHydroK sweeps there - ping-pong in LDS, one barrier per sweep, the valid region one ring
//                   smaller after each - and stores the tile's h, d, s to the other set of planes.  A call of N iterations is
//                   ceil(N / kHydroK) launches, the last with the remainder.  Cells beyond the rectangle load as zeros (mask 0:
//                   no edge reaches them) and are never stored.
//   k_hydro_end     hydro_byte(h, s) where the mask is positive
//
// Every cell of a sweep is hydro_edge x 4 and hydro_cell over the previous sweep's values in the header's order, so the bits depend
// neither on the tile nor on the sweeps per launch.  The kernels are untimed, like the brush's.
#include "vr_internal.h"
#include "vr_dirty.h"
#include "vr_hydro.h"
#include "vr_brush_dev.h"

#include <string.h>

constexpr int kHydroTileW = 56, kHydroTileH = 36, kHydroK = 4;
constexpr int kHydroStrip = 4;                                   // a lane sweeps a column of this many cells, the column's three rows in registers
constexpr int kHydroRW = kHydroTileW + 2 * kHydroK, kHydroRH = kHydroTileH + 2 * kHydroK;
constexpr int kHydroCells = kHydroRW * kHydroRH, kHydroStrips = kHydroRW * (kHydroRH / kHydroStrip);
constexpr int kHydroThreads = kHydroStrips;                      // of k_hydro_steps: one strip per lane, 11 waves
constexpr int kHydroPlanes = 7;                                  // in LDS: (h, d, s) x 2 + mask; in memory: mask + (h, d, s) x 2
constexpr int kHydroLds = kHydroCells * kHydroPlanes * (int)sizeof(float);
// A wave's 64 lanes take 64 consecutive strips: one whole row of the image, so every access of a wave is to 64 consecutive words -
// each half-wave to the 32 banks once: conflict-free, in all seven planes (a plane is a whole number of rows).
static_assert(kHydroRW % 32 == 0 && kHydroRH % kHydroStrip == 0, "k_hydro_steps' LDS layout");
static_assert(kHydroThreads % 64 == 0 && kHydroThreads <= 1024 && kHydroCells % kHydroThreads == 0, "whole waves, a whole number of cells per lane");
static_assert(kHydroLds == 78848 && 2 * kHydroLds <= 160 * 1024, "seven planes of 64 x 44 cells: two workgroups per CU");
static_assert(kHydroK >= 1 && 2 * kHydroK < kHydroRH, "a tile remains inside the halo");

// `map`: level 0 of the heightmap; `r`: the rectangle, inside the map; `dabs`: n of them, none empty; mask, h, d, s: planes of r's size
__global__ __launch_bounds__(256) void k_hydro_begin(const uint8_t* __restrict__ map, int w0, int h0, DirtyRect r, const BrushDab* __restrict__ dabs, uint32_t n,
                                                     float rain, float* __restrict__ mask, float* __restrict__ ph, float* __restrict__ pd, float* __restrict__ ps)
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
    ph[at] = h;
    pd[at] = hydro_rain(rain, m);
    ps[at] = 0.0f;
}

// src, dst: three rw x rh planes each (h, d, s; `plane` floats apart); mask: one; steps: 1 .. kHydroK sweeps
__global__ __launch_bounds__(kHydroThreads) void k_hydro_steps(const float* __restrict__ src, float* __restrict__ dst, const float* __restrict__ mask, size_t plane,
                                                               int rw, int rh, int steps, HydroConst k)
{
    __shared__ float s_m[kHydroCells];
    __shared__ float s_f[2][3][kHydroCells];
    const int tid = (int)threadIdx.x;
    const int ox = (int)blockIdx.x * kHydroTileW - kHydroK, oy = (int)blockIdx.y * kHydroTileH - kHydroK;     // the LDS image's origin in the plane
    for (int i = tid; i < kHydroCells; i += kHydroThreads) {
        const int ly = i / kHydroRW, lx = i - ly * kHydroRW;
        const int x = ox + lx, y = oy + ly;
        const bool in = x >= 0 && x < rw && y >= 0 && y < rh;
        const size_t at = (size_t)brush_clampi(y, 0, rh - 1) * (size_t)rw + (size_t)brush_clampi(x, 0, rw - 1);
        const float h = src[at], d = src[plane + at], s = src[2 * plane + at], m = mask[at];
        s_f[0][0][i] = in ? h : 0.0f;
        s_f[0][1][i] = in ? d : 0.0f;
        s_f[0][2][i] = in ? s : 0.0f;
        s_m[i] = in ? m : 0.0f;
    }
    steps = brush_clampi(steps, 0, kHydroK);                       // (a kernel argument: uniform) more sweeps than the halo holds would read stale rings
    __syncthreads();
    int cur = 0;
    // Sweep s leaves the cells at least s rings inside the image valid; it reads ring s - 1 and inwards of the sweep before.
    for (int s = 1; s <= steps; s++) {
        const float* __restrict__ hin = s_f[cur][0];
        const float* __restrict__ din = s_f[cur][1];
        const float* __restrict__ sdin = s_f[cur][2];
        float* __restrict__ hout = s_f[cur ^ 1][0];
        float* __restrict__ dout = s_f[cur ^ 1][1];
        float* __restrict__ sout = s_f[cur ^ 1][2];
        for (int idx = tid; idx < kHydroStrips; idx += kHydroThreads) {
            const int sy = idx / kHydroRW, lx = idx - sy * kHydroRW, y0 = sy * kHydroStrip;
            if (lx < s || lx >= kHydroRW - s || y0 + kHydroStrip <= s || y0 >= kHydroRH - s) continue;      // nothing of this strip is valid after the sweep
            const int xl = lx - 1, xr = lx + 1;                    // 1 <= s <= lx < kHydroRW - s: both inside the row
            // the column's rows a (above) and c (the cell's); a row index is clamped before it addresses LDS
            const int ra = brush_clampi(y0 - 1, 0, kHydroRH - 1) * kHydroRW + lx, rc = y0 * kHydroRW + lx;
            float ha = hin[ra], da = din[ra], sa = sdin[ra], ma = s_m[ra];
            float hc = hin[rc], dc = din[rc], sc = sdin[rc], mc = s_m[rc];
#pragma unroll
            for (int r = 0; r < kHydroStrip; r++) {
                const int ly = y0 + r, row = ly * kHydroRW;
                const int rb = brush_clampi(ly + 1, 0, kHydroRH - 1) * kHydroRW + lx;
                const float hb = hin[rb], db = din[rb], sb = sdin[rb], mb = s_m[rb];
                if (ly >= s && ly < kHydroRH - s) {
                    HydroAcc acc = { 0.0f, 0.0f, 0.0f };
                    hydro_edge(acc, hc, dc, sc, mc, ha, da, sa, ma, k.flow);                                                                    // (0, -1)
                    hydro_edge(acc, hc, dc, sc, mc, hin[row + xl], din[row + xl], sdin[row + xl], s_m[row + xl], k.flow);                        // (-1, 0)
                    hydro_edge(acc, hc, dc, sc, mc, hin[row + xr], din[row + xr], sdin[row + xr], s_m[row + xr], k.flow);                        // (1, 0)
                    hydro_edge(acc, hc, dc, sc, mc, hb, db, sb, mb, k.flow);                                                                    // (0, 1)
                    float h1, d1, s1;
                    hydro_cell(hc, dc, sc, mc, acc, k, &h1, &d1, &s1);
                    hout[row + lx] = h1; dout[row + lx] = d1; sout[row + lx] = s1;
                }
                ha = hc; da = dc; sa = sc; ma = mc;
                hc = hb; dc = db; sc = sb; mc = mb;
            }
        }
        __syncthreads();                                           // every lane arrives: the loop bounds are uniform
        cur ^= 1;
    }
#pragma unroll
    for (int f = 0; f < 3; f++) {
        const float* __restrict__ fin = s_f[cur][f];
        for (int i = tid; i < kHydroTileW * kHydroTileH; i += kHydroThreads) {
            const int ty = i / kHydroTileW, tx = i - ty * kHydroTileW;
            const int x = (int)blockIdx.x * kHydroTileW + tx, y = (int)blockIdx.y * kHydroTileH + ty;
            if (x < rw && y < rh) dst[(size_t)f * plane + (size_t)y * (size_t)rw + (size_t)x] = fin[(ty + kHydroK) * kHydroRW + (tx + kHydroK)];
        }
    }
}

__global__ __launch_bounds__(256) void k_hydro_end(uint8_t* __restrict__ map, int w0, DirtyRect r, const float* __restrict__ mask, const float* __restrict__ ph,
                                                   const float* __restrict__ ps)
{
    const int x = r.x0 + (int)blockIdx.x * kBrushTileW + ((int)threadIdx.x & 31), y = r.y0 + (int)blockIdx.y * kBrushTileH + ((int)threadIdx.x >> 5);
    if (x >= r.x1 || y >= r.y1) return;
    const size_t at = (size_t)(y - r.y0) * (size_t)(r.x1 - r.x0) + (size_t)(x - r.x0);
    if (mask[at] > 0.0f) map[(size_t)y * (size_t)w0 + (size_t)x] = hydro_byte(ph[at], ps[at]);
}

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
static bool host_finite(float x) { return x == x && fabsf(x) <= 3.402823466e38f; }

// sweeps per step launch: kHydroK unless the measurement tool asked for fewer (the bytes are the same)
static int g_hydro_sweeps = kHydroK;

extern "C" VR_API int vr_debug_hydro_config(int32_t out[4])
{
    VR_REQUIRE(out != nullptr, "out is NULL");
    out[0] = kHydroTileW; out[1] = kHydroTileH; out[2] = kHydroK; out[3] = 0;
    return VR_OK;
}

extern "C" VR_API int vr_debug_hydro_sweeps_per_launch(int32_t sweeps)
{
    VR_REQUIRE(sweeps >= 0 && sweeps <= kHydroK, "sweeps outside 0 .. the build's sweeps per launch");
    g_hydro_sweeps = sweeps ? sweeps : kHydroK;
    return VR_OK;
}

// The seven planes hold `plane_bytes` each, in one block, before anything is launched: all or none (a refusal leaves the terrain as it was).
static int hydro_reserve(vr_terrain* t, size_t plane_bytes)
{
    if (plane_bytes <= t->hydro_plane_bytes) return VR_OK;
    size_t want = t->hydro_plane_bytes ? t->hydro_plane_bytes * 2 : (size_t)1 << 16;
    while (want < plane_bytes) want *= 2;
    const auto idle = [t]() -> int { return vr_brush_consumed(t); };
    void** const slots[1] = { (void**)&t->d_hydro };
    const auto grow = [&](size_t bytes) -> int {
        const size_t sizes[1] = { bytes * kHydroPlanes };
        const int rc = vr_grow_group(slots, sizes, idle);
        if (!rc) t->hydro_plane_bytes = bytes;
        return rc;
    };
    int rc = grow(want);
    if (rc == VR_ERR_OUT_OF_MEMORY && want > plane_bytes) rc = grow(plane_bytes);
    if (rc == VR_ERR_OUT_OF_MEMORY) vr_set_error("terrain erode_hydraulic: 7 x %zu bytes for the mask and state planes", plane_bytes);
    return rc;
}

extern "C" VR_API int vr_terrain_erode_hydraulic(vr_terrain* t, const vr_hydro_params* p, const vr_brush_dab* dabs, uint32_t n, int32_t out_rect[4])
{
    static_assert(sizeof(vr_hydro_params) == 32, "vr_hydro_params layout");
    static_assert(VR_HYDRO_MAX_ITERATIONS == kHydroMaxIterations, "vr_hydro.h's limit");
    // the argument checks come before any use of the device (and leave the terrain alone)
    VR_REQUIRE(t != nullptr, "terrain is NULL");
    VR_REQUIRE(p != nullptr, "params is NULL");
    VR_REQUIRE(dabs != nullptr || n == 0, "dabs is NULL with n > 0");
    VR_REQUIRE(n <= VR_MAX_BRUSH_DABS, "more than VR_MAX_BRUSH_DABS dabs");
    VR_REQUIRE(p->iterations >= 1 && p->iterations <= VR_HYDRO_MAX_ITERATIONS, "iterations outside 1 .. VR_HYDRO_MAX_ITERATIONS");
    VR_REQUIRE(host_finite(p->rain) && host_finite(p->flow) && host_finite(p->capacity) && host_finite(p->dissolve) && host_finite(p->deposit) && host_finite(p->evaporation),
               "a parameter is NaN or infinite");
    VR_REQUIRE(p->rain >= 0.0f && p->rain <= 16.0f, "rain outside [0, 16]");
    VR_REQUIRE(p->flow > 0.0f && p->flow <= 1.0f, "flow outside (0, 1]");
    VR_REQUIRE(p->capacity >= 0.0f && p->capacity <= 64.0f, "capacity outside [0, 64]");
    VR_REQUIRE(p->dissolve >= 0.0f && p->dissolve <= 1.0f, "dissolve outside [0, 1]");
    VR_REQUIRE(p->deposit >= 0.0f && p->deposit <= 1.0f, "deposit outside [0, 1]");
    VR_REQUIRE(p->evaporation >= 0.0f && p->evaporation <= 1.0f, "evaporation outside [0, 1]");
    VR_REQUIRE(p->reserved == 0, "reserved must be zero");
    { const int rc = vr_brush_check_dabs(dabs, n, VR_BRUSH_FLATTEN); if (rc) return rc; }        // strength is an opacity
    const DevTex& tex = t->height;
    const DirtyRect dirty = vr_brush_prepare_dabs(t, tex, dabs, n);
    const std::vector<BrushDab>& prepared = t->brush_prepared;
    if (out_rect) { out_rect[0] = out_rect[1] = out_rect[2] = out_rect[3] = 0; }
    if (prepared.empty()) return VR_OK;                            // n == 0, or every dab misses the map: nothing is launched

    vr_context* ctx = t->ctx;
    VR_HIP(hipSetDevice(ctx->device));
    const int rw = dirty.x1 - dirty.x0, rh = dirty.y1 - dirty.y0;
    const size_t plane = (size_t)rw * (size_t)rh;
    // everything is reserved before anything is launched
    { const int rc = vr_brush_reserve(t, 0); if (rc) return rc; }
    { const int rc = hydro_reserve(t, plane * sizeof(float)); if (rc) return rc; }
    // the one wait on the host: only where the previous stroke or erosion has not been consumed yet
    { const int rc = vr_brush_consumed(t); if (rc) return rc; }
    const uint32_t nd = (uint32_t)prepared.size();
    memcpy(t->h_brush_dabs, prepared.data(), (size_t)nd * sizeof(BrushDab));

    const int iterations = p->iterations, per_launch = g_hydro_sweeps;
    const HydroConst k = { p->rain, p->flow, p->capacity, p->dissolve, p->deposit, hydro_keep(p->evaporation) };
    // the block: the mask, then two sets of h, d, s, each plane `plane` floats (the call's rectangle) long
    float* const d_mask = t->d_hydro;
    float* const d_set[2] = { t->d_hydro + plane, t->d_hydro + 4 * plane };
    uint8_t* mem = const_cast<uint8_t*>(tex.base);
    const int rc = vr_derive_level0_write(t, 0, dirty, [&](hipStream_t s) -> int {
        { const int hrc = vr_history_capture(t, 0, dirty, s); if (hrc) return hrc; }           // history on: the rectangle as it is, first
        VR_HIP(hipMemcpyAsync(t->d_brush_dabs, t->h_brush_dabs, (size_t)nd * sizeof(BrushDab), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_hydro_begin, tiles_32x8(dirty), dim3(256), 0, s, (const uint8_t*)mem, tex.w0, tex.h0, dirty, t->d_brush_dabs, nd, k.rain,
                           d_mask, d_set[0], d_set[0] + plane, d_set[0] + 2 * plane);
        const dim3 grid((unsigned)((rw + kHydroTileW - 1) / kHydroTileW), (unsigned)((rh + kHydroTileH - 1) / kHydroTileH));
        int cur = 0;
        for (int done = 0; done < iterations; done += per_launch, cur ^= 1) {
            const int steps = iterations - done < per_launch ? iterations - done : per_launch;
            hipLaunchKernelGGL(k_hydro_steps, grid, dim3(kHydroThreads), 0, s, (const float*)d_set[cur], d_set[cur ^ 1], (const float*)d_mask, plane, rw, rh, steps, k);
        }
        hipLaunchKernelGGL(k_hydro_end, tiles_32x8(dirty), dim3(256), 0, s, mem, tex.w0, dirty, (const float*)d_mask, (const float*)d_set[cur], (const float*)(d_set[cur] + 2 * plane));
        VR_HIP(hipGetLastError());
        VR_HIP(hipEventRecord(t->ev_brush, s));
        t->brush_pending = true;
        return VR_OK;
    });
    if (rc) return rc;
    if (out_rect) { out_rect[0] = dirty.x0; out_rect[1] = dirty.y0; out_rect[2] = dirty.x1 - dirty.x0; out_rect[3] = dirty.y1 - dirty.y0; }
    return VR_OK;
}
