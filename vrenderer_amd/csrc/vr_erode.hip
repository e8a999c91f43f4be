// vr_terrain_erode and vr_terrain_erode_hydraulic: thermal (talus) and hydraulic erosion of level 0 of the heightmap under a brush
// mask, on the device, through vr_brush_call (vr_level0.h).  The definitions, texel by texel, are
// vr_erode.h and vr_hydro.h; this file holds nothing of them but the order in which the headers' functions are called.  The kernels
// are written once, over a model type (the models: 4u, 4v):
//
//   k_sweep_begin   the tile frame and brush_tile_mask of vr_brush_dev.h: the mask (fp32) and the model's F state fields into planes of the rectangle's size
//   k_sweep_steps   the hot path, temporally blocked: a workgroup loads a tile of the F fields and the mask plus a halo of K texels
//                   into LDS (2F + 1 planes: the fields twice, the mask once), runs up to K sweeps there - ping-pong in LDS, one
//                   barrier per sweep, the valid region one ring smaller after each - and stores the tile's fields to the other set
//                   of planes.  A lane sweeps a strip: a column of the model's strip height, by the model's strip body.  A call of N
//                   iterations is ceil(N / K) launches, the last with the remainder.  Cells beyond the rectangle load as zeros
//                   (mask 0: no edge reaches them) and are never stored.
//   k_sweep_end     the model's byte where the mask is positive
//
// In memory: one block (vr_terrain::d_erode) of the mask plane and two sets of F planes, `plane` floats apart.  Every cell of a sweep
// is the model's header functions over the previous sweep's values in the header's order, so the bits depend neither on the tile nor
// on the sweeps per launch.  The kernels are untimed, like the brush's.
//
// A model supplies: kTileW, kTileH, kK, kStrip, kFields, kThreads; Const, the call's constants (trivially copyable); begin(byte,
// mask, k, f[F]), a lane's initial fields; end(state, plane, at), the byte of texel `at`; and its strip body, which stands in
// k_sweep_steps' one `if constexpr` over the model, in the kernel's own text (a call costs the thermal kernel registers).
#include "vr_level0.h"
#include "vr_hydro.h"

#include <type_traits>

template <class M> struct Sweep {
    static constexpr int kRW = M::kTileW + 2 * M::kK, kRH = M::kTileH + 2 * M::kK;                 // the LDS image: the tile and its halo
    static constexpr int kCells = kRW * kRH, kStrips = kRW * (kRH / M::kStrip);
    static constexpr int kPlanes = 2 * M::kFields + 1;                                           // in LDS: fields x 2 + mask; in memory: mask + fields x 2
    static constexpr int kLds = kCells * kPlanes * (int)sizeof(float);
    // A wave's 64 lanes take 64 consecutive strips: consecutive columns, and - the row length being a multiple of the 32 banks a
    // 4-byte access sees - consecutive banks across the end of a row of strips as well, so every row access is conflict-free, in
    // every plane (a plane is a whole number of rows).
    static_assert(kRW % 32 == 0 && kRH % M::kStrip == 0, "k_sweep_steps' LDS layout");
    static_assert(M::kThreads % 64 == 0 && M::kThreads <= 1024 && kCells % M::kThreads == 0, "whole waves, a whole number of cells per lane");
    static_assert(M::kK >= 1 && 2 * M::kK < kRH, "a tile remains inside the halo");
    static_assert(2 * kLds <= 160 * 1024, "two workgroups per CU");
};

struct Thermal {
    static constexpr int kTileW = 80, kTileH = 40, kK = 8, kFields = 1;
    static constexpr int kStrip = 8;                               // a lane sweeps a column of this many cells, its 3 x 3 window in registers
    static constexpr int kThreads = 768;                           // one strip per lane (672 strips); 256 and 1024 were slower
    struct Const { float talus, talus_d, rate; };                  // talus_d: the diagonals' talus
    static __device__ __forceinline__ void begin(float byte, float, const Const&, float (&f)[1]) { f[0] = byte; }
    static __device__ __forceinline__ uint8_t end(const float* __restrict__ st, size_t, size_t at) { return erode_byte(st[at]); }
};
static_assert(Sweep<Thermal>::kLds == 64512 && Sweep<Thermal>::kLds <= 65536, "state x 2 + mask of 96 x 56 cells: two workgroups per CU");
static_assert(Thermal::kK >= 4, "a launch advances at least four iterations");

struct Hydraulic {
    static constexpr int kTileW = 56, kTileH = 36, kK = 4, kFields = 3;                           // the fields: h, d, s
    static constexpr int kStrip = 4;                               // a lane sweeps a column of this many cells, the column's three rows in registers
    static constexpr int kThreads = 704;                           // one strip per lane, 11 waves: a wave takes one whole row of the image
    using Const = HydroConst;
    static __device__ __forceinline__ void begin(float byte, float m, const Const& k, float (&f)[3]) { f[0] = byte; f[1] = hydro_rain(k.rain, m); f[2] = 0.0f; }
    static __device__ __forceinline__ uint8_t end(const float* __restrict__ st, size_t plane, size_t at) { return hydro_byte(st[at], st[2 * plane + at]); }
};
static_assert(Hydraulic::kThreads == Sweep<Hydraulic>::kStrips, "one strip per lane");
static_assert(Sweep<Hydraulic>::kLds == 78848, "seven planes of 64 x 44 cells: two workgroups per CU");

// `map`: level 0 of the heightmap; `r`: the rectangle, inside the map; `dabs`: n of them, none empty; mask: a plane of r's size;
// state: F of them, `plane` floats apart
template <class M>
__global__ __launch_bounds__(256) void k_sweep_begin(const uint8_t* __restrict__ map, int w0, int h0, DirtyRect r, const BrushDab* __restrict__ dabs, uint32_t n,
                                                     typename M::Const k, float* __restrict__ mask, float* __restrict__ state, size_t plane)
{
    __shared__ uint16_t list[kBrushChunk];
    __shared__ uint32_t wave_total[4];
    const BrushTile tile = brush_tile(r);
    const int x = tile.x, y = tile.y;
    // every lane stays to the end; one outside the rectangle works on the rectangle's nearest texel (not the map's: no tile.cx, tile.cy)
    const int cx = brush_clampi(x, r.x0, r.x1 - 1), cy = brush_clampi(y, r.y0, r.y1 - 1);
    const float h = (float)map[(size_t)brush_clampi(cy, 0, h0 - 1) * (size_t)w0 + (size_t)brush_clampi(cx, 0, w0 - 1)];
    const float m = brush_tile_mask(dabs, n, tile, list, wave_total);
    if (!tile.inside) return;
    const size_t at = (size_t)(y - r.y0) * (size_t)(r.x1 - r.x0) + (size_t)(x - r.x0);
    float f[M::kFields];
    M::begin(h, m, k, f);
    mask[at] = m;
#pragma unroll
    for (int i = 0; i < M::kFields; i++) state[(size_t)i * plane + at] = f[i];
}

// src, dst: F planes of rw x rh cells each, `plane` floats apart; mask: one; steps: 1 .. K sweeps
template <class M>
__global__ __launch_bounds__(M::kThreads) void k_sweep_steps(const float* __restrict__ src, float* __restrict__ dst, const float* __restrict__ mask, size_t plane,
                                                             int rw, int rh, int steps, typename M::Const k)
{
    using S = Sweep<M>;
    constexpr int F = M::kFields, kRW = S::kRW, kRH = S::kRH;
    __shared__ float s_m[S::kCells];
    __shared__ float s_f[2][F * S::kCells];                       // a set: the F planes one after the other
    const int tid = (int)threadIdx.x;
    const int ox = (int)blockIdx.x * M::kTileW - M::kK, oy = (int)blockIdx.y * M::kTileH - M::kK;   // the LDS image's origin in the plane
    for (int i = tid; i < S::kCells; i += M::kThreads) {
        const int ly = i / S::kRW, lx = i - ly * S::kRW;
        const int x = ox + lx, y = oy + ly;
        const bool in = x >= 0 && x < rw && y >= 0 && y < rh;
        const size_t at = (size_t)brush_clampi(y, 0, rh - 1) * (size_t)rw + (size_t)brush_clampi(x, 0, rw - 1);
        float v[F];
#pragma unroll
        for (int f = 0; f < F; f++) v[f] = src[(size_t)f * plane + at];
        const float m = mask[at];
#pragma unroll
        for (int f = 0; f < F; f++) s_f[0][f * S::kCells + i] = in ? v[f] : 0.0f;
        s_m[i] = in ? m : 0.0f;
    }
    steps = brush_clampi(steps, 0, M::kK);                         // (a kernel argument: uniform) more sweeps than the halo holds would read stale rings
    __syncthreads();
    int cur = 0;
    // Sweep s leaves the cells at least s rings inside the image valid; it reads ring s - 1 and inwards of the sweep before.
    for (int s = 1; s <= steps; s++) {
        const float* __restrict__ hin = s_f[cur];
        float* __restrict__ hout = s_f[cur ^ 1];
        for (int idx = tid; idx < S::kStrips; idx += M::kThreads) {
            const int sy = idx / S::kRW, lx = idx - sy * S::kRW, y0 = sy * M::kStrip;
            if (lx < s || lx >= S::kRW - s || y0 + M::kStrip <= s || y0 >= S::kRH - s) continue;    // nothing of this strip is valid after the sweep
            // The model's strip body: sweep s of the strip whose column is lx and whose first row is y0, from hin to hout.  It stands
            // here, not behind a call: routed through a function of the model, forced inline or not, the unchanged thermal body took
            // 76 - 79 VGPRs instead of 74.
            if constexpr (std::is_same<M, Thermal>::value) {
                const float talus = k.talus, talus_d = k.talus_d, rate = k.rate;
                const int xl = lx - 1, xr = lx + 1;                        // 1 <= s <= lx < kRW - s: both inside the row
                // rows a (above), c (the cell's) and b (below), three columns each; a row index is clamped before it addresses LDS
                const int ra = brush_clampi(y0 - 1, 0, kRH - 1) * kRW, rc = y0 * kRW;
                float ha0 = hin[ra + xl], ha1 = hin[ra + lx], ha2 = hin[ra + xr], ma0 = s_m[ra + xl], ma1 = s_m[ra + lx], ma2 = s_m[ra + xr];
                float hc0 = hin[rc + xl], hc1 = hin[rc + lx], hc2 = hin[rc + xr], mc0 = s_m[rc + xl], mc1 = s_m[rc + lx], mc2 = s_m[rc + xr];
#pragma unroll
                for (int r = 0; r < M::kStrip; r++) {
                    const int ly = y0 + r;
                    const int rb = brush_clampi(ly + 1, 0, kRH - 1) * kRW;
                    const float hb0 = hin[rb + xl], hb1 = hin[rb + lx], hb2 = hin[rb + xr], mb0 = s_m[rb + xl], mb1 = s_m[rb + lx], mb2 = s_m[rb + xr];
                    if (ly >= s && ly < kRH - s) {
                        float acc = 0.0f;
                        acc = erode_edge(acc, hc1, ha0, mc1, ma0, talus_d, rate);
                        acc = erode_edge(acc, hc1, ha1, mc1, ma1, talus, rate);
                        acc = erode_edge(acc, hc1, ha2, mc1, ma2, talus_d, rate);
                        acc = erode_edge(acc, hc1, hc0, mc1, mc0, talus, rate);
                        acc = erode_edge(acc, hc1, hc2, mc1, mc2, talus, rate);
                        acc = erode_edge(acc, hc1, hb0, mc1, mb0, talus_d, rate);
                        acc = erode_edge(acc, hc1, hb1, mc1, mb1, talus, rate);
                        acc = erode_edge(acc, hc1, hb2, mc1, mb2, talus_d, rate);
                        hout[ly * kRW + lx] = hc1 + acc;
                    }
                    ha0 = hc0; ha1 = hc1; ha2 = hc2; ma0 = mc0; ma1 = mc1; ma2 = mc2;
                    hc0 = hb0; hc1 = hb1; hc2 = hb2; mc0 = mb0; mc1 = mb1; mc2 = mb2;
                }
            } else {
                static_assert(std::is_same<M, Thermal>::value || std::is_same<M, Hydraulic>::value, "a new model brings its strip body here");
                const float* __restrict__ din = hin + S::kCells;
                const float* __restrict__ sdin = hin + 2 * S::kCells;
                float* __restrict__ dout = hout + S::kCells;
                float* __restrict__ sout = hout + 2 * S::kCells;
                const int xl = lx - 1, xr = lx + 1;                        // 1 <= s <= lx < kRW - s: both inside the row
                // the column's rows a (above) and c (the cell's); a row index is clamped before it addresses LDS
                const int ra = brush_clampi(y0 - 1, 0, kRH - 1) * kRW + lx, rc = y0 * kRW + lx;
                float ha = hin[ra], da = din[ra], sa = sdin[ra], ma = s_m[ra];
                float hc = hin[rc], dc = din[rc], sc = sdin[rc], mc = s_m[rc];
#pragma unroll
                for (int r = 0; r < M::kStrip; r++) {
                    const int ly = y0 + r, row = ly * kRW;
                    const int rb = brush_clampi(ly + 1, 0, kRH - 1) * kRW + lx;
                    const float hb = hin[rb], db = din[rb], sb = sdin[rb], mb = s_m[rb];
                    if (ly >= s && ly < kRH - s) {
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
        }
        __syncthreads();                                           // every lane arrives: the loop bounds are uniform
        cur ^= 1;
    }
#pragma unroll
    for (int f = 0; f < F; f++) {
        const float* __restrict__ fin = s_f[cur] + f * S::kCells;
        for (int i = tid; i < M::kTileW * M::kTileH; i += M::kThreads) {
            const int ty = i / M::kTileW, tx = i - ty * M::kTileW;
            const int x = (int)blockIdx.x * M::kTileW + tx, y = (int)blockIdx.y * M::kTileH + ty;
            if (x < rw && y < rh) dst[(size_t)f * plane + (size_t)y * (size_t)rw + (size_t)x] = fin[(ty + M::kK) * S::kRW + (tx + M::kK)];
        }
    }
}

template <class M>
__global__ __launch_bounds__(256) void k_sweep_end(uint8_t* __restrict__ map, int w0, DirtyRect r, const float* __restrict__ mask, const float* __restrict__ state, size_t plane)
{
    const int x = brush_tile_x(r.x0) + brush_lane_x(), y = brush_tile_y(r.y0) + brush_lane_y();
    if (x >= r.x1 || y >= r.y1) return;
    const size_t at = (size_t)(y - r.y0) * (size_t)(r.x1 - r.x0) + (size_t)(x - r.x0);
    if (mask[at] > 0.0f) map[(size_t)y * (size_t)w0 + (size_t)x] = M::end(state, plane, at);
}

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
// sweeps per hydraulic step launch: the build's K unless the measurement tool asked for fewer (the bytes are the same)
static int g_hydro_sweeps = Hydraulic::kK;

template <class M> static int sweep_config(int32_t out[4])
{
    VR_REQUIRE(out != nullptr, "out is NULL");
    out[0] = M::kTileW; out[1] = M::kTileH; out[2] = M::kK; out[3] = 0;
    return VR_OK;
}
extern "C" VR_API int vr_debug_erode_config(int32_t out[4]) { return sweep_config<Thermal>(out); }
extern "C" VR_API int vr_debug_hydro_config(int32_t out[4]) { return sweep_config<Hydraulic>(out); }

extern "C" VR_API int vr_debug_hydro_sweeps_per_launch(int32_t sweeps)
{
    VR_REQUIRE(sweeps >= 0 && sweeps <= Hydraulic::kK, "sweeps outside 0 .. the build's sweeps per launch");
    g_hydro_sweeps = sweeps ? sweeps : Hydraulic::kK;
    return VR_OK;
}

// One call of the model M behind its entry point's own checks (vr_brush_call, vr_level0.h): the block's 2F + 1 planes of the
// rectangle reserved, then begin, ceil(iterations / per_launch) step launches and end.  What the launches left is recorded on the
// terrain for vr_debug_terrain_sweep_state: a refused call leaves the record as it was, a call whose dabs all miss clears it.
template <class M>
static int sweep_call(vr_terrain* t, const char* who, const vr_brush_dab* dabs, uint32_t n, int32_t out_rect[4], int iterations, int per_launch, const typename M::Const& k)
{
    size_t plane = 0;                                              // floats from one plane to the next: the rectangle's, rounded up to 256 bytes
    const int call_rc = vr_brush_call(t, 0, dabs, n, VR_BRUSH_FLATTEN, out_rect,                              // strength is an opacity
        [&](const DirtyRect& r) -> int {
            plane = ((size_t)(r.x1 - r.x0) * (size_t)(r.y1 - r.y0) + 63) & ~(size_t)63;
            { const int rc = vr_brush_reserve(t, 0); if (rc) return rc; }
            const int rc = vr_brush_grow(t, &t->d_erode, &t->erode_bytes, plane * sizeof(float) * Sweep<M>::kPlanes);
            if (rc == VR_ERR_OUT_OF_MEMORY) vr_set_error("terrain %s: %d x %zu bytes for the mask and state planes", who, Sweep<M>::kPlanes, plane * sizeof(float));
            if (rc == VR_OK) t->erode_last = {};                   // past the last refusal: the block is this call's from here on
            return rc;
        },
        [&](hipStream_t s, const DirtyRect& r, uint32_t nd) -> int {
            const int rw = r.x1 - r.x0, rh = r.y1 - r.y0;
            // the block: the mask, then two sets of F planes
            float* const d_mask = (float*)t->d_erode;
            float* const d_set[2] = { d_mask + plane, d_mask + (1 + M::kFields) * plane };
            hipLaunchKernelGGL(k_sweep_begin<M>, tiles_32x8(r), dim3(256), 0, s, (const uint8_t*)t->height.base, t->height.w0, t->height.h0, r, t->d_brush_dabs, nd, k, d_mask, d_set[0], plane);
            const dim3 grid((unsigned)((rw + M::kTileW - 1) / M::kTileW), (unsigned)((rh + M::kTileH - 1) / M::kTileH));
            int cur = 0;
            for (int done = 0; done < iterations; done += per_launch, cur ^= 1) {
                const int steps = iterations - done < per_launch ? iterations - done : per_launch;
                hipLaunchKernelGGL(k_sweep_steps<M>, grid, dim3(M::kThreads), 0, s, (const float*)d_set[cur], d_set[cur ^ 1], (const float*)d_mask, plane, rw, rh, steps, k);
            }
            hipLaunchKernelGGL(k_sweep_end<M>, tiles_32x8(r), dim3(256), 0, s, const_cast<uint8_t*>(t->height.base), t->height.w0, r, (const float*)d_mask, (const float*)d_set[cur], plane);
            t->erode_last.x = r.x0; t->erode_last.y = r.y0; t->erode_last.w = rw; t->erode_last.h = rh;
            t->erode_last.fields = M::kFields; t->erode_last.set = cur; t->erode_last.plane = plane;
            return VR_OK;
        });
    if (call_rc == VR_OK && t->brush_prepared.empty()) t->erode_last = {};                      // n == 0, or every dab misses the map
    return call_rc;
}

// The planes the last erosion call left: the mask, then the F fields of the set its last step launch wrote, each packed to rw * rh
// floats.  The copy runs on the context's stream behind the erosion's event (the call may have run on another stream) and the
// entry returns when it has completed, as a query's download does.
extern "C" VR_API int vr_debug_terrain_sweep_state(vr_terrain* t, int32_t out_rect[4], int32_t* out_fields, float* out, size_t capacity_floats)
{
    VR_REQUIRE(t != nullptr, "terrain is NULL");
    VR_REQUIRE(out_rect != nullptr && out_fields != nullptr, "out_rect or out_fields is NULL");
    const vr_terrain::ErodeRecord rec = t->erode_last;
    const size_t cells = (size_t)rec.w * (size_t)rec.h, need = (size_t)(1 + rec.fields) * cells;
    if (!(out == nullptr && capacity_floats == 0)) {
        VR_REQUIRE(out != nullptr, "out is NULL with a capacity");
        VR_REQUIRE(rec.fields == 0 || capacity_floats >= need, "capacity below (1 + fields) * w * h floats");
    }
    out_rect[0] = rec.x; out_rect[1] = rec.y; out_rect[2] = rec.w; out_rect[3] = rec.h;
    *out_fields = rec.fields;
    if (out == nullptr || rec.fields == 0) return VR_OK;
    VR_HIP(hipSetDevice(t->ctx->device));
    hipStream_t s = t->ctx->stream;
    { const int rc = order_side_begin(t->ord_brush, VrOrderOps(), s); if (rc) return rc; }
    const float* const d_mask = (const float*)t->d_erode;
    const float* const d_set = d_mask + (size_t)(1 + rec.set * rec.fields) * rec.plane;
    VR_HIP(hipMemcpyAsync(out, d_mask, cells * sizeof(float), hipMemcpyDeviceToHost, s));
    for (int f = 0; f < rec.fields; f++)
        VR_HIP(hipMemcpyAsync(out + (size_t)(1 + f) * cells, d_set + (size_t)f * rec.plane, cells * sizeof(float), hipMemcpyDeviceToHost, s));
    VR_HIP(hipStreamSynchronize(s));
    return VR_OK;
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
    const Thermal::Const k = { p->talus, erode_diagonal_talus(p->talus), p->rate };
    return sweep_call<Thermal>(t, "erode", dabs, n, out_rect, p->iterations, Thermal::kK, k);
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
    const HydroConst k = { p->rain, p->flow, p->capacity, p->dissolve, p->deposit, hydro_keep(p->evaporation) };
    return sweep_call<Hydraulic>(t, "erode_hydraulic", dabs, n, out_rect, p->iterations, g_hydro_sweeps, k);
}
