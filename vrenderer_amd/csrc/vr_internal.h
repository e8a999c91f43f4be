// Internal declarations shared by the translation units of libvrterrain.so.
// gfx950 (MI355X) only; wave = 64 lanes everywhere.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>
#include <stdlib.h>
#include <functional>
#include <string>
#include <vector>

#include "../../include/vrterrain.h"
#include "vr_brush.h"
#include "vr_devbuf.h"
#include "vr_gbuffer_state.h"
#include "vr_geosets.h"
#include "vr_history.h"
#include "vr_light_plan.h"
#include "vr_light_domain.h"
#include "vr_order.h"
#include "vr_path.h"
#include "vr_region.h"
#include "vr_scratch.h"
#include "vr_tonemap_plan.h"

// ---- error plumbing -------------------------------------------------------------
void vr_set_error(const char* fmt, ...);
#define VR_HIP(expr)                                                                  \
    do {                                                                              \
        hipError_t e__ = (expr);                                                      \
        if (e__ != hipSuccess) {                                                      \
            vr_set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(e__)); \
            return e__ == hipErrorOutOfMemory ? VR_ERR_OUT_OF_MEMORY : VR_ERR_HIP;    \
        }                                                                             \
    } while (0)
#define VR_REQUIRE(cond, msg)                                                         \
    do { if (!(cond)) { vr_set_error("%s:%d: %s", __FILE__, __LINE__, msg); return VR_ERR_INVALID_ARGUMENT; } } while (0)
inline bool host_finite(float x) { return x == x && fabsf(x) <= 3.402823466e38f; }    // of an argument: neither a NaN nor an infinity

// ---- device buffers that grow (vr_devbuf.h) ----------------------------------------
// Every buffer that a larger one replaces while the library runs goes through these: the new block is allocated first, `quiesce`
// (the call site's stream synchronisations) runs in front of the free, and a failure - VR_ERR_OUT_OF_MEMORY, or quiesce's own
// code - leaves pointer and capacity as they were.  vr_dev_alloc (vr_host.hip) is their one allocate function.
bool vr_dev_alloc(void** out, size_t bytes);
inline void vr_dev_free(void* p) { (void)hipFree(p); }
inline int vr_grow_code(int rc) { return rc == kDevBufNoMemory ? VR_ERR_OUT_OF_MEMORY : rc; }
template <class T, class Quiesce> int vr_grow(T** ptr, size_t* capacity_bytes, size_t bytes, Quiesce&& quiesce)
{ return vr_grow_code(vr_devbuf_grow((void**)ptr, capacity_bytes, bytes, vr_dev_alloc, vr_dev_free, quiesce)); }
template <size_t N, class Quiesce> int vr_grow_group(void** const (&slot)[N], const size_t (&bytes)[N], Quiesce&& quiesce)
{ return vr_grow_code(vr_devbuf_grow_group(slot, bytes, vr_dev_alloc, vr_dev_free, quiesce)); }
// a buffer that follows the largest request so far: from 64 KiB by doubling (vr_devbuf_reserve)
template <class T, class Quiesce> int vr_reserve(T** ptr, size_t* capacity_bytes, size_t bytes, Quiesce&& quiesce)
{ return vr_grow_code(vr_devbuf_reserve((void**)ptr, capacity_bytes, bytes, vr_dev_alloc, vr_dev_free, quiesce)); }

// ---- cross-stream order (vr_order.h) -----------------------------------------------------
// The protocol's three operations on HIP's streams and events; its steps return what these return.
struct VrOrderOps {
    int record(hipEvent_t e, hipStream_t s) const { VR_HIP(hipEventRecord(e, s)); return VR_OK; }
    int wait(hipStream_t s, hipEvent_t e) const { VR_HIP(hipStreamWaitEvent(s, e, 0)); return VR_OK; }
    int sync(hipEvent_t e) const { VR_HIP(hipEventSynchronize(e)); return VR_OK; }
};
using VrOrderSet = OrderSet<hipStream_t, hipEvent_t>;
using VrOrderSide = OrderSide<hipStream_t, hipEvent_t>;
using VrEventRef = EventRef<hipEvent_t>;

// ---- geometry constants -----------------------------------------------------------
constexpr int kGrid = 32;                    // GRID_SIZE (TerrainPass.h:28)
constexpr int kSide = kGrid + 1;             // 33 vertices per side
constexpr int kVertsPerInst = kSide * kSide; // 1089
constexpr int kTrisPerInst = kGrid * kGrid * 2; // 2048
constexpr int kRecGroups = 8;                // 16-byte groups per triangle record (vr_raster.hip: write_tri_rec)
constexpr int kRasterTile = 64;              // raster/bin tile (pixels) of large frames; also the upper bound of either size
// Tile edge of the raster / bin grid for a w x h target: 64, or 32 when this rank draws fewer than kTile64Min 64-pixel
// tiles.  A 64-pixel tile amortises the per-workgroup work (tables, bin header, barrier) over four times the pixels and
// sweeps a triangle of the 8K frame (30-60 pixels) in one or two tiles instead of four; 32-pixel tiles are four times as
// many workgroups (launch waves, tail) and five instead of four of them fit a CU.  Measured again in the second session of
// round 3 with that round's tile pass, frame time of the bench, 64- vs 32-pixel tiles: 4K 0.248 vs 0.231 ms, 5120x2880
// 0.312 vs 0.287, 6400x3600 0.414 vs 0.404, 7040x3960 0.475 vs 0.475, 8K 0.541 vs 0.552; a rank of an N-way split of the
// 8K frame (tile pass alone in brackets): N = 2 0.400 vs 0.378 ms, N = 4 0.232 vs 0.210 (149 vs 124 us), N = 8 0.154 vs 0.130
// (profiles/r03_tile_size_thresholds.txt).  Round 2's thresholds - 2560 tiles for the whole frame, 1536 per rank -
// came from a tile pass that was 40 % slower per pixel and cost N = 2 and N = 4 5-10 %.  With the 32-pixel variants at six waves
// per SIMD (vr_raster.hip) they win up to ~9.6K x 5.4K: 8K 0.544 vs 0.527 ms, 7040x3960 0.472 vs 0.455, 9600x5400 0.796 vs 0.792,
// 12288x6912 1.250 vs 1.265 - hence 13000.
// Round 4: with the plane-state tracking (region states exist on 32-pixel tiles only: vr_gbuffer) and the pre-set-up bin entries
// 32-pixel tiles win at every size that was measured - 11520x6480 0.902 vs 0.983 ms, 15360x8640 1.589 vs 1.694 (the lighting pass
// reads what the states let it skip: 324 vs 384 us and 575 vs 683 us; the tile pass itself 560 vs 577 and 996 vs 989 us) - so the
// rule now picks 32 for any target the library accepts; 64-pixel tiles remain behind VR_OPT_RASTER_TILE.
constexpr long kTile64Min = 1L << 40;
// `force`: 0 = the rule above, 5 / 6 = 32- / 64-pixel tiles whatever the size (vr_context_set_option(VR_OPT_RASTER_TILE): tests
// compare both variants with the oracle at sizes the oracle finishes in seconds; a host may pin the choice)
inline int vr_raster_tile_shift(int w, int h, int world = 1, int force = 0)
{
    if (force == 5 || force == 6) return force;
    const long tiles64 = (long)((w + 63) / 64) * (long)((h + 63) / 64);
    return tiles64 / (world > 1 ? world : 1) < kTile64Min ? 5 : 6;
}
constexpr int kMaxLights = 16;               // terrain_cb.h:15 / Donut DEFERRED_MAX_LIGHTS
constexpr int kMaxLevels = 16;
constexpr float kGuardBand = 100.0f;
// linear -> sRGB8 start table: one bucket per (exponent, top 7 mantissa bits) from 2^-13 to 1.0
constexpr int kEncTabBase = (127 - 13) << 7;
constexpr int kEncTabSize = (13 << 7) + 1;

// Mip chain in device memory, passed to kernels by value.
struct DevTex {
    const uint8_t* base;        // level 0 first, then the coarser levels
    const uint32_t* off;        // device table: byte offset of each level (kMaxLevels entries)
    int levels;
    int w0, h0;                 // level l is max(1, w0 >> l) x max(1, h0 >> l)
    uint32_t chain_bytes;       // bytes of the mip chain at `base` (bound of the buffer resource the tile pass reads texels through)
    // R8 textures only: per level a (w+2) x (h+2) table of bilinear footprints.  Entry (ix, iy)
    // packs the four clamp-addressed texels (x0,y0) (x1,y0) (x0,y1) (x1,y1) for floor(x) = ix-1,
    // floor(y) = iy-1 into one dword, so a bilinear tap is ONE load instead of four byte loads.
    const uint32_t* quad;
    const uint32_t* qoff;       // device table: dword offset of each level's quad table
    uint32_t quad_bytes, pad;   // bytes of all quad tables at `quad`
    // The same footprints decoded: per entry (t00, t10 - t00, t01, t11 - t01) as floats (t = byte / 255), same indexing.
    // A height tap is then one 16-byte load and 7 float operations - no byte extraction, no conversion table.
    const float4* quadf;
    // SRGBA8 textures only: the chain decoded to linear floats, one float4 per texel (r, g, b, 0); level l starts at byte
    // 4 * off[l].  An albedo texel is then one aligned 16-byte load with nothing to extract or look up, at (index << 4).
    const float* rgbf;
    // Both kinds, for the tile pass's fast variant (heightmap and albedo of one size): per level a (w+3) x (h+3) table of
    // 16-byte entries - R8: the footprint (t00, t10 - t00, t01, t11 - t01) whose floor is (ix-1, iy-1); SRGBA8: the decoded
    // texel (r, g, b, 0) at (ix-1, iy-1) - clamp-addressed, so that a bilinear footprint needs no clamp: texel (x, y),
    // x in [-1, w], y in [-1, h], is entry (x+1, y+1) and its right / lower neighbours are +16 / +row bytes.  Textures of
    // one size get identical layouts, so ONE set of byte offsets addresses the height taps and the albedo footprint.
    // fast_lv[l] = { byte offset of entry (1, 1), row bytes, (float)w, (float)h } (what a pixel needs of level l).
    const float4* fast;
    const uint4* fast_lv;
    uint32_t fast_bytes, pad2;
};

// Where the levels and the tables of a DevTex begin, on the host (the device reads the same figures from DevTex::off / qoff /
// fast_lv): enough to derive everything from the texture's one allocation before there is a DevTex (vr_derive_chain).
struct TexLayout {
    uint32_t off[kMaxLevels];          // bytes into the chain
    uint32_t qoff[kMaxLevels];         // entries into quad / quadf (R8 only)
    uint32_t fast_entry[kMaxLevels];   // entries into fast
    size_t quad_at, quadf_at, rgbf_at, fast_at;     // bytes from the chain's first to each table (0: the texture has none)
    // SRGBA8 only: the packed footprint table of the fused tile pass (vr_packed.h) - entry for entry where `fast` has its own
    // (fast_entry, fast_lv and DevTex::fast_bytes hold for both), so it is not part of DevTex: the fused launch is handed the pointer
    size_t pack_at;
};

// Per-light constants the deferred kernel reads (host precomputes the half-angle terms).
struct DevLight {
    float dir[3];  int type;
    float pos[3];  float inv_range;
    float color[3]; float intensity;
    float cosH, sinH, tanH, radius;   // radius > 0: spherical source (half angle per pixel)
    float inner_angle, outer_angle;   // spot cone (radians)
    float cone_cos, cone_sin;         // vr_deferred_light_tiled_ex only: cone_cull_terms() of a spot light (vr_light_cull.h); 0 elsewhere
};

// Transformed vertex: clip position, world xz and the snapped screen vertex.
struct DevVert {
    float cx, cy, cz, cw;
    float wx, wz;
    int32_t X, Y;      // 24.8 fixed point, valid when cw > 0
    float z, iw;
    uint32_t pad0, pad1;
};
static_assert(sizeof(DevVert) == 48, "DevVert layout");

// Explicit triangle (output of the clipper for triangles that cross the near plane
// or leave the guard band): indices into the vertex array's extra region, the
// draw-order key and the raster-tile rectangle it touches.
struct HardTriRec { uint32_t v0, v1, v2, order_key; uint32_t rect_lo, rect_hi, pad0, pad1; };
static_assert(sizeof(HardTriRec) == 32, "HardTriRec layout");

// Bin entry (round 4): a triangle as ONE raster tile sees it, set up once by k_fill - per (triangle, tile) pair, one lane each,
// full waves - instead of by every tile-pass workgroup from the triangle's record: edge functions at the centre of the tile's
// pixel (0, 0) and their steps per pixel, the triangle's pixel box inside the tile, the depth plane with the tile's origin
// relative to the plane's anchor, and the draw-order word of the visibility buffer.  64 bytes = four 16-byte groups, so that
// a sparse bin's entries can be read with scalar loads (the entry index is wave-uniform) straight into SGPRs: no per-lane
// record fetch, no per-lane set-up, no v_readlane broadcast in the tile pass.  (With the resolve's planes in the
// entry as well - 128 bytes - the tile pass alone gained 2.5 %, and k_fill, which runs beside it, cost the frame 2 %: not kept.)
struct TileEntry {
    int32_t e0, e1, e2;                    // E_i at the tile's first pixel centre (bias NOT subtracted); exact when kTeFits32 is set
    int32_t sx0, sy0, sx1, sy1, sx2, sy2;  // steps per pixel: A_i * 256, B_i * 256
    uint32_t box;                          // x0 | y0 << 8 | x1 << 16 | y1 << 24, tile-local, inclusive (clamped to tile and viewport)
    float z0, zx, zy;                      // depth plane about the triangle's anchor pixel
    uint32_t offs;                         // (tile origin - anchor): x & 0xffff | y << 16
    uint32_t order;                        // ~(key + 1): low word of the visibility buffer
    uint32_t flags;                        // bias0..2 (bits 0-2), kTeFits32, kTeValid, kTeSmall
};
static_assert(sizeof(TileEntry) == 64, "TileEntry layout");
constexpr int kTeGroups = 4;                // 16-byte groups per entry
constexpr int kTeSlotBits = 5;              // a bin of up to 32 entries keeps its triangles' planes in LDS: slot = low bits of the visibility word
constexpr uint32_t kTeFits32 = 8u, kTeValid = 16u, kTeSmall = 32u;     // kTeSmall: every |A_i|, |B_i| <= 2^14 (the row hand-out's 24-bit products)

// Screen-tile partition of a w x h frame for one rank of `world`: built once, immutable afterwards.
struct PartTables {
    int w = 0, h = 0, rank = 0, world = 1;
    int tile_shift = 0;                 // raster tile edge the table of raster tiles was built for (part of the cache key)
    int32_t* d_owned_tiles = nullptr;   // owner-tile ids (128x128) owned by this rank
    int32_t* d_tile_slot = nullptr;     // per owner tile: rank * max_owned + local index
    int32_t* d_raster_tiles = nullptr;  // raster-tile ids (64x64 or 32x32) inside owned owner tiles
    int num_owned = 0, max_owned = 0, num_raster_tiles = 0;
};

struct vr_context {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev_sysfence = nullptr;   // the one event WITH a system-scope release (vr_comm.hip: in front of a collective)
    float* d_srgb_lut = nullptr;   // 256 floats: sRGB8 -> linear
    float* d_srgb_thr = nullptr;   // 256 floats: encode thresholds
    float h_srgb_lut[256];
    float h_srgb_thr[256];
    uint8_t* d_enc_tab = nullptr;  // kEncTabSize bytes: sRGB8 code of the smallest float of each bucket
    // partition tables (device), one set per (w,h,rank,world) seen; they live as long as the context, so a
    // kernel queued on any stream can never read a freed or foreign table (a frame alternates between the
    // shadow map's and the main view's geometry every frame)
    std::vector<PartTables*> part_tables;
    bool async_geometry = true;    // VR_OPT_ASYNC_GEOMETRY
    bool scratch_worst_case = false;   // VR_OPT_SCRATCH_WORST_CASE: terrains created from now on size their scratch for max_instances up front
    bool plane_tracking = true;    // VR_OPT_PLANE_TRACKING: the tile pass does not rewrite a G-buffer plane the library knows to be all zero (vr_gbuffer)
    bool frame_fusion = true;      // VR_OPT_FRAME_FUSION: vr_frame_submit shades in the tile pass where its G-buffer-keeping flavour applies
    bool gbuffer_lazy = true;      // VR_OPT_GBUFFER_LAZY: a fused frame leaves its colour planes to their first reader (vr_gbuffer_state.h)
    int raster_tile_force = 0;     // VR_OPT_RASTER_TILE: 0 = by size (vr_raster_tile_shift), 5 / 6 = 32- / 64-pixel raster tiles
    // Start / stop events of the launches (vr_events.h): the timing level and pool, VR_OPT_DISPATCH_EVENTS and the ring the stamped
    // events of ordinary runs come from, the pairs vr_timing_collect reads.  Only vr_host.hip changes it, through that header's transitions.
    EventSupply<hipEvent_t> events;
    // light list of vr_deferred_light_tiled
    DevLight* d_lights = nullptr; size_t light_bytes = 0; std::vector<DevLight> h_lights, h_lights_on_device;   // (the list d_lights holds)
    uint32_t* d_macro_scratch = nullptr; size_t macro_scratch_bytes = 0;   // per macro tile: lights touching its box (k_light_cull's first stage)
    uint32_t* d_light_lists = nullptr; size_t light_list_bytes = 0;    // per 32x32 light tile: count + light indices (k_light_cull)
    uint32_t* d_flags = nullptr;
    int last_light_variant = -1, last_light_cull = -1;          // what the last lighting pass launched (vr_debug_light_variant)
    int list_stride = 0, list_tiles_x = 0, list_tiles_y = 0;   // layout of d_light_lists as the last tiled pass left it (vr_debug_tile_light_list)
};

// One kernel launch's event pair, when it gets one (events_take): RAII over vr_events.h's transitions.
// by_dispatch: the events are not recorded as separate stream operations; the launch passes them to hipExtLaunchKernelGGL
// (launch), which stamps them from the dispatch itself.
class VrKernelScope {
    vr_context* c; EventPair<hipEvent_t, hipStream_t> pair;
public:
    VrKernelScope(vr_context* ctx, int id, hipStream_t stream, bool by_dispatch = false);
    VrKernelScope(const VrKernelScope&) = delete;
    // the launch of a scope created with by_dispatch = true, on the scope's stream
    template <class Kernel, class... Args> void launch(Kernel kernel, dim3 grid, dim3 block, const Args&... args)
    {
        if (pair.stamps()) {
            hipExtLaunchKernelGGL(kernel, grid, block, 0, pair.stream, pair.begin, pair.end, 0, args...);
            events_launched(c->events, pair, c->stream);
        } else hipLaunchKernelGGL(kernel, grid, block, 0, pair.stream, args...);
    }
    VrEventRef stop() const { return events_stop(c->events, pair); }      // this launch's own stop event as a dependency; none: not stamped, or no launch
    ~VrKernelScope();
};
struct vr_gbuffer {
    vr_context* ctx;
    int w, h;
    float* depth; uint32_t* diffuse; uint32_t* specular; uint2* normals; uint2* emissive;
    // Depth range (bits of the smallest / largest depth below 1.0) of every 32x32 light tile, left behind by a tile pass that
    // was asked for it (vr_render_params::depth_ranges) and consumed - and reset to "none" = (0x7f800000, 0) - by the tiled
    // lighting pass's culling stage, which then need not read the depth plane a second time.
    uint2* d_ranges = nullptr;
    size_t ranges_bytes = 0;
    uint8_t* d_region = nullptr;     // one state byte per region (kRegionClear / kRegionSpec), kept by the fast tile pass
    // What the library knows of the planes and of the two arrays (vr_gbuffer_state.h).  Only vr_host.hip assigns it, through
    // that header's transitions; it owns the arrays, the fills and the error codes.
    GbufferState st;
    // GbufferState::planes_pending: the frame whose unfused tile pass produces the colour planes and the region bytes.  The terrain
    // holds the target in turn (vr_terrain::pending_target): whatever changes what the frame would draw materialises it first.
    // (The target's size is the object's own - a resize is destroy + create; a lazy clear the frame consumed is consumed in `st`.)
    struct PendingFrame { vr_terrain* terrain = nullptr; vr_view view; vr_render_params rp; } pending;
};
// Whoever reads the planes or the region state, or writes part of them: pending colour planes (the recorded frame's unfused tile pass,
// on the context's stream), then a pending clear (written now, on `s`).  An error is the caller's to report; what was pending stays so.
int vr_gbuffer_materialise(vr_gbuffer* g, hipStream_t s);
int vr_gbuffer_materialise_planes(vr_gbuffer* g);              // (vr_raster.hip) the first half alone
int vr_terrain_materialise_pending(vr_terrain* t);             // in front of anything that changes what the terrain's recorded frame would draw
// the state no longer says planes_pending (a clear, a pass that replaces the record, the materialisation itself): the record goes
void vr_gbuffer_record_settle(vr_gbuffer* g);
void vr_gbuffer_record_unlink(vr_gbuffer* g);                  // the terrain named by the record no longer holds this target (the record is about to name another)
// A tile pass as raster_plan() decided it (vr_raster_plan.h), once nothing but this call can refuse the launch any more: the
// arrays it needs, their fills, then the state behind the pass (*region; NULL: not kept).  A refusal leaves the state as it was.
struct RasterPlan;
int vr_gbuffer_apply_plan(vr_gbuffer* g, const RasterPlan& plan, hipStream_t s, int rank, int world, uint8_t** region);
// the tiled lighting pass takes the depth ranges if they are VALID for this split: asked first, and committed - they are "none"
// again once its culling stage has run - only when nothing can refuse the call any more
bool vr_gbuffer_ranges_usable(const vr_gbuffer* g, int rank, int world);
void vr_gbuffer_consume_ranges(vr_gbuffer* g, int rank, int world);
// What a pass that READS the G-buffer may take from the tracking instead of from memory (the lighting passes).
struct PlaneHints {
    const uint8_t* region;       // region states (NULL: nothing known per region)
    uint32_t spec_const;         // the value kRegionSpec stands for
    int emissive_zero;           // the emissive plane holds only zeros
    int tiles32_x;               // regions are indexed [32-pixel tile][wave of the tile = 8 rows]
};
int vr_gbuffer_plane_hints(vr_gbuffer* g, hipStream_t s, PlaneHints* out);
uint32_t vr_specular_constant(const vr_context* c);     // main_ps's specular output as the G-buffer holds it (terrain_ps.hlsl:76 -> SRGBA8)

struct vr_image {
    vr_context* ctx;
    int w, h;
    void* data;
    bool owned;
    size_t capacity_bytes;
    OrderImage<hipEvent_t> ord;          // vr_frame_submit's cross-stream order (vr_order.h): who wrote it, who still reads it
};

struct vr_ldr_image {
    vr_context* ctx;
    int w, h;
    void* data;
    bool owned;
    size_t capacity_bytes;
};

// Everything one frame's geometry stages produce and its tile pass consumes.  Three sets rotate: the tile pass of
// frame N reads one while the geometry of frames N+1 and N+2 is built in the other two (vr_terrain_prepare).  Which set a call
// gets - current, prepared, holding a selection - is vr_terrain::slots (vr_geosets.h); a GeoSet is the memory and its order.
static_assert(kGeoSets == kScratchSets, "ScratchState::pending has one flag per geometry set");
struct GeoSet {
    uint32_t* d_node_ids = nullptr;      // select outputs
    vr_instance* d_instances = nullptr;
    uint32_t* d_counters = nullptr;      // 64 words: the status words and k_scan's classes (vr_scratch.h: C_*)
    uint32_t* d_sel_scratch = nullptr;   // k_select: the frontiers' overflow beyond their LDS part and the selected keys (one workgroup's scratch)
    DevVert* d_verts = nullptr;          // max_instances*1089 regular + extra (clipper) region
    uint64_t* d_rect = nullptr;          // per triangle: tile rect or ~0 when culled
    uint4* d_recs = nullptr;             // per surviving triangle: its set-up record (kRecGroups x 16 B), then the clipper's (hard_cap * 4)
    uint32_t* d_hard_list = nullptr;     // triangle ids that need the clipper
    HardTriRec* d_hard_tris = nullptr;   // capacity hard_cap * 4
    uint32_t* d_hard_first = nullptr;    // per regular triangle id: first HardTriRec index
    uint32_t* d_tile_count = nullptr;    // per raster tile
    uint32_t* d_tile_offset = nullptr;
    uint32_t* d_tile_cursor = nullptr;
    int32_t* d_tile_order = nullptr;     // launch order of the tile pass: this frame's tiles by falling bin length
    TileEntry* d_bin_entries = nullptr;   // ScratchState::bin_capacity entries of 64 B (k_fill)
    int scratch_tiles = 0;
    int last_tiles = 0;                  // raster tiles of the target the last chain was built for (the stride of d_tile_order's class regions)
    VrOrderSet ord;                      // the set's stream, marks and pending readers (vr_order.h)
};

struct vr_terrain {
    vr_context* ctx;
    vr_terrain_params p;
    int num_lods;
    float lod_ranges[VR_MAX_LODS];
    DevTex height, albedo;
    TexLayout height_layout, albedo_layout;
    uint8_t* d_height = nullptr; uint8_t* d_albedo = nullptr;
    uint64_t bytes_textures = 0, bytes_scratch = 0;     // vr_terrain_memory_bytes
    uint32_t extra_vert_cap = 0, hard_cap = 0;
    // Per-frame scratch by high-water mark (vr_scratch.h): its capacities, what completed frames wanted, what is still to be reported.
    ScratchState scratch;
    // where the regions behind the per-node ones begin
    uint32_t scratch_tris() const { return (uint32_t)scratch.cap_instances * (uint32_t)kTrisPerInst; }     // regular triangles; the clipper's follow
    size_t clip_rec_base() const { return (size_t)scratch.cap_instances * kTrisPerInst * kRecGroups; }      // 16-byte groups into d_recs
    uint32_t extra_vert_base() const { return (uint32_t)scratch.cap_instances * kVertsPerInst; }            // the clipper's vertices in d_verts
    uint32_t* h_status = nullptr;          // kGeoSets x kStatusWords, hipHostMalloc (mapped)
    uint32_t* d_status = nullptr;          // the device's view of it
    GeoSet sets[kGeoSets];
    GeoSlots<GeoKey> slots;                 // the current set, the prepared frames, the selections (vr_geosets.h)
    // Two geometry streams, taken in turns by successive chains.  Not one per set: HIP multiplexes streams onto 4 hardware
    // queues by default (GPU_MAX_HW_QUEUES), and a frame loop with an exchange stage already uses 2-3 of its own; streams
    // that share a queue serialise (measured: a fifth stream cost the N = 8 rank emulation 0.23 -> 0.39 ms per frame).
    hipStream_t geo_streams[2] = { nullptr, nullptr };
    unsigned geo_turn = 0;
    // QuadTree::SetHeight results: (position.y, extents.y) per node id; m_HeightLoaded
    float2* d_node_heights = nullptr;
    uchar2* d_minmax = nullptr;          // raw (min, max) bytes per node, surface by surface: the mip-style SetHeight's levels (an edit recomputes a node from its children's)
    bool height_loaded = false;
    float texel_size[2] = { 0.0f, 0.0f };   // m_TexelSize (QuadTree.cpp:29)
    int surfaces_per_side = 1;              // WORLD_SIZE / SURFACE_SIZE (TerrainPass.cpp:97)
    // Geometry stream: select / vertex / setup / bins depend only on the view, so they run on their own
    // stream and overlap whatever the context's stream is doing (the lighting pass of the previous frame,
    // or - after vr_terrain_prepare - its tile pass); the tile pass on the context's stream waits for them.
    OrderTerrain<hipEvent_t> ord;          // vr_order.h
    // The three side resources (vr_order.h: order_side_begin / _end / _idle) - the only ordering state of the pyramid, of the
    // journal's arena and of the brush's and the erosions' buffers.  Each event is made with its resource and destroyed with it.
    VrOrderSide ord_pyramid, ord_journal, ord_brush;
    // Terrain queries (vr_query.hip): the min / max pyramid over the surface, built by the first ray cast on the context's stream and
    // kept until vr_terrain_destroy, and the staging memory of the host-pointer mode (grown by doubling).
    uchar2* d_pyramid = nullptr; uint64_t pyramid_bytes = 0;
    void* d_query_stage = nullptr; size_t query_stage_bytes = 0;
    // Brush strokes (vr_brush.hip): the prepared dabs of the latest stroke in pinned host memory and their copy on the device
    // (VR_MAX_BRUSH_DABS each, from the first stroke on) and SMOOTH's snapshot of the map (grown to the largest rectangle so far);
    // ord_brush's event lies behind the latest stroke's kernel - the one reader of all three.  vr_terrain_brush synchronises
    // nothing, so this memory is its own and not d_query_stage, whose users leave it idle when they return: the next stroke
    // takes order_side_idle where the previous stroke has not been consumed yet, whichever stream that one ran on.
    std::vector<BrushDab> brush_prepared;       // a stroke's dabs as they are prepared, before anything touches the device
    BrushDab* h_brush_dabs = nullptr; BrushDab* d_brush_dabs = nullptr;
    std::vector<PathPoint> path_points;         // vr_terrain_path: the caller's points and the segments prepared from them (vr_path.h), host
    std::vector<PathSeg> path_prepared;         // memory that keeps its room from call to call; the segments travel in the dab buffers
    std::vector<RegionVertex> region_verts;     // vr_terrain_region: the vertices and the edges prepared from them (vr_region.h), likewise
    std::vector<RegionEdge> region_prepared;
    void* d_brush_snap = nullptr; size_t brush_snap_bytes = 0;
    // Erosion, thermal and hydraulic (vr_erode.hip): one block of fp32 planes - the mask and two sets of the model's state fields,
    // three planes or seven - of the largest call so far.  Its one reader is the erosion's kernels, which run in front of
    // ord_brush's event: an erosion shares the brush's dab buffers and its side resource, so strokes and erosions of one terrain
    // order against each other, and one erosion against the next one's growth of the block, whichever stream they ran on.
    void* d_erode = nullptr; size_t erode_bytes = 0;
    // What the last erosion call that launched left in the block, for vr_debug_terrain_sweep_state (host side only): the rectangle,
    // the model's field count (0: no record), the floats from one plane to the next and which of the two sets holds the final state.
    struct ErodeRecord { int x = 0, y = 0, w = 0, h = 0, fields = 0, set = 0; size_t plane = 0; } erode_last;
    // History (vr_history.hip): the journal's bookkeeping (vr_history.h) over a table of kHistoryMaxRecords records and one device
    // arena, both from vr_terrain_history_enable on; ord_journal's event lies behind the latest journal kernel.
    vr_gbuffer* pending_target = nullptr;       // the (at most one) G-buffer whose colour planes wait for a frame of this terrain
    HistoryState history;
    std::vector<HistoryRecord> history_table;
    uint8_t* d_history = nullptr;
};
// the map `which` names (0: the heightmap, 1: the albedo) and its layout
inline const DevTex& vr_terrain_map(const vr_terrain* t, int which) { return which == 0 ? t->height : t->albedo; }
inline const TexLayout& vr_terrain_layout(const vr_terrain* t, int which) { return which == 0 ? t->height_layout : t->albedo_layout; }
void vr_query_release(vr_terrain* t);      // frees the above (vr_query.hip)
void vr_brush_release(vr_terrain* t);      // the brush's and the erosions' memory and their event (vr_brush.hip)
// What vr_terrain_brush, vr_terrain_erode and vr_terrain_erode_hydraulic share (vr_brush.hip).  check_dabs: the dab refusals of a stroke of `op` (an opacity
// op for the erosion).  prepare_dabs: the dabs that meet the map `tex`, in order, into t->brush_prepared; returns the hull of their
// spans.  reserve: the event, the pinned and the device dab list and `snap_bytes` of snapshot, before anything is launched.
// grow: one of the buffers read in front of ord_brush's event to `bytes` (vr_reserve).  consumed: order_side_idle(ord_brush), the
// one wait on the host.  (vr_brush_call, the whole path from the dab checks to the recorded event around the
// caller's reserve step and launches, is a template: vr_level0.h.)
struct DirtyRect;
int vr_brush_grow(vr_terrain* t, void** ptr, size_t* capacity, size_t bytes);
int vr_brush_check_dabs(const vr_brush_dab* dabs, uint32_t n, int op);
DirtyRect vr_brush_prepare_dabs(vr_terrain* t, const DevTex& tex, const vr_brush_dab* dabs, uint32_t n);
int vr_brush_reserve(vr_terrain* t, size_t snap_bytes);
int vr_brush_consumed(vr_terrain* t);
void vr_history_release(vr_terrain* t);    // the journal's arena and event; history is off afterwards (vr_history.hip)
// In front of a write of the rectangle `dirty` of level 0 (inside vr_derive_level0_write's write_level0, so behind its waits): with
// history on, a record is appended and the kernel that captures the rectangle is queued on `s`.  Synchronises nothing; with
// history off it does nothing at all.  Its one caller is vr_level0_call (vr_level0.h).
int vr_history_capture(vr_terrain* t, int which, const DirtyRect& dirty, hipStream_t s);
// the staging memory holds at least `bytes` (grown by doubling; on failure the terrain keeps what it had); whoever uses it
// synchronises the context's stream before it returns
int vr_query_reserve_stage(vr_terrain* t, size_t bytes);
constexpr int kPyrMaxLevels = 16;           // (16384 + 1) cells on a side halve to 1 in 16 levels
struct PyrDesc {
    uint32_t off[kPyrMaxLevels];            // first cell of each level, in cells
    int levels;
    int cw, ch;                             // cells of level 0: w0 + 1, h0 + 1
};
PyrDesc vr_pyramid_desc(const vr_terrain* t, size_t* cells);     // (cells: all levels together; may be NULL)
// QuadTree::SetHeight's per-surface inputs (vr_select.hip): the surface's location and, where the mip-style path applies to it,
// the texel origin of its root and the texels per leaf node
struct NodeSurface { float loc[3]; bool dyadic; int rx0, ry0, leaf; };
NodeSurface vr_node_surface(const vr_terrain* t, int surf);
int vr_node_heights_surface(vr_terrain* t, int surf, const NodeSurface& ns);     // the whole reduction of one surface, queued on the context's stream
// Everything derived from a map, (re)built inside a rectangle of its level 0 (vr_derive.hip; rectangles: vr_dirty.h).  Creating a
// terrain passes the whole map, vr_terrain_edit what it replaced.  The three queue launches and report nothing: hipGetLastError
// afterwards.
struct DirtyRect;
// levels 1 .. of the chain at `mem` and the texture's tables (quad, quadf, fast of an R8 map; fast, rgbf, pack of an SRGBA8 one), on the context's stream
void vr_derive_chain(vr_context* ctx, uint8_t* mem, const TexLayout& lay, int w0, int h0, int levels, int texel_bytes, const DirtyRect& dirty);
// the node heights of one surface on the mip-style path (ns.dyadic; d_node_heights and d_minmax exist), on the context's stream
void vr_derive_node_heights(vr_terrain* t, int surf, const NodeSurface& ns, const DirtyRect& dirty);
// the query pyramid at `pyramid`; l0, l1: the rectangle in levels 0 and 1 of the heightmap (a one-level chain: l1 = l0)
void vr_derive_pyramid(const DevTex& hm, const PyrDesc& pd, uchar2* pyramid, const DirtyRect& l0, const DirtyRect& l1, hipStream_t s);
// A write of the rectangle `dirty` of level 0 of a map (which: 0 heightmap, 1 albedo) and everything that follows from it, on the
// context's stream - the one path of vr_level0_call (vr_level0.h: every edit) and of undo and redo: the write waits behind every chain and tile pass queued
// so far, prepared geometry is dropped, write_level0(stream) queues the write itself, then the chain and the tables, the node
// heights and the query pyramid are brought up to date inside their dirty rectangles and every set's next chain runs behind it.
int vr_derive_level0_write(vr_terrain* t, int which, const DirtyRect& dirty, const std::function<int(hipStream_t)>& write_level0);

struct vr_tonemap;
vr_context* vr_tonemap_context(vr_tonemap* tm);
// ---- cross-TU entry points ----------------------------------------------------------
int vr_tex_upload_and_mip(vr_context* ctx, const uint8_t* host, int w, int h, int texel_bytes,
                          DevTex* out, uint8_t** out_mem, uint64_t* out_bytes = nullptr, TexLayout* layout = nullptr);
int vr_select_launch(vr_terrain* t, GeoSet& g, const vr_view* view, float max_height, hipStream_t stream);
// In front of a frame's geometry (vr_terrain_prepare, the tile pass; vr_select.hip).  Completed chains' status words are read (no
// wait) and the scratch grows if due; with `report` a completed frame's device-side condition comes back once, in *earlier - it
// does not stop the frame.  Then target(&tiles) - the call site's RasterArgs, which read the capacities - says how many raster tiles
// this rank draws, the bins get room for them and *bin_capacity is what they hold.  Any other code ends the call at once.
int vr_terrain_frame_scratch(vr_terrain* t, bool report, const std::function<int(size_t* tiles)>& target, int* earlier, uint32_t* bin_capacity);
// vr_frame_submit's tile pass under VR_OPT_FRAME_FUSION (vr_raster.hip): vr_terrain_render of the whole frame that also shades
// into hdr_out where the G-buffer-keeping fused flavour applies (*fused; *fused_stop = that launch's dispatch-stamped stop event
// or NULL) and is exactly vr_terrain_render where it does not - as wherever sky_is_zero (vr_light_domain.h, from vr_light_check) is false
int vr_terrain_render_keep(vr_terrain* t, const vr_view* view, vr_gbuffer* gb, const vr_render_params* rp, const vr_light* lights,
                           int32_t num_lights, const float ambient_top[3], const float ambient_bottom[3], vr_image* hdr_out,
                           bool sky_is_zero, bool* fused, VrEventRef* fused_stop);
// the lighting passes as vr_frame_submit queues them: vr_light_check, vr_light_queue (vr_deferred_dev.h)
// The tone-map stage (vr_tonemap.hip): the steps of `steps` (TmStep, vr_tonemap_plan.h) in their order - reset, histogram, all-reduce
// over `comm`, exposure, render - behind every refusal of every one of them; queue = false: the refusals alone.  `frame`:
// vr_frame_submit's descriptor, whose stage also answers for the exchange that follows it (frame_device: the terrain's).
struct TmStageCall {
    unsigned steps;
    const vr_tonemap_params* p; float frame_time;
    vr_image* hdr; int w, h; void* ldr; size_t ldr_capacity; const vr_partition* part;
    void* comm;
    const vr_frame_desc* frame; int frame_device;
};
int vr_tonemap_stage(vr_tonemap* tm, const TmStageCall& c, bool queue);
int vr_rccl_load();       // the RCCL entry points, resolved at first use (vr_comm.hip); VR_OK, or the refusal that names what is missing
// the de-tile kernels' refusals, for the wrappers that put a collective in front of them (vr_comm.hip)
int vr_frame_detile_check(vr_context* ctx, const void* gathered, int32_t world, vr_image* frame);
int vr_frame_detile_ldr_check(vr_context* ctx, const void* gathered, int32_t world, int32_t w, int32_t h, void* frame);
// tables of (w, h, part); part == NULL is the whole frame as rank 0 of 1
int vr_partition_tables(vr_context* ctx, int w, int h, const vr_partition* part, const PartTables** out);
// any cached table set of (w, h, world): the slot table does not depend on the rank
int vr_partition_slot_tables(vr_context* ctx, int w, int h, int world, const PartTables** out);

// The geometry kernels (select, vertex, setup, clip, scan, fill) are short and latency-bound and run on CUs full of
// tile-pass waves: they raise their waves' issue priority so that their few instructions are not queued behind the tile
// pass's many (the sequencer arbitrates by priority, then age).
#ifndef VR_GEOMETRY_PRIO
#define VR_GEOMETRY_PRIO 3
#endif
#define VR_GEOMETRY_PRIORITY() __builtin_amdgcn_s_setprio(VR_GEOMETRY_PRIO)

// ---- device helpers shared by kernels ---------------------------------------------------
__device__ __forceinline__ float vr_max(float a, float b) { return a > b ? a : b; }
__device__ __forceinline__ float vr_min(float a, float b) { return a < b ? a : b; }
// x clamped to [lo, hi] in one instruction (v_med3_f32); x must not be NaN
__device__ __forceinline__ float vr_clampf(float x, float lo, float hi) { return __builtin_amdgcn_fmed3f(x, lo, hi); }
// 1 / d and sqrt(x), correctly rounded, for operands well inside the normal range (2^-60 < |d|, x < 2^60): short sequences
// found by exhaustive search (tools/micro/exact_math.hip, profiles/r03_exact_math_search.txt: every float of the range
// compared with 1.0f / d and sqrtf(x) on the device; the product's copies are swept again by vr_debug_fastmath_check).
//   reciprocal : v_rcp_f32 (1 ulp) + ONE Newton step with an exact fma residual      (the compiler's IEEE division: 10 instructions)
//   square root: v_rsq_f32 + the compiler's own refinement without the range scaling (no compare / select)
__device__ __forceinline__ float vr_rcp_exact(float d)
{
    const float r = __builtin_amdgcn_rcpf(d);
    const float e = __builtin_fmaf(-d, r, 1.0f);
    return __builtin_fmaf(e, r, r);
}
__device__ __forceinline__ float vr_sqrt_exact(float x)
{
    const float r = __builtin_amdgcn_rsqf(x);
    float s = x * r, h = 0.5f * r;
    const float e = __builtin_fmaf(-h, s, 0.5f);
    h = __builtin_fmaf(h, e, h);
    s = __builtin_fmaf(s, e, s);
    const float d = __builtin_fmaf(-s, s, x);
    return __builtin_fmaf(d, h, s);
}
__device__ __forceinline__ float vr_saturate(float x) { return vr_min(vr_max(x, 0.0f), 1.0f); }
__device__ __forceinline__ float vr_dot3(float ax, float ay, float az, float bx, float by, float bz)
{
    return (ax * bx + ay * by) + az * bz;
}
