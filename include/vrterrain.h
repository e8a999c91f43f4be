/*
 * vrterrain.h — C ABI of libvrterrain.so: the MI355X-native (gfx950) terrain +
 * deferred-shading hot path of Viictor/vrenderer.
 *
 * Every entry point names the reference interface it replaces (file:line relative
 * to the reference tree).  Conventions:
 *   - POD structs, opaque handles, `int` status (0 = VR_OK), no exceptions cross
 *     the boundary;
 *   - host memory is caller-owned, device memory is library-owned unless an entry
 *     point says "device pointer";
 *   - all GPU work is stream-ordered on the context's stream (vr_context_set_stream
 *     takes a caller hipStream_t); nothing synchronises unless it returns host data;
 *   - one context per device, not thread-safe per context (the reference drives the
 *     path from one thread and one command list, Renderer.cpp:321-454).
 *
 * Matrices are row-major float4x4 used with ROW vectors (v' = v * M), exactly the
 * layout of Donut's PlanarViewConstants consumed by terrain_vs.hlsl:60-61.
 */
#ifndef VRTERRAIN_H
#define VRTERRAIN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VR_API __attribute__((visibility("default")))

/* ---- status codes -------------------------------------------------------- */
enum {
    VR_OK = 0,
    VR_ERR_INVALID_ARGUMENT = 1,
    VR_ERR_NO_DEVICE = 2,        /* no HIP device / HIP runtime error            */
    VR_ERR_OUT_OF_MEMORY = 3,
    VR_ERR_TOO_MANY_INSTANCES = 4, /* select produced > max_instances nodes
                                      (reference: assert, TerrainPass.cpp:238)   */
    VR_ERR_OVERFLOW = 5,         /* an internal work list overflowed             */
    VR_ERR_HIP = 6
};

/* ---- compile-time settings of the reference, as runtime fields ------------ */
/* TerrainSettings (TerrainPass.h:23-30), QuadTree::MAX_LODS (QuadTree.h:67),
 * minLodDistance (QuadTree.cpp:236), morph start (terrain_vs.hlsl:20). */
#define VR_MAX_LODS 12

typedef struct vr_terrain_params {
    int32_t max_instances;    /* MAX_INSTANCES = 4096                          */
    float   surface_size;     /* SURFACE_SIZE  = 2048 (quadtree width=height)  */
    float   world_size;       /* WORLD_SIZE    = 2048                          */
    int32_t grid_size;        /* GRID_SIZE     = 32 (must be 32 in this build) */
    float   min_lod_distance; /* 4.0                                           */
    float   morph_start;      /* 0.85                                          */
    float   location[3];      /* quadtree centre (TerrainPass.cpp:108)         */
    int32_t reserved;
} vr_terrain_params;

/* What the path reads from donut::engine::IView / PlanarViewConstants
 * (terrain_vs.hlsl:46,60-61; TerrainPass.cpp:181,280-282,301-302). */
typedef struct vr_view {
    float   world_to_view[16];
    float   view_to_clip[16];
    float   world_to_clip[16];
    float   clip_to_world[16];
    float   camera_pos[4];      /* matViewToWorld[3] = IView::GetViewOrigin()     */
    float   planes[6][4];       /* dm::frustum: outward normal xyz, distance w;
                                   order NEAR, FAR, LEFT, RIGHT, TOP, BOTTOM;
                                   a point is outside when dot(n,p) - w > 0      */
    int32_t viewport_x, viewport_y, viewport_w, viewport_h;
    int32_t mirrored;           /* IView::IsMirrored() -> frontCounterClockwise   */
    int32_t reverse_depth;      /* IView::IsReverseDepth() (must be 0 here)       */
    int32_t reserved[2];
} vr_view;

/* Donut InstanceData as filled by TerrainPass::UpdateTransforms
 * (TerrainPass.cpp:243-253): 16-byte header + two float3x4 (row-major rows). */
typedef struct vr_instance {
    uint32_t padding;
    uint32_t first_geometry_instance_index;
    uint32_t first_geometry_index;
    uint32_t num_geometries;
    float    transform[12];
    float    prev_transform[12];
} vr_instance;

/* TerrainPass::RenderParams (TerrainPass.h:68-73) + EditorParams::m_MaxHeight
 * (Renderer.h:40, read at TerrainPass.cpp:155). */
typedef struct vr_render_params {
    int32_t wireframe;    /* EditorParams::m_Wireframe -> RasterFillMode::Wireframe (TerrainPass.cpp:476): triangle edges as aliased lines */
    int32_t lock_view;    /* reuse the previous selection (TerrainPass.cpp:173,191)  */
    int32_t depth_only;   /* PS = null (TerrainPass.cpp:465)                         */
    int32_t assume_cleared; /* extension: 1 = caller guarantees the G-buffer holds its
                               clear values, so the pass need not read depth back and
                               writes clear values itself (fuses RenderTargets::Clear,
                               Renderer.cpp:382)                                     */
    float   max_height;   /* EditorParams::m_MaxHeight = 400                         */
    int32_t depth_ranges; /* extension: 1 = leave the depth range of every 32x32 light tile with the G-buffer
                             (needs assume_cleared, shaded fill mode); vr_deferred_light_tiled's culling
                             stage then takes them instead of reading the depth plane again.  Any other
                             write to the G-buffer in between (clear, upload, another render) drops them,
                             and a G-buffer whose pointers were handed out (vr_gbuffer_describe) never
                             gets them; results are identical either way                      */
    int32_t reserved[2];
} vr_render_params;

/* Donut LightConstants subset consumed by the deferred pass (ShadeSurface): directional lights
 * (direction, irradiance, angular size), point and spot lights (position, 1/range, optional source
 * radius; spot: cone axis = direction, inner/outer half angles in radians). */
enum { VR_LIGHT_DIRECTIONAL = 1, VR_LIGHT_SPOT = 2, VR_LIGHT_POINT = 3 };
typedef struct vr_light {
    float   direction[3];  int32_t type;
    float   position[3];   float   radius;            /* source radius (0 = punctual) */
    float   color[3];      float   intensity;         /* irradiance (directional)     */
    float   angular_size_or_inv_range;                /* radians | 1/range            */
    float   inner_angle, outer_angle;
    float   out_of_bounds_shadow;
} vr_light;
/* Every float field a light's type reads must be finite (directional: direction, color, intensity, angular size,
 * out_of_bounds_shadow; point: position, color, intensity, 1/range, radius; spot: a point light's and direction, inner_angle,
 * outer_angle): every entry that takes lights refuses a NaN or an infinity with VR_ERR_INVALID_ARGUMENT and names the field. */

/* G-buffer planes (Donut GBufferRenderTargets formats; 28 B/pixel, row-major):
 *   depth    float32                 (cleared to 1.0)
 *   diffuse  SRGBA8_UNORM   (u32)    rgb albedo, a opacity
 *   specular SRGBA8_UNORM   (u32)    rgb F0,     a occlusion
 *   normals  RGBA16_SNORM   (2xu32)  xyz normal, w roughness
 *   emissive RGBA16_FLOAT   (2xu32)  rgb emissive
 * HDR colour: RGBA16_FLOAT (8 B/pixel, Renderer.h:69-79). */
typedef struct vr_gbuffer_desc {
    int32_t width, height;
    void*   depth;     /* device pointers */
    void*   diffuse;
    void*   specular;
    void*   normals;
    void*   emissive;
} vr_gbuffer_desc;

/* Screen-tile partition of one frame over the GPUs of a node. */
#define VR_OWNER_TILE 128
typedef struct vr_partition {
    int32_t rank, world_size;   /* owner(tx,ty) = (tx + ty) mod world_size; 1 <= world_size <= 64 */
} vr_partition;

typedef struct vr_context  vr_context;
typedef struct vr_terrain  vr_terrain;
typedef struct vr_gbuffer  vr_gbuffer;
typedef struct vr_image    vr_image;    /* RGBA16F image in device memory        */

/* ---- context --------------------------------------------------------------- */
/* nvrhi::IDevice + the single command list (main.cpp:57-61, Renderer.cpp:48). */
VR_API int  vr_context_create(int device_ordinal, vr_context** out);
VR_API void vr_context_destroy(vr_context* ctx);
/* What the host owes: the new stream runs behind the work the library queued on the old one (a wait for an event recorded
 * there, or a synchronise).  This orders everything a terrain keeps on the context's stream alone: the maps, their chains and
 * tables, the query pyramid, the history journal, the brush and erosion buffers, and device-pointer queries not yet waited for. */
VR_API int  vr_context_set_stream(vr_context* ctx, void* hip_stream);
VR_API int  vr_context_synchronize(vr_context* ctx);          /* Renderer::Submit + wait */
/* Options.  VR_OPT_ASYNC_GEOMETRY (default 1): vr_terrain_render runs its view-dependent geometry
 * stages (select, vertex, setup, bins) on a second stream, so that they overlap whatever the caller
 * queued on the context's stream after the previous vr_terrain_render (typically vr_deferred_light
 * of the previous frame); the tile pass stays on the context's stream.  0 = everything on one stream. */
/* VR_OPT_DISPATCH_EVENTS (default 1): the two big kernels of a frame (tile pass, lighting pass) are launched with
 * hipExtLaunchKernelGGL, whose start/stop events are stamped by the dispatch itself, and the stop events double as the
 * cross-stream dependencies - no event-record packets sit between the two kernels.  0 = explicit hipEventRecord. */
/* VR_OPT_RASTER_TILE (default 0): edge of the tile pass's raster tiles - 0 = chosen by frame size and split (32 pixels below
 * ~13000 64-pixel tiles per rank, i.e. up to about 9.6K x 5.4K; 64 above), 32 or 64 = pinned.  The rendered frame does not depend on it. */
/* VR_OPT_PLANE_TRACKING (default 1): main_ps writes 0 to the emissive target for every pixel (terrain_ps.hlsl:80) and Clear writes 0
 * everywhere, so on this path the emissive plane - 8 of the G-buffer's 28 B/pixel - only ever holds zeros.  While the library knows
 * the plane is all zero (it cleared it - vr_gbuffer_create / vr_gbuffer_clear - or a tile pass that writes every pixel ran since the
 * last foreign write) the tile pass does not rewrite it; the plane's contents are the same either way.  vr_gbuffer_upload of the
 * plane ends that knowledge until the next clear or whole-target pass; vr_gbuffer_describe ends it for good (the pointers have left
 * the library), and likewise the depth ranges of vr_render_params::depth_ranges.  0 = every pass writes all five planes. */
/* VR_OPT_SCRATCH_WORST_CASE (default 0): a terrain's per-frame scratch (vertices, triangle records, bins: three rotating sets) is sized
 * by the high-water mark of the node counts its frames select - 1024 nodes to begin with (1.3 GB for the three sets), doubled before a
 * frame can exceed it - instead of for max_instances (4096: 5 GB).  1 (set BEFORE vr_terrain_create): worst case up front, no growth,
 * no frame can ever be truncated by the scratch. */
/* VR_OPT_FRAME_FUSION (default 1; a context starts with 0 where the environment holds VR_FRAME_FUSION=0): vr_frame_submit shades
 * the pixels in the tile pass itself and STILL writes the whole G-buffer - one kernel (timed as VR_K_RASTER_LIT) instead of tile pass +
 * lighting pass, the same bits in all five planes, HdrColor, the region states and the plane knowledge.  Taken for: the whole frame
 * (part == NULL), not tiled, no shadow, at most 16 directional / punctual point lights, the tile pass's fast variant on 32-pixel
 * tiles, a target known cleared (assume_cleared = 1 or a pending vr_gbuffer_clear), shaded fill mode without depth ranges, a
 * viewport that covers the target, a width that is a multiple of 4, and VR_OPT_PLANE_TRACKING with the emissive plane known zero.
 * Any other frame - and every frame with 0 - queues the two passes as before. */
/* VR_OPT_GBUFFER_LAZY (default 1; a context starts with 0 where the environment holds VR_GBUFFER_LAZY=0): a frame that
 * VR_OPT_FRAME_FUSION shades in the tile pass leaves the G-buffer's diffuse, specular and normals planes (and the region states) to
 * their first reader.  The frame's one kernel stores depth and HdrColor - the same bits - and the library records the frame (view,
 * render parameters, terrain).  Every call that reads those planes or the region states, writes part of them, or changes what the
 * recorded frame would draw first queues the frame's plain tile pass on the context's stream, so that each of them finds exactly what
 * the eager frame leaves: vr_deferred_light*, vr_gbuffer_download / _upload / _describe / _region_census, a vr_terrain_render* that
 * does not write every pixel of every plane (keep-what-is-there, a partition, depth only, wireframe, vr_terrain_render_lit),
 * vr_terrain_edit / _brush / _texture / _stamp / _erode / _erode_hydraulic / _noise / _path / _region / _occlusion / _undo / _redo / _update_heights, vr_terrain_destroy.  Its error, if any, is that call's.  The next
 * whole-frame pass over a cleared target, or vr_gbuffer_clear, replaces the record: a frame nobody looked at costs nothing.  Depth is
 * never pending.  The first time a target's planes have to be produced this way ends the laziness for that target for good: a host
 * that reads the G-buffer pays one extra tile pass once and gets the G-buffer-keeping frames from then on.  The record holds the
 * vr_terrain pointer: destroy the target, or let a reader run, before a terrain with frames still recorded is handed to another
 * thread.  Not taken with lock_view.  0 = every fused frame writes the whole G-buffer. */
enum { VR_OPT_ASYNC_GEOMETRY = 1, VR_OPT_DISPATCH_EVENTS = 2, VR_OPT_RASTER_TILE = 3, VR_OPT_PLANE_TRACKING = 4, VR_OPT_SCRATCH_WORST_CASE = 5,
       VR_OPT_FRAME_FUSION = 6, VR_OPT_GBUFFER_LAZY = 7 };
VR_API int  vr_context_set_option(vr_context* ctx, int option, int value);
VR_API const char* vr_last_error(void);
VR_API const char* vr_version(void);
/* 0 for a product build.  Non-zero: the library was built with timing-experiment or profiling switches
 * (csrc/vr_experiments.h: -DVR_EXPERIMENT_BUILD + VR_EXP_* / VR_*_PROFILE) and may render wrong images on purpose. */
VR_API uint32_t vr_build_experiments(void);

/* Per-kernel timing with HIP events recorded on the context's stream, the analogue of
 * the reference's PROFILE_GPU_SCOPE timestamp queries (Profiler.h:55-125,
 * Renderer.cpp:326-437).  Kernel ids: */
enum { VR_K_SELECT = 0, VR_K_VERTEX, VR_K_SETUP, VR_K_CLIP, VR_K_SCAN, VR_K_FILL, VR_K_RASTER,
       VR_K_DEFERRED, VR_K_DETILE, VR_K_CLEAR, VR_K_DEFERRED_TILED, VR_K_NODE_HEIGHTS,
       VR_K_TM_HISTOGRAM, VR_K_TM_EXPOSURE, VR_K_TONEMAP, VR_K_DETILE_LDR, VR_K_RASTER_DEPTH, VR_K_LIGHT_CULL, VR_K_RASTER_LIT,
       VR_K_QUERY_HEIGHTS, VR_K_QUERY_RAYS, VR_K_QUERY_PYRAMID, VR_K_COUNT };
/* (VR_K_COUNT grows when kernels are added - 16 in round 2, 18 in round 3, 19 in round 4, 22 with the terrain queries: size vr_timing_collect's arrays with the
 * constant of the header the host is compiled against AND check vr_timing_kernel_count() at run time) */
VR_API int  vr_timing_kernel_count(void);
VR_API int  vr_timing_enable(vr_context* ctx, int enable);     /* also resets the samples; 1 = every kernel (two event records per
                                                                * launch), 2 = only the tile pass and the lighting passes, whose
                                                                * events the dispatch stamps at no host cost */
/* Synchronises the stream; per kernel id: summed milliseconds and launch count since
 * the last enable/collect; resets the samples. */
VR_API int  vr_timing_collect(vr_context* ctx, float ms_sum[VR_K_COUNT], int32_t launches[VR_K_COUNT]);
VR_API const char* vr_kernel_name(int id);

/* ---- host helper: what FirstPersonCamera::LookAt + perspProjD3DStyle +
 * PlanarView::UpdateCache produce (Renderer.cpp:97,312-319).  Pure host code. -- */
VR_API int vr_view_from_camera(const float eye[3], const float target[3], const float up[3],
                               float vertical_fov_radians, float z_near, float z_far,
                               int32_t width, int32_t height, vr_view* out);
VR_API void vr_terrain_default_params(vr_terrain_params* out);
VR_API void vr_render_default_params(vr_render_params* out);

/* ---- terrain --------------------------------------------------------------- */
/* TerrainPass::Init + QuadTree::QuadTree/Init (TerrainPass.cpp:34-141,
 * QuadTree.cpp:10-52).  height_r8: hm_w*hm_h bytes; albedo_srgba8: al_w*al_h*4
 * bytes (decoded with sRGB=true, Renderer.cpp:55).  Both are copied to the device
 * and mip chains are generated there (Donut TextureCache mip generation).
 * Limits: each texture at most 16384 texels on a side and 2^26 texels in all (8192 x 8192): the tile pass
 * reads decoded copies (16 B per texel / footprint, x 4/3 for the mips) through 32-bit offsets.  The albedo has
 * one such table more, the sRGB8 codes of every bilinear footprint packed into 16 B, which the fused frame kernel
 * reads instead of the decoded texels: +90 MB per 2048 x 2048 terrain, and the steady-state frame then touches
 * 180 MB of tables (90 of height footprints, 90 of packed albedo footprints) through a quarter of the albedo
 * fetches.  Device memory held by a terrain: vr_terrain_memory_bytes(). */
VR_API int  vr_terrain_create(vr_context* ctx, const vr_terrain_params* params,
                              const uint8_t* height_r8, int32_t hm_w, int32_t hm_h,
                              const uint8_t* albedo_srgba8, int32_t al_w, int32_t al_h,
                              vr_terrain** out);
VR_API void vr_terrain_destroy(vr_terrain* t);
VR_API int  vr_terrain_num_lods(const vr_terrain* t);                 /* QuadTree::GetNumLods  */
VR_API int  vr_terrain_lod_ranges(const vr_terrain* t, float out[VR_MAX_LODS]); /* GetLodRanges */
/* test/IO helper: read back one level of the device mip chain (which: 0 heightmap R8,
 * 1 albedo SRGBA8); *w,*h receive the level size; host may be NULL to query sizes. */
VR_API int  vr_terrain_download_mip(vr_terrain* t, int which, int level, void* host, size_t bytes,
                                    int32_t* w, int32_t* h, int32_t* levels);
/* In-place edit of level 0 of a terrain's heightmap (which = 0, R8: 1 byte per texel) or albedo (which = 1, SRGBA8: 4 bytes per
 * texel): the w x h texels at (x, y) are replaced by `texels` (rows row_pitch_bytes apart; 0 = tightly packed).  Afterwards
 * every call on the terrain behaves exactly as on a terrain created from the edited arrays: the mip chain and the decoded
 * tables, the node heights (where vr_terrain_update_heights(t, 1) is in force) and the query pyramid (where a ray cast has built
 * it) are rebuilt inside the dirty rectangle of each, with the arithmetic vr_terrain_create uses.  Geometry prepared ahead
 * (vr_terrain_prepare, vr_frame_desc::prepare_views) is stale after an edit of either map and is built again by the frame that
 * would have used it; a lock_view frame keeps reusing the selection of the last unlocked frame.
 * Order: the edit is stream-ordered on the context's stream, behind every geometry chain and tile pass queued so far.
 *   device_pointer = 1: `texels` is device memory; the call synchronises nothing, and the caller keeps `texels` alive and
 *     unchanged until the stream has passed the edit.
 *   device_pointer = 0: `texels` is the caller's host memory; the call returns once it has been consumed (it synchronises the
 *     stream, as vr_terrain_create does; staging memory is kept with the terrain, shared with the queries).
 * w == 0 or h == 0 is VR_OK and queues nothing.  VR_ERR_INVALID_ARGUMENT, checked before the first use of the device, with the
 * terrain untouched and nothing launched: a NULL pointer with a non-empty rectangle; `which` not 0 or 1; a negative coordinate
 * or extent; a rectangle not wholly inside level 0; a non-zero pitch smaller than w texels; a device pointer (or its pitch) not
 * aligned to the texel size.  An edit allocates nothing once it has begun to write: the staging memory of the host-pointer mode
 * is reserved before anything is launched, and a refusal (VR_ERR_OUT_OF_MEMORY) leaves the terrain as it was.
 * Timing: the node-height work counts under VR_K_NODE_HEIGHTS, the pyramid work under VR_K_QUERY_PYRAMID; the mip and table
 * kernels are untimed, as at create time. */
VR_API int vr_terrain_edit(vr_terrain* t, int which, int32_t x, int32_t y, int32_t w, int32_t h,
                           const void* texels, size_t row_pitch_bytes, int device_pointer);
/* A brush stroke - one op and up to VR_MAX_BRUSH_DABS dabs, applied in list order - on level 0 of the heightmap (RAISE, FLATTEN,
 * SMOOTH) or the albedo (PAINT), computed on the device from the map as it is there, followed by the refresh vr_terrain_edit does:
 * afterwards the terrain is the one vr_terrain_create builds from the stroked maps.  A dab is a disc of `radius` world units
 * about (x, z) - the world spans [-world_size/2, world_size/2]^2, as for the queries - with weight 1 out to hardness * radius and
 * a smoothstep fall-off to 0 at the rim.  Each texel's value (0 .. 255, the stored byte; four for the albedo) is carried in fp32
 * through the dabs that cover it, with a = weight * strength:
 *   VR_BRUSH_RAISE    value += weight * strength      strength signed, in heightmap steps (1/255 of max_height), |strength| <= 255
 *   VR_BRUSH_FLATTEN  value += a * (target - value)   strength = opacity in [0, 1], target in [0, 255]
 *   VR_BRUSH_SMOOTH   value += a * (mean - value)     mean of the 3 x 3 clamped neighbourhood in the map BEFORE the stroke
 *   VR_BRUSH_PAINT    per channel c of channel_mask (bit c = byte c of the SRGBA8 texel, alpha included):
 *                     value_c += a * (color[c] - value_c), color in [0, 255] in the stored encoding
 * clamped to [0, 255] after every dab and rounded to the nearest byte once, after the last: sub-step strengths accumulate inside
 * a stroke, and a stroke split over two calls is two roundings.  A texel no dab covers keeps its byte.  The arithmetic is defined
 * bit for bit in vrenderer_amd/csrc/vr_brush.h.
 * out_rect (may be NULL) receives {x, y, w, h} of the level-0 rectangle the call treated as dirty - the hull of the dabs'
 * conservative spans, clipped to the map; no texel outside it changes - or {0, 0, 0, 0} when that is empty.
 * `dabs` is host memory and may be reused as soon as the call returns.  The call is stream-ordered on the context's stream, like
 * a device-pointer edit, and synchronises nothing: the host waits only where the previous stroke of this terrain has not been
 * consumed yet.  n == 0, or a stroke whose dabs all miss the map, is VR_OK and launches nothing.
 * VR_ERR_INVALID_ARGUMENT, checked before the first use of the device, with the terrain untouched: NULL t or stroke, NULL dabs
 * with n > 0; n > VR_MAX_BRUSH_DABS; an unknown op; a NaN or an infinity in target, color or a dab; radius <= 0; hardness outside
 * [0, 1); a strength outside its op's range; FLATTEN with target outside [0, 255]; PAINT with a color outside [0, 255] or a
 * channel_mask of 0 or above 15.  The memory a stroke needs is reserved before anything is launched (VR_ERR_OUT_OF_MEMORY leaves
 * the terrain as it was).  Timing: as for vr_terrain_edit; the brush kernel itself is untimed. */
#define VR_MAX_BRUSH_DABS 4096
enum { VR_BRUSH_RAISE = 0, VR_BRUSH_FLATTEN = 1, VR_BRUSH_SMOOTH = 2, VR_BRUSH_PAINT = 3 };
typedef struct vr_brush_dab    { float x, z, radius, hardness, strength; float reserved[3]; } vr_brush_dab;      /* 32 B */
typedef struct vr_brush_stroke { int32_t op; uint32_t channel_mask; float target; float color[4]; int32_t reserved; } vr_brush_stroke; /* 32 B */
VR_API int vr_terrain_brush(vr_terrain* t, const vr_brush_stroke* stroke, const vr_brush_dab* dabs, uint32_t n, int32_t out_rect[4]);
/* Level 0 of the albedo painted by rule from the heightmap's shape - rock on steep ground, snow above a line, grass on the flats -
 * under a brush mask or over the whole map, computed on the device from both maps as they are there and followed by the refresh
 * vr_terrain_edit does: afterwards the terrain is the one vr_terrain_create builds from the heightmap and the textured albedo.
 * Each albedo texel samples the heightmap bilinearly at its own centre: the height h (in heightmap steps) and the gradient by
 * central differences of level 0, scaled by max_height and the world's size to the squared tangent of the slope.  A layer weighs
 *   wl = band(h; alt_lo, alt_hi, alt_fade) * band(slope; slope_lo, slope_hi, slope_fade) * opacity
 * where a band is 1 inside [lo, hi], falls to 0 by a smoothstep over `fade` outside each end (a fade of 0 is a hard edge) and the
 * slope band is evaluated on squared tangents: lo - fade clamps at 0 degrees, hi + fade at 89.5.  The layers are applied in list
 * order, as PAINT dabs are: per channel c of the layer's channel_mask value_c += (m * wl) * (color[c] - value_c), clamped to
 * [0, 255] after every layer and rounded to the nearest byte once, after the last.  m is the mask of vr_terrain_erode (below) of
 * the dabs, prepared for the albedo map with their strength an opacity - per texel the largest weight * strength, so their order
 * does not matter - or 1 on every texel with VR_TEXTURE_WHOLE_MAP, which needs dabs == NULL and n == 0 and whose rectangle is the
 * whole map.  A texel with mask 0 is not written; one whose layers all weigh 0 keeps its byte.  The arithmetic is defined bit for
 * bit in vrenderer_amd/csrc/vr_texture.h, without a division, a square root or trigonometry on the device.
 * out_rect, `dabs`, the stream order and what the host waits for are vr_terrain_brush's: the call synchronises nothing, and is
 * ordered against the strokes and erosions of the terrain; the heightmap is read behind its last writer.  `layers` is host memory,
 * consumed before the call returns.  With history on, one call is one record.  n == 0 without the flag, or dabs that all miss the
 * map, is VR_OK and launches nothing.
 * VR_ERR_INVALID_ARGUMENT, checked before the first use of the device, with the terrain untouched: NULL t, p or layers; num_layers
 * outside 1 .. VR_TEXTURE_MAX_LAYERS; unknown flag bits; VR_TEXTURE_WHOLE_MAP together with dabs; NULL dabs with n > 0;
 * n > VR_MAX_BRUSH_DABS; a non-zero reserved word; max_height NaN, infinite or <= 0; a NaN or an infinity in a layer; a color
 * outside [0, 255]; an opacity outside [0, 1]; alt_lo > alt_hi; a negative fade; slope bounds outside 0 <= lo <= hi <= 89; a
 * channel_mask of 0 or above 15; the dab refusals of vr_terrain_brush with an opacity for a strength.  The memory a call needs is
 * reserved before anything is launched (VR_ERR_OUT_OF_MEMORY leaves the terrain as it was).  Timing: as for vr_terrain_edit; the
 * texture kernel itself is untimed. */
#define VR_TEXTURE_MAX_LAYERS 8
enum { VR_TEXTURE_WHOLE_MAP = 1 };
typedef struct vr_texture_layer {      /* 64 B */
    float color[4];                    /* stored encoding, [0, 255], like PAINT's */
    float opacity;                     /* [0, 1] */
    float alt_lo, alt_hi, alt_fade;    /* world units of height; the band [alt_lo, alt_hi], faded over alt_fade outside each end */
    float slope_lo, slope_hi, slope_fade; /* degrees, 0 <= lo <= hi <= 89; fade >= 0; lo - fade clamps at 0, hi + fade at 89.5 */
    uint32_t channel_mask;             /* 1 .. 15, like PAINT's */
    int32_t reserved[4];               /* zero */
} vr_texture_layer;
typedef struct vr_texture_params { int32_t num_layers; uint32_t flags; float max_height; int32_t reserved[5]; } vr_texture_params; /* 32 B */
VR_API int vr_terrain_texture(vr_terrain* t, const vr_texture_params* p, const vr_texture_layer* layers,
                              const vr_brush_dab* dabs, uint32_t n, int32_t out_rect[4]);
/* Sky visibility (ambient occlusion, "cavity") baked into level 0 of the albedo by horizon marching - a valley floor darker than a
 * ridge with the same normal - under a brush mask or over the whole map, computed on the device from both maps as they are there and
 * followed by the refresh vr_terrain_edit does: afterwards the terrain is the one vr_terrain_create builds from the heightmap and
 * the new albedo.  The renderer is unchanged: no occlusion reaches shading except through the albedo's bytes.
 * Each albedo texel stands on the height texel under its centre and marches level 0 of the heightmap from there along `directions`
 * (4, 8 or 16) fixed directions - steps of (1,0), (2,1), (1,1), (1,2), ... height texels - out to `radius` world units.  A direction
 * keeps its steepest horizon, the largest rise over distance of the samples inside the map (a sample outside the map is skipped),
 * as a tangent t >= 0 less `bias`, and sees v = 1 - sin(atan(t)) of the sky, by a 64-interval table over t in [0, 8].  The texel's
 * visibility is the mean of its directions' and its occlusion o = min((1 - visibility) * gain, 1).
 *   VR_OCCLUSION_TINT   per channel c of channel_mask value_c += (m * (o * opacity)) * (color[c] - value_c)
 *   VR_OCCLUSION_STORE  per channel c of channel_mask value_c += (m * opacity) * (255 * (1 - o) - value_c): the visibility as a byte,
 *                       into a spare channel for instance
 * clamped to [0, 255] and rounded to the nearest byte.  m is the mask of vr_terrain_texture: the dabs prepared for the albedo with
 * their strength an opacity, or 1 on every texel with VR_OCCLUSION_WHOLE_MAP, which needs dabs == NULL and n == 0 and whose
 * rectangle is the whole map.  A texel with mask 0 is not written.  The arithmetic is defined bit for bit in
 * vrenderer_amd/csrc/vr_occlusion.h, without a division, a square root or trigonometry on the device.
 * out_rect, `dabs`, the stream order and what the host waits for are vr_terrain_texture's: the call synchronises nothing, and the
 * heightmap is read behind its last writer.  With history on, one call is one record.  n == 0 without the flag, or dabs that all
 * miss the map, is VR_OK and launches nothing.
 * VR_ERR_INVALID_ARGUMENT, checked before the first use of the device, with the terrain and its history untouched: NULL t or p;
 * unknown flag bits; VR_OCCLUSION_WHOLE_MAP together with dabs; NULL dabs with n > 0; n > VR_MAX_BRUSH_DABS; a non-zero reserved
 * word; an unknown mode; directions not 4, 8 or 16; a NaN or an infinity in a float; radius <= 0; max_height <= 0; gain outside
 * [0, 16]; bias outside [0, 8); opacity outside [0, 1]; a color outside [0, 255]; a channel_mask of 0 or above 15; the dab refusals
 * of vr_terrain_brush with an opacity for a strength; and a radius whose march reaches more than VR_OCCLUSION_MAX_REACH height
 * texels on either axis in some direction (steps * max(|dx|, |dz|) > 64) - refused, not clamped.  Timing: as for vr_terrain_edit;
 * the occlusion kernel itself is untimed. */
#define VR_OCCLUSION_MAX_REACH 64          /* height texels, per axis */
#define VR_OCCLUSION_TINT  0
#define VR_OCCLUSION_STORE 1
#define VR_OCCLUSION_WHOLE_MAP 1u
typedef struct vr_occlusion_params {       /* 64 B */
    float    radius;                       /* world units, > 0 */
    float    max_height;                   /* the world height of byte 255: finite, > 0 (as vr_texture_params) */
    float    gain;                         /* [0, 16]: occlusion = min((1 - visibility) * gain, 1) */
    float    bias;                         /* [0, 8): subtracted from every horizon tangent; hides 8-bit terracing */
    float    opacity;                      /* [0, 1] */
    float    color[4];                     /* TINT: the shadow colour, stored encoding, [0, 255] */
    uint32_t channel_mask;                 /* 1 .. 15 */
    int32_t  directions;                   /* 4, 8 or 16 */
    uint32_t mode;                         /* VR_OCCLUSION_TINT / _STORE */
    uint32_t flags;                        /* VR_OCCLUSION_WHOLE_MAP */
    uint32_t reserved[3];                  /* zero */
} vr_occlusion_params;
VR_API int vr_terrain_occlusion(vr_terrain* t, const vr_occlusion_params* p, const vr_brush_dab* dabs, uint32_t n, int32_t out_rect[4]);
/* Procedural noise on level 0 of the heightmap (which = 0) or the albedo (1) - roughen a plateau, break up a smooth flank, speckle
 * an albedo, or make a fractal base terrain on a flat map - under a brush mask or over the whole map, computed on the device from
 * the map as it is there and followed by the refresh vr_terrain_edit does: afterwards the terrain is the one vr_terrain_create
 * builds from the noised maps.  The noise lives in world space: octave o (0 .. octaves - 1) is a lattice of frequency *
 * lacunarity^o cells per world unit over the world position plus (offset_x, offset_z), so the same parameters give the same
 * landscape on maps of different resolution.  Each lattice corner is hashed with seed + o; a texel's centre falls into a cell at
 * (tx, tz) and is interpolated with the quintic fade t^3 (t (6 t - 15) + 10):
 *   VR_NOISE_VALUE     the corner's value is the hash's top 24 bits in [-1, 1); n = the faded bilinear interpolation
 *   VR_NOISE_GRADIENT  the corner takes one of eight unit gradients (four axis directions, four diagonals) by three hash bits; n =
 *                      the faded interpolation of the gradients' dot products with the offsets to the corners, times sqrt 2
 * Either n lies in [-1, 1].  The octaves are summed in ascending order with the weights a_o = gain^o / sum of gain^k, which sum to 1:
 *   VR_NOISE_FBM     f += a_o * n_o
 *   VR_NOISE_BILLOW  f += a_o * (2 |n_o| - 1)
 *   VR_NOISE_RIDGED  f += a_o * (1 - 2 |n_o|)
 * so f lies in [-1, 1].  Per channel c of channel_mask (as PAINT's; the heightmap has the one channel, mask 1; every selected
 * channel of an albedo texel receives the same f):
 *   VR_NOISE_ADD    value_c += m * (amplitude * f)                           amplitude signed, in stored units, |amplitude| <= 255
 *   VR_NOISE_BLEND  value_c += m * ((base + amplitude * f) - value_c)        base in [0, 255]
 * clamped to [0, 255] and rounded to the nearest byte once.  m is the mask of vr_terrain_erode (below) of the dabs, prepared for map
 * `which` with their strength an opacity - per texel the largest weight * strength, so their order does not matter - or 1 on every
 * texel with VR_NOISE_WHOLE_MAP, which needs dabs == NULL and n == 0 and whose rectangle is the whole map.  A texel with mask 0 is not
 * written.  A texel is a function of its own byte, its position, the parameters and its mask alone.  The arithmetic is defined bit for
 * bit in vrenderer_amd/csrc/vr_noise.h, without a division, a power or anything transcendental on the device.
 * out_rect, `dabs`, the stream order and what the host waits for are vr_terrain_brush's: the call synchronises nothing, and is
 * ordered against the strokes and erosions of the terrain.  With history on, one call is one record.  n == 0 without the flag, or
 * dabs that all miss the map, is VR_OK and launches nothing.
 * VR_ERR_INVALID_ARGUMENT, checked before the first use of the device, with the terrain untouched: NULL t or p; `which` not 0 or 1;
 * octaves outside 1 .. VR_NOISE_MAX_OCTAVES; an unknown basis, fractal, op or flag bit; VR_NOISE_WHOLE_MAP together with dabs; NULL
 * dabs with n > 0; n > VR_MAX_BRUSH_DABS; a NaN or an infinity in a field; frequency <= 0; lacunarity outside [1, 4]; gain outside
 * [0, 1]; |amplitude| > 255; base outside [0, 255]; a channel_mask of 0 or above 15, or other than 1 on the heightmap; a non-zero
 * reserved word; the dab refusals of vr_terrain_brush with an opacity for a strength.  One more refusal needs the map's size and is
 * checked behind those, before anything is queued: an octave whose lattice coordinate - (texel centre's world position + offset) *
 * frequency * lacunarity^o - reaches 2^22 in magnitude at one of the map's four corners.  Below that bound the cell index is an
 * exact int32 and the position inside the cell keeps at least a bit of fraction; beyond it the noise would be meaningless, not
 * merely coarse.  The memory a call needs is reserved before anything is launched (VR_ERR_OUT_OF_MEMORY leaves the terrain as it
 * was).  Timing: as for vr_terrain_edit; the noise kernel itself is untimed. */
#define VR_NOISE_MAX_OCTAVES 12
enum { VR_NOISE_VALUE = 0, VR_NOISE_GRADIENT = 1 };
enum { VR_NOISE_FBM = 0, VR_NOISE_BILLOW = 1, VR_NOISE_RIDGED = 2 };
enum { VR_NOISE_ADD = 0, VR_NOISE_BLEND = 1 };
enum { VR_NOISE_WHOLE_MAP = 1 };
typedef struct vr_noise_params {       /* 64 B */
    float frequency;                   /* lattice cells per world unit of octave 0, > 0 */
    float offset_x, offset_z;          /* added to the world position: the lattice origin lies at world (-offset_x, -offset_z) */
    float lacunarity;                  /* frequency ratio of successive octaves, [1, 4] */
    float gain;                        /* weight ratio of successive octaves, [0, 1] */
    float amplitude;                   /* stored units, signed, |amplitude| <= 255 */
    float base;                        /* BLEND's level, [0, 255] */
    uint32_t seed;
    int32_t octaves;                   /* 1 .. VR_NOISE_MAX_OCTAVES */
    int32_t basis;                     /* VR_NOISE_VALUE, VR_NOISE_GRADIENT */
    int32_t fractal;                   /* VR_NOISE_FBM, VR_NOISE_BILLOW, VR_NOISE_RIDGED */
    int32_t op;                        /* VR_NOISE_ADD, VR_NOISE_BLEND */
    uint32_t channel_mask;             /* 1 .. 15, like PAINT's; 1 on the heightmap */
    uint32_t flags;                    /* VR_NOISE_WHOLE_MAP */
    int32_t reserved[2];               /* zero */
} vr_noise_params;
VR_API int vr_terrain_noise(vr_terrain* t, int which, const vr_noise_params* p, const vr_brush_dab* dabs, uint32_t n, int32_t out_rect[4]);
/* A path on level 0 of the heightmap (which = 0: LEVEL, CUT, FILL) or the albedo (1: PAINT) - a road, a railway embankment, a river
 * bed, a dam, a piste, a painted track: a corridor of half-width `radius` world units along the polyline through `points`, computed on
 * the device from the map as it is there and followed by the refresh vr_terrain_edit does: afterwards the terrain is the one
 * vr_terrain_create builds from the map with the path in it.  `points` are world (x, z), as for dabs, each with the target `height` in
 * stored heightmap units ([0, 255], like FLATTEN's target; PAINT ignores it).  n points make n - 1 segments, or n with VR_PATH_CLOSED
 * (the last point joined to the first; needs n >= 3); n == 1 is a single disc, and a repeated point makes a zero-length segment, a
 * disc too - it is legal.  Across the path the weight is a dab's: with q = (distance to the polyline / radius)^2 it is 1 out to
 * q <= hardness^2 and the dab's smoothstep to 0 at q = 1.  Per texel the NEAREST segment counts - the one with the smallest q, of equal
 * ones the first in the list - with its parameter t in [0, 1] and the target = height_a + t * (height_b - height_a); with
 * a = weight * opacity the texel's value (the stored byte; four for the albedo) changes ONCE, however many segments pass nearby and
 * however the path bends - no beads, no joints applied twice:
 *   VR_PATH_LEVEL  value += a * (target - value)
 *   VR_PATH_CUT    value += a * (min(value, target) - value)       only lowers: a river bed, a cutting
 *   VR_PATH_FILL   value += a * (max(value, target) - value)       only raises: an embankment, a dam
 *   VR_PATH_PAINT  per channel c of channel_mask (as vr_terrain_brush's PAINT): value_c += a * (color[c] - value_c)
 * clamped to [0, 255] and rounded to the nearest byte once.  LEVEL, CUT and FILL need which = 0 and channel_mask == 1, PAINT which = 1.
 * A texel farther than `radius` from every segment is not written.  A texel is a function of its own byte, its position and the call
 * alone.  The arithmetic is defined bit for bit in vrenderer_amd/csrc/vr_path.h, without a division, a square root or
 * trigonometry on the device.
 * out_rect, the stream order and what the host waits for are vr_terrain_brush's: the call synchronises nothing, is ordered against
 * the strokes, erosions and the other writers of the terrain, and `points` is host memory that may be reused as soon as the call
 * returns.  With history on, one call is one record.  n == 0, or a path that misses the map, is VR_OK and launches nothing.
 * Not here: a width per point; splines (the caller tessellates - a point every few texels of a curve is plenty, and VR_MAX_PATH_POINTS
 * of them fit a call); heights snapped to the ground (vr_terrain_query_heights gives them, one call before); both maps in one call
 * (a road and its paint are two calls with the same points).
 * VR_ERR_INVALID_ARGUMENT, checked before the first use of the device, with the terrain untouched: NULL t or p; NULL points with
 * n > 0; n > VR_MAX_PATH_POINTS; `which` not 0 or 1; an unknown op, or one that does not fit the map; unknown flag bits;
 * VR_PATH_CLOSED with n < 3; a NaN or an infinity anywhere; radius <= 0; hardness outside [0, 1); opacity outside [0, 1]; a height or
 * a color outside [0, 255]; a channel_mask of 0 or above 15, or other than 1 on the heightmap; a non-zero reserved word, a point's
 * included.  The memory a call needs is reserved before anything is launched (VR_ERR_OUT_OF_MEMORY leaves the terrain as it was).
 * Timing: as for vr_terrain_edit; the path kernel itself is untimed. */
#define VR_MAX_PATH_POINTS 4096
enum { VR_PATH_LEVEL = 0, VR_PATH_CUT = 1, VR_PATH_FILL = 2, VR_PATH_PAINT = 3 };
enum { VR_PATH_CLOSED = 1 };
typedef struct vr_path_point  { float x, z, height, reserved; } vr_path_point;             /* 16 B */
typedef struct vr_path_params { int32_t op; uint32_t channel_mask; float radius, hardness, opacity;
                                float color[4]; uint32_t flags; int32_t reserved[6]; } vr_path_params; /* 64 B */
VR_API int vr_terrain_path(vr_terrain* t, int which, const vr_path_params* p,
                           const vr_path_point* points, uint32_t n, int32_t out_rect[4]);
/* A region on level 0 of the heightmap (which = 0: LEVEL, CUT, FILL, RAISE) or the albedo (1: PAINT) - a lake bed, a plateau, a
 * building pad, a quarry, a field, a painted zone: the inside of a polygon, with a feathered outline, computed on the device from the
 * map as it is there and followed by the refresh vr_terrain_edit does: afterwards the terrain is the one vr_terrain_create builds from
 * the map with the region in it.  `points` are world (x, z), as for dabs and path points.  They form num_contours closed contours of
 * contour_counts[c] consecutive points each (at least 3; the counts sum to n; the last point of a contour is joined to its first);
 * contour_counts == NULL with num_contours == 0 is one contour of all n points.  A texel is inside by the even-odd rule over all edges
 * of all contours: a second contour inside the first is a hole (an island in a lake), a bow-tie has two lobes.  A vertex or an edge
 * exactly on a row of texel centres is decided by a half-open rule, so neighbouring polygons that share an edge share no texel.
 * The weight f of a texel: with q = (distance to the nearest edge / feather)^2 and f0 the dab's smoothstep of hardness 0 - 1 at the
 * outline, 0 at q = 1 -
 *   default                     inside f = 1; outside f = f0 where q < 1: the polygon plus a soft skirt, C1 across the outline
 *   VR_REGION_FEATHER_INSIDE    inside f = 1 - f0 where q < 1, else 1; outside is not written: the feather stays within the outline
 *   feather == 0                inside f = 1; outside is not written: a hard edge, and no distance is evaluated at all
 * and with a = f * opacity the texel's value (the stored byte; four for the albedo) changes ONCE:
 *   VR_REGION_LEVEL  value += a * (target - value)
 *   VR_REGION_CUT    value += a * (min(value, target) - value)       only lowers: a lake bed, a quarry
 *   VR_REGION_FILL   value += a * (max(value, target) - value)       only raises: a pad, a plateau
 *   VR_REGION_RAISE  value += a * target                             target a signed delta in [-255, 255]
 *   VR_REGION_PAINT  per channel c of channel_mask (as vr_terrain_brush's PAINT): value_c += a * (color[c] - value_c)
 * clamped to [0, 255] and rounded to the nearest byte once.  The four height ops need which = 0 and channel_mask == 1, PAINT which = 1.
 * A texel is a function of its own byte, its position and the call alone.  The arithmetic is defined bit for bit in
 * vrenderer_amd/csrc/vr_region.h, without a division, a square root or trigonometry on the device.
 * out_rect, the stream order and what the host waits for are vr_terrain_path's: the call synchronises nothing, is ordered against
 * the strokes, erosions, paths and the other writers of the terrain, and `points` and `contour_counts` are host memory that may be
 * reused as soon as the call returns.  With history on, one call is one record.  n == 0, or a region that misses the map, is VR_OK
 * and launches nothing.
 * Not here: a sloped target plane; per-vertex heights; non-zero winding (even-odd is the one rule); curves (the caller tessellates -
 * VR_MAX_REGION_POINTS points fit a call); both maps in one call (a pad and its paint are two calls with the same points).
 * VR_ERR_INVALID_ARGUMENT, checked before the first use of the device, with the terrain untouched: NULL t or p; NULL points with
 * n > 0; n > VR_MAX_REGION_POINTS; `which` not 0 or 1; an unknown op, or one that does not fit the map; unknown flag bits; a contour
 * of fewer than 3 points, counts that do not sum to n, num_contours > 0 with NULL counts, or no counts with 0 < n < 3; a NaN or an
 * infinity anywhere; feather < 0; opacity outside [0, 1]; target outside [0, 255] ([-255, 255] for RAISE); a color outside [0, 255];
 * a channel_mask of 0 or above 15, or other than 1 on the heightmap; a non-zero reserved word.  The memory a call needs is reserved
 * before anything is launched (VR_ERR_OUT_OF_MEMORY leaves the terrain as it was).
 * Timing: as for vr_terrain_edit; the region kernel itself is untimed. */
#define VR_MAX_REGION_POINTS 4096
enum { VR_REGION_LEVEL = 0, VR_REGION_CUT = 1, VR_REGION_FILL = 2, VR_REGION_RAISE = 3, VR_REGION_PAINT = 4 };
enum { VR_REGION_FEATHER_INSIDE = 1 };
typedef struct vr_region_point  { float x, z; } vr_region_point;                       /*  8 B */
typedef struct vr_region_params { int32_t op; uint32_t channel_mask; float target, feather, opacity;
                                  float color[4]; uint32_t flags; int32_t reserved[6]; } vr_region_params; /* 64 B */
VR_API int vr_terrain_region(vr_terrain* t, int which, const vr_region_params* p,
                             const vr_region_point* points, uint32_t n,
                             const uint32_t* contour_counts, uint32_t num_contours, int32_t out_rect[4]);
/* Stamps: a prepared patch - a mountain, a crater, a scanned tile, an albedo decal - kept in device memory and set into level 0 of a
 * map at a position, size and angle, with a blend rule.  A vr_stamp is w x h texels, 1 .. 4096 per side, of one of the maps' formats:
 * VR_STAMP_R8 (the heightmap's, = which 0) or VR_STAMP_SRGBA8 (the albedo's, = which 1).  It belongs to the context it was created
 * on, may be stamped on any terrain of that context any number of times, and is destroyed before the context.
 *   vr_stamp_create        copies w x h texels (rows row_pitch_bytes apart; 0 = tightly packed).  device_pointer = 0: `texels` is host
 *                          memory and the call returns once it has been consumed (it synchronises the stream, as a host-pointer
 *                          vr_terrain_edit does).  device_pointer = 1: `texels` is device memory, aligned like vr_terrain_edit's; the
 *                          copy is stream-ordered on the context's stream, nothing is synchronised, and the caller keeps `texels`
 *                          alive and unchanged until the stream has passed it.
 *   vr_stamp_from_terrain  the w x h texels at (x, y) of level 0 of the terrain's heightmap (which = 0) or albedo (1) as they are on
 *                          the device - the clone tool's source: a device copy on the context's stream, behind the map's last
 *                          writer; nothing is synchronised and the map never visits the host.
 *   vr_stamp_destroy       waits on the host until nothing queued can still touch the stamp, then frees it.  NULL is allowed.
 *   vr_stamp_info          format and size (each pointer may be NULL).
 *   vr_stamp_download      test / IO helper, synchronous: the w * h texels, tightly packed, into `host` (bytes >= their size).
 * vr_terrain_stamp sets the stamp into level 0 of map `which`, computed on the device from the map as it is there, followed by the
 * refresh vr_terrain_edit does: afterwards the terrain is the one vr_terrain_create builds from the stamped maps.  The stamp's centre
 * lies at world (x, z); its own u axis points along (cos rotation, sin rotation) in world (x, z) and is size_x world units long, its
 * v axis along (-sin, cos), size_z long.  Every map texel whose centre lies inside that rectangle is covered: it samples the stamp
 * bilinearly (clamp addressing), s' = s * gain + offset in stored units, and weighs a = wf * opacity, where wf falls from 1 to 0 by
 * a smoothstep over the outer `feather` share of each half-extent (0 = a hard edge) and, with VR_STAMP_USE_ALPHA, a is scaled by the
 * stamp's sampled alpha / 255.  Per channel c of channel_mask (as PAINT's; an R8 map has the one channel, mask 1):
 *   VR_STAMP_BLEND  value_c += a * (s'_c - value_c)
 *   VR_STAMP_ADD    value_c += a * s'_c                  VR_STAMP_SUB  value_c -= a * s'_c
 *   VR_STAMP_MAX    value_c += a * (max(value_c, s'_c) - value_c)       VR_STAMP_MIN likewise with min
 * clamped to [0, 255] and rounded to the nearest byte once.  A texel that is not covered is not written; a covered one with a == 0
 * keeps its byte.  The arithmetic is defined bit for bit in vrenderer_amd/csrc/vr_stamp.h, without a division or
 * trigonometry on the device.  Sampling is bilinear only: a stamp minified by more than about 2 aliases, and filtering it first is
 * the caller's business.
 * out_rect (may be NULL) receives {x, y, w, h} of the level-0 rectangle the call treated as dirty - the hull of the stamp's corners
 * grown by one texel, clipped to the map; no texel outside it changes - or {0, 0, 0, 0} when the stamp misses the map, which is VR_OK
 * and launches nothing.  The call is stream-ordered on the context's stream like a device-pointer edit and synchronises nothing; it
 * is ordered against every other user of the stamp, whichever stream that ran on.  With history on, one call is one record.
 * VR_ERR_INVALID_ARGUMENT, checked before the first use of the device, with nothing touched: a NULL handle, pointer or `out`; a
 * format that is not VR_STAMP_R8 / _SRGBA8 or differs from `which`; a stamp of another context; a side outside 1 .. 4096; a
 * rectangle not wholly inside level 0; a pitch smaller than a row, or a device pointer or pitch not aligned to the texel; a NaN or an
 * infinity in a field; size_x or size_z <= 0; opacity or feather outside [0, 1]; |gain| > 256; |offset| > 255; an unknown op or flag;
 * VR_STAMP_USE_ALPHA on R8; a channel_mask of 0 or above 15, or other than 1 on R8; a non-zero reserved word.  Memory is reserved
 * before anything is launched (VR_ERR_OUT_OF_MEMORY leaves everything as it was).  Timing: as for vr_terrain_edit; the stamp kernel
 * itself is untimed. */
typedef struct vr_stamp vr_stamp;      /* a patch in device memory, owned by a context */
enum { VR_STAMP_R8 = 0, VR_STAMP_SRGBA8 = 1 };          /* = the `which` of the map it can be stamped on */
VR_API int  vr_stamp_create(vr_context* ctx, int format, int32_t w, int32_t h, const void* texels, size_t row_pitch_bytes,
                            int device_pointer, vr_stamp** out);
VR_API int  vr_stamp_from_terrain(vr_terrain* t, int which, int32_t x, int32_t y, int32_t w, int32_t h, vr_stamp** out);
VR_API void vr_stamp_destroy(vr_stamp* stamp);
VR_API int  vr_stamp_info(const vr_stamp* stamp, int32_t* format, int32_t* w, int32_t* h);
VR_API int  vr_stamp_download(vr_stamp* stamp, void* host, size_t bytes);
enum { VR_STAMP_BLEND = 0, VR_STAMP_ADD = 1, VR_STAMP_SUB = 2, VR_STAMP_MAX = 3, VR_STAMP_MIN = 4 };
enum { VR_STAMP_USE_ALPHA = 1 };       /* SRGBA8 only: the stamp's alpha scales the weight */
typedef struct vr_stamp_params {       /* 64 B */
    float x, z;                        /* centre, world units */
    float size_x, size_z;              /* world extent of the stamp along its own axes, > 0 */
    float rotation;                    /* radians about y */
    float opacity;                     /* [0, 1] */
    float feather;                     /* [0, 1]: share of each half-extent over which the weight falls to 0 at the border; 0 = hard edge */
    float gain, offset;                /* s' = s * gain + offset, in stored units; |gain| <= 256, |offset| <= 255 */
    int32_t op;                        /* VR_STAMP_BLEND .. VR_STAMP_MIN */
    uint32_t channel_mask;             /* 1 .. 15, like PAINT's; 1 on R8 */
    uint32_t flags;                    /* VR_STAMP_USE_ALPHA */
    int32_t reserved[4];               /* zero */
} vr_stamp_params;
VR_API int vr_terrain_stamp(vr_terrain* t, int which, vr_stamp* stamp, const vr_stamp_params* params, int32_t out_rect[4]);
/* Thermal (talus) erosion of level 0 of the heightmap under a brush mask, computed on the device from the map as it is there and
 * followed by the refresh vr_terrain_edit does: afterwards the terrain is the one vr_terrain_create builds from the eroded map.
 * The dabs are those of a stroke on the heightmap, their strength an opacity in [0, 1]; they form a mask, per texel the largest
 * weight * strength of the dabs that cover it (0 where none does), so their order does not matter.  A texel's height h (fp32, in
 * heightmap steps, the stored byte to begin with) is then relaxed `iterations` times, every texel of a sweep from the heights of
 * the sweep before.  For each of the eight neighbours n inside the map, in the order (-1,-1) (0,-1) (1,-1) (-1,0) (1,0) (-1,1)
 * (0,1) (1,1) of (dx, dy): T = talus for an axis neighbour and talus * 1.41421354f for a diagonal one, w = min(mask, mask_n); where
 * w > 0 and the difference |h - h_n| exceeds T by e > 0, the higher of the two gives up (rate * e) * w and the lower receives it -
 * both ends of an edge compute the same amount, bit for bit.  Nothing is clamped between sweeps; with rate <= 1/8 the heights
 * stay between the lowest and the highest of the neighbourhood.  After the last sweep a texel with a positive mask is stored as
 * the nearest byte of min(max(h, 0), 255); a texel with mask 0 keeps its byte (it is not written).  The arithmetic is defined bit
 * for bit in vrenderer_amd/csrc/vr_erode.h; the result does not depend on how the device divides the work.
 * out_rect, `dabs`, the stream order and what the host waits for are vr_terrain_brush's: the call synchronises nothing, and strokes
 * and erosions of one terrain are ordered against each other.  With history on, one call is one record.  n == 0, or dabs that all
 * miss the map, is VR_OK and launches nothing.  The device advances several sweeps per launch: a call costs about
 * iterations / 8 short kernels on top of the refresh.
 * VR_ERR_INVALID_ARGUMENT, checked before the first use of the device, with the terrain untouched: NULL t or p, NULL dabs with
 * n > 0; n > VR_MAX_BRUSH_DABS; iterations < 1 or > VR_ERODE_MAX_ITERATIONS; talus or rate NaN or infinite; talus outside
 * [0, 255]; rate <= 0 or > 0.125; a non-zero reserved word; the dab refusals of vr_terrain_brush with an opacity for a strength.
 * The memory a call needs - three fp32 planes of the rectangle's size, kept with the terrain and counted under scratch by
 * vr_terrain_memory_bytes - is reserved before anything is launched (VR_ERR_OUT_OF_MEMORY leaves the terrain as it was).  Timing: as
 * for vr_terrain_edit; the erosion kernels themselves are untimed. */
#define VR_ERODE_MAX_ITERATIONS 1024
typedef struct vr_erode_params { int32_t iterations; float talus; float rate; int32_t reserved[5]; } vr_erode_params; /* 32 B */
VR_API int vr_terrain_erode(vr_terrain* t, const vr_erode_params* p, const vr_brush_dab* dabs, uint32_t n, int32_t out_rect[4]);
/* test helper: {tile width, tile height, sweeps per launch, 0} of this build's erosion kernel */
VR_API int vr_debug_erode_config(int32_t out[4]);
/* test helper: the fp32 planes the last vr_terrain_erode or vr_terrain_erode_hydraulic of this terrain left on the device, before
 * the final rounding to bytes.  out_rect receives the call's {x, y, w, h}, *out_fields its model's state fields (1: h; 3: h, d, s),
 * and `out` (1 + fields) planes of w * h floats each, row-major: the mask, then the fields.  The copy runs on the context's stream
 * behind the erosion, on whichever stream that ran, and the entry returns when it has completed.  out == NULL with
 * capacity_floats == 0 is a size query: the rectangle and the field count only.  A refused erosion call leaves the record of the
 * call before it; a call that launched nothing (n == 0, or dabs that all miss the map) clears it.  With no record: VR_OK,
 * *out_fields == 0, a zero rectangle, `out` untouched.  VR_ERR_INVALID_ARGUMENT, with nothing written: NULL t, out_rect or
 * out_fields; NULL out with a capacity; a capacity below (1 + fields) * w * h. */
VR_API int vr_debug_terrain_sweep_state(vr_terrain* t, int32_t out_rect[4], int32_t* out_fields, float* out, size_t capacity_floats);
/* Hydraulic erosion of level 0 of the heightmap under a brush mask - water that runs downhill, dissolves the terrain where it runs
 * fast and lays the load down where it slows: gullies and fans, which the talus relaxation of vr_terrain_erode cannot make.  It is
 * computed on the device from the map as it is there and followed by the refresh vr_terrain_edit does: afterwards the terrain is the
 * one vr_terrain_create builds from the eroded map.  The mask m is vr_terrain_erode's (per texel the largest weight * strength of the
 * dabs that cover it, strength an opacity in [0, 1]).  A texel carries three fp32 values: h, the terrain in heightmap steps (the
 * stored byte to begin with), d, the water depth (rain * m to begin with), and s, the suspended sediment (0 to begin with).  They
 * are advanced `iterations` times, every texel of a sweep from the sweep before.  For each of the four axis neighbours n inside the
 * map, in the order (0,-1) (-1,0) (1,0) (0,1) of (dx, dy), with w = min(m, m_n) > 0: the end with the higher surface S = h + d
 * gives the share phi = min(flow * (S_high - S_low), 0.25) * w of its water, q = phi * d, and of its sediment, phi * s, to the
 * other - both ends compute the same amounts, bit for bit; `out` is the water the texel gave.  Then d and s are clamped at 0, the
 * capacity is C = capacity * out, and a texel with s < C dissolves e = dissolve * (C - s) * m of its terrain (h -= e, s += e) while
 * one with s >= C deposits g = deposit * (s - C) (h += g, s -= g); the water becomes d * (1 - evaporation) + rain * m.  After the
 * last sweep a texel with a positive mask is stored as the nearest byte of min(max(h + s, 0), 255) - what is still suspended
 * settles where it is; a texel with mask 0 keeps its byte (it is not written).  rain = 0 or capacity = 0 leaves the map as it is.
 * The arithmetic is defined bit for bit in vrenderer_amd/csrc/vr_hydro.h, without a division or a square root;
 * the result does not depend on how the device divides the work.
 * out_rect, `dabs`, the stream order and what the host waits for are vr_terrain_brush's: the call synchronises nothing, and
 * strokes and erosions of both kinds of one terrain are ordered against each other.  With history on, one call is one record.
 * n == 0, or dabs that all miss the map, is VR_OK and launches nothing.  The device advances several sweeps per launch: a call
 * costs about iterations / 4 short kernels on top of the refresh.
 * VR_ERR_INVALID_ARGUMENT, checked before the first use of the device, with the terrain untouched: NULL t or p, NULL dabs with
 * n > 0; n > VR_MAX_BRUSH_DABS; iterations < 1 or > VR_HYDRO_MAX_ITERATIONS; a parameter NaN or infinite; rain outside [0, 16];
 * flow <= 0 or > 1; capacity outside [0, 64]; dissolve, deposit or evaporation outside [0, 1]; a non-zero reserved word; the dab
 * refusals of vr_terrain_brush with an opacity for a strength.  The memory a call needs - seven fp32 planes of the rectangle's
 * size, kept with the terrain and counted under scratch by vr_terrain_memory_bytes - is reserved before anything is launched
 * (VR_ERR_OUT_OF_MEMORY leaves the terrain as it was).  Timing: as for vr_terrain_edit; the erosion kernels themselves are untimed. */
#define VR_HYDRO_MAX_ITERATIONS 1024
typedef struct vr_hydro_params { int32_t iterations; float rain, flow, capacity, dissolve, deposit, evaporation; int32_t reserved; } vr_hydro_params; /* 32 B */
VR_API int vr_terrain_erode_hydraulic(vr_terrain* t, const vr_hydro_params* p, const vr_brush_dab* dabs, uint32_t n, int32_t out_rect[4]);
/* test helper: {tile width, tile height, sweeps per launch, 0} of this build's hydraulic kernel */
VR_API int vr_debug_hydro_config(int32_t out[4]);
/* measurement helper, process-wide: later calls advance `sweeps` (1 .. the build's figure; 0 = that figure again) sweeps per
 * launch.  The bytes are the same; only the number of launches changes.  VR_ERR_INVALID_ARGUMENT outside that range. */
VR_API int vr_debug_hydro_sweeps_per_launch(int32_t sweeps);
/* History: undo and redo of vr_terrain_edit, vr_terrain_brush, vr_terrain_texture, vr_terrain_occlusion, vr_terrain_noise, vr_terrain_path, vr_terrain_region, vr_terrain_stamp, vr_terrain_erode and vr_terrain_erode_hydraulic, kept on the device. Off by default: every call then queues
 * exactly what it queues without it, undo / redo / commit are VR_OK and apply nothing, and the status is all zero.
 *   enable(budget_bytes)  one device arena of that size (vr_terrain_memory_bytes counts it under scratch; vr_terrain_destroy frees
 *                         it) and the host-side table of records, VR_HISTORY_MAX_RECORDS of them - nothing is allocated later.  The
 *                         budget it already has: nothing happens.  Any other budget drops all steps; 0 switches history off and
 *                         frees the arena.  A refusal is VR_ERR_OUT_OF_MEMORY with the terrain and the existing history untouched.
 *   records               with history on, every vr_terrain_edit, _brush, _texture, _occlusion, _noise, _path, _region, _stamp, _erode and _erode_hydraulic that writes (not w == 0, n == 0 or a stroke
 *                         that misses the map) first captures its level-0 rectangle as it is, by a kernel on the context's stream
 *                         in front of the write.  Nothing more is synchronised: a stroke with history on still synchronises nothing.
 *   steps                 records join the open step; commit closes it (a drag of many brush calls becomes one undo step; with no
 *                         open step commit does nothing).  undo and redo close an open step first.  A new record discards all redo
 *                         steps and frees their room.
 *   undo / redo           undo applies the newest closed step, its records newest first; redo re-applies the step undone last, its
 *                         records oldest first.  Per record a kernel exchanges the rectangle between the record and level 0 in place
 *                         and the refresh of vr_terrain_edit follows, so afterwards every call on the terrain behaves exactly as on a
 *                         terrain created from the maps of that point in history; prepared geometry is stale, as after an edit.
 *                         Both are stream-ordered on the context's stream and synchronise nothing.  *applied (may be NULL) is 1 if
 *                         a step was applied, 0 if there was none - then nothing is queued.
 *   budget                the arena is a ring of contiguous records: a record's rows lie at a pitch that is a multiple of 16 bytes,
 *                         the first byte of a row (x * texel bytes) mod 16 bytes into it (the exact size: vr_history.h,
 *                         DESIGN.md 4t).  Room is made by dropping the oldest undo steps whole, one count of dropped_steps each; a
 *                         full table of records is treated like a full arena.  History never refuses or alters a write: if room
 *                         could only be made by dropping the open step itself, or one record is larger than the arena, the write
 *                         happens unrecorded, ALL steps are dropped (nothing older can be restored across an unrecorded change), and
 *                         the open step is lost - it records nothing more until commit.  dropped_steps counts every step lost,
 *                         that one included.
 * VR_ERR_INVALID_ARGUMENT, before any use of the device: NULL t; NULL out for the status.  Timing: the refresh counts as for
 * vr_terrain_edit; the capture and swap kernels are untimed. */
#define VR_HISTORY_MAX_RECORDS 4096
typedef struct vr_history_status {
    uint32_t undo_steps, redo_steps;   /* closed steps that undo / redo can apply now */
    uint32_t open_records;             /* records of the step still open (0 = none open) */
    uint32_t dropped_steps;            /* steps lost to the budget since enable (monotonic) */
    uint64_t bytes_used, bytes_budget; /* arena bytes held by live records / the arena's size */
} vr_history_status;                   /* 32 B */
VR_API int vr_terrain_history_enable(vr_terrain* t, size_t budget_bytes); /* 0 = off: drops all steps, frees the arena */
VR_API int vr_terrain_history_commit(vr_terrain* t);                      /* closes the open step; no open step = VR_OK */
VR_API int vr_terrain_undo(vr_terrain* t, int32_t* applied);              /* *applied (may be NULL) = 1 or 0 */
VR_API int vr_terrain_redo(vr_terrain* t, int32_t* applied);
VR_API int vr_terrain_history_status(const vr_terrain* t, vr_history_status* out);

/* QuadTree::SetHeight for every node (QuadTree.cpp:164-208) as a device reduction over the heightmap,
 * and m_HeightLoaded (QuadTree.h:70).  The reference wrote this and left its launch commented out
 * (QuadTree.cpp:46-51), so the default is "not loaded": cull boxes span y in [0, camera.y].  With
 * enable != 0 the per-node (position.y, extents.y) are computed and NodeSelect culls with
 * [min.y, max.y] * max_height (QuadTree.cpp:87-91); UpdateTransforms then carries them too.
 * enable == 0 returns to the tree as built (y = location.y, extents.y = 0, not loaded). */
VR_API int  vr_terrain_update_heights(vr_terrain* t, int enable);
/* test helper: (position.y, extents.y) of node ids [first, first+count) */
VR_API int  vr_terrain_download_node_heights(vr_terrain* t, uint32_t first, uint32_t count, float* out);

/* QuadTree::ClearSelectedNodes + NodeSelect + TerrainPass::UpdateTransforms +
 * EditorParams::m_NumChunks (TerrainPass.cpp:173-198, QuadTree.cpp:80-131).
 * Runs on the device; optional host outputs (may be NULL) force a stream sync.
 * node_ids: id = (4^d-1)/3 + iz*2^d + ix, in the reference's m_SelectedNodes order. */
VR_API int  vr_terrain_select(vr_terrain* t, const vr_view* view, float max_height,
                              uint32_t* node_ids, vr_instance* instances, uint32_t* count);

/* TerrainPass::Render into the G-buffer framebuffer (TerrainPass.cpp:143-232;
 * terrain_vs.hlsl, terrain_ps.hlsl; raster state TerrainPass.cpp:460-485).
 * `part` may be NULL (= whole frame on this device).
 * The call is asynchronous.  Conditions only the device can detect - more than max_instances nodes selected
 * (VR_ERR_TOO_MANY_INSTANCES, the reference's assert at TerrainPass.cpp:238), a full bin / clipper work list or a frame that
 * outgrew the scratch (VR_ERR_OVERFLOW: triangles or nodes were dropped) - are STICKY: every geometry chain leaves its counters
 * in pinned host memory, and the next vr_terrain_render / vr_terrain_prepare after such a chain has completed returns the code
 * once (vr_last_error() names the frame's node count).  The call that returns it has still queued its own frame.
 * vr_terrain_num_chunks() waits for the current frame's geometry and returns its condition directly. */
VR_API int  vr_terrain_render(vr_terrain* t, const vr_view* view, const vr_view* view_prev,
                              vr_gbuffer* gb, const vr_render_params* rp,
                              const vr_partition* part);
/* Opt-in fused variant: TerrainPass::Render + DeferredLightingPass::Render in ONE pass over the pixels.  The tile
 * pass's resolve encodes each pixel to the G-buffer's formats in registers, decodes and shades it with the lighting pass's own
 * arithmetic and writes depth + hdr_out only (the other four G-buffer planes keep what they held): 12 bytes per pixel reach memory
 * instead of 28 + 36.  depth and hdr_out (HdrColor, or this rank's packed RGB16F tiles with a partition) are bit-identical to
 * vr_terrain_render(assume_cleared = 1) + vr_deferred_light on the same inputs.  Needs render->assume_cleared = 1, shaded fill
 * mode, <= 16 lights.  The fused kernel covers the reference's case (heightmap and albedo of one size, power-of-two world size,
 * directional / punctual point lights, no shadow term); for anything else the call runs the two passes one after the other.
 * vr_terrain_prepare works as for vr_terrain_render.  The unfused pair stays the default path (and the measured one). */
VR_API int  vr_terrain_render_lit(vr_terrain* t, const vr_view* view, vr_gbuffer* gb, const vr_render_params* rp,
                                  const vr_partition* part, const vr_light* lights, int32_t num_lights,
                                  const float ambient_top[3], const float ambient_bottom[3], vr_image* hdr_out);
/* Optional: build the view-dependent geometry (select .. bins) of an upcoming vr_terrain_render ahead of
 * time, on one of the terrain's two geometry streams.  Called right after vr_terrain_render of frame N with frame
 * N+1's view, it overlaps frame N's tile pass (and leaves its lighting pass alone).  Up to two frames may be prepared
 * ahead (N+1 and N+2: three geometry sets rotate, two chains are in flight - what keeps small frames and a rank's share
 * of a split frame from waiting for the latency-bound chain); naming a frame that is already prepared is a no-op, a
 * third distinct frame replaces the oldest.  A later vr_terrain_render uses a prepared set when view, max_height,
 * target size and partition are identical; sets that are never used are simply overwritten.
 * Extension; the reference has no counterpart (its frames are strictly serial).
 * Note for hosts with many streams of their own: HIP maps streams onto 4 hardware queues by default and streams that
 * share a queue serialise; the library uses the context's stream + 2.  GPU_MAX_HW_QUEUES raises the limit. */
VR_API int  vr_terrain_prepare(vr_terrain* t, const vr_view* view, vr_gbuffer* gb, const vr_render_params* rp,
                               const vr_partition* part);
/* EditorParams::m_NumChunks of the last render/select (syncs the stream). */
VR_API int  vr_terrain_num_chunks(vr_terrain* t, uint32_t* count);

/* ---- terrain queries ------------------------------------------------------------- */
/* The reference declares the seed of this and never grew it: QuadTree::GetHeightValue (QuadTree.h:84, QuadTree.cpp:153-162) is
 * one nearest-texel lookup on the CPU.  Here the surface that is queried is the one the drawn vertices carry (terrain_vs.hlsl:27-33):
 *   H(x, z) = SampleLevel(heightmap, linear-clamp, uv, 0.1).r * max_height,  uv = ((x, z) + world_size / 2) / world_size
 * = 0.9 * bilinear(level 0) + 0.1 * bilinear(level 1), continuous and piecewise bilinear; like the vertex stage it does not
 * depend on vr_terrain_params::location.  Outside uv in [0,1]^2 the clamp addressing holds for height queries; rays are clipped
 * to the box x, z in [-world_size/2, world_size/2], y in [min(0, max_height), max(0, max_height)].
 * Normal: normalize(-dH/dx, 1, -dH/dz) from the analytic partial derivatives of the two bilinear interpolants at the point
 * (on a cell boundary: of the cell with the larger coordinate) - not main_ps's central difference, which depends on a
 * screen-space LOD a query does not have.
 * Arrays: device_pointers = 0 - the caller's host memory; the call copies in, runs, copies out and returns when the results are
 * there (staging memory is kept with the terrain and grows by doubling).  device_pointers = 1 - device memory; the call is
 * stream-ordered on the context's stream and synchronises nothing; xz must then be 8-byte aligned and rays / hits 16-byte aligned
 * (the kernels move them as float2 / float4; anything else is VR_ERR_INVALID_ARGUMENT).  n = 0 is VR_OK and launches nothing; NULL arrays with n > 0
 * and a max_height that is NaN or infinite are VR_ERR_INVALID_ARGUMENT.  A negative max_height is valid (the vertex stage
 * multiplies by it as it is; the surface is then below y = 0). */
typedef struct vr_ray     { float origin[3]; float t_max; float dir[3]; uint32_t reserved; } vr_ray;      /* 32 B; dir need not be unit length; t in units of |dir| */
typedef struct vr_ray_hit { float t; float position[3]; float normal[3]; uint32_t status; } vr_ray_hit;   /* 32 B */
enum { VR_RAY_MISS = 0, VR_RAY_HIT = 1, VR_RAY_INVALID = 2 /* NaN/Inf/zero dir, NaN/Inf origin (an infinite origin has no point on it to clip), t_max < 0 or NaN */, VR_RAY_STEP_LIMIT = 3 };

/* QuadTree::GetHeightValue (QuadTree.h:84) for n points (x, z) -> H and, when out_normal != NULL, the normal (3 floats per
 * point).  The heights are bit for bit what the vertex stage gives a vertex at (x, z). */
VR_API int vr_terrain_query_heights(vr_terrain* t, const float* xz, uint32_t n, float max_height,
                                    float* out_height, float* out_normal, int device_pointers);
/* Ray casts against the same surface (grown from QuadTree.h:84): the first t in [max(0, t_enter), min(t_max, t_exit)] with
 * origin.y + t dir.y <= H(origin.xz + t dir.xz); a ray that starts at or below the surface hits at its first t inside the box.
 * hits[i] is written for every i: a hit has position.xz = origin.xz + t dir.xz, position.y = H there and the normal there;
 * anything else has t = t_max, zero position and normal, and its status.  The first cast of a terrain builds a min / max
 * pyramid over the surface on the context's stream (vr_terrain_memory_bytes counts it under textures); every loop of the walk
 * has a hard iteration cap, and a ray that reaches it returns VR_RAY_STEP_LIMIT. */
VR_API int vr_terrain_cast_rays(vr_terrain* t, const vr_ray* rays, uint32_t n, float max_height,
                                vr_ray_hit* hits, int device_pointers);
/* test helper: the min / max pyramid vr_terrain_cast_rays walks, as it is on the device.  *out_levels receives the number of levels,
 * out_dims the cells per level - {cw, ch} of level l at out_dims[2 l], out_dims[2 l + 1], zeros beyond the last level - and `out` the
 * levels in order, cw * ch pairs of bytes (lo, hi) each, row-major: level 0 has (w0 + 1) x (h0 + 1) cells, cell (ix, iz) bounding the
 * surface over the texel-centre interval [ix - 1, ix] x [iz - 1, iz] by lo / 255 <= H / max_height <= hi / 255; every further level is
 * the min / max of 2 x 2 cells of the one below, (c + 1) / 2 cells a side, down to 1 x 1.  The copy runs on the context's stream
 * behind the pyramid's last writer (the first cast, or the refresh of an edit, a stroke, an erosion, an undo or a redo, on whichever
 * stream that ran) and the entry returns when it has completed.  out == NULL with capacity_bytes == 0 is a size query: the levels and
 * their cells only.  On a terrain on which no ray has been cast there is no pyramid and none is built: VR_OK, *out_levels == 0, zero
 * out_dims, `out` untouched.  VR_ERR_INVALID_ARGUMENT, checked before the first use of the device, with nothing written: NULL t,
 * out_levels or out_dims; NULL out with a capacity; a capacity below 2 bytes per cell of all levels together. */
VR_API int vr_debug_terrain_query_pyramid(vr_terrain* t, int32_t* out_levels, int32_t out_dims[2 * 16], uint8_t* out, size_t capacity_bytes);
/* test helper: one level of one decoded table of a map - what every tile pass and every height query reads instead of the mip chain -
 * as it is on the device.  which: 0 heightmap, 1 albedo.  Level l of a w0 x h0 map has w = max(1, w0 >> l) by h = max(1, h0 >> l) texels;
 * t(x, y) = (float)byte / 255.0f of the clamp-addressed texel (min(max(x, 0), w - 1), min(max(y, 0), h - 1)), lin() the sRGB decode:
 *   VR_DEBUG_TABLE_QUAD   heightmap  (w + 2) x (h + 2) uint32   entry (ix, iy): bytes (ix-1, iy-1) | (ix, iy-1) << 8 | (ix-1, iy) << 16 | (ix, iy) << 24
 *   VR_DEBUG_TABLE_QUADF  heightmap  (w + 2) x (h + 2) float[4] (t00, t10 - t00, t01, t11 - t01) of the same four texels
 *   VR_DEBUG_TABLE_FAST   both       (w + 3) x (h + 3) float[4] heightmap: as QUADF; albedo: (lin r, lin g, lin b, 0) of texel (ix-1, iy-1)
 *   VR_DEBUG_TABLE_RGBF   albedo     w x h float[4]             (lin r, lin g, lin b, 0) of texel (ix, iy)
 *   VR_DEBUG_TABLE_PACK   albedo     (w + 3) x (h + 3) uint32[4] the sRGB8 codes of the footprint (ix-1, iy-1) (ix, iy-1) (ix-1, iy) (ix, iy), a dword
 *                                                               per texel: r << 2 | g << 12 | b << 22 (what the fused tile pass reads instead of FAST)
 * out_dims receives {entries per row, rows} and `out` the entries, row-major and densely packed (padding between levels is never shown).
 * The copy runs on the context's stream - behind the tables' last writer as a tile pass's read of them is - and the entry returns when
 * it has completed; no kernel is launched and nothing is built.  out == NULL with capacity_bytes == 0 is a size query.  A table the map
 * does not have (QUAD / QUADF of the albedo, RGBF of the heightmap) or a level beyond the chain: VR_OK, zero out_dims, `out` untouched.
 * VR_ERR_INVALID_ARGUMENT, checked before the first use of the device, with nothing written: NULL t or out_dims; which not 0 or 1; an
 * unknown table; a negative level; NULL out with a capacity; a capacity below the level's entries. */
enum { VR_DEBUG_TABLE_QUAD = 0, VR_DEBUG_TABLE_QUADF = 1, VR_DEBUG_TABLE_FAST = 2, VR_DEBUG_TABLE_RGBF = 3 };
enum { VR_DEBUG_TABLE_PACK = 5 };     /* (4 is no table: it stays the unknown id the entry refuses) */
VR_API int vr_debug_terrain_tables(vr_terrain* t, int which, int table, int32_t level, int32_t out_dims[2], void* out, size_t capacity_bytes);
/* Host only (picking; QuadTree.h:84 is what the reference would have called with it): the ray through the centre of pixel
 * (px, py) of view's viewport - screen point (px + 0.5, py + 0.5); fractional px, py are allowed.  The two ends are the
 * points world_to_clip sends to (x, y, 0) and (x, y, 1), solved in double (the inverse of the matrix a renderer projects with;
 * the fp32 clip_to_world is ill-conditioned at the far plane), so origin + t_max * dir lies on the far plane.  The origin is an
 * fp32 point, and next to the eye one ulp of a coordinate is a visible angle (1e-3 NDC at coordinates near 1000, z_near 0.1): it
 * is the fp32 point within 64 ulp of its largest coordinate behind the near plane, on the ray, that projects closest to the
 * pixel's centre (within 5e-5 NDC where one exists).  Its clip z / w is therefore 0 only to that distance over z_near. */
VR_API int vr_view_pixel_ray(const vr_view* view, float px, float py, vr_ray* out);

/* ---- render targets ---------------------------------------------------------- */
/* RenderTargets::Init / Clear (Renderer.h:60-101, Renderer.cpp:382).
 * Under VR_OPT_PLANE_TRACKING (default) the clear is lazy: the next vr_terrain_render that shades the whole frame runs as
 * "over a cleared target" (what vr_render_params::assume_cleared asks for explicitly) and writes each pixel once; anything else
 * that looks at the planes first - a lighting pass, a rank's share, a depth-only pass, vr_gbuffer_download / _upload /
 * _describe - has the clear values written then.  What the planes read as never differs from an eager clear. */
VR_API int  vr_gbuffer_create(vr_context* ctx, int32_t width, int32_t height, vr_gbuffer** out);
VR_API void vr_gbuffer_destroy(vr_gbuffer* gb);
VR_API int  vr_gbuffer_clear(vr_gbuffer* gb);
/* The device pointers of the planes, for interop.  From this call on the library assumes nothing about the planes' contents
 * (a host may write through the pointers at any time): vr_render_params::depth_ranges is ignored and every tile pass writes
 * all five planes (VR_OPT_PLANE_TRACKING) for the rest of this G-buffer's life. */
VR_API int  vr_gbuffer_describe(vr_gbuffer* gb, vr_gbuffer_desc* out);
/* 1 when the library knows `plane` (4 = emissive; others: 0) holds only zeros and the next tile pass will not rewrite it. */
VR_API int  vr_gbuffer_plane_known_zero(vr_gbuffer* gb, int plane);
/* Plane-state tracking per region (VR_OPT_PLANE_TRACKING; a region = 8 rows x 32 pixels, what one wave of a 32-pixel raster
 * tile resolves): counts[0] regions nothing is known about, counts[1] regions whose specular plane holds the terrain
 * shader's one constant in every pixel (terrain_ps.hlsl:76: the next tile pass that covers such a region completely does not
 * rewrite that plane), counts[2] regions that hold the clear values in all planes (a tile pass over a cleared target that
 * draws nothing there writes nothing), counts[3] their total.  The planes' contents never depend on the tracking; this is
 * what a bench needs to say how many bytes a tile pass really wrote.  Waits for the context's stream. */
VR_API int  vr_gbuffer_region_census(vr_gbuffer* gb, uint32_t counts[4]);
/* test/IO helpers: copy planes host<->device (synchronous). plane: 0 depth,
 * 1 diffuse, 2 specular, 3 normals, 4 emissive. */
VR_API int  vr_gbuffer_download(vr_gbuffer* gb, int plane, void* host, size_t bytes);
VR_API int  vr_gbuffer_upload(vr_gbuffer* gb, int plane, const void* host, size_t bytes);

/* HdrColor (Renderer.h:69-79).  external_device_mem may be NULL (library allocates)
 * or a caller-owned device buffer of width*height*8 bytes. */
VR_API int  vr_image_create(vr_context* ctx, int32_t width, int32_t height,
                            void* external_device_mem, vr_image** out);
VR_API void vr_image_destroy(vr_image* img);
VR_API void* vr_image_device_ptr(vr_image* img);
VR_API int  vr_image_download(vr_image* img, void* host, size_t bytes);
VR_API int  vr_image_upload(vr_image* img, const void* host, size_t bytes);

/* ---- deferred lighting --------------------------------------------------------- */
/* The domain of the lighting entries (vr_deferred_light, _shadowed, _tiled, _tiled_ex, vr_terrain_render_lit, vr_frame_submit):
 *  - a NaN or an infinity in view->clip_to_world, view->camera_pos, an ambient channel or a light field its type reads is
 *    refused (VR_ERR_INVALID_ARGUMENT, the field named) before anything is queued: nothing the call touches changes;
 *  - finite inputs under which a cleared texel (sky) is not guaranteed to shade to +0 - a clip_to_world that sends depth 1 to
 *    w = 0 (an infinite far plane), a light on the far plane, intensity / color / ambient beyond 2^40, a source radius or a spot
 *    cone below 2^-20 ... - are accepted by vr_deferred_light[_shadowed] and vr_frame_submit, which then shade EVERY texel
 *    (no plane-state shortcut, no fused frame: same results, the speed of the plain pass); vr_deferred_light_tiled[_ex] and
 *    vr_terrain_render_lit, whose kernels give a sky texel +0 unshaded, refuse them with VR_ERR_INVALID_ARGUMENT.
 * The bounds: vrenderer_amd/csrc/vr_light_domain.h. */
/* DeferredLightingPass::Render(cmd, view, Inputs{GBuffer, ambientColorTop/Bottom,
 * lights, output}) (Renderer.cpp:417-428).  `part` NULL = whole frame, output
 * row-major; otherwise only owned tiles are shaded and written to `hdr_out` as a
 * packed tile-major buffer (vr_partition_packed_bytes). */
VR_API int  vr_deferred_light(vr_context* ctx, const vr_view* view, vr_gbuffer* gb,
                              const vr_light* lights, int32_t num_lights,
                              const float ambient_top[3], const float ambient_bottom[3],
                              vr_image* hdr_out, const vr_partition* part);

/* The same pass for many lights (BASELINE config 5: 1024 point lights): a culling kernel tests the
 * lights against the world-space bounds of every 128x128 macro tile and of its sixteen 32x32 light
 * tiles (frustum cells over the tiles' depth ranges) and leaves one list per light tile; the shading
 * kernel walks only that list.  Same inputs/outputs as vr_deferred_light; up to 65536 lights in all and
 * VR_TILE_LIGHT_CAP lights per tile after culling.  A tile that keeps more drops the excess (in
 * light order) and raises a device-side flag; the launch stays asynchronous, so the condition is
 * reported by vr_deferred_tiled_status.  The light array is uploaded only when it differs from the
 * one the previous call left on the device.  Device memory: (w/32) x (h/32) lists of
 * min(num_lights, VR_TILE_LIGHT_CAP) + 1 words, kept by the context.
 * This entry point takes directional and punctual point lights only (a spot light or a radius > 0 is
 * VR_ERR_INVALID_ARGUMENT) and has no shadow term: vr_deferred_light_tiled_ex, below, lifts both. */
#define VR_TILE_LIGHT_CAP 1024
VR_API int  vr_deferred_light_tiled(vr_context* ctx, const vr_view* view, vr_gbuffer* gb,
                                    const vr_light* lights, int32_t num_lights,
                                    const float ambient_top[3], const float ambient_bottom[3],
                                    vr_image* hdr_out, const vr_partition* part);
/* Waits for the tiled passes queued so far on this context and returns VR_ERR_OVERFLOW if any of their
 * tiles kept more than VR_TILE_LIGHT_CAP lights since the last call (the flag is cleared), else VR_OK. */
VR_API int  vr_deferred_tiled_status(vr_context* ctx);

/* ---- terrain shadows ---------------------------------------- */
/* The reference renders the terrain depth-only from the sun into a 2048^2 one-cascade shadow map every
 * frame and the deferred pass consumes it (Renderer.cpp:83-93, 333-367, 427).  CascadedShadowMap and the
 * shadow lookup are Donut code (absent): [DONUT-RECOLLECTION] "stable" cascade = bounding sphere of the
 * camera frustum slice [0, maxShadowDistance], centre snapped to shadow texels in light space,
 * orthographic D3D projection; lookup = 4x4 GatherCmp tent PCF (weights [1-f,1,1,f]^2 / 9), LessEqual. */
typedef struct vr_shadow_params {
    int32_t resolution;            /* 2048 (Renderer.cpp:83) */
    float   max_shadow_distance;   /* WORLD_SIZE (:349) */
    float   light_space_z_up;      /* WORLD_SIZE (:350-352) */
    float   light_space_z_down;    /* WORLD_SIZE */
    float   depth_bias;            /* in shadow-map depth units, subtracted from the receiver; 0: the terrain
                                      depth pass has no raster bias (TerrainPass.cpp:467-471) */
    int32_t reserved[3];
} vr_shadow_params;
VR_API void vr_shadow_default_params(vr_shadow_params* out, float world_size);
/* CascadedShadowMap::SetupForPlanarViewStable(light, projectionFrustum, inverseViewMatrix, maxShadowDistance,
 * zUp, zDown, exponent, 0, 1) for the single cascade (Renderer.cpp:345-352): the light's view, to be
 * rendered with vr_terrain_render(depth_only = 1) into a resolution^2 vr_gbuffer (m_ShadowFramebuffer). */
VR_API int  vr_shadow_view_setup(const vr_light* light, const vr_view* camera_view, const vr_shadow_params* p,
                                 vr_view* out_light_view);
/* what DirectionalLight::shadowMap hands to the lighting pass */
typedef struct vr_shadow_binding {
    const vr_view* light_view;
    vr_gbuffer*    shadow_map;     /* its depth plane is sampled */
    int32_t        light_index;    /* which entry of `lights` casts it */
    float          depth_bias;
} vr_shadow_binding;
/* vr_deferred_light with the shadow term on one light (vr_light.out_of_bounds_shadow outside the map). */
VR_API int  vr_deferred_light_shadowed(vr_context* ctx, const vr_view* view, vr_gbuffer* gb,
                                       const vr_light* lights, int32_t num_lights,
                                       const float ambient_top[3], const float ambient_bottom[3],
                                       vr_image* hdr_out, const vr_partition* part,
                                       const vr_shadow_binding* shadow);
/* vr_deferred_light_tiled for every light type, with the sun's shadow term: the inputs, outputs, limits, overflow report
 * (vr_deferred_tiled_status) and packed output of vr_deferred_light_tiled, and in addition
 *  - VR_LIGHT_SPOT and spherical sources (radius > 0), shaded with the arithmetic of vr_deferred_light; a spot light still needs
 *    outer_angle > inner_angle.  A spot light is culled by its range as a point light is and, when its outer_angle is below
 *    pi/2 and its direction is of unit length, also dropped from the tiles that lie outside its cone;
 *  - shadow (may be NULL): the conditions and the shadow term of vr_deferred_light_shadowed on lights[shadow->light_index] - a
 *    directional light, a square map that matches the light view, on this device; out_of_bounds_shadow outside the map.
 * A list without spot or spherical lights and without a binding runs vr_deferred_light_tiled's kernels. */
VR_API int  vr_deferred_light_tiled_ex(vr_context* ctx, const vr_view* view, vr_gbuffer* gb,
                                       const vr_light* lights, int32_t num_lights,
                                       const float ambient_top[3], const float ambient_bottom[3],
                                       vr_image* hdr_out, const vr_partition* part,
                                       const vr_shadow_binding* shadow /* may be NULL */);

/* LdrColor: SRGBA8_UNORM render target (Renderer.h:81-92), width*height*4 bytes of device memory, or - as a
 * multi-GPU send buffer - the packed RGB8 tiles of one rank (capacity_bytes >= vr_partition_packed_bytes_ldr).
 * capacity_bytes 0 = width*height*4.  external != NULL wraps caller-owned device memory of that capacity. */
typedef struct vr_ldr_image vr_ldr_image;
VR_API int    vr_ldr_image_create(vr_context* ctx, int32_t width, int32_t height, size_t capacity_bytes, void* external_device_ptr,
                                  vr_ldr_image** out);
VR_API void   vr_ldr_image_destroy(vr_ldr_image* im);
VR_API void*  vr_ldr_image_device_ptr(vr_ldr_image* im);
VR_API size_t vr_ldr_image_capacity(vr_ldr_image* im);
VR_API int    vr_ldr_image_download(vr_ldr_image* im, void* host, size_t bytes);   /* synchronous; bytes <= capacity */
VR_API int    vr_ldr_image_upload(vr_ldr_image* im, const void* host, size_t bytes);

/* ---- multi-GPU frame assembly (new) -------------------------------- */
VR_API int    vr_partition_num_tiles(int32_t width, int32_t height, const vr_partition* part,
                                     int32_t* tiles_x, int32_t* tiles_y, int32_t* owned,
                                     int32_t* max_owned);
VR_API size_t vr_partition_packed_bytes(int32_t width, int32_t height, int32_t world_size);
/* Builds the partition tables of a context up front (they are otherwise built on first use by
 * vr_terrain_render / vr_deferred_light); needed when vr_frame_detile runs on its own context/stream. */
VR_API int    vr_partition_prepare(vr_context* ctx, int32_t width, int32_t height, const vr_partition* part);
/* After the all-gather: gathered = world_size consecutive packed buffers (device pointer; packed
 * tiles are RGB16F, 6 B/pixel - HdrColor's alpha is always 0 on this path and is not exchanged);
 * rebuilds the row-major RGBA16F frame. */
VR_API int    vr_frame_detile(vr_context* ctx, const void* gathered_device, int32_t world_size,
                              vr_image* frame_out);

/* The exchange itself (vr_frame_allgather).  `nccl_comm` is the caller's ncclComm_t for the ranks of the
 * split (one process per GPU; rank = vr_partition.rank, nranks = world_size).  ncclAllGather of this rank's packed
 * tiles (vr_partition_packed_bytes of RGB16F out of vr_deferred_light(part)) into `gathered_device`
 * (world_size x that), queued on the context's stream, followed by vr_frame_detile into frame_out - every rank ends
 * with the whole row-major RGBA16F frame.  RCCL is resolved at first use from the copy already in the process (the
 * one that made the communicator), else from librccl.so; libvrterrain.so itself does not link it. */
VR_API int    vr_frame_allgather(vr_context* ctx, void* nccl_comm, const void* packed_device, void* gathered_device,
                                 int32_t world_size, vr_image* frame_out);

/* The all-gather alone, for a host that de-tiles on another stream (vr_frame_detile[_ldr] on a second context, so that the
 * de-tile of frame i runs under the all-gather of frame i+1): ncclAllGather of bytes_per_rank bytes (vr_partition_packed_bytes
 * or vr_partition_packed_bytes_ldr) from packed_device into gathered_device (world_size x that) on the context's stream. */
VR_API int    vr_frame_allgather_tiles(vr_context* ctx, void* nccl_comm, const void* packed_device, void* gathered_device,
                                       int32_t world_size, size_t bytes_per_rank);

/* ---- tone mapping to LdrColor ------------------------------- */
/* donut::render::ToneMappingPass as used by the reference: created with default CreateParameters
 * (Renderer.cpp:256-257), AdvanceFrame(seconds) (:188-189), SimpleRender(cmd, ToneMappingParameters(),
 * view, HdrColor) into LdrColor SRGBA8 (:430-431, Renderer.h:81-95).  [DONUT-RECOLLECTION: luminance
 * histogram (256 bins over log2 luminance, fixed-point weights split over two bins) -> average
 * log luminance between two percentiles -> eye adaptation -> extended Reinhard on luminance.]
 * Integer results (histogram, SRGBA8 pixels) are bit-exact against the oracle.
 * Bin weights: a pixel adds Q = 64 >> s, split over two bins, where s is the smallest shift with Q * width * height
 * <= 2^32 - 1 (the whole frame's width * height, also with a partition, so every rank uses the same Q and the bins summed
 * over the ranks fit): Q = 64 below 2^26 pixels, and no 32-bit bin can wrap for ONE frame per reset_histogram (adding
 * several frames without a reset can).  A frame of 2^32 pixels or more is VR_ERR_INVALID_ARGUMENT.
 * Eye adaptation: adapted := old + (target - old)(1 - e^(-dt * speed)), speed = eye_adaptation_speed_up when target > old,
 * else eye_adaptation_speed_down.  An adapted value <= 0 ("unset") jumps to the target, and so does a direction whose speed
 * is <= 0 (it does not hold still).
 * Operator: mapped / luminance is one fused division; where its denominator overflows it is evaluated in the written order
 * (s (1 + s / wp^2) / (1 + s), then / luminance), so an extreme exposure saturates instead of giving inf / inf.  A pixel
 * whose luminance is +inf is NaN through that formula and encodes to 0, as do NaN, zero and negative luminances. */
typedef struct vr_tonemap_params {          /* ToneMappingParameters defaults + CreateParameters' log range */
    float histogram_low_percentile;         /* 0.8  */
    float histogram_high_percentile;        /* 0.95 */
    float eye_adaptation_speed_up;          /* 1.0  */
    float eye_adaptation_speed_down;        /* 0.5  */
    float min_adapted_luminance;            /* 0.02 */
    float max_adapted_luminance;            /* 0.5  */
    float exposure_bias;                    /* -0.5 */
    float white_point;                      /* 3.0  */
    float min_log_luminance;                /* -10  */
    float max_log_luminance;                /*  4   */
} vr_tonemap_params;
#define VR_TONEMAP_BINS 256
typedef struct vr_tonemap vr_tonemap;       /* the pass object: histogram + adapted-luminance (exposure) buffer */
VR_API void vr_tonemap_default_params(vr_tonemap_params* out);
VR_API int  vr_tonemap_create(vr_context* ctx, vr_tonemap** out);
VR_API void vr_tonemap_destroy(vr_tonemap* tm);
/* ResetExposure(cmd, initialExposure): adapted luminance := value (0 = "unset": the next ComputeExposure jumps to its target) */
VR_API int  vr_tonemap_reset_exposure(vr_tonemap* tm, float adapted_luminance);
VR_API int  vr_tonemap_reset_histogram(vr_tonemap* tm);
/* AddFrameToHistogram: `hdr` is a row-major RGBA16F frame (part NULL) or the packed RGB16F tiles that
 * vr_deferred_light wrote for `part` (only this rank's pixels are counted). */
VR_API int  vr_tonemap_add_frame_to_histogram(vr_tonemap* tm, const vr_tonemap_params* p, vr_image* hdr,
                                              int32_t width, int32_t height, const vr_partition* part);
/* Device pointer to the VR_TONEMAP_BINS uint32 bins: with a partition, sum it over the ranks
 * (ncclAllReduce, ncclUint32, ncclSum) between add_frame_to_histogram and compute_exposure. */
VR_API void* vr_tonemap_histogram_device_ptr(vr_tonemap* tm);
VR_API int  vr_tonemap_compute_exposure(vr_tonemap* tm, const vr_tonemap_params* p, float frame_time_seconds);
/* Render: HdrColor -> LdrColor.  part NULL: row-major SRGBA8 (width*height*4 bytes at ldr_device).
 * Otherwise packed tiles in, packed RGB8 tiles out (3 B/pixel, alpha is always 255 and is not
 * exchanged; vr_partition_packed_bytes_ldr); rebuild the frame with vr_frame_detile_ldr. */
VR_API int  vr_tonemap_render(vr_tonemap* tm, const vr_tonemap_params* p, vr_image* hdr, int32_t width, int32_t height,
                              void* ldr_device, size_t ldr_capacity_bytes, const vr_partition* part);
/* SimpleRender = ResetHistogram + AddFrameToHistogram + ComputeExposure + Render on one GPU. */
VR_API int  vr_tonemap_simple_render(vr_tonemap* tm, const vr_tonemap_params* p, float frame_time_seconds, vr_image* hdr,
                                     void* ldr_device, size_t ldr_capacity_bytes);
/* test/IO helpers (synchronous) */
VR_API int  vr_tonemap_download(vr_tonemap* tm, uint32_t histogram[VR_TONEMAP_BINS], float* adapted_luminance);
VR_API size_t vr_partition_packed_bytes_ldr(int32_t width, int32_t height, int32_t world_size);
/* gathered = world_size consecutive packed RGB8 buffers -> row-major SRGBA8 frame (device pointers) */
VR_API int  vr_frame_detile_ldr(vr_context* ctx, const void* gathered_device, int32_t world_size,
                                int32_t width, int32_t height, void* ldr_frame_device);

/* The same exchange for tone-mapped frames (3 B/pixel on the wire): ncclAllGather of the packed RGB8 tiles out of
 * vr_tonemap_render(part) + vr_frame_detile_ldr; and the tone mapper's one real exchange step, the sum of the 256
 * histogram bins over the ranks (ncclAllReduce, in place, on the tone mapper's context stream) between
 * vr_tonemap_add_frame_to_histogram(part) and vr_tonemap_compute_exposure. */
VR_API int  vr_frame_allgather_ldr(vr_context* ctx, void* nccl_comm, const void* packed_ldr_device, void* gathered_device,
                                   int32_t world_size, int32_t width, int32_t height, void* ldr_frame_device);
VR_API int  vr_tonemap_allreduce_histogram(vr_tonemap* tm, void* nccl_comm);

/* ---- a whole frame in one call ---------------------------------------------------- */
/* The terrain part of Renderer::RecordCommand (Renderer.cpp:321-446: ONE command list per frame) as one entry point:
 * vr_terrain_render(view) [RenderTargets::Clear fused when render->assume_cleared] -> vr_terrain_prepare for up to two upcoming
 * frames -> vr_deferred_light / _tiled / _tiled_ex / _shadowed -> optionally ToneMappingPass::SimpleRender on the tone mapper's own context
 * (reset + add_frame_to_histogram [+ vr_tonemap_allreduce_histogram] + compute_exposure + render) [+ vr_frame_allgather_ldr].
 * It queues what those calls queue, in that order, on the same streams; it exists because a frame is otherwise about nine calls
 * and a rank of an 8-way split of the 8K frame has a period near 0.1 ms.  When the tone mapper's context uses another stream than
 * the terrain's, the library orders the two: the stage waits for the lighting pass, and a later lighting pass into the same
 * hdr_out waits for the stage that still reads it (rotate two images to keep both streams busy). */
typedef struct vr_frame_desc {
    const vr_view*          view;               /* this frame's view (IView of Renderer::RenderScene) */
    const vr_view*          prepare_views[2];   /* geometry of upcoming frames to build ahead; NULL = none */
    const vr_render_params* render;
    const vr_partition*     part;               /* NULL = whole frame */
    const vr_light*         lights;
    int32_t                 num_lights;
    int32_t                 tiled;              /* 0 = vr_deferred_light[_shadowed]; 1 = vr_deferred_light_tiled (many lights; it has no
                                                   shadow term: `shadow` is ignored); 2 = vr_deferred_light_tiled_ex with `shadow` */
    float                   ambient_top[3], ambient_bottom[3];
    const vr_shadow_binding* shadow;            /* optional: vr_deferred_light_shadowed (tiled = 0), vr_deferred_light_tiled_ex (tiled = 2) */
    vr_image*               hdr_out;            /* HdrColor, or this rank's packed RGB16F tiles */
    /* optional tone-map stage: tonemap NULL = none */
    struct vr_tonemap*      tonemap;
    const vr_tonemap_params* tonemap_params;
    float                   frame_time_seconds;
    int32_t                 reserved0;
    void*                   ldr_out;            /* device: LdrColor SRGBA8, or this rank's packed RGB8 tiles */
    size_t                  ldr_capacity;
    /* optional exchange behind it (N ranks; all NULL = none): the host's ncclComm_t, world x packed bytes, the whole SRGBA8 frame */
    void*                   nccl_comm;
    void*                   gathered;
    void*                   ldr_frame;
} vr_frame_desc;
VR_API int vr_frame_submit(vr_terrain* t, vr_gbuffer* gb, const vr_frame_desc* frame);

/* ---- synthetic inputs (media/ is absent from the reference checkout;
 * SURVEY §8d): seeded integer-hash fBm heightmap and banded albedo, generated on
 * the device and copied to host buffers. ------------------------------------------ */
VR_API int vr_synth_heightmap(vr_context* ctx, int32_t size, uint32_t seed, uint8_t* out_r8);
VR_API int vr_synth_albedo(vr_context* ctx, int32_t size, uint32_t seed,
                           const uint8_t* height_r8, uint8_t* out_srgba8);

/* diagnostics of the last vr_terrain_render (synchronises): out[0] selected nodes, [1] status flags,
 * [2] clipper sub-triangles, [3] clipper vertices, [4] triangles sent to the clipper, [5] bin entries,
 * [6] largest bin, [7] non-empty bins */
VR_API int vr_debug_render_stats(vr_terrain* t, uint32_t out[8]);
/* Test helper: the launch order of the last vr_terrain_render's tile pass - the raster tiles the frame (or this rank) covers,
 * longest bins first in eight classes (k_scan) - and each of those tiles' bin lengths, in that order.  `capacity` entries per
 * array; *out_count = number of tiles (0 if nothing was rendered).  Synchronises. */
VR_API int vr_debug_tile_order(vr_terrain* t, int32_t* out_tiles, uint32_t* out_bin_lengths, int32_t capacity, int32_t* out_count);
/* Test helper: the light indices (into the pass's `lights`, in rising order) that the culling stage of this context's last tiled
 * lighting pass - either entry point - left for the 32x32 light tile (tile_x, tile_y).  *out_count = the length of the list; the
 * first min(*out_count, capacity) indices go to `out`.  A pass over a partition writes its own tiles' lists only.  Synchronises. */
VR_API int vr_debug_tile_light_list(vr_context* ctx, int32_t tile_x, int32_t tile_y, uint32_t* out, int32_t capacity, int32_t* out_count);
/* Test helpers.  vr_debug_light_domain: what the lighting entries make of a set of inputs, without a context or a device - *refused
 * and *sky_is_zero as 0 / 1, in `why` the field or the first bound that failed.  vr_debug_light_variant: which instantiation of the
 * shading kernel (and, of a tiled pass, of the culling kernel) this context's last lighting pass launched, as vr_light_plan.h numbers them; -1: none. */
VR_API int vr_debug_light_domain(const vr_view* view, int32_t w, int32_t h, const vr_light* lights, int32_t num_lights,
                                 const float ambient_top[3], const float ambient_bottom[3], int32_t* refused,
                                 int32_t* sky_is_zero, char* why, int32_t why_capacity);
VR_API int vr_debug_light_variant(vr_context* ctx, int32_t* shade, int32_t* cull);
/* Device memory a terrain holds, in bytes: out[0] textures (chains + decoded tables, and the query pyramid once a ray was cast), out[1] per-frame geometry scratch
 * (three rotating sets: instances, vertices, triangle records, bins - sized for params->max_instances) plus the staging
 * memory of host-pointer queries, out[2] node heights (after vr_terrain_update_heights), out[3] the sum. */
VR_API int vr_terrain_memory_bytes(const vr_terrain* t, uint64_t out[4]);
/* Test helper: the vertex stage's output (main_vs, terrain_vs.hlsl:35-62) of the last vr_terrain_render for `count`
 * vertices starting at vertex `first` of the instanced draw (vertex = instance * 1089 + row * 33 + column, rows = z):
 * six floats per vertex - o_position.xyzw (clip space) and o_vtx.pos.xz (world space).  Synchronises. */
VR_API int vr_debug_download_vertices(vr_terrain* t, uint32_t first, uint32_t count, float* out_xyzw_wxwz);
/* test helper: the device's linear -> sRGB8 render-target conversion applied to n host floats */
VR_API int vr_debug_srgb_encode(vr_context* ctx, const float* in, size_t n, uint8_t* out);
/* Test helper: sweeps every float with an exponent in [-60, 60) through the pixel shader's short reciprocal and square-root
 * sequences and counts differences from 1.0f / x and sqrtf(x): out[0] reciprocal, out[1] square root, out[2] values swept. */
VR_API int vr_debug_fastmath_check(vr_context* ctx, unsigned long long out[3]);

#ifdef __cplusplus
}
#endif
#endif /* VRTERRAIN_H */
