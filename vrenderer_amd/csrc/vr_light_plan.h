// The lighting pass's host decisions as one pure function: which instantiation of the shading kernel and of k_light_cull runs,
// over which grids, how the light lists are laid out and whether the G-buffer's depth ranges are taken.  Plain C++17: no HIP, no
// library types - a CPU program enumerates every input (tests/host/light_plan_check.cpp).  vr_light_check (vr_deferred.hip) gathers
// the facts behind its refusals; deferred_light and deferred_light_tiled ask light_plan() and launch what it names.
//
// The streaming pass: k_deferred, which asks first what it need not read, where the plane-state tracking knows something (hinted),
// else the pure stream k_deferred_stream (the question costs that case 10 us: 221 vs 210 us at 8K) - also where the call's inputs are
// outside sky_is_zero (vr_light_domain.h): k_deferred stores +0 for a cleared texel without shading it.  A shadow binding compiles in
// EXTRA as well: shade_pixel<EXTRA, SHADOW> exists as <false, false>, <true, false>, <true, true>.  A width that is no multiple
// of 4 runs k_deferred_scalar, whole frames only: every light type compiled in, the shadow term a run-time argument.
// The tiled pass: EXTRA and SHADOW are independent (a shadowed sun over plain point lights stages no TiledExtra); CONE only where
// a spot light has cone_cos > 0; RANGES - the depth ranges the tile pass left instead of a second pass over the depth plane -
// where the G-buffer's state says they are usable for this split; taking them consumes them (the kernel resets each entry).
// vr_deferred_light_tiled has no shadow term and refuses spot and spherical lights: it only ever gets the plain kernels, and
// vr_deferred_light_tiled_ex with a plain list and no binding gets exactly those.
// NT (streaming loads and stores): the row-major quad kernels, at every frame size, like the tile pass's stores (vr_raster.hip:
// measured per size).  An 8K frame's lighting pass moves 1.2 GB through the caches and leaves 265 MB of dirty lines; the NEXT
// frame's tile pass then finds its texel tables evicted.  Measured (tools/exp_serial.py, profiles/r03_serial_cache_experiment.txt):
// tile pass 373-379 us behind a lighting pass with plain loads and stores, 325-332 us behind one that streams both (= its time with
// no lighting pass in between); streaming only the loads or only the stores changes nothing; the lighting pass itself goes from
// 199-205 to 207 us.  Only the row-major output streams: the packed kernels (a rank's share) and the scalar one do not.
#pragma once
#include <stddef.h>

enum LightEntry { LIGHT_STREAM = 0, LIGHT_TILED, LIGHT_TILED_EX };    // vr_deferred_light[_shadowed] / _tiled / _tiled_ex
constexpr int kPlanOwnerTile = 128, kPlanLightTile = 32, kPlanTileLightCap = 1024;    // VR_OWNER_TILE, kLightTile, VR_TILE_LIGHT_CAP (vr_deferred.hip asserts)

// one value per launched instantiation of a shading kernel, in the order of vr_deferred.hip's kernel tables; within a family:
// plain, EXTRA, SHADOW (streaming: EXTRA + SHADOW), EXTRA + SHADOW (tiled)
enum LightVariant {
    LV_STREAM_ROW, LV_STREAM_ROW_EXTRA, LV_STREAM_ROW_SHADOW, LV_STREAM_PACKED, LV_STREAM_PACKED_EXTRA, LV_STREAM_PACKED_SHADOW,      // k_deferred_stream
    LV_HINTED_ROW, LV_HINTED_ROW_EXTRA, LV_HINTED_ROW_SHADOW, LV_HINTED_PACKED, LV_HINTED_PACKED_EXTRA, LV_HINTED_PACKED_SHADOW,      // k_deferred
    LV_SCALAR,                                                                                                                          // k_deferred_scalar
    LV_TILED_ROW, LV_TILED_ROW_EXTRA, LV_TILED_ROW_SHADOW, LV_TILED_ROW_EXTRA_SHADOW,                                                   // k_deferred_tiled
    LV_TILED_PACKED, LV_TILED_PACKED_EXTRA, LV_TILED_PACKED_SHADOW, LV_TILED_PACKED_EXTRA_SHADOW,
    LV_COUNT
};
enum LightCull { LC_DEPTH, LC_RANGES, LC_DEPTH_CONE, LC_RANGES_CONE, LC_COUNT };      // one value per k_light_cull<RANGES, CONE>

struct LightPlanIn {
    LightEntry entry;
    bool packed;                   // a partition was given (even of one rank): the packed tile-major output
    bool width_mult4, shadow;      // (shadow: a binding was given)
    bool extra, cone;              // a spot or spherical light is in the list; a spot light has cone_cos > 0 (cone_cull_terms)
    bool hinted;                   // PlaneHints: a region array, or the emissive plane known zero (the streaming pass's question)
    bool ranges_usable;            // the G-buffer's depth ranges are VALID for this split
    bool sky_not_zero;             // vr_light_domain.h: sky_is_zero could NOT be shown - a cleared texel may shade to something but +0 (false: every shortcut holds)
    int num_lights, w, h, num_owned;       // (num_owned: owner tiles of this rank, packed)
};
struct LightPlan {
    bool launch;                   // false: this rank owns no tile - the call succeeds and queues no kernel
    LightVariant shade; unsigned shade_grid;
    LightCull cull; unsigned cull_grid;     // the tiled entry points only, like everything below
    int macro_x, tiles32_x, tiles32_y;      // owner (= macro) tiles per row; the grid of light tiles
    int list_stride;               // words per light tile: count + up to min(num_lights, VR_TILE_LIGHT_CAP) indices
    size_t list_words, scratch_words;       // (scratch: per macro tile, the lights that touch its box, in four regions - one per wave of k_light_cull)
    bool consume_ranges;           // k_light_cull<RANGES>: the state is CLEAN behind the call
};

// The widths the entry points refuse, in front of everything they do: the quad kernels need a multiple of 4, and only the
// whole-frame streaming pass has a kernel for anything else.  light_plan() is asked for accepted widths only.
inline bool light_width_ok(const LightPlanIn& in) { return in.width_mult4 || (in.entry == LIGHT_STREAM && !in.packed); }

// Outside sky_is_zero only a kernel that shades every texel may run: k_deferred_stream and k_deferred_scalar.  k_deferred stores +0
// for a wave of cleared texels and k_deferred_tiled gives its background pixels no light, whatever the host knows - so the
// streaming pass drops the question (hinted) and the tiled entry points, which have no such kernel (and take up to 65536 lights
// where the streaming pass takes 16), refuse.  light_plan() is asked for accepted calls only.
inline bool light_sky_ok(const LightPlanIn& in) { return !in.sky_not_zero || in.entry == LIGHT_STREAM; }

inline LightPlan light_plan(const LightPlanIn& in)
{
    LightPlan p{};
    // vr_deferred_light_tiled: no binding reaches it and fill_light has refused what `extra` and `cone` stand for
    const bool plain_only = in.entry == LIGHT_TILED;
    const bool shadow = in.shadow && !plain_only, extra = in.extra && !plain_only, cone = in.cone && in.entry == LIGHT_TILED_EX;
    const size_t npx = (size_t)in.w * (size_t)in.h;
    p.launch = !in.packed || in.num_owned > 0;
    if (in.entry == LIGHT_STREAM) {
        // packed: a block = 8 rows of an owner tile; row-major: 256 quads, or 256 pixels of the scalar kernel
        p.shade_grid = in.packed ? (unsigned)in.num_owned * 16u : (unsigned)(((in.width_mult4 ? npx / 4 : npx) + 255) / 256);
        p.shade = !in.width_mult4 ? LV_SCALAR : (LightVariant)((in.hinted && !in.sky_not_zero ? LV_HINTED_ROW : LV_STREAM_ROW) + (in.packed ? 3 : 0) + (shadow ? 2 : extra ? 1 : 0));
        return p;
    }
    p.shade = (LightVariant)((in.packed ? LV_TILED_PACKED : LV_TILED_ROW) + (extra ? 1 : 0) + (shadow ? 2 : 0));
    p.consume_ranges = in.ranges_usable;
    p.cull = (LightCull)((p.consume_ranges ? LC_RANGES : LC_DEPTH) + (cone ? LC_DEPTH_CONE : 0));
    // light lists: one per 32x32 light tile; the culling stage: one workgroup per 128x128 macro tile (= owner tile, 4x4 light tiles)
    p.macro_x = (in.w + kPlanOwnerTile - 1) / kPlanOwnerTile;
    const int macro_y = (in.h + kPlanOwnerTile - 1) / kPlanOwnerTile;
    p.tiles32_x = (in.w + kPlanLightTile - 1) / kPlanLightTile; p.tiles32_y = (in.h + kPlanLightTile - 1) / kPlanLightTile;
    p.list_stride = (in.num_lights < kPlanTileLightCap ? in.num_lights : kPlanTileLightCap) + 1;
    p.list_words = (size_t)p.tiles32_x * p.tiles32_y * p.list_stride;
    p.scratch_words = (size_t)p.macro_x * macro_y * (size_t)(((in.num_lights + 3) / 4) * 4) + 4;
    p.cull_grid = in.packed ? (unsigned)in.num_owned : (unsigned)(p.macro_x * macro_y);
    p.shade_grid = in.packed ? (unsigned)in.num_owned * 16u : (unsigned)(p.tiles32_x * p.tiles32_y);
    return p;
}
