// The tile pass's host decisions as one pure function: which k_raster instantiation runs and what the pass does to the
// library's knowledge of the G-buffer (GbufferState, vr_gbuffer_state.h).  Plain C++17: no HIP, no library types - a CPU program
// enumerates every input (tests/host/raster_plan_check.cpp).  terrain_render_impl (vr_raster.hip) gathers the facts, asks
// raster_plan() and hands the answer to vr_gbuffer_apply_plan (vr_host.hip: gbs_pass_prepare, the HIP work, commit).
//
// Clear handling.  RenderTargets::Clear is lazy under the plane-state tracking (GbufferState::clear_pending): a shaded pass over
// the whole frame writes every pixel of every plane anyway and runs as "over a cleared target" - Clear + Render is one pass
// over the memory (consume_pending_clear); any other pass (a rank's share, depth only, the fused LIT variant) needs the clear
// values in memory first (materialise_first).
//
// The fast variant: heightmap and albedo of one size (the albedo footprint shares the height taps' coordinates), a
// power-of-two world size, the five planes of the G-buffer within 4 GB (one buffer resource), filled and shaded.  Only it
//   - leaves the light tiles' depth ranges behind, if asked for and over a target it fills completely (ranges);
//   - skips the emissive plane while that is known zero (noemi): it would only write zeros again;
//   - keeps the region states, on 32-pixel tiles (track_regions); any other variant writes the planes without keeping them;
//   - shades in the same pass (fuse) for a plain light list: LIT writes depth + HdrColor only, KEEP the G-buffer as well.
// A plane is skipped, and a state kept, only while the plane is known: never once the pointers have escaped.
//
// A KEEP request (vr_frame_submit) is decided in front of everything else: the flavour exists for the whole frame on 32-pixel
// tiles over a target known cleared, with the emissive plane known zero and a light list the streaming lighting pass takes as
// its plain case.  Where it does not apply the call goes on as the plain tile pass - the caller queues the lighting pass behind
// it as it always did and any error is that pass's to report.
#pragma once
#include "vr_gbuffer_state.h"

enum RasterRequest { RASTER_REQ_NONE = 0, RASTER_REQ_LIT, RASTER_REQ_KEEP };     // vr_terrain_render / _render_lit / vr_frame_submit

// one value per k_raster instantiation (vr_raster.hip: raster_kernel)
enum RasterVariant {
    RV_WIRE_32, RV_GENERIC_32, RV_DEPTH_32, RV_FAST_32, RV_FAST_NOEMI_32, RV_FAST_RANGES_32, RV_FAST_RANGES_NOEMI_32,
    RV_WIRE_64, RV_GENERIC_64, RV_DEPTH_64, RV_FAST_64, RV_FAST_NOEMI_64, RV_FAST_RANGES_64, RV_FAST_RANGES_NOEMI_64,
    RV_LIT_32, RV_LIT_64, RV_KEEP_32,
    RV_COUNT
};

struct RasterPlanIn {
    bool wireframe, depth_only, assume_cleared, depth_ranges;      // vr_render_params
    int world;                     // ranks the frame is split over (1: the whole frame)
    int tile_shift;                // 5 or 6
    bool tex_same;                 // heightmap and albedo of one size and level count
    bool ws_pow2;
    bool one_rsrc;                 // the planes within 4 GB of each other, depth first
    bool plane_tracking;           // the context's option
    bool clear_pending, emissive_zero, escaped;     // the G-buffer's state before the pass
    bool viewport_full;            // the view's viewport is the G-buffer
    bool width_mult4;
    RasterRequest request;
    bool lit_inputs_ok;            // KEEP: pointers, light count and device (LIT: its entry point has refused anything else)
    bool lit_plain;                // vr_deferred_make_args took the light list, without `extra` lights, inside sky_is_zero (vr_light_domain.h)
    bool hdr_fits;                 // KEEP: the frame fits the image (LIT: the host refuses an image too small)
    bool lazy_ok;                  // KEEP: the colour planes may stay pending (gbs_lazy_allowed)
};

struct RasterPlan {
    RasterVariant variant;
    bool fast;
    bool assume_cleared;           // what the kernel is told
    bool materialise_first;        // a pending clear must be written before the pass ...
    bool consume_pending_clear;    // ... or the pass is that clear
    bool ranges;                   // the pass leaves the depth ranges: VALID behind it (false: touched)
    bool noemi, fuse, keep;
    bool track_regions;            // the pass gets the region array; otherwise region_fill = 0
    bool emissive_zero_after;      // the plane is known zero behind the pass (false: the state is left as it is)
    bool lazy;                     // a KEEP frame that stores depth + HdrColor only (RV_LIT_32): planes_pending behind it
};

inline RasterPlan raster_plan(const RasterPlanIn& in)
{
    RasterPlan p{};
    const bool whole = in.world <= 1, tile32 = in.tile_shift == 5;
    const bool tracking_live = ::tracking_live(in.plane_tracking, in.escaped);
    const bool emissive_skip = tracking_live && in.emissive_zero;
    p.fast = in.tex_same && in.ws_pow2 && in.one_rsrc && !in.wireframe && !in.depth_only;
    p.keep = in.request == RASTER_REQ_KEEP && whole && p.fast && tile32 && (in.assume_cleared || in.clear_pending) && !in.depth_ranges
          && emissive_skip && in.viewport_full && in.width_mult4 && in.lit_inputs_ok && in.hdr_fits && in.lit_plain;
    // VR_OPT_GBUFFER_LAZY: the whole-frame LIT kernel in KEEP's place; the planes, the region bytes and a pending clear are left alone
    p.lazy = p.keep && in.lazy_ok;
    if (p.lazy) {
        p.assume_cleared = true; p.noemi = true; p.fuse = true;
        p.consume_pending_clear = in.clear_pending;      // (depth is written everywhere; the planes' share of the clear is the recorded pass's, over a "cleared" target)
        p.variant = RV_LIT_32;
        return p;
    }
    const bool lit = in.request == RASTER_REQ_LIT;           // (a KEEP request that does not qualify: a plain render from here on)
    // a pending clear: a whole-frame shaded pass is that clear, unless it is the LIT variant (depth + HdrColor only)
    p.consume_pending_clear = in.clear_pending && whole && !in.depth_only && !lit;
    p.materialise_first = in.clear_pending && !p.consume_pending_clear;
    p.assume_cleared = in.assume_cleared || p.consume_pending_clear;
    p.ranges = in.depth_ranges && p.fast && p.assume_cleared && !in.escaped;
    // (a clear written in front of the pass leaves the emissive plane known zero)
    p.noemi = p.fast && tracking_live && (in.emissive_zero || p.materialise_first);
    // LIT: only where the fast variant applies and the light list is the plain case (the host refuses a partial viewport there)
    p.fuse = p.keep || (lit && p.fast && !p.ranges && in.lit_plain && in.width_mult4);
    p.track_regions = p.fast && (!p.fuse || p.keep) && tile32 && tracking_live;
    // a shaded pass over a cleared target writes the emissive texel (0) of EVERY pixel of the frame, covered or not: the plane is
    // known zero again, whatever it held (a partitioned or keep-what-is-there pass writes zeros to some pixels, the fused variant
    // writes depth only: the state stays what it was)
    p.emissive_zero_after = !p.fuse && !p.noemi && !in.depth_only && p.assume_cleared && whole;
    const int edge = tile32 ? 0 : RV_WIRE_64 - RV_WIRE_32;
    if (p.keep) p.variant = RV_KEEP_32;
    else if (p.fuse) p.variant = tile32 ? RV_LIT_32 : RV_LIT_64;
    else if (in.wireframe) p.variant = (RasterVariant)(RV_WIRE_32 + edge);
    else if (p.fast) p.variant = (RasterVariant)(RV_FAST_32 + edge + (p.noemi ? 1 : 0) + (p.ranges ? 2 : 0));
    else p.variant = (RasterVariant)((in.depth_only ? RV_DEPTH_32 : RV_GENERIC_32) + edge);
    return p;
}
