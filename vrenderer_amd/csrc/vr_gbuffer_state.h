// What the library believes about a G-buffer's contents, as one value, and everything that can happen to it as pure functions.
// Plain C++17: no HIP, no library types - a CPU program runs every short sequence of events against a model of the memory
// (tests/host/gbuffer_state_check.cpp).  vr_host.hip embeds the value in vr_gbuffer, asks the functions below and does the HIP
// work they name; vr_raster_plan.h (which sits above this header) decides what a tile pass is.
//
// The rule: knowledge is written BEHIND the work it describes.  A transition returns the state behind the event and the work the
// host must queue for it; the host does every call that can fail (allocation, fill, memset) and only then assigns the state.  A
// refusal on the way leaves the knowledge as it was.  What has truly happened by then is recorded where it happened: an array
// allocated (its contents: anything), the ranges reset, a clear written.
//
// Plane-state tracking (VR_OPT_PLANE_TRACKING): main_ps writes 0 to the emissive target for every pixel it shades
// (terrain_ps.hlsl:80) and RenderTargets::Clear writes 0 everywhere, so on this path the plane only ever holds zeros - 8 of the
// G-buffer's 28 bytes per pixel.  While the library KNOWS the plane is all zero (it cleared it, or a tile pass that writes every
// pixel of the target has run since the last foreign write) the tile pass does not rewrite it.  The same idea per REGION (the
// 8 rows x 32 pixels one wave of a 32-pixel raster tile resolves), one byte each, kept on the device by the fast variant of the
// tile pass: kRegionClear = every pixel holds the clear values in all planes; kRegionSpec = every pixel holds the pass's one
// specular constant (terrain_ps.hlsl:76).  A sky region known clear is not written again, a terrain region keeps its specular
// plane - the planes' contents are what they would be anyway.
//
// RenderTargets::Clear under the tracking is LAZY: the next tile pass that writes every pixel of every plane anyway (whole frame,
// shaded) runs as "over a cleared target" and the clear values are never written twice; anything else that looks at the planes
// first (a lighting pass, a partitioned / depth-only / fused pass, download, upload, describe) materialises the clear.
//
// Foreign writes: an upload of a plane -> nothing known of it; describe -> the pointers have left the library for good
// (`escaped`): nothing is assumed ever again, no hint, no skip, no depth ranges (tracking_live).
//
// The colour planes of a fused frame are LAZY as well (VR_OPT_GBUFFER_LAZY): vr_frame_submit's one kernel shades in registers and
// the tone-map stage reads HdrColor, so nothing in the frame reads diffuse, specular and normals.  Where the G-buffer-keeping fused
// flavour would run, the flavour that stores depth + HdrColor alone runs instead and the state remembers `planes_pending`: the three
// planes and the region bytes are those of the last materialised frame (consistent with each other; a clear that was pending is
// consumed - the recorded pass runs "over a cleared target", as the frame did, and writes what the clear would have), depth is the new frame's, and the host keeps the record of the frame (vr_gbuffer: view, parameters, terrain).  Whoever
// looks at the planes or the regions, writes part of them, or changes what the recorded frame would draw, first has the
// unfused tile pass queued for the record (gbs_planes_materialised behind it).  That pass over a cleared target writes - or, by
// the region bytes, knows to hold already - every pixel of every plane and leaves region bytes that depend on the frame alone, so
// frames nobody looked at drop out without a trace: a whole-frame pass over a cleared target, a Clear, or the next lazy frame
// replaces the record.  The first materialisation a target needs ends its laziness for good (`lazy_off`): a host that does read the
// G-buffer pays one extra tile pass once.  Depth is never pending.
#pragma once
#include <stdint.h>

constexpr uint32_t kRegionSpec = 1u, kRegionClear = 2u;
// the light tiles' depth ranges.  CLEAN: every entry "none"; VALID: the last writer of the depth plane left them; DIRTY: stale
enum { RANGES_NONE = 0, RANGES_CLEAN, RANGES_VALID, RANGES_DIRTY };

struct GbufferState {
    bool clear_pending = false;      // a Clear was asked for and has been neither written nor consumed by a tile pass
    bool cleared_once = false;       // (the clear at creation is a real one: the allocation holds anything)
    bool escaped = false;
    bool emissive_zero = false;      // the emissive plane holds only zeros
    int region_fill = 0;             // -1: the device array is current, else the byte it has to be filled with before its next use
    bool region_allocated = false;   //     (0 after anything foreign wrote a plane, kRegionClear after a clear)
    int ranges_state = RANGES_NONE;
    int ranges_rank = 0, ranges_world = 1;     // the screen-tile split a VALID array was rendered for
    bool ranges_allocated = false;
    bool planes_pending = false;     // diffuse, specular, normals and the region bytes are the last materialised frame's; the current frame is recorded
    bool lazy_off = false;           // a materialisation was needed once: this target's frames keep their planes from now on
};

inline bool tracking_live(bool plane_tracking, bool escaped) { return plane_tracking && !escaped; }
inline bool tracking_live(const GbufferState& s, bool plane_tracking) { return tracking_live(plane_tracking, s.escaped); }

// VR_OPT_GBUFFER_LAZY's policy: may a frame that qualifies for the G-buffer-keeping fused flavour leave its colour planes pending?
inline bool gbs_lazy_allowed(const GbufferState& s, bool plane_tracking, bool lazy_option, bool lock_view)
{ return lazy_option && tracking_live(s, plane_tracking) && !s.lazy_off && !lock_view; }
// Behind the unfused tile pass of the recorded frame (that pass's own step has been committed: gbs_pass_prepare ends `planes_pending`).
inline GbufferState gbs_planes_materialised(GbufferState s) { s.planes_pending = false; s.lazy_off = true; return s; }
// The record is given up without its pass: the target is destroyed or its terrain is, and nothing may be assumed of the planes.
inline GbufferState gbs_planes_abandoned(GbufferState s) { if (s.planes_pending) { s.planes_pending = false; s.lazy_off = true; s.region_fill = 0; } return s; }
// May a tile pass run over pending planes as it is?  Only one that leaves no trace of them: a shaded pass of the whole frame over a
// cleared target (it writes every plane; the next lazy frame among them).  Anything else has the record materialised first.
template <class Plan> inline bool gbs_pass_replaces_pending(const Plan& plan, bool whole, bool shaded, bool viewport_full)
{ return whole && shaded && viewport_full && plan.assume_cleared && (!plan.fuse || plan.keep); }

// The HIP work of a step, in the order the host does it.
struct GbufferWork {
    bool clear_now = false;          // write the clear values to the five planes
    bool alloc_ranges = false, alloc_region = false;
    bool reset_ranges = false;       // every entry of the ranges array becomes "none"
    int region_byte = -1;            // >= 0: fill the region array with it
};
struct GbufferStep {
    GbufferState after;              // assigned once `work` is queued
    GbufferWork work;
    bool region_usable = false;      // the region array goes to the kernel (PlaneHints::region, k_raster's region)
    bool emissive_zero = false;      // a reader's PlaneHints::emissive_zero
};

// (anything that writes the depth plane without leaving ranges: they are stale)
inline GbufferState gbs_touched(GbufferState s) { if (s.ranges_state == RANGES_VALID) s.ranges_state = RANGES_DIRTY; return s; }

// ---- clear ------------------------------------------------------------------------------------------------------------------------
// vr_gbuffer_clear.  The state is assigned in front of the work here: the planes are about to be overwritten (ranges stale) and
// the object has seen its first clear, whether the fills then succeed or not; gbs_clear_written follows them.
inline GbufferStep gbs_clear_requested(const GbufferState& s, bool plane_tracking)
{
    GbufferStep r; r.after = gbs_touched(s);
    r.after.planes_pending = false;          // (the clear replaces whatever the recorded frame would have left; depth is not pending)
    if (tracking_live(s, plane_tracking) && s.cleared_once) r.after.clear_pending = true;      // lazy
    else { r.after.cleared_once = true; r.work.clear_now = true; }
    return r;
}
// whoever looks at the planes first: a pending clear is written now (assigned in front of the work, as above)
inline GbufferStep gbs_materialise(const GbufferState& s)
{
    GbufferStep r; r.after = s;
    if (s.clear_pending) { r.after = gbs_touched(s); r.work.clear_now = true; }
    return r;
}
// (stream-ordered: every later pass on the stream sees the clear values; the region array is filled when next asked for)
inline GbufferState gbs_clear_written(GbufferState s) { s.emissive_zero = true; s.region_fill = (int)kRegionClear; s.clear_pending = false; return s; }

// ---- the arrays -------------------------------------------------------------------------------------------------------------------
inline GbufferState gbs_ranges_allocated(GbufferState s) { s.ranges_allocated = true; s.ranges_state = RANGES_NONE; return s; }
inline GbufferState gbs_region_allocated(GbufferState s) { s.region_allocated = true; if (s.region_fill < 0) s.region_fill = 0; return s; }
inline GbufferState gbs_ranges_reset(GbufferState s) { s.ranges_state = RANGES_CLEAN; return s; }
// the region array handed out by a step: allocated and current behind it
inline void gbs_region_current(const GbufferState& s, GbufferStep& r)
{
    r.work.alloc_region = !s.region_allocated;
    r.work.region_byte = (!s.region_allocated && s.region_fill < 0) ? 0 : s.region_fill;
    r.after.region_allocated = true; r.after.region_fill = -1;
    r.region_usable = true;
}

// ---- readers ----------------------------------------------------------------------------------------------------------------------
// A pass that reads the planes (the lighting passes), behind gbs_materialise: what it may take from the tracking instead.
inline GbufferStep gbs_reader(const GbufferState& s, bool plane_tracking)
{
    GbufferStep r; r.after = s;
    if (!tracking_live(s, plane_tracking)) return r;
    gbs_region_current(s, r);
    r.emissive_zero = s.emissive_zero;
    return r;
}
// the tiled lighting pass takes the depth ranges if they are VALID for this split (its culling stage resets what it reads)
inline GbufferState gbs_consume_ranges(GbufferState s, int rank, int world, bool* use)
{
    *use = s.ranges_state == RANGES_VALID && s.ranges_allocated && s.ranges_world == world && s.ranges_rank == rank;
    if (*use) s.ranges_state = RANGES_CLEAN;
    return s;
}
// vr_gbuffer_region_census without the device: every region counts as this state (0: nothing known); -1: read the array
inline int gbs_census(const GbufferState& s, bool plane_tracking)
{
    if (!tracking_live(s, plane_tracking)) return 0;
    if (s.clear_pending) return (int)kRegionClear;             // (cleared, as far as anyone can tell)
    if (!s.region_allocated || s.region_fill >= 0) return s.region_fill == (int)kRegionClear ? (int)kRegionClear : 0;
    return -1;
}
inline bool gbs_plane_known_zero(const GbufferState& s, bool plane_tracking, int plane)
{ return plane == 4 && tracking_live(s, plane_tracking) && (s.emissive_zero || s.clear_pending); }

// ---- writers ----------------------------------------------------------------------------------------------------------------------
// A tile pass as raster_plan() decided it (Plan: RasterPlan), for (rank, world).  PREPARE: the state behind the pass and the
// work in front of it - depth ranges reset and VALID, or stale; the region array current, or nothing known per region any more;
// a pending clear consumed; the emissive plane known zero if the pass leaves it so.  COMMIT is the assignment of `after`, once
// nothing can refuse the launch any more.
template <class Plan> inline GbufferStep gbs_pass_prepare(const GbufferState& s, const Plan& plan, int rank, int world)
{
    GbufferStep r; r.after = s;
    if (plan.consume_pending_clear) r.after.clear_pending = false;
    if (plan.lazy) {             // depth + HdrColor only: the planes and the region bytes stay as they are, consistent with each other
        r.after = gbs_touched(r.after);
        r.after.planes_pending = true;
        return r;
    }
    r.after.planes_pending = false;      // (materialised in front of the pass, or the pass leaves no trace of them)
    if (plan.ranges) {
        r.work.alloc_ranges = !s.ranges_allocated;
        r.work.reset_ranges = !s.ranges_allocated || s.ranges_state != RANGES_CLEAN;
        r.after.ranges_allocated = true; r.after.ranges_state = RANGES_VALID; r.after.ranges_rank = rank; r.after.ranges_world = world;
    } else r.after = gbs_touched(r.after);
    if (plan.track_regions) gbs_region_current(s, r);
    else r.after.region_fill = 0;
    if (plan.emissive_zero_after) r.after.emissive_zero = true;
    return r;
}
// something outside the library's passes wrote the plane (no region is known clear - that includes the emissive plane - or constant any more)
inline GbufferState gbs_foreign_write(GbufferState s, int plane)
{
    s = gbs_touched(s);
    if (plane == 4) s.emissive_zero = false;
    s.region_fill = 0;
    return s;
}
// the device pointers have left the library: whatever the caller writes through them is unknown here, now and for as long as the G-buffer lives
inline GbufferState gbs_escape(GbufferState s)
{
    s = gbs_touched(s);
    s.escaped = true; s.emissive_zero = false; s.region_fill = 0;
    return s;
}
