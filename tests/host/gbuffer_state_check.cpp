// vr_gbuffer_state.h against a transcription of the code it replaced, and against a model of the memory it speaks about.
//
// (a) The transcription ("Old") is vr_host.hip's G-buffer bookkeeping as it stood when it lived in ten loose fields of vr_gbuffer
//     (gbuffer_touch, gbuffer_clear_now, vr_gbuffer_clear, _materialise, gbuffer_region_prepare, vr_gbuffer_plane_hints,
//     _region_census, _plane_known_zero, gbuffer_ranges_prepare, vr_gbuffer_settle_clear, _apply_plan, _foreign_write, _escape,
//     _consume_ranges), HIP calls replaced by a list of the fills they queue.  The other side ("New") is what vr_host.hip does now
//     around the header's transitions.  The two intended differences are switches of the transcription:
//       fix_clear   a render refused after it would have consumed a pending clear leaves the clear pending
//                   (clear_pending falls with the rest of the pass's state, not in front of the geometry chain);
//       fix_apply   a tile pass whose preparation fails leaves ranges, region and emissive knowledge as they were
//                   (allocations first, then the fills, the state last; what has happened by then - an array allocated, the
//                   ranges reset - is recorded as it happens).
//     With both on, states, return codes, answers and queued fills agree after every event of every sequence; with both off
//     (the parent as it was) they agree on every sequence up to its first refused render.
// (b) The memory model.  Two regions of two pixels, five planes; a pixel of a plane holds the clear value, the specular constant,
//     a foreign value or "pass n's terrain" (the emissive plane's terrain value IS the clear value: main_ps writes 0 there).  Two
//     ranges entries (none / left by pass n / unusable); region 0 is rank 0's and region 1 rank 1's when the world size is 2.
//     REAL memory gets what the library queues: lazy clears, skipped regions, skipped planes.  The SHADOW gets every clear at
//     once and every store of every pass.  The claims, checked after every event, are listed at check_claims().
//
//   gbuffer_state_check                is the header right?
//   gbuffer_state_check --break-each   is the model alive?  One transition at a time is weakened; each must be reported by (b).
//
// g++ -std=c++17 -O1 -Wall -Werror -I vrenderer_amd/csrc tests/host/gbuffer_state_check.cpp
#include "vr_raster_plan.h"

#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>

// ---- the world ---------------------------------------------------------------------------------------------------------------------
enum { P_DEPTH = 0, P_DIFF, P_SPEC, P_NRM, P_EMI, N_PLANES };
constexpr int V_CLEAR = 0, V_SPEC = 1, V_FOREIGN = 2, V_PASS = 16;        // V_PASS + n: what pass n drew
constexpr int R_NONE = -1, R_UNUSABLE = -2;                                 // a ranges entry (else: the pass that left it)
constexpr int B_POISON = 0xff;                                              // a region byte nobody has written
struct Mem { int px[2][2][N_PLANES]; };
static bool same(const Mem& a, const Mem& b) { return memcmp(&a, &b, sizeof(Mem)) == 0; }
static bool region_clear(const Mem& m, int r) { for (int p = 0; p < 2; p++) for (int k = 0; k < N_PLANES; k++) if (m.px[r][p][k] != V_CLEAR) return false; return true; }

enum Kind { K_CLEAR, K_RENDER, K_LIGHT_STREAM, K_LIGHT_TILED, K_UPLOAD, K_DOWNLOAD, K_DESCRIBE, K_POINTER_WRITE, K_TRACKING };
enum Shape { S_FAST, S_NOT_ELIGIBLE, S_WIRE, S_DEPTH, S_WIRE_DEPTH, N_SHAPES };
// where a render is refused: the geometry chain / order_tile_pass_begin / the VR_REQUIREs on the HDR image (all between the clear's
// settlement and vr_gbuffer_apply_plan), or one of apply_plan's own four fallible calls
enum Refuse { F_NO = 0, F_BEFORE_APPLY, F_RANGES_ALLOC, F_REGION_ALLOC, F_RANGES_FILL, F_REGION_MEMSET, N_REFUSE };
struct Ev {
    int kind = K_CLEAR, arg = 0;                   // plane / on-off / split
    int shape = S_FAST, tile_shift = 5, request = RASTER_REQ_NONE, refuse = F_NO;
    bool assume_cleared = false, depth_ranges = false;
    int split = 0;                                 // 0: whole frame, 1: rank 0 of 2, 2: rank 1 of 2
    int cov[2] = { 0, 0 };                         // per region: 0 none, 1 both pixels, 2 pixel 0 only
};
static int split_world(int split) { return split ? 2 : 1; }
static int split_rank(int split) { return split == 2 ? 1 : 0; }
static bool in_split(int split, int region) { return split == 0 || split_rank(split) == region; }

static const char* const kBreakNames[] = {
    "none",
    "neither a lazy clear nor its materialisation touches the ranges", "foreign write forgets region_fill = 0", "foreign write of the emissive plane keeps emissive_zero",
    "foreign write does not touch the ranges", "escape forgets `escaped`", "consume ignores the split", "consume leaves the ranges VALID",
    "commit in front of the fallible calls", "a pass without ranges does not touch them", "a pass without region tracking forgets region_fill = 0",
    "the pending clear falls in front of the refusals", "DIRTY ranges are not reset", "a reader gets hints without live tracking",
    "the region array is handed out unfilled", "every pass leaves emissive_zero" };
enum { BRK_NONE = 0, BRK_MATERIALISE_TOUCH, BRK_FOREIGN_REGION, BRK_FOREIGN_EMISSIVE, BRK_FOREIGN_TOUCH, BRK_ESCAPE, BRK_CONSUME_SPLIT, BRK_CONSUME_CLEAN,
       BRK_COMMIT_EARLY, BRK_PASS_TOUCH, BRK_PASS_REGION, BRK_CLEAR_EARLY, BRK_DIRTY_RESET, BRK_READER_LIVE, BRK_REGION_UNFILLED, BRK_EMISSIVE_ALWAYS, N_BREAKS };
static int g_break = BRK_NONE;

// what a call queued and answered
enum { OP_CLEAR = 1, OP_RANGES_RESET = 2, OP_REGION_FILL = 16 };            // OP_REGION_FILL + byte
struct Out {
    int rc = 0, nops = 0, ops[8] = {};
    bool region = false, emissive_zero = false, use_ranges = false;
    RasterPlan plan = {};
    void op(int o) { if (nops < 8) ops[nops] = o; nops++; }
};
static bool same(const Out& a, const Out& b)
{ return (a.rc != 0) == (b.rc != 0) && a.nops == b.nops && memcmp(a.ops, b.ops, sizeof(a.ops)) == 0 && a.region == b.region && a.emissive_zero == b.emissive_zero
      && a.use_ranges == b.use_ranges && memcmp(&a.plan, &b.plan, sizeof(RasterPlan)) == 0; }

static bool same(const GbufferState& a, const GbufferState& b)
{ return a.clear_pending == b.clear_pending && a.cleared_once == b.cleared_once && a.escaped == b.escaped && a.emissive_zero == b.emissive_zero && a.region_fill == b.region_fill
      && a.region_allocated == b.region_allocated && a.ranges_state == b.ranges_state && a.ranges_rank == b.ranges_rank && a.ranges_world == b.ranges_world && a.ranges_allocated == b.ranges_allocated; }

static RasterPlanIn plan_in(const Ev& e, bool tracking, bool clear_pending, bool emissive_zero, bool escaped)
{
    RasterPlanIn in{};
    in.wireframe = e.shape == S_WIRE || e.shape == S_WIRE_DEPTH; in.depth_only = e.shape == S_DEPTH || e.shape == S_WIRE_DEPTH;
    in.assume_cleared = e.assume_cleared; in.depth_ranges = e.depth_ranges;
    in.world = split_world(e.split); in.tile_shift = e.tile_shift;
    in.tex_same = e.shape != S_NOT_ELIGIBLE; in.ws_pow2 = true; in.one_rsrc = true;
    in.plane_tracking = tracking; in.clear_pending = clear_pending; in.emissive_zero = emissive_zero; in.escaped = escaped;
    in.viewport_full = true; in.width_mult4 = true; in.request = (RasterRequest)e.request; in.lit_inputs_ok = true; in.lit_plain = true; in.hdr_fits = true;
    return in;
}

// ---- (a) the transcription ---------------------------------------------------------------------------------------------------------
struct Old {
    bool d_ranges = false; int ranges_state = RANGES_NONE, ranges_rank = 0, ranges_world = 1;
    bool emissive_zero = false, escaped = false;
    bool d_region = false; int region_fill = 0;
    bool clear_pending = false, cleared_once = false;
    bool fix_clear = false, fix_apply = false;

    void touch() { if (ranges_state == RANGES_VALID) ranges_state = RANGES_DIRTY; }
    void clear_now(Out& o) { touch(); o.op(OP_CLEAR); emissive_zero = true; region_fill = (int)kRegionClear; clear_pending = false; }
    void clear(bool tracking, Out& o)
    {
        if (tracking && !escaped && cleared_once) { touch(); clear_pending = true; return; }
        cleared_once = true;
        clear_now(o);
    }
    void materialise(Out& o) { if (clear_pending) clear_now(o); }
    int region_prepare(Out& o, int refuse)
    {
        if (!d_region) {
            if (refuse == F_REGION_ALLOC) return 1;
            d_region = true;
            if (region_fill < 0) region_fill = 0;
        }
        if (region_fill >= 0) {
            if (refuse == F_REGION_MEMSET) return 1;
            o.op(OP_REGION_FILL + region_fill);
            region_fill = -1;
        }
        return 0;
    }
    void plane_hints(bool tracking, Out& o)
    {
        materialise(o);
        if (!tracking || escaped) return;
        if (region_prepare(o, F_NO)) return;
        o.region = true; o.emissive_zero = emissive_zero;
    }
    int census(bool tracking) const
    {
        if (!tracking || escaped) return 0;
        if (clear_pending) return 2;
        if (!d_region || region_fill >= 0) return region_fill == (int)kRegionClear ? 2 : 0;
        return -1;
    }
    bool known_zero(bool tracking) const { return tracking && (emissive_zero || clear_pending) && !escaped; }
    int ranges_prepare(Out& o, int refuse)
    {
        if (!d_ranges) {
            if (refuse == F_RANGES_ALLOC) return 1;
            d_ranges = true;
            ranges_state = RANGES_NONE;
        }
        if (ranges_state != RANGES_CLEAN) {
            if (refuse == F_RANGES_FILL) return 1;
            o.op(OP_RANGES_RESET);
            ranges_state = RANGES_CLEAN;
        }
        return 0;
    }
    int apply_plan(const RasterPlan& plan, int rank, int world, Out& o, int refuse)
    {
        if (plan.ranges) {
            if (ranges_prepare(o, refuse)) return 1;
            ranges_state = RANGES_VALID; ranges_rank = rank; ranges_world = world;
        } else touch();
        if (plan.track_regions) { if (region_prepare(o, refuse)) return 1; o.region = true; }
        else region_fill = 0;
        if (plan.emissive_zero_after) emissive_zero = true;
        return 0;
    }
    // fix_apply: the same work on a copy, the allocations in front of the fills; the object learns the result on success and
    // only what has happened (an array allocated, the ranges reset) on a refusal
    int apply_plan_all_or_nothing(const RasterPlan& plan, int rank, int world, Out& o, int refuse)
    {
        if (plan.ranges && !d_ranges) { if (refuse == F_RANGES_ALLOC) return 1; d_ranges = true; ranges_state = RANGES_NONE; }
        if (plan.track_regions && !d_region) { if (refuse == F_REGION_ALLOC) return 1; d_region = true; if (region_fill < 0) region_fill = 0; }
        Old t = *this;
        Out ot = o;
        if (t.apply_plan(plan, rank, world, ot, refuse)) {
            if (ot.nops > o.nops) { o = ot; o.region = false; ranges_state = RANGES_CLEAN; }       // (the reset was queued; the memset was not)
            return 1;
        }
        const bool fc = fix_clear, fa = fix_apply;
        *this = t; fix_clear = fc; fix_apply = fa; o = ot;
        return 0;
    }
    void render(const Ev& e, bool tracking, Out& o)
    {
        const RasterPlan plan = raster_plan(plan_in(e, tracking, clear_pending, emissive_zero, escaped));
        o.plan = plan;
        if (plan.consume_pending_clear && !fix_clear) clear_pending = false;       // vr_gbuffer_settle_clear
        if (plan.materialise_first) materialise(o);
        if (e.refuse == F_BEFORE_APPLY) { o.rc = 1; return; }
        o.rc = fix_apply ? apply_plan_all_or_nothing(plan, split_rank(e.split), split_world(e.split), o, e.refuse)
                         : apply_plan(plan, split_rank(e.split), split_world(e.split), o, e.refuse);
        if (o.rc) o.region = false;
        if (!o.rc && plan.consume_pending_clear && fix_clear) clear_pending = false;
    }
    void foreign_write(int plane) { touch(); if (plane == 4) emissive_zero = false; region_fill = 0; }
    void escape() { touch(); escaped = true; emissive_zero = false; region_fill = 0; }
    bool consume_ranges(int rank, int world)
    {
        const bool use = ranges_state == RANGES_VALID && d_ranges && ranges_world == world && ranges_rank == rank;
        if (use) ranges_state = RANGES_CLEAN;
        return use;
    }
    void event(const Ev& e, bool tracking, Out& o)
    {
        switch (e.kind) {
        case K_CLEAR: clear(tracking, o); break;
        case K_RENDER: render(e, tracking, o); break;
        case K_LIGHT_STREAM: plane_hints(tracking, o); break;
        case K_LIGHT_TILED: plane_hints(tracking, o); o.use_ranges = consume_ranges(split_rank(e.arg), split_world(e.arg)); break;
        case K_UPLOAD: materialise(o); foreign_write(e.arg); break;
        case K_DOWNLOAD: materialise(o); break;
        case K_DESCRIBE: materialise(o); escape(); break;
        default: break;
        }
    }
    bool same_state(const GbufferState& s) const
    { return d_ranges == s.ranges_allocated && ranges_state == s.ranges_state && ranges_rank == s.ranges_rank && ranges_world == s.ranges_world && emissive_zero == s.emissive_zero
          && escaped == s.escaped && d_region == s.region_allocated && region_fill == s.region_fill && clear_pending == s.clear_pending && cleared_once == s.cleared_once; }
};

// ---- what vr_host.hip does around the header (each weakening of --break-each sits where the transition is used) --------------------
struct New {
    GbufferState st;
    void clear_step(const GbufferStep& step, Out& o)       // gbuffer_clear_step
    {
        st = step.after;
        if (!step.work.clear_now) return;
        o.op(OP_CLEAR);
        st = gbs_clear_written(st);
    }
    void materialise(Out& o)
    {
        GbufferStep step = gbs_materialise(st);
        if (g_break == BRK_MATERIALISE_TOUCH) step.after.ranges_state = st.ranges_state;
        clear_step(step, o);
    }
    int run_step(GbufferStep step, Out& o, int refuse)    // gbuffer_run_step
    {
        if (g_break == BRK_COMMIT_EARLY) st = step.after;
        if (g_break == BRK_REGION_UNFILLED) step.work.region_byte = -1;
        const GbufferWork& w = step.work;
        if (w.alloc_ranges) { if (refuse == F_RANGES_ALLOC) return 1; st = gbs_ranges_allocated(st); }
        if (w.alloc_region) { if (refuse == F_REGION_ALLOC) return 1; st = gbs_region_allocated(st); }
        if (w.reset_ranges) { if (refuse == F_RANGES_FILL) return 1; o.op(OP_RANGES_RESET); st = gbs_ranges_reset(st); }
        if (w.region_byte >= 0) { if (refuse == F_REGION_MEMSET) return 1; o.op(OP_REGION_FILL + w.region_byte); }
        st = step.after;
        return 0;
    }
    void plane_hints(bool tracking, Out& o)
    {
        materialise(o);
        GbufferState view = st;
        if (g_break == BRK_READER_LIVE) { view.escaped = false; tracking = true; }
        GbufferStep s2 = gbs_reader(view, tracking);
        s2.after.escaped = st.escaped;
        if (run_step(s2, o, F_NO)) return;
        o.region = s2.region_usable; o.emissive_zero = s2.emissive_zero;
    }
    void render(const Ev& e, bool tracking, Out& o)
    {
        const RasterPlan plan = raster_plan(plan_in(e, tracking, st.clear_pending, st.emissive_zero, st.escaped));
        o.plan = plan;
        if (g_break == BRK_CLEAR_EARLY && plan.consume_pending_clear) st.clear_pending = false;
        if (plan.materialise_first) materialise(o);
        if (e.refuse == F_BEFORE_APPLY) { o.rc = 1; return; }
        GbufferStep step = gbs_pass_prepare(st, plan, split_rank(e.split), split_world(e.split));
        if (g_break == BRK_PASS_TOUCH && !plan.ranges) step.after.ranges_state = st.ranges_state;
        if (g_break == BRK_PASS_REGION && !plan.track_regions) step.after.region_fill = st.region_fill;
        if (g_break == BRK_DIRTY_RESET && st.ranges_state == RANGES_DIRTY) step.work.reset_ranges = false;
        if (g_break == BRK_EMISSIVE_ALWAYS) step.after.emissive_zero = true;
        o.rc = run_step(step, o, e.refuse);
        o.region = !o.rc && step.region_usable;
    }
    void event(const Ev& e, bool tracking, Out& o)
    {
        switch (e.kind) {
        case K_CLEAR: {
            GbufferStep step = gbs_clear_requested(st, tracking);
            if (g_break == BRK_MATERIALISE_TOUCH && !step.work.clear_now) step.after.ranges_state = st.ranges_state;
            clear_step(step, o);
            break; }
        case K_RENDER: render(e, tracking, o); break;
        case K_LIGHT_STREAM: plane_hints(tracking, o); break;
        case K_LIGHT_TILED: {
            plane_hints(tracking, o);
            const int rank = split_rank(e.arg), world = split_world(e.arg);
            const GbufferState before = st;
            st = gbs_consume_ranges(st, g_break == BRK_CONSUME_SPLIT ? st.ranges_rank : rank, g_break == BRK_CONSUME_SPLIT ? st.ranges_world : world, &o.use_ranges);
            if (g_break == BRK_CONSUME_CLEAN) st = before;
            break; }
        case K_UPLOAD: {
            materialise(o);
            const GbufferState before = st;
            st = gbs_foreign_write(st, e.arg);
            if (g_break == BRK_FOREIGN_REGION) st.region_fill = before.region_fill;
            if (g_break == BRK_FOREIGN_EMISSIVE) st.emissive_zero = before.emissive_zero;
            if (g_break == BRK_FOREIGN_TOUCH) st.ranges_state = before.ranges_state;
            break; }
        case K_DOWNLOAD: materialise(o); break;
        case K_DESCRIBE: materialise(o); st = gbs_escape(st); if (g_break == BRK_ESCAPE) st.escaped = false; break;
        default: break;
        }
    }
};

// ---- (b) the memory the New side's work lands in -----------------------------------------------------------------------------------
struct Sim {
    Old pure, fixed;            // the transcription as it was / with both intended differences
    New lib;
    bool tracking = true;
    bool pure_comparable = true;
    Mem real, shadow;
    int region[2] = { B_POISON, B_POISON };        // d_region
    int ranges[2] = { R_UNUSABLE, R_UNUSABLE };    // d_ranges
    int serial = 0;                                 // passes so far
    int valid_pass = -1;                            // the pass that left the ranges the state calls VALID
    bool escaped_for_real = false;                  // the caller holds the pointers
};

static long failures = 0, sequences = 0, events_run = 0;
static bool g_quiet = false;
static std::string show(const Ev& e)
{
    char b[160];
    static const char* const shapes[] = { "fast", "not-eligible", "wire", "depth", "wire+depth" };
    static const char* const refs[] = { "", " REFUSED before apply", " REFUSED ranges alloc", " REFUSED region alloc", " REFUSED ranges fill", " REFUSED region memset" };
    switch (e.kind) {
    case K_CLEAR: return "clear";
    case K_RENDER: snprintf(b, sizeof b, "render(%s tile%d req%d ac%d dr%d split%d cov%d%d%s)", shapes[e.shape], 1 << e.tile_shift, e.request, (int)e.assume_cleared, (int)e.depth_ranges,
                            e.split, e.cov[0], e.cov[1], refs[e.refuse]); return b;
    case K_LIGHT_STREAM: return "light";
    case K_LIGHT_TILED: snprintf(b, sizeof b, "light_tiled(split%d)", e.arg); return b;
    case K_UPLOAD: snprintf(b, sizeof b, "upload(%d)", e.arg); return b;
    case K_DOWNLOAD: return "download";
    case K_DESCRIBE: return "describe";
    case K_POINTER_WRITE: snprintf(b, sizeof b, "pointer_write(%d)", e.arg); return b;
    case K_TRACKING: return e.arg ? "tracking on" : "tracking off";
    }
    return "?";
}
static const Ev* g_seq[64]; static int g_len = 0;
static void fail(const char* what)
{
    if (failures++ < 10 && !g_quiet) {
        printf("FAIL %s\n   ", what);
        for (int i = 0; i < g_len; i++) printf(" %s;", show(*g_seq[i]).c_str());
        printf("\n");
    }
}

static void clear_mem(Mem& m) { memset(&m, 0, sizeof m); }
static bool covered(const Ev& e, int r, int p) { return e.cov[r] == 1 || (e.cov[r] == 2 && p == 0); }

// The tile pass on REAL memory.  Which planes a variant stores per covered / uncovered pixel: k_raster's resolve (vr_raster.hip:1639-1717:
// an uncovered pixel is stored - with the clear values - only over a cleared target; LIT stores depth alone, depth-only likewise,
// NOEMI leaves the emissive plane, skip_spec the specular one).  The region rule is vr_raster.hip:1574-1591, transcribed: none / all /
// partial coverage x assume_cleared x old byte -> new byte, skip_all, skip_spec.  The whole-tile early-out at :1291 (nothing binned,
// cleared target, every region of the tile known clear) is the none-covered, known-clear row of that rule for all regions of the tile at
// once: nothing stored, no byte changed, no range left.
static void pass_real(Sim& s, const Ev& e, const Out& o, int n)
{
    const RasterPlan& plan = o.plan;
    const bool depth_only = e.shape == S_DEPTH || e.shape == S_WIRE_DEPTH;
    const bool lit = plan.fuse && !plan.keep, noemi = plan.noemi || plan.keep;
    const bool track = o.region;
    if (track && !(plan.fast && e.tile_shift == 5 && (!plan.fuse || plan.keep))) fail("(b) the region array went to a variant that does not keep it");
    for (int r = 0; r < 2; r++) {
        if (!in_split(e.split, r)) continue;
        const bool none_cov = e.cov[r] == 0, all_cov = e.cov[r] == 1;
        bool skip_all = false, skip_spec = false;
        if (track) {
            const int st = s.region[r];
            if (st == B_POISON) { fail("(b) the tile pass read a region byte nobody wrote"); }
            int nst;
            if (none_cov) { skip_all = plan.assume_cleared ? st == (int)kRegionClear : true; nst = plan.assume_cleared ? (int)kRegionClear : st; }
            else if (all_cov) { skip_spec = st == (int)kRegionSpec; nst = (int)kRegionSpec; }
            else nst = (!plan.assume_cleared && st == (int)kRegionSpec) ? (int)kRegionSpec : 0;
            s.region[r] = nst;
        }
        if (plan.keep && skip_all && !region_clear(s.shadow, r)) fail("(b) KEEP stored +0 HdrColor for a region that is not clear");
        for (int p = 0; p < 2 && !skip_all; p++) {
            const bool cov = covered(e, r, p);
            if (!cov && !plan.assume_cleared) continue;
            int* px = s.real.px[r][p];
            px[P_DEPTH] = cov ? V_PASS + n : V_CLEAR;
            if (lit || depth_only) continue;
            px[P_DIFF] = px[P_NRM] = cov ? V_PASS + n : V_CLEAR;
            if (!skip_spec) px[P_SPEC] = cov ? V_SPEC : V_CLEAR;
            if (!noemi) px[P_EMI] = V_CLEAR;
        }
        if (plan.ranges && !none_cov) s.ranges[r] = s.ranges[r] == R_NONE ? n : R_UNUSABLE;      // (atomicMin / Max into what the entry held)
    }
}
// ... and on the SHADOW: the clear happened when it was asked for, nothing is ever skipped
static void pass_shadow(Sim& s, const Ev& e, const Out& o, int n)
{
    const bool depth_only = e.shape == S_DEPTH || e.shape == S_WIRE_DEPTH, lit = o.plan.fuse && !o.plan.keep;
    for (int r = 0; r < 2; r++) {
        if (!in_split(e.split, r)) continue;
        for (int p = 0; p < 2; p++) {
            const bool cov = covered(e, r, p);
            if (!cov && !e.assume_cleared) continue;
            int* px = s.shadow.px[r][p];
            px[P_DEPTH] = cov ? V_PASS + n : V_CLEAR;
            if (lit || depth_only) continue;
            px[P_DIFF] = px[P_NRM] = cov ? V_PASS + n : V_CLEAR;
            px[P_SPEC] = cov ? V_SPEC : V_CLEAR;
            px[P_EMI] = V_CLEAR;
        }
    }
}
// a lighting pass: what it takes for every pixel of its share, from the hints or from memory, against the shadow
static void read_lit(Sim& s, const Out& o, int split)
{
    for (int r = 0; r < 2; r++) {
        if (!in_split(split, r)) continue;
        const int st = o.region ? s.region[r] : 0;
        if (o.region && st == B_POISON) fail("(b) a lighting pass read a region byte nobody wrote");
        for (int p = 0; p < 2; p++) for (int k = 0; k < N_PLANES; k++) {
            int v = s.real.px[r][p][k];
            if (st == (int)kRegionClear) v = V_CLEAR;
            else if (st == (int)kRegionSpec && k == P_SPEC) v = V_SPEC;
            if (o.emissive_zero && k == P_EMI) v = V_CLEAR;
            if (v != s.shadow.px[r][p][k]) { fail("(b) a lighting pass saw something else than memory with every clear eager and nothing skipped"); return; }
        }
    }
}
// the ranges of a split against the depth plane: an entry is "none" over a tile without depth below 1.0, else pass n's over a tile
// whose every such depth is pass n's
static bool ranges_true(const Sim& s, int split, int n)
{
    for (int r = 0; r < 2; r++) {
        if (!in_split(split, r)) continue;
        bool any = false, all_n = true;
        for (int p = 0; p < 2; p++) { const int d = s.real.px[r][p][P_DEPTH]; if (d != V_CLEAR) { any = true; all_n = all_n && d == V_PASS + n; } }
        if (any ? !(s.ranges[r] == n && all_n) : s.ranges[r] != R_NONE) return false;
    }
    return true;
}

// The claims, after every event:
//   1  a current region byte kRegionClear: every plane of both its pixels holds the clear value; kRegionSpec: both hold the constant
//   2  region_fill == kRegionClear says the same of every region
//   3  emissive_zero: the emissive plane is zero in all four pixels               (1-3: unless escaped - finding F1 in main())
//   4  no clear pending: REAL memory is the SHADOW, bit for bit (so every skipped store was a no-op); a clear pending: the host
//      answers (census, known zero) as the shadow stands.  Readers are compared where they read (read_lit, download, describe).
//   5  ranges VALID for (r, w): a pass for that split left them, no depth write since, the entries are that pass's; CLEAN: all "none"
//   6  a refused render leaves the state as it was and the shadow untouched (step(): what is recorded is what happened)
//   7  once escaped: no hint, no skip, no ranges, ever again, and memory is the shadow at every moment
static void check_claims(Sim& s)
{
    const GbufferState& st = s.lib.st;
    if (!st.escaped) {
        if (st.region_allocated && st.region_fill < 0)
            for (int r = 0; r < 2; r++) {
                if (s.region[r] == (int)kRegionClear && !region_clear(s.real, r)) fail("(b) claim 1: a region byte says clear, the memory does not");
                if (s.region[r] == (int)kRegionSpec && (s.real.px[r][0][P_SPEC] != V_SPEC || s.real.px[r][1][P_SPEC] != V_SPEC)) fail("(b) claim 1: a region byte says constant, the memory does not");
                if (s.region[r] == B_POISON) fail("(b) claim 1: the region array counts as current and was never filled");
            }
        if (st.region_fill == (int)kRegionClear && !(region_clear(s.real, 0) && region_clear(s.real, 1))) fail("(b) claim 2: region_fill says clear, the memory does not");
        if (st.emissive_zero) for (int r = 0; r < 2; r++) for (int p = 0; p < 2; p++) if (s.real.px[r][p][P_EMI] != V_CLEAR) { fail("(b) claim 3: emissive_zero over a plane that is not"); r = 2; break; }
    }
    if (!st.clear_pending && !same(s.real, s.shadow)) fail("(b) claim 4: memory differs from the shadow with no clear pending");
    {
        const int census = gbs_census(st, s.tracking);
        const bool all_clear = region_clear(s.shadow, 0) && region_clear(s.shadow, 1);
        if (census == (int)kRegionClear && !all_clear) fail("(b) claim 4: the census says clear, the shadow does not");
        if (gbs_plane_known_zero(st, s.tracking, 4))
            for (int r = 0; r < 2; r++) for (int p = 0; p < 2; p++) if (s.shadow.px[r][p][P_EMI] != V_CLEAR) { fail("(b) claim 4: known zero over a plane that is not"); r = 2; break; }
        if (census != s.fixed.census(s.tracking) || gbs_plane_known_zero(st, s.tracking, 4) != s.fixed.known_zero(s.tracking)) fail("(a) census / known zero differ from the transcription");
    }
    if (st.ranges_state == RANGES_VALID) {
        if (!st.ranges_allocated || s.valid_pass < 0 || !ranges_true(s, st.ranges_world == 1 ? 0 : 1 + st.ranges_rank, s.valid_pass)) fail("(b) claim 5: ranges VALID and not the depth plane's");
    }
    if (st.ranges_state == RANGES_CLEAN && (s.ranges[0] != R_NONE || s.ranges[1] != R_NONE)) fail("(b) claim 5: ranges CLEAN with an entry that is not none");
    if (st.ranges_state != RANGES_NONE && !st.ranges_allocated) fail("(b) claim 5: a ranges state without the array");
    if (s.escaped_for_real && !(st.escaped && same(s.real, s.shadow))) fail("(b) claim 7: escaped, and the library skipped or forgot");
}

static void step(Sim& s, const Ev& e)
{
    events_run++;
    if (e.kind == K_POINTER_WRITE) {               // the caller writes through the pointers vr_gbuffer_describe gave it: nobody is told
        if (s.escaped_for_real) for (int r = 0; r < 2; r++) for (int p = 0; p < 2; p++) s.real.px[r][p][e.arg] = s.shadow.px[r][p][e.arg] = V_FOREIGN;
        check_claims(s);
        return;
    }
    if (e.kind == K_TRACKING) { s.tracking = e.arg != 0; check_claims(s); return; }
    Out on, of, op;
    const GbufferState before = s.lib.st;
    s.lib.event(e, s.tracking, on);
    s.fixed.event(e, s.tracking, of);
    s.pure.event(e, s.tracking, op);
    if (g_break == BRK_NONE) {
        if (!same(on, of) || !s.fixed.same_state(s.lib.st)) fail("(a) the header and the transcription (intended differences on) disagree");
        if (on.rc || op.rc) s.pure_comparable = false;
        if (s.pure_comparable && (!same(on, op) || !s.pure.same_state(s.lib.st))) fail("(a) the header and the transcription as it was disagree before any refusal");
    }
    // the host asked: the shadow learns it at once
    if (e.kind == K_CLEAR) clear_mem(s.shadow);
    // what was queued, in order
    bool reset_queued = false;
    for (int i = 0; i < on.nops && i < 8; i++) {
        if (on.ops[i] == OP_CLEAR) clear_mem(s.real);
        else if (on.ops[i] == OP_RANGES_RESET) { s.ranges[0] = s.ranges[1] = R_NONE; reset_queued = true; }
        else s.region[0] = s.region[1] = on.ops[i] - OP_REGION_FILL;
    }
    if (s.lib.st.escaped && (on.region || on.emissive_zero || on.use_ranges)) fail("(b) claim 7: a hint from an escaped G-buffer");
    switch (e.kind) {
    case K_RENDER:
        if (s.lib.st.escaped && (on.plan.noemi || on.plan.ranges || on.plan.track_regions || on.region)) fail("(b) claim 7: a skip on an escaped G-buffer");
        if (on.rc) {
            // claim 6.  What may differ from the state behind the clear's settlement: an array allocated, the ranges reset.
            GbufferState want = before;
            if (on.plan.materialise_first && before.clear_pending) want = gbs_clear_written(gbs_touched(before));
            GbufferState got = s.lib.st;
            if (got.ranges_allocated && !want.ranges_allocated) want = gbs_ranges_allocated(want);
            if (got.region_allocated && !want.region_allocated) want = gbs_region_allocated(want);
            if (reset_queued) want = gbs_ranges_reset(want);
            if (!same(got, want)) fail("(b) claim 6: a refused render changed the state");
            break;
        }
        if (!on.plan.assume_cleared)               // the pass reads the depth it draws over
            for (int r = 0; r < 2; r++) for (int p = 0; p < 2; p++) if (in_split(e.split, r) && s.real.px[r][p][P_DEPTH] != s.shadow.px[r][p][P_DEPTH]) { fail("(b) the tile pass drew over a depth plane that is not the shadow's"); r = 2; break; }
        pass_shadow(s, e, on, s.serial);
        pass_real(s, e, on, s.serial);
        if (on.plan.ranges) s.valid_pass = s.serial;
        s.serial++;
        // the lighting pass behind a lit request the tile pass did not fuse (vr_terrain_render_lit, vr_frame_submit)
        if (e.request != RASTER_REQ_NONE && !on.plan.fuse) {
            Out ol, olf, olp;
            Ev l; l.kind = K_LIGHT_STREAM;
            s.lib.event(l, s.tracking, ol); s.fixed.event(l, s.tracking, olf); s.pure.event(l, s.tracking, olp);
            for (int i = 0; i < ol.nops && i < 8; i++) { if (ol.ops[i] == OP_CLEAR) clear_mem(s.real); else if (ol.ops[i] >= OP_REGION_FILL) s.region[0] = s.region[1] = ol.ops[i] - OP_REGION_FILL; }
            read_lit(s, ol, e.split);
        }
        break;
    case K_LIGHT_STREAM: read_lit(s, on, 0); break;
    case K_LIGHT_TILED:
        read_lit(s, on, e.arg);
        if (on.use_ranges) {
            if (s.valid_pass < 0 || !ranges_true(s, e.arg, s.valid_pass)) fail("(b) claim 5: the culling stage took ranges that are not the depth plane's");
            for (int r = 0; r < 2; r++) if (in_split(e.arg, r)) s.ranges[r] = R_NONE;        // k_light_cull<true> resets what it reads
        }
        break;
    case K_UPLOAD: for (int r = 0; r < 2; r++) for (int p = 0; p < 2; p++) s.real.px[r][p][e.arg] = s.shadow.px[r][p][e.arg] = V_FOREIGN; break;
    case K_DOWNLOAD: if (!same(s.real, s.shadow)) fail("(b) a download saw something else than the shadow"); break;
    case K_DESCRIBE: s.escaped_for_real = true; if (!same(s.real, s.shadow)) fail("(b) describe handed out memory that is not the shadow"); break;
    default: break;
    }
    check_claims(s);
}

// ---- the sequences -----------------------------------------------------------------------------------------------------------------
static std::vector<Ev> g_all, g_small;          // every event / a few of each kind, for the longer exhaustive runs
static void make_events()
{
    auto add_render = [](std::vector<Ev>& to, int shape, int tile, int req, bool ac, bool dr, int split, int c0, int c1, int refuse) {
        Ev e; e.kind = K_RENDER; e.shape = shape; e.tile_shift = tile; e.request = req; e.assume_cleared = ac; e.depth_ranges = dr; e.split = split; e.cov[0] = c0; e.cov[1] = c1; e.refuse = refuse;
        to.push_back(e);
    };
    for (int req = RASTER_REQ_NONE; req <= RASTER_REQ_KEEP; req++)
        for (int shape = 0; shape < N_SHAPES; shape++) for (int tile = 5; tile <= 6; tile++) for (int ac = 0; ac < 2; ac++) for (int dr = 0; dr < 2; dr++) for (int split = 0; split < 3; split++) {
            // vr_terrain_render_lit refuses anything but a shaded pass over a cleared target without ranges; vr_frame_submit has no partition
            if (req != RASTER_REQ_NONE && shape > S_NOT_ELIGIBLE) continue;
            if (req == RASTER_REQ_LIT && (!ac || dr)) continue;
            if (req == RASTER_REQ_KEEP && split) continue;
            for (int c = 0; c < 9; c++) add_render(g_all, shape, tile, req, ac, dr, split, c / 3, c % 3, F_NO);
            for (int f = F_BEFORE_APPLY; f < N_REFUSE; f++) add_render(g_all, shape, tile, req, ac, dr, split, 1, 1, f);       // (a refused pass covers nothing)
        }
    for (int ac = 0; ac < 2; ac++) for (int dr = 0; dr < 2; dr++) for (int split = 0; split < 2; split++) for (int c = 0; c < 2; c++) {
        add_render(g_small, S_FAST, 5, RASTER_REQ_NONE, ac, dr, split, c ? 2 : 0, c ? 2 : 1, F_NO);
        add_render(g_small, S_DEPTH, 5, RASTER_REQ_NONE, ac, dr, split, c ? 2 : 0, c ? 2 : 1, F_NO);
    }
    add_render(g_small, S_FAST, 5, RASTER_REQ_KEEP, true, false, 0, 0, 1, F_NO);
    add_render(g_small, S_FAST, 5, RASTER_REQ_KEEP, true, false, 0, 2, 2, F_NO);
    add_render(g_small, S_FAST, 5, RASTER_REQ_LIT, true, false, 0, 0, 1, F_NO);
    for (int f = F_BEFORE_APPLY; f < N_REFUSE; f++) add_render(g_small, S_FAST, 5, RASTER_REQ_NONE, true, true, 0, 1, 1, f);
    auto add = [](int kind, int arg) { Ev e; e.kind = kind; e.arg = arg; g_all.push_back(e); g_small.push_back(e); };
    add(K_CLEAR, 0); add(K_LIGHT_STREAM, 0);
    for (int split = 0; split < 3; split++) add(K_LIGHT_TILED, split);
    for (int p = 0; p < N_PLANES; p++) add(K_UPLOAD, p);
    add(K_DOWNLOAD, 0); add(K_DESCRIBE, 0);
    add(K_POINTER_WRITE, P_DEPTH); add(K_POINTER_WRITE, P_SPEC); add(K_POINTER_WRITE, P_EMI);
    add(K_TRACKING, 0); add(K_TRACKING, 1);
}
// a G-buffer as vr_gbuffer_create leaves it: the allocation holds anything, the clear at creation is a real one
static Sim fresh()
{
    Sim s;
    s.fixed.fix_clear = s.fixed.fix_apply = true;
    for (int r = 0; r < 2; r++) for (int p = 0; p < 2; p++) for (int k = 0; k < N_PLANES; k++) s.real.px[r][p][k] = s.shadow.px[r][p][k] = V_FOREIGN;
    Ev c; c.kind = K_CLEAR;
    g_len = 0;
    step(s, c);
    return s;
}
static void enumerate(const Sim& s, const std::vector<Ev>& events, int depth)
{
    for (const Ev& e : events) {
        Sim t = s;
        g_seq[g_len++] = &e;
        step(t, e);
        sequences++;
        if (depth > 1) enumerate(t, events, depth - 1);
        g_len--;
    }
}
static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return (uint32_t)(g_rng >> 32); }
static void run_all(int all_depth, int small_depth, long random_sequences)
{
    const Sim s0 = fresh();
    enumerate(s0, g_all, all_depth);
    enumerate(s0, g_small, small_depth);
    // the longer ones: mostly the small set (states are reached through clears, uploads and lighting passes), one event in three of all
    g_rng = 0x9e3779b97f4a7c15ull;
    for (long i = 0; i < random_sequences; i++) {
        Sim s = s0;
        g_len = 0;
        for (int k = 0; k < 12; k++) {
            const Ev& e = rnd() % 3 == 0 ? g_all[rnd() % g_all.size()] : g_small[rnd() % g_small.size()];
            g_seq[g_len++] = &e;
            step(s, e);
        }
        sequences++;
    }
    g_len = 0;
}

int main(int argc, char** argv)
{
    make_events();
    if (argc > 1 && !strcmp(argv[1], "--break-each")) {
        int reported = 0;
        g_quiet = true;
        for (int b = 1; b < N_BREAKS; b++) {
            g_break = b; failures = 0; sequences = 0;
            run_all(1, 3, 20000);
            printf("  %-62s %s (%ld claims failed)\n", kBreakNames[b], failures ? "reported" : "NOT REPORTED", failures);
            reported += failures ? 1 : 0;
        }
        printf("%d of %d weakenings reported\n", reported, N_BREAKS - 1);
        return reported == N_BREAKS - 1 ? 0 : 1;
    }
    run_all(2, 4, 200000);
    // Findings: claims of the issue's wording that intended behaviour falsifies.  Kept as behaviour, narrowed as claims.
    //   F1  "region_fill == kRegionClear / emissive_zero mean what they say" holds only while the pointers have not escaped.  Shortest
    //       sequence: describe; clear; pointer_write(4).  gbuffer_clear_step sets both on an escaped G-buffer (its clears are eager and
    //       the fields are true for the moment); the caller's next store through the pointers falsifies them.  Nothing reads them
    //       then: every consumer asks tracking_live first (claim 7 holds).  Claims 1-3 are checked unless escaped.
    //   F2  "a refused call changes nothing": a render refused at the region array's memset, behind a reset of the ranges already queued,
    //       leaves the ranges CLEAN where they were DIRTY / NONE / VALID.  Shortest: render(... dr1 ... REFUSED region memset).  The reset
    //       has happened; any other record would be false.  An array allocated on the way is recorded likewise.
    //   F3  a lazy clear touches the ranges twice, when it is asked for and when it is written (gbs_clear_requested, gbs_materialise);
    //       either alone would do - every consumer of ranges materialises first - so --break-each drops both at once.
    printf("%zu + %zu events, %ld sequences, %ld events run, %ld failures\n", g_all.size(), g_small.size(), sequences, events_run, failures);
    return failures ? 1 : 0;
}
