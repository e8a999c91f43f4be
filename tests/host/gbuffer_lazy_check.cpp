// VR_OPT_GBUFFER_LAZY without a device: the state and policy code of vr_gbuffer_state.h / vr_raster_plan.h, driven as the host
// drives it (terrain_render_impl, vr_gbuffer_materialise, vr_derive_level0_write: the call order is transcribed below), over
// random sequences of frames, readers, partial writers, clears, uploads, edits, resizes, option flips and failed
// materialisations on two targets and two terrains (a frame draws either terrain into either target).  The model is the same world with the option off: it keeps whole
// eager copies - every fused frame writes its planes at once.  Memory is a set of content words: a pass that writes every pixel
// leaves a word made of (frame, terrain version at the time the pass RUNS), a partial writer one made of what was there as well.
//   - at every reader the lazy world has nothing pending any more and shows the model's colour planes, depth, emissive plane,
//     region census and plane knowledge;
//   - a target that needed a materialisation once never takes a lazy frame again;
//   - a terrain holds a target exactly while that target's record names the terrain (a destroyed target is held by nobody);
//   - a call that is refused (its materialisation fails) leaves the whole world as it was, the model does not run it either.
// gbuffer_lazy_check [seeds [ops]]; gbuffer_lazy_check break N: the same with one rule of the host's broken - failures expected.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <initializer_list>

#include "vr_raster_plan.h"

enum { BRK_NONE = 0, BRK_EDIT_NO_MATERIALISE, BRK_STICKY_FORGOTTEN, BRK_CENSUS_NO_MATERIALISE, BRK_PARTIAL_WRITER_REPLACES, BRK_UPLOAD_NO_MATERIALISE, BRK_OLD_LINK_KEPT, N_BREAKS };
static const char* const kBreakNames[N_BREAKS] = { "none", "an edit leaves the recorded frame pending", "lazy_off is forgotten",
    "the census does not materialise", "a partial writer replaces the record", "an upload does not materialise",
    "a lazy frame over another terrain's record leaves that terrain holding the target" };
static int g_break = BRK_NONE;

static uint64_t mix(uint64_t a, uint64_t b) { uint64_t x = (a ^ (b + 0x9e3779b97f4a7c15ull + (a << 6) + (a >> 2))) * 0xff51afd7ed558ccdull; return x ^ (x >> 33); }
static uint64_t word(uint64_t tag, uint64_t a, uint64_t b) { return mix(mix(tag, a), b); }
constexpr uint64_t kClearWord = 0x1111, kDepthClear = 0x2222, kZero = 0;

struct Rng { uint64_t s; uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); } uint32_t below(uint32_t n) { return next() % n; } };

struct Target {
    GbufferState st;
    bool rec = false; int rec_frame = 0, rec_terrain = 0;                 // vr_gbuffer::pending
    uint64_t colour = 0xdead, depth = 0xdead, emissive = 0xdead, region = 0xdead;     // device memory (an allocation holds anything)
    bool ever_materialised = false;                                        // the checker's own note, for the sticky rule
};
struct World {
    Target tg[2];
    int terrain[2] = { 0, 0 };       // version of each terrain's maps
    int pending_target[2] = { -1, -1 };      // vr_terrain::pending_target
    bool opt_lazy = true, opt_track = true, opt_fusion = true;
    bool eager = false;              // the model: the option is off whatever is asked
    bool fail_next = false;          // the next materialisation of planes is refused
    // counts
    long lazy_frames = 0, materialised = 0, replaced = 0, refused = 0;
};
static bool same(const GbufferState& a, const GbufferState& b, bool with_lazy)
{
    return a.clear_pending == b.clear_pending && a.cleared_once == b.cleared_once && a.escaped == b.escaped && a.emissive_zero == b.emissive_zero
        && (!with_lazy || a.region_fill == b.region_fill) && a.ranges_state == b.ranges_state && a.ranges_rank == b.ranges_rank && a.ranges_world == b.ranges_world
        && (!with_lazy || (a.region_allocated == b.region_allocated && a.ranges_allocated == b.ranges_allocated)) && (!with_lazy || (a.planes_pending == b.planes_pending && a.lazy_off == b.lazy_off));
}
static bool same(const Target& a, const Target& b)
{ return same(a.st, b.st, true) && a.rec == b.rec && (!a.rec || (a.rec_frame == b.rec_frame && a.rec_terrain == b.rec_terrain)) && a.colour == b.colour && a.depth == b.depth
      && a.emissive == b.emissive && a.region == b.region; }
static bool same(const World& a, const World& b)
{ return same(a.tg[0], b.tg[0]) && same(a.tg[1], b.tg[1]) && a.terrain[0] == b.terrain[0] && a.terrain[1] == b.terrain[1] && a.pending_target[0] == b.pending_target[0] && a.pending_target[1] == b.pending_target[1] && a.opt_lazy == b.opt_lazy && a.opt_track == b.opt_track && a.opt_fusion == b.opt_fusion; }

static long g_cases = 0, g_failures = 0;
static void fail(const char* what, long seq, int op) { if (g_failures++ < 10) printf("FAIL (sequence %ld, op %d): %s\n", seq, op, what); }

// ---- the host, transcribed -----------------------------------------------------------------------------------------------------------
static void record_unlink(World& w, int ti)        // vr_gbuffer_record_unlink
{
    Target& t = w.tg[ti];
    if (!t.rec) return;
    if (w.pending_target[t.rec_terrain] == ti) w.pending_target[t.rec_terrain] = -1;
    t.rec = false;
}
static void record_settle(World& w, int ti) { if (!w.tg[ti].st.planes_pending) record_unlink(w, ti); }       // vr_gbuffer_record_settle
static void clear_step(World& w, int ti, const GbufferStep& step)      // gbuffer_clear_step
{
    Target& t = w.tg[ti];
    t.st = step.after;
    record_settle(w, ti);
    if (!step.work.clear_now) return;
    t.colour = kClearWord; t.depth = kDepthClear; t.emissive = kZero;
    t.st = gbs_clear_written(t.st);
}
static void run_step(Target& t, const GbufferStep& step)               // gbuffer_run_step (nothing refuses here)
{
    if (step.work.alloc_ranges) t.st = gbs_ranges_allocated(t.st);
    if (step.work.alloc_region) t.st = gbs_region_allocated(t.st);
    if (step.work.reset_ranges) t.st = gbs_ranges_reset(t.st);
    if (step.work.region_byte >= 0) t.region = word(0x5e, (uint64_t)step.work.region_byte, 0);
    t.st = step.after;
}

struct Pass { RasterRequest request; bool assume_cleared, depth_only, wireframe; int world; bool lock_view; int terrain; };
static int materialise_planes(World& w, int ti);
// terrain_render_impl.  `frame`: what the pass draws; the terrain version is the one of NOW.
static int run_pass(World& w, int ti, const Pass& d, int frame, bool materialising, RasterPlan* plan_out = nullptr)
{
    Target& t = w.tg[ti];
    auto inputs = [&]() {
        RasterPlanIn in{};
        in.wireframe = d.wireframe; in.depth_only = d.depth_only; in.assume_cleared = d.assume_cleared; in.depth_ranges = false;
        in.world = d.world; in.tile_shift = 5; in.tex_same = true; in.ws_pow2 = true; in.one_rsrc = true;
        in.plane_tracking = w.opt_track || materialising; in.clear_pending = t.st.clear_pending; in.emissive_zero = t.st.emissive_zero; in.escaped = t.st.escaped;
        in.viewport_full = true; in.width_mult4 = true; in.request = d.request; in.lit_inputs_ok = true; in.lit_plain = true; in.hdr_fits = true;
        in.lazy_ok = d.request == RASTER_REQ_KEEP && !w.eager && gbs_lazy_allowed(t.st, w.opt_track, w.opt_lazy, d.lock_view);
        return in;
    };
    RasterPlanIn in = inputs();
    RasterPlan plan = raster_plan(in);
    if (t.st.planes_pending && !materialising) {
        bool replaces = gbs_pass_replaces_pending(plan, d.world <= 1, !d.depth_only && !d.wireframe, in.viewport_full);
        if (g_break == BRK_PARTIAL_WRITER_REPLACES) replaces = true;
        if (!replaces) {
            if (int rc = materialise_planes(w, ti)) return rc;
            in = inputs(); plan = raster_plan(in);
        } else w.replaced++;
    }
    const int held = w.pending_target[d.terrain];
    if (plan.lazy && held >= 0 && held != ti) if (int rc = materialise_planes(w, held)) return rc;
    if (plan.lazy && t.ever_materialised) return -2;                     // (the checker: sticky-off)
    if (plan.materialise_first) clear_step(w, ti, gbs_materialise(t.st));
    const GbufferStep step = gbs_pass_prepare(t.st, plan, 0, d.world);
    run_step(t, step);
    record_settle(w, ti);
    // the kernel
    const uint64_t T = (uint64_t)w.terrain[d.terrain] * 2u + (uint64_t)d.terrain, F = (uint64_t)frame;
    const bool over_cleared = plan.assume_cleared && d.world <= 1;
    if (plan.lazy || (plan.fuse && !plan.keep)) t.depth = word(0xd, F, T);                     // depth + HdrColor of every pixel
    else {
        t.depth = over_cleared ? word(0xd, F, T) : mix(t.depth, word(0xd, F, T));
        if (!d.depth_only) {
            t.colour = over_cleared ? word(d.wireframe ? 0xcc : 0xc, F, T) : mix(t.colour, word(0xc, F, T));     // (uncovered pixels get the clear values)
            if (!plan.noemi) t.emissive = over_cleared ? kZero : mix(t.emissive, 1);
            if (plan.track_regions) t.region = over_cleared ? word(0xe, F, T) : mix(t.region, word(0xe, F, T));
        }
    }
    if (plan.lazy) {
        if (g_break != BRK_OLD_LINK_KEPT) record_unlink(w, ti);          // (a replaced record may name the other terrain)
        t.rec = true; t.rec_frame = frame; t.rec_terrain = d.terrain;
        w.pending_target[d.terrain] = ti; w.lazy_frames++;
    }
    if (plan_out) *plan_out = plan;
    return 0;
}
static int materialise_planes(World& w, int ti)      // vr_gbuffer_materialise_planes
{
    Target& t = w.tg[ti];
    if (!t.st.planes_pending) return 0;
    if (w.fail_next) { w.fail_next = false; w.refused++; return 1; }
    const Pass replay = { RASTER_REQ_NONE, true, false, false, 1, false, t.rec_terrain };
    if (int rc = run_pass(w, ti, replay, t.rec_frame, true)) return rc;
    t.st = gbs_planes_materialised(t.st);
    if (g_break == BRK_STICKY_FORGOTTEN) t.st.lazy_off = false;
    record_settle(w, ti);
    t.ever_materialised = true; w.materialised++;
    return 0;
}
static int materialise(World& w, int ti)             // vr_gbuffer_materialise
{
    if (int rc = materialise_planes(w, ti)) return rc;
    clear_step(w, ti, gbs_materialise(w.tg[ti].st));
    return 0;
}

// what a reader sees
struct Seen { uint64_t colour, depth, emissive, census; bool known_zero; };
static Seen look(World& w, int ti)
{
    Target& t = w.tg[ti];
    const int all = gbs_census(t.st, w.opt_track);
    const bool cp = t.st.clear_pending;          // (nobody sees the planes in front of a pending clear: whoever looks has it written first)
    return { cp ? kClearWord : t.colour, cp ? kDepthClear : t.depth, cp ? kZero : t.emissive, all >= 0 ? (uint64_t)all : t.region, gbs_plane_known_zero(t.st, w.opt_track, 4) };
}

enum { OP_SUBMIT, OP_SUBMIT_CLEAR, OP_DOWNLOAD, OP_CENSUS, OP_LIGHT, OP_UPLOAD, OP_DESCRIBE, OP_RENDER_KEEP, OP_RENDER_PART, OP_RENDER_DEPTH, OP_RENDER_WIRE,
       OP_RENDER_LIT, OP_RENDER_WHOLE, OP_CLEAR, OP_EDIT, OP_RESIZE, OP_FLIP_LAZY, OP_FLIP_TRACK, OP_FLIP_FUSION, OP_FAIL_NEXT, OP_SUBMIT_LOCKED, N_OPS };
struct Op { int kind, target, arg; };

// one API call on one world; reader = the call shows the target to its caller
static int apply(World& w, const Op& o, int frame, bool* reader)
{
    Target& t = w.tg[o.target];
    const int terr = o.arg >= 3 ? 1 : 0;         // the terrain a frame draws / an edit changes
    *reader = false;
    switch (o.kind) {
    case OP_SUBMIT: case OP_SUBMIT_CLEAR: case OP_SUBMIT_LOCKED: {      // (OP_SUBMIT_CLEAR: the runner has called Clear in front)
        // vr_frame_submit: the KEEP request under VR_OPT_FRAME_FUSION, else the plain tile pass; the lighting pass behind an unfused one
        const Pass p = { w.opt_fusion ? RASTER_REQ_KEEP : RASTER_REQ_NONE, o.kind != OP_SUBMIT_CLEAR, false, false, 1, o.kind == OP_SUBMIT_LOCKED, terr };
        RasterPlan plan{};
        if (int rc = run_pass(w, o.target, p, frame, false, &plan)) return rc;
        if (!plan.keep) { if (int rc = materialise(w, o.target)) return rc; run_step(t, gbs_reader(t.st, w.opt_track)); }
        return 0; }
    case OP_DOWNLOAD: if (int rc = materialise(w, o.target)) return rc; *reader = true; return 0;
    case OP_CENSUS:
        if (g_break != BRK_CENSUS_NO_MATERIALISE) if (int rc = materialise_planes(w, o.target)) return rc;
        *reader = true; return 0;
    case OP_LIGHT: if (int rc = materialise(w, o.target)) return rc; run_step(t, gbs_reader(t.st, w.opt_track)); *reader = true; return 0;
    case OP_UPLOAD: {
        if (g_break != BRK_UPLOAD_NO_MATERIALISE) { if (int rc = materialise(w, o.target)) return rc; }
        else clear_step(w, o.target, gbs_materialise(t.st));
        const int plane = o.arg % 5;
        t.st = gbs_foreign_write(t.st, plane);
        const uint64_t v = word(0xf, (uint64_t)frame, (uint64_t)plane);
        if (plane == 0) t.depth = v; else if (plane == 4) t.emissive = v; else t.colour = mix(t.colour, v);
        *reader = true; return 0; }
    case OP_DESCRIBE: if (int rc = materialise(w, o.target)) return rc; t.st = gbs_escape(t.st); *reader = true; return 0;
    case OP_RENDER_KEEP: return run_pass(w, o.target, { RASTER_REQ_NONE, false, false, false, 1, false, terr }, frame, false);
    case OP_RENDER_PART: return run_pass(w, o.target, { RASTER_REQ_NONE, true, false, false, 2, false, terr }, frame, false);
    case OP_RENDER_DEPTH: return run_pass(w, o.target, { RASTER_REQ_NONE, true, true, false, 1, false, terr }, frame, false);
    case OP_RENDER_WIRE: return run_pass(w, o.target, { RASTER_REQ_NONE, true, false, true, 1, false, terr }, frame, false);
    case OP_RENDER_LIT: return run_pass(w, o.target, { RASTER_REQ_LIT, true, false, false, 1, false, terr }, frame, false);
    case OP_RENDER_WHOLE: return run_pass(w, o.target, { RASTER_REQ_NONE, true, false, false, 1, false, terr }, frame, false);
    case OP_CLEAR: clear_step(w, o.target, gbs_clear_requested(t.st, w.opt_track)); return 0;
    case OP_EDIT:        // vr_derive_level0_write (edit, brush, undo, redo, history swaps), vr_terrain_update_heights
        if (g_break != BRK_EDIT_NO_MATERIALISE && w.pending_target[terr] >= 0) if (int rc = materialise_planes(w, w.pending_target[terr])) return rc;
        w.terrain[terr]++;
        return 0;
    case OP_RESIZE: {    // vr_gbuffer_destroy + vr_gbuffer_create
        t.st = gbs_planes_abandoned(t.st);
        record_settle(w, o.target);
        t = Target();
        clear_step(w, o.target, gbs_clear_requested(t.st, w.opt_track));
        return 0; }
    case OP_FLIP_LAZY: w.opt_lazy = !w.opt_lazy; return 0;
    case OP_FLIP_TRACK: w.opt_track = !w.opt_track; return 0;
    case OP_FLIP_FUSION: w.opt_fusion = !w.opt_fusion; return 0;
    case OP_FAIL_NEXT: w.fail_next = true; return 0;
    }
    return 0;
}

static void run_sequence(long seq, Rng& rng, int n_ops, World& totals)
{
    World lazy, eager;
    eager.eager = true;
    for (World* w : { &lazy, &eager }) for (int i = 0; i < 2; i++) clear_step(*w, i, gbs_clear_requested(w->tg[i].st, w->opt_track));     // vr_gbuffer_create
    // weights: frames and readers dominate, as in a host's loop
    static const int kWeights[N_OPS] = { 30, 8, 6, 5, 4, 3, 1, 3, 2, 2, 1, 2, 3, 4, 6, 2, 2, 1, 1, 3, 1 };
    int total = 0; for (int x : kWeights) total += x;
    for (int i = 0; i < n_ops; i++) {
        int r = (int)rng.below((uint32_t)total), kind = 0;
        while (r >= kWeights[kind]) r -= kWeights[kind++];
        const Op o = { kind, (int)rng.below(4) == 0 ? 1 : 0, (int)rng.below(5) };
        const int frame = (int)(seq * 1000 + i);
        g_cases++;
        if (kind == OP_SUBMIT_CLEAR) for (World* w : { &lazy, &eager }) clear_step(*w, o.target, gbs_clear_requested(w->tg[o.target].st, w->opt_track));     // RenderTargets::Clear, its own call
        const World before = lazy;
        bool reader = false, reader_e = false;
        const bool armed = lazy.fail_next;
        const int rc = apply(lazy, o, frame, &reader);
        if (rc == -2) { fail("a target that was materialised once took a lazy frame again", seq, i); return; }
        if (rc) {
            if (!armed) fail("a call was refused though no failure was injected", seq, i);
            if (!same(lazy, before)) fail("a refused call changed the world", seq, i);
            continue;                                                       // the model does not run a refused call either
        }
        if (o.kind == OP_FAIL_NEXT) continue;                               // (the model never materialises)
        eager.fail_next = false;
        if (apply(eager, o, frame, &reader_e)) { fail("the model refused a call", seq, i); return; }
        if (eager.tg[0].st.planes_pending || eager.tg[1].st.planes_pending || eager.lazy_frames) { fail("the model went lazy", seq, i); return; }
        if (reader) {
            if (lazy.tg[o.target].st.planes_pending) fail("a reader returned with the planes still pending", seq, i);
            const Seen a = look(lazy, o.target), b = look(eager, o.target);
            if (a.colour != b.colour) fail("colour planes differ from the model's at a reader", seq, i);
            if (a.depth != b.depth) fail("depth differs from the model's at a reader", seq, i);
            if (a.emissive != b.emissive) fail("the emissive plane differs from the model's at a reader", seq, i);
            if (a.census != b.census) fail("the region census differs from the model's at a reader", seq, i);
            if (a.known_zero != b.known_zero) fail("plane_known_zero differs from the model's at a reader", seq, i);
            if (!same(lazy.tg[o.target].st, eager.tg[o.target].st, false)) fail("the state behind a reader differs from the model's", seq, i);
        }
        for (int k = 0; k < 2; k++) {
            const Target& t = lazy.tg[k];
            if (t.depth != eager.tg[k].depth) fail("depth differs from the model's (depth is never pending)", seq, i);
            if (t.st.planes_pending != t.rec) fail("planes_pending without a record, or a record without it", seq, i);
            if (t.st.planes_pending && lazy.pending_target[t.rec_terrain] != k) fail("a pending target its record's terrain does not hold", seq, i);
            if (t.st.planes_pending && t.ever_materialised) fail("a target that was materialised once is pending again", seq, i);
        }
        for (int k = 0; k < 2; k++) {
            const int held = lazy.pending_target[k];
            if (held >= 0 && !(lazy.tg[held].st.planes_pending && lazy.tg[held].rec && lazy.tg[held].rec_terrain == k))
                fail("a terrain holds a target whose record does not name it (or that has nothing pending)", seq, i);
        }
        if (g_failures > 50) return;
    }
    // the end of the sequence: both targets are looked at
    for (int k = 0; k < 2; k++) {
        lazy.fail_next = false;
        bool rd;
        const Op o = { OP_DOWNLOAD, k, 0 };
        if (apply(lazy, o, 0, &rd) || apply(eager, o, 0, &rd)) { fail("the final download was refused", seq, n_ops); continue; }
        const Seen a = look(lazy, k), b = look(eager, k);
        if (a.colour != b.colour || a.depth != b.depth || a.emissive != b.emissive || a.census != b.census || a.known_zero != b.known_zero)
            fail("the final download differs from the model's", seq, n_ops);
    }
    totals.lazy_frames += lazy.lazy_frames; totals.materialised += lazy.materialised; totals.replaced += lazy.replaced; totals.refused += lazy.refused;
}

int main(int argc, char** argv)
{
    long seqs = 40000; int ops = 24;
    if (argc >= 3 && !strcmp(argv[1], "break")) { g_break = atoi(argv[2]); if (g_break <= 0 || g_break >= N_BREAKS) return 2; seqs = 4000; }
    else { if (argc >= 2) seqs = atol(argv[1]); if (argc >= 3) ops = atoi(argv[2]); }
    World totals;
    Rng rng{ 20261020 };
    for (long s = 0; s < seqs && g_failures <= 50; s++) run_sequence(s, rng, ops, totals);
    if (g_break) printf("broken rule: %s\n", kBreakNames[g_break]);
    printf("lazy_frames %ld materialised %ld replaced %ld refused %ld\n", totals.lazy_frames, totals.materialised, totals.replaced, totals.refused);
    printf("%ld sequences, %ld cases, %ld failures\n", seqs, g_cases, g_failures);
    return g_break ? (g_failures ? 0 : 1) : (g_failures ? 1 : 0);
}
