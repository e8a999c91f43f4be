// Check of the cross-stream ordering protocol (vrenderer_amd/csrc/vr_order.h) over generated sequences of API calls:
//  (a) SPECIFICATION: a flat transcription of the ordering code as the .hip files held it before the header existed (commit
//      a8c67ef; the numbers in comments are that commit's lines of vr_raster.hip, vr_select.hip and vr_frame.hip), written as
//      that code wrote it.  It and the protocol drive the same recording `ops`; for every sequence the two traces of
//      (record | wait, stream, event) must be equal, operation for operation.  The intended differences are switches of the
//      transcription (struct Intended), each beside the parent's line it changes; the comparison is against the transcription
//      with all of them on, and exact.
//  (b) HAPPENS-BEFORE MODEL of HIP's stream semantics: one vector clock per stream; a record snapshots the stream's clock into the
//      event, a wait joins it, a dispatch-stamped event is a snapshot right behind its launch; a host-side synchronise joins the
//      stream's (event's) clock into everything queued later.  Every kernel that touches a set's selection, a set's vertices and
//      bins, the node heights, an HDR image, one of the two maps (level 0, chain and tables), the query pyramid, the journal's
//      arena, the brush buffers or the query staging registers a read or a write; a conflicting pair (write/write, read/write)
//      that the clocks do not order is a failure, and so is memory the host frees or rewrites (host_touch) while something it has
//      not waited for may still use it.  The protocol must pass; where the plain transcription does not, that is a finding
//      about the parent, and one of the intended differences must be what repairs it.
//      The editing path (edit, brush / erode, undo / redo, history_enable, queries, sweep_state) is transcribed from commit 605778b,
//      the last one with its three private event records; the numbers beside it are that commit's lines.  The pyramid's read-back
//      (vr_debug_terrain_query_pyramid) is younger than that commit: a reader of the pyramid, it is given the wait of the cast's walk.
//  (c) every sequence up to kExhaustive calls, then a fixed-seed random sample of longer ones.
//      The stamped launches take their events from the real supplier (vr_events.h) with a ring of FOUR events, two launches, so
//      slots are reissued inside the short sequences; a re-stamped event is what it is - a wait on it orders against the new
//      occupant only - and every re-stamp must come behind the event's previous occupant (the rule vr_events.h states for a wait
//      on a ring handle that is no longer live).
// What the model is not: the HIP runtime (it assumes the documented semantics of the two calls).
//   order_check                 the check; prints sequences and failures
//   order_check --drop-each     is the model alive?  The transcription (intended differences on) loses one wait site at a time;
//                               prints for each site in how many sequences (b) reports it, and for a site that no sequence
//                               reports the reason it orders nothing (dead_reason) - a site with neither fails the run
// Which set a call gets is not this program's: Host keeps a GeoSlots<int> (the key: a view's number) and the calls below go through
// the transitions of vr_geosets.h as the .hip files do; tests/host/geosets_check.cpp holds that header to the code it replaced.
// Plain C++17, no GPU: g++ -std=c++17 -Wall -Werror -I vrenderer_amd/csrc tests/host/order_check.cpp
#include "vr_geosets.h"
#include "vr_order.h"

#include <array>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

// ---- the world: trace, clocks, accesses -----------------------------------------------------------
enum Stream { S_NONE = 0, G0, G1, M0, M1, TM, N_STREAMS };       // two geometry streams, the context's (a host may switch), the tone mapper's
static const char* const kStreamName[N_STREAMS] = { "-", "geo0", "geo1", "main0", "main1", "tonemap" };
// (a map: its level 0, its mip chain and its tables; the brush buffers: dab lists, snapshot and the erosions' block)
enum Res { SEL0, SEL1, SEL2, GEO0, GEO1, GEO2, HEIGHTS, IMG0, IMG1, HMAP, AMAP, PYRAMID, JOURNAL, BRUSHBUF, STAGE, N_RES };
static const char* const kResName[N_RES] = { "selection 0", "selection 1", "selection 2", "verts+bins 0", "verts+bins 1", "verts+bins 2",
                                             "node heights", "image 0", "image 1", "heightmap", "albedo", "query pyramid", "journal arena",
                                             "brush buffers", "query staging" };
// own events (0 = none); stamped events follow
enum { EV_GEO_DONE = 1, EV_RASTER_DONE = 4, EV_SEL_READ = 7, EV_MAIN_DEP = 10, EV_SEL_COPY, EV_RASTER_BEGIN, EV_WRITTEN, EV_READ_DONE = 15, EV_PYRAMID = 17, EV_JOURNAL, EV_BRUSH, EV_FIRST_STAMPED,
       N_EVENTS = 128 };
typedef std::array<uint32_t, N_STREAMS> Clock;
static void join(Clock& a, const Clock& b) { for (int i = 0; i < N_STREAMS; i++) if (b[i] > a[i]) a[i] = b[i]; }

struct Op { uint8_t wait, stream; uint16_t event; };              // wait: 0 record, 1 wait, 2 the host's synchronise (no stream)
struct World {
    std::vector<Op> trace;
    Clock clk[N_STREAMS], host, ev[N_EVENTS];
    bool ev_recorded[N_EVENTS];
    int next_event;
    struct Acc { Clock c; int stream; };
    Acc last_write[N_RES]; bool has_write[N_RES];
    Acc reads[N_RES][128]; int n_reads[N_RES];
    int unordered;                   // conflicting pairs the clocks do not order (+ waits on an event never recorded)
    std::string first;
    int drop_site;                   // the transcription's wait site that is left out (0: none)

    void reset(int drop)
    {
        trace.clear();
        memset(clk, 0, sizeof(clk)); memset(&host, 0, sizeof(host)); memset(ev, 0, sizeof(ev)); memset(ev_recorded, 0, sizeof(ev_recorded));
        memset(has_write, 0, sizeof(has_write)); memset(n_reads, 0, sizeof(n_reads));
        next_event = EV_FIRST_STAMPED; unordered = 0; first.clear(); drop_site = drop;
    }
    void op_on(int s) { join(clk[s], host); }                    // whatever the host waited for is before anything it queues later
    int record(int e, int s) { op_on(s); ev[e] = clk[s]; ev_recorded[e] = true; trace.push_back({ 0, (uint8_t)s, (uint16_t)e }); return 0; }
    int wait(int s, int e)
    {
        op_on(s);
        if (!ev_recorded[e]) fail("a wait on an event that was never recorded");
        join(clk[s], ev[e]);
        trace.push_back({ 1, (uint8_t)s, (uint16_t)e });
        return 0;
    }
    void kernel(int s) { op_on(s); clk[s][s]++; }
    static bool behind(const Clock& a, const Clock& b) { for (int i = 0; i < N_STREAMS; i++) if (a[i] > b[i]) return false; return true; }
    void stamp(int e, int s)                                     // by the dispatch: right behind the kernel just queued
    {
        if (ev_recorded[e] && !behind(ev[e], clk[s])) fail("an event re-stamped for a launch that is not ordered behind its previous occupant");
        ev[e] = clk[s]; ev_recorded[e] = true;
    }
    void sync_stream(int s) { join(host, clk[s]); }
    void sync_event(int e) { join(host, ev[e]); }
    int sync(int e) { sync_event(e); trace.push_back({ 2, 0, (uint16_t)e }); return 0; }                  // a side resource's order_side_idle
    void host_touch(int r)                                       // the host frees the resource's memory, or writes pinned memory that queued work reads
    {
        auto check = [&](const Acc& a, const char* kind) {
            if (a.c[a.stream] > host[a.stream]) fail(std::string(kResName[r]) + ": " + kind + " on " + kStreamName[a.stream] + " not waited for by the host");
        };
        if (has_write[r]) check(last_write[r], "write");
        for (int i = 0; i < n_reads[r]; i++) check(reads[r][i], "read");
        n_reads[r] = 0; has_write[r] = false;
    }
    void host_orders(int later, int earlier) { join(clk[later], clk[earlier]); }      // what a host owes when it moves work to another stream
    void fail(const std::string& what) { if (!unordered++) first = what; }
    void access(int r, bool write, int s)                        // by the kernel just queued on s
    {
        const Clock& now = clk[s];
        auto check = [&](const Acc& a, const char* kind) {
            if (a.c[a.stream] > now[a.stream])
                fail(std::string(kResName[r]) + ": " + kind + " on " + kStreamName[a.stream] + " not ordered before " + (write ? "write" : "read") + " on " + kStreamName[s]);
        };
        if (has_write[r]) check(last_write[r], "write");
        if (write) {
            for (int i = 0; i < n_reads[r]; i++) check(reads[r][i], "read");
            n_reads[r] = 0; has_write[r] = true; last_write[r] = { now, s };
        } else if (n_reads[r] < 128) reads[r][n_reads[r]++] = { now, s };
        else fail("too many reads between two writes for the model");
    }
};
struct Ops { World* w; int record(int e, int s) const { return w->record(e, s); } int wait(int s, int e) const { return w->wait(s, e); }
             int sync(int e) const { return w->sync(e); } };

// ---- what the .hip files decide (the same for both protocols): the context and the terrain's slot policy (vr_geosets.h) ------
struct Host {
    int main = M0;
    bool async_geometry = true, frame_fusion = true;
    // the real supplier, small: a ring of two launches, no events made ahead (timing level 0 or 2: only the stamped launches are
    // timed; level 1 synchronises more)
    EventSupply<int> events;
    struct EvOps { World* w; const Host* h;
        bool create(int* e) const { if (h->fail_create || w->next_event >= N_EVENTS) return false; *e = w->next_event++; return true; }
        void destroy(int) const {}
        void record(int e, int s) const { w->record(e, s); }
        int sync_stream(int s) const { w->sync_stream(s); return 0; }
        int sync_event(int e) const { w->sync_event(e); return 0; }
        int elapsed(float*, int, int) const { return 0; } };
    Host() { events.ring_size = 4; events.precreate[1] = events.precreate[2] = 0; }
    unsigned not_stamped = 0;         // bit k: the k-th stamped launch from now gets no events if it has to create one (the only way to get none)
    bool fail_create = false;
    bool launched = false;
    GeoSlots<int> slots;              // vr_terrain::slots
    int frame_no = 0;
    unsigned geo_turn = 0;
    // the editing path: the pyramid exists (d_pyramid), history is on, the steps that can be undone / redone (the map of each),
    // an erosion has left its planes (vr_terrain::erode_last)
    bool pyramid_built = false, history_on = false, sweep_left = false;
    std::vector<int> undo, redo;
    // VrKernelScope(by_dispatch) + launch on the context's stream: the kernel, and VrKernelScope::stop
    EventRef<int> stamped_launch(World& w)
    {
        const EvOps ops{ &w, this };
        fail_create = (not_stamped & 1u) != 0;
        not_stamped >>= 1; launched = true;
        EventPair<int, int> pair = events_take(events, ops, 0, main, true);
        fail_create = false;
        w.kernel(main);
        if (pair.stamps()) { w.stamp(pair.begin, main); w.stamp(pair.end, main); events_launched(events, pair, main); }
        const EventRef<int> stop = events_stop(events, pair);
        events_release(events, ops, pair);
        return stop;
    }
};
static const int kGeo[2] = { G0, G1 };

// ---- (a) the parent's ordering code ----------------------------------------------------------------
struct Intended {
    bool own_stop;          // vr_frame_submit waits for the lighting pass's OWN stop event, or records; never ctx->last_stop
    bool heights_behind;    // the node-height update runs behind every chain queued so far (found by (b): see main)
    bool common_order;      // vr_terrain_select queues its waits in launch_geometry's order (the permitted reorder)
    bool sweep_dead_wait;   // vr_debug_terrain_sweep_state does not wait for the erosion's event on the stream that recorded it (a dead wait)
    bool ring_handles;      // a mark that holds a RING event is not dropped when the timing epoch advances: its handle is live until the slot
                            // is reissued (vr_events.h) - a wait more, for a launch the recycler's synchronise has seen complete
};
enum Site { W_LG_CHAIN = 1, W_LG_SEL_READ, W_LG_RASTER, W_LG_MAIN_DEP, W_LG_SEL_COPY, W_PREP_HINT, W_PREP_NOW, W_TILE_CHAIN, W_KEEP_READER, W_AHEAD,
            W_SEL_MAIN_DEP, W_SEL_CHAIN, W_SEL_SEL_READ, W_SEL_RASTER, W_FRAME_READER, W_FRAME_WRITTEN, W_HEIGHTS_CHAIN,
            W_MAPS_CHAIN, W_MAPS_RASTER, W_PYR_CAST, W_PYR_WRITE, W_JOURNAL, S_JOURNAL_IDLE, S_BRUSH_IDLE, W_SWEEP, W_SWEEP_DEAD, N_SITES };
static const char* const kSiteName[N_SITES] = { "", "launch_geometry: previous chain", "launch_geometry: lock_view copy out of the set", "launch_geometry: tile pass",
    "launch_geometry: main dependency", "launch_geometry: lock_view source complete", "prepare: start hint", "prepare: context's stream waits now",
    "tile pass: chain", "fused tile pass: image's reader", "tile pass: deferred waits of sets prepared ahead", "select: main dependency", "select: previous chain",
    "select: lock_view copy out of the set", "select: tile pass", "frame: image's reader", "frame: tone-map stage behind the writer",
    "heights: chains queued so far (intended difference)",
    "level-0 write: chains queued so far", "level-0 write: tile passes", "cast_rays: pyramid's last writer", "level-0 write: pyramid's last user",
    "journal kernel: the journal's last kernel", "history_enable: host waits for the journal", "brush / erode: host waits for the previous one",
    "sweep_state: the erosion on another stream", "sweep_state: the erosion on this stream (dropped: intended difference)" };
// Sites that (b) is expected NOT to report, and why.  All but the first order work on the context's stream of before a set_stream
// against work on the stream of after it, which the host has ordered already ("what the host owes", SET_STREAM below).
static const char* dead_reason(int site)
{
    switch (site) {
    case W_PREP_HINT: return "a hint: it says when a prepared chain becomes runnable, it orders nothing";
    case W_MAPS_RASTER: case W_PYR_CAST: case W_PYR_WRITE: case W_JOURNAL: case W_SWEEP:
        return "both sides ran on the context's stream, and the host orders the new stream behind the old one at set_stream";
    case W_SWEEP_DEAD: return "a wait on the stream that recorded the event";
    default: return nullptr;
    }
}

struct Parent {
    World& w; Host& h; Intended in;
    struct Set { int ev_geo_done, ev_raster_done, raster_done = 0; uint64_t raster_done_epoch = 0; bool raster_recorded = false, geo_recorded = false, raster_ring = false;
                 int ev_sel_read; bool sel_read_pending = false, main_waited = false; int main_wait_stream = 0, stream = G0; bool main_dep_pending = false; } sets[3];
    int ev_sel_copy = EV_SEL_COPY, ev_main_dep = EV_MAIN_DEP, ev_raster_begin = EV_RASTER_BEGIN;
    bool raster_begin_recorded = false, start_hint_ring = false; int start_hint = 0; uint64_t start_hint_epoch = 0;
    struct Image { int ev_written, ev_read_done; bool read_pending = false; } img[2];
    Parent(World& w_, Host& h_, Intended in_) : w(w_), h(h_), in(in_)
    {
        for (int i = 0; i < 3; i++) { sets[i].ev_geo_done = EV_GEO_DONE + i; sets[i].ev_raster_done = EV_RASTER_DONE + i; sets[i].ev_sel_read = EV_SEL_READ + i; }
        for (int i = 0; i < 2; i++) { img[i].ev_written = EV_WRITTEN + i; img[i].ev_read_done = EV_READ_DONE + i; }
    }
    // the editing path's three private records (vr_internal.h of the parent: ev_pyramid / pyramid_stream with d_pyramid as the flag,
    // ev_history / history_stream / history_queued, ev_brush / brush_pending)
    int ev_pyramid = EV_PYRAMID, pyramid_stream = 0;
    int ev_history = EV_JOURNAL, history_stream = 0; bool history_queued = false;
    int ev_brush = 0; bool brush_pending = false;
    int brush_stream = 0;   // (no field of the parent: what Intended::sweep_dead_wait needs to tell the dead wait from the live one)
    void R(int e, int s) { w.record(e, s); }
    void W(int site, int s, int e) { if (site != w.drop_site) w.wait(s, e); }
    void S(int site, int e) { if (site != w.drop_site) w.sync(e); }
    int stream(int gi) const { return sets[gi].stream; }
    bool epoch_ok(uint64_t epoch, bool ring) const { return epoch == 0 || epoch == h.events.epoch || (in.ring_handles && ring); }

    void begin_chain(int gi)                                  // launch_geometry, vr_raster.hip
    {
        Set& g = sets[gi];
        /* 1787 */ g.stream = kGeo[h.geo_turn++ & 1u];
        /* 1788 */ g.main_waited = false;
        /* 1789 */ const int s = h.main, gs = g.stream;
        /* 1790 */ if (!h.async_geometry) {
        /* 1791 */     R(ev_main_dep, s);
        /* 1792 */     g.main_dep_pending = true;
                   }
        /* 1795 */ if (g.geo_recorded) W(W_LG_CHAIN, gs, g.ev_geo_done);
        /* 1796 */ if (g.sel_read_pending) { W(W_LG_SEL_READ, gs, g.ev_sel_read); g.sel_read_pending = false; }
        /* 1798 */ if (g.raster_recorded && epoch_ok(g.raster_done_epoch, g.raster_ring)) W(W_LG_RASTER, gs, g.raster_done);
        /* 1799 */ if (g.main_dep_pending) { W(W_LG_MAIN_DEP, gs, ev_main_dep); g.main_dep_pending = false; }
    }
    template <class Copy> void copy_selection(int gi, int from, Copy&& copy)
    {
        Set& g = sets[gi]; Set* selection_from = &sets[from]; const int gs = g.stream;
        /* 1806 */ R(ev_sel_copy, selection_from->stream);
        /* 1807 */ W(W_LG_SEL_COPY, gs, ev_sel_copy);
        /* 1808-1810 */ copy();
        /* 1812 */ R(selection_from->ev_sel_read, gs);
        /* 1813 */ selection_from->sel_read_pending = true;
    }
    void end_chain(int gi)
    {
        Set& g = sets[gi];
        /* 1852 */ R(g.ev_geo_done, g.stream);
        /* 1853 */ g.geo_recorded = true;
    }
    void prepare_start()                                      // vr_terrain_prepare
    {
        /* 1925 */ if (raster_begin_recorded && epoch_ok(start_hint_epoch, start_hint_ring))
        /* 1926 */     W(W_PREP_HINT, kGeo[h.geo_turn & 1u], start_hint);
    }
    void prepare_wait(int gi)
    {
        Set& g = sets[gi];
        /* 1936-1937 */ const bool other_prepared = geoslots_other_prepared(h.slots, gi);
        /* 1938 */ if (other_prepared) g.main_waited = false;
        /* 1939 */ else { W(W_PREP_NOW, h.main, g.ev_geo_done); g.main_waited = true; g.main_wait_stream = h.main; }
    }
    void tile_pass_begin(int gi, bool use_prepared)           // terrain_render_impl
    {
        Set& g = sets[gi]; const int s = h.main;
        /* 2040 */ if (!(use_prepared && g.main_waited && g.main_wait_stream == s)) W(W_TILE_CHAIN, s, g.ev_geo_done);
        /* 2041 */ g.main_waited = false;
        /* 2045 */ if (h.events.dispatch_events && h.events.last_stop.ev) { start_hint = h.events.last_stop.ev; start_hint_epoch = h.events.epoch; raster_begin_recorded = true; }
        /* 2046 */ else { R(ev_raster_begin, s); start_hint = ev_raster_begin; start_hint_epoch = 0; raster_begin_recorded = true; }
        start_hint_ring = start_hint_epoch && h.events.last_stop.slot != 0;
    }
    void keep_writer_begins(int im)
    {
        /* 2057 */ if (img[im].read_pending) { W(W_KEEP_READER, h.main, img[im].ev_read_done); img[im].read_pending = false; }
    }
    void tile_pass_launched(int gi, EventRef<int> stop)       // pass_stop: 2075
    {
        Set& g = sets[gi]; const int s = h.main, pass_stop = stop.ev;
        /* 2078 */ if (pass_stop) { g.raster_done = pass_stop; g.raster_done_epoch = h.events.epoch; g.raster_ring = stop.slot != 0; }
        /* 2079 */ else { R(g.ev_raster_done, s); g.raster_done = g.ev_raster_done; g.raster_done_epoch = 0; }
        /* 2080 */ g.raster_recorded = true;
        /* 2082 */ for (int pi = 0; pi < 3; pi++) { Set& p = sets[pi];
        /* 2083 */     if (pi != gi && h.slots.slot[pi].prepared && !(p.main_waited && p.main_wait_stream == s) && p.geo_recorded) { W(W_AHEAD, s, p.ev_geo_done); p.main_waited = true; p.main_wait_stream = s; } }
    }
    void select_begin(int gi)                                 // vr_terrain_select, vr_select.hip
    {
        Set& g = sets[gi];
        /* 750 */ g.stream = kGeo[h.geo_turn++ & 1u];
        if (!in.common_order)
        /* 751 */ if (g.main_dep_pending) { W(W_SEL_MAIN_DEP, g.stream, ev_main_dep); g.main_dep_pending = false; }
        /* 753 */ if (g.geo_recorded) W(W_SEL_CHAIN, g.stream, g.ev_geo_done);
        /* 754 */ if (g.sel_read_pending) { W(W_SEL_SEL_READ, g.stream, g.ev_sel_read); g.sel_read_pending = false; }
        /* 755 */ if (g.raster_recorded && epoch_ok(g.raster_done_epoch, g.raster_ring)) W(W_SEL_RASTER, g.stream, g.raster_done);
        if (in.common_order)                                  // the same waits; the main dependency last, as launch_geometry has it
        /* 751 */ if (g.main_dep_pending) { W(W_SEL_MAIN_DEP, g.stream, ev_main_dep); g.main_dep_pending = false; }
    }
    void select_end(int gi)
    {
        Set& g = sets[gi];
        /* 759 */ R(g.ev_geo_done, g.stream);
        /* 760 */ g.geo_recorded = true;
    }
    void heights_begin()                                      // vr_terrain_update_heights: the parent queued nothing in front of the kernels
    {
        if (in.heights_behind)
            for (Set& g : sets) if (g.geo_recorded) W(W_HEIGHTS_CHAIN, h.main, g.ev_geo_done);
    }
    void heights_end()
    {
        /* 456 */ R(ev_main_dep, h.main);
        /* 457 */ for (Set& g : sets) g.main_dep_pending = true;
    }
    void maps_begin()                                         // vr_derive_level0_write, vr_derive.hip (the header's two steps, flat)
    {
        /* 230 */ for (Set& g : sets) if (g.geo_recorded) W(W_MAPS_CHAIN, h.main, g.ev_geo_done);
        /* 231 */ for (Set& g : sets) if (g.raster_recorded && epoch_ok(g.raster_done_epoch, g.raster_ring)) W(W_MAPS_RASTER, h.main, g.raster_done);
    }
    void maps_end() { /* 260 */ heights_end(); }
    void pyramid_begin(bool write)
    {
        const int s = h.main;
        if (!write) { /* vr_query.hip 368 */ if (s != pyramid_stream) W(W_PYR_CAST, s, ev_pyramid); }
        else { /* vr_derive.hip 248 */ if (s != pyramid_stream) W(W_PYR_WRITE, s, ev_pyramid); }
    }
    void pyramid_end()
    {
        /* vr_query.hip 385 / vr_derive.hip 256 */ R(ev_pyramid, h.main);
        /* 390 / 257 */ pyramid_stream = h.main;
    }
    void journal_begin() { /* vr_history.hip 80 */ if (history_queued && h.main != history_stream) W(W_JOURNAL, h.main, ev_history); }
    void journal_end()
    {
        /* 91 */ R(ev_history, h.main);
        /* 92 */ history_stream = h.main; history_queued = true;
    }
    void journal_idle()                                       // history_idle
    {
        /* 106 */ if (history_queued) S(S_JOURNAL_IDLE, ev_history);
        /* 107 */ history_queued = false;
    }
    void brush_idle()                                         // vr_brush_consumed, vr_brush.hip
    {
        /* 129 */ ev_brush = EV_BRUSH;                        // (vr_brush_reserve, in front of it)
        /* 119 */ if (!brush_pending) return;
        /* 120 */ S(S_BRUSH_IDLE, ev_brush);
        /* 121 */ brush_pending = false;
    }
    void brush_end()                                          // vr_brush_call, vr_brush_dev.h
    {
        /* 92 */ R(ev_brush, h.main);
        /* 93 */ brush_pending = true;
        brush_stream = h.main;
    }
    void sweep_begin()                                        // vr_debug_terrain_sweep_state, vr_erode.hip
    {
        if (!in.sweep_dead_wait) {
        /* 287 */ if (ev_brush) W(brush_pending && brush_stream != h.main ? W_SWEEP : W_SWEEP_DEAD, h.main, ev_brush);
        } else if (brush_pending && brush_stream != h.main) W(W_SWEEP, h.main, ev_brush);
    }
    void light_writer_begins(int im)                          // vr_frame_submit, vr_frame.hip
    {
        /* 38 */ if (img[im].read_pending) { W(W_FRAME_READER, h.main, img[im].ev_read_done); img[im].read_pending = false; }
    }
    void image_written(int im, bool fused, EventRef<int> fused_stop, EventRef<int> light_stop, int reader)
    {
        Image* hdr = &img[im];
        /* 55 */ int done = fused ? fused_stop.ev : (h.events.dispatch_events && h.events.last_stop.ev) ? h.events.last_stop.ev : 0;
        if (in.own_stop && !fused) done = light_stop.ev;
        /* 56 */ if (!done) {
        /* 58 */     R(hdr->ev_written, h.main);
        /* 59 */     done = hdr->ev_written;
                 }
        /* 61 */ W(W_FRAME_WRITTEN, reader, done);
    }
    void reader_done(int im, int reader)
    {
        /* 71 */ R(img[im].ev_read_done, reader);
        /* 72 */ img[im].read_pending = true;
    }
};

// ---- the protocol as the .hip files call it now ------------------------------------------------------
struct Protocol {
    World& w; Host& h; Ops ops;
    OrderTerrain<int> t; OrderSet<int, int> sets[3]; OrderImage<int> img[2];
    OrderSide<int, int> pyramid, journal, brush;
    Protocol(World& w_, Host& h_) : w(w_), h(h_), ops{ &w_ }
    {
        pyramid.ev = EV_PYRAMID; journal.ev = EV_JOURNAL; brush.ev = EV_BRUSH;
        t.ev_changed = EV_MAIN_DEP; t.ev_sel_ready = EV_SEL_COPY; t.hint.own = EV_RASTER_BEGIN;
        for (int i = 0; i < 3; i++) { sets[i].stream = G0; sets[i].chain.own = EV_GEO_DONE + i; sets[i].tile_pass.own = EV_RASTER_DONE + i;
                                      sets[i].sel_read.ev = EV_SEL_READ + i; sets[i].main_dep.ev = t.ev_changed; }
        for (int i = 0; i < 2; i++) { img[i].written.own = EV_WRITTEN + i; img[i].read_done.ev = EV_READ_DONE + i; }
    }
    int stream(int gi) const { return sets[gi].stream; }
    void begin_chain(int gi) { order_begin_chain(t, sets[gi], ops, kGeo, h.geo_turn, h.main, !h.async_geometry, h.events); }
    template <class Copy> void copy_selection(int gi, int from, Copy&& copy) { order_copy_selection(t, sets[gi], sets[from], ops, [&]() -> int { copy(); return 0; }); }
    void end_chain(int gi) { order_end_chain(sets[gi], ops); }
    void prepare_start() { order_prepare_start(t, ops, kGeo, h.geo_turn, h.events); }
    void prepare_wait(int gi) { order_prepare_wait(sets[gi], ops, h.main, geoslots_other_prepared(h.slots, gi)); }
    void tile_pass_begin(int gi, bool use_prepared) { order_tile_pass_begin(t, sets[gi], ops, h.main, use_prepared, events_start_hint(h.events)); }
    void keep_writer_begins(int im) { order_image_writer_begins(img[im], ops, h.main); }
    void tile_pass_launched(int gi, EventRef<int> pass_stop)
    {
        order_tile_pass_launched(sets[gi], ops, h.main, pass_stop);
        for (int p = 0; p < 3; p++) if (p != gi && h.slots.slot[p].prepared) order_wait_ahead(sets[p], ops, h.main);
    }
    void select_begin(int gi) { order_begin_chain(t, sets[gi], ops, kGeo, h.geo_turn, h.main, false, h.events); }
    void select_end(int gi) { order_end_chain(sets[gi], ops); }
    void heights_begin() { OrderSet<int, int>* const all[3] = { &sets[0], &sets[1], &sets[2] }; order_terrain_changing(all, ops, h.main); }
    void heights_end() { OrderSet<int, int>* const all[3] = { &sets[0], &sets[1], &sets[2] }; order_terrain_changed(t, all, ops, h.main); }
    void maps_begin()
    {
        OrderSet<int, int>* const all[3] = { &sets[0], &sets[1], &sets[2] };
        order_terrain_changing(all, ops, h.main); order_terrain_tables_changing(all, ops, h.main, h.events);
    }
    void maps_end() { heights_end(); }
    void pyramid_begin(bool) { order_side_begin(pyramid, ops, h.main); }
    void pyramid_end() { order_side_end(pyramid, ops, h.main); }
    void journal_begin() { order_side_begin(journal, ops, h.main); }
    void journal_end() { order_side_end(journal, ops, h.main); }
    void journal_idle() { order_side_idle(journal, ops); }
    void brush_idle() { order_side_idle(brush, ops); }
    void brush_end() { order_side_end(brush, ops, h.main); }
    void sweep_begin() { order_side_begin(brush, ops, h.main); }
    void light_writer_begins(int im) { order_image_writer_begins(img[im], ops, h.main); }
    void image_written(int im, bool fused, EventRef<int> fused_stop, EventRef<int> light_stop, int reader)
    { order_image_written(img[im], ops, h.main, reader, fused ? fused_stop : light_stop, h.events); }
    void reader_done(int im, int reader) { order_image_reader_done(img[im], ops, reader); }
};

// ---- the API calls: what the .hip files do around the ordering steps, with the kernels' accesses ------------------------------
enum Call { RENDER0, RENDER1, RENDER2, PREPARE0, PREPARE1, PREPARE2, RENDER_LOCKED, SELECT, HEIGHTS_UPDATE, SET_STREAM, ASYNC_TOGGLE, DISPATCH_TOGGLE,
            FUSION_TOGGLE, NOT_STAMPED_1ST, NOT_STAMPED_2ND, TIMING_ON, TIMING_OFF, SUBMIT_A_CROSS, SUBMIT_A_SAME, SUBMIT_B_CROSS, SUBMIT_B_SAME,
            EDIT_HOST, EDIT_DEVICE, EDIT_ALBEDO_DEVICE, BRUSH, UNDO_REDO, HISTORY_ENABLE, CAST_HOST, CAST_DEVICE, QUERY_DEVICE, SWEEP_STATE, QUERY_PYRAMID, OTHER_TERRAIN_FRAME, N_CALLS };
static const char* const kCallName[N_CALLS] = { "render(0)", "render(1)", "render(2)", "prepare(0)", "prepare(1)", "prepare(2)", "render(lock_view)", "select",
    "update_heights", "set_stream", "async_geometry^", "dispatch_events^", "frame_fusion^", "next launch not stamped", "launch after next not stamped",
    "timing_enable(2)", "timing_enable(0)/collect", "submit(image A, tone mapper on another stream)", "submit(image A, same stream)",
    "submit(image B, another stream)", "submit(image B, same stream)",
    "edit(heightmap, host pointer)", "edit(heightmap, device pointer)", "edit(albedo, device pointer)", "brush/erode", "undo/redo", "history_enable",
    "cast_rays(host pointers)", "cast_rays(device pointers)", "query_heights(device pointers)", "sweep_state", "query_pyramid", "frame of another terrain" };

template <class P> struct Driver {
    World& w; Host& h; P& p;
    void geometry(int gi, int sel)                            // launch_geometry
    {
        p.begin_chain(gi);
        const int gs = p.stream(gi);
        if (sel < 0) { w.kernel(gs); w.access(HEIGHTS, false, gs); w.access(SEL0 + gi, true, gs); geoslots_selected(h.slots, gi); }
        else if (sel != gi) {
            p.copy_selection(gi, sel, [&]() { w.kernel(gs); w.access(SEL0 + sel, false, gs); w.access(SEL0 + gi, true, gs); });
            geoslots_selected(h.slots, gi);
        }
        w.kernel(gs); w.access(SEL0 + gi, false, gs); w.access(HMAP, false, gs); w.access(GEO0 + gi, true, gs);      // (the vertex stage samples the heightmap)
        p.end_chain(gi);
    }
    void prepare(int view)                                    // vr_terrain_prepare
    {
        if (geoslots_find(h.slots, view) >= 0) return;
        const int gi = geoslots_pick(h.slots);
        geoslots_claim(h.slots, gi);
        p.prepare_start();
        geometry(gi, -1);
        p.prepare_wait(gi);
        geoslots_prepared(h.slots, gi, view);
    }
    EventRef<int> render(int view, bool lock, int keep_image) // terrain_render_impl; returns the pass's stop event (keep: the fused launch's)
    {
        int gi = lock ? -1 : geoslots_find(h.slots, view);
        const bool use_prepared = gi >= 0;
        if (!use_prepared) gi = geoslots_pick(h.slots);
        geoslots_claim(h.slots, gi);
        if (!use_prepared) geometry(gi, geoslots_selection_source(h.slots, lock));
        geoslots_current(h.slots, gi);
        p.tile_pass_begin(gi, use_prepared);
        if (keep_image >= 0) p.keep_writer_begins(keep_image);
        const EventRef<int> pass_stop = h.stamped_launch(w);
        w.access(SEL0 + gi, false, h.main); w.access(GEO0 + gi, false, h.main);
        w.access(HMAP, false, h.main); w.access(AMAP, false, h.main);                                                    // (both maps' tables)
        if (keep_image >= 0) w.access(IMG0 + keep_image, true, h.main);
        p.tile_pass_launched(gi, pass_stop);
        return pass_stop;
    }
    void select()                                             // vr_terrain_select (asynchronous form)
    {
        const int gi = geoslots_pick(h.slots);
        p.select_begin(gi);
        geoslots_claim(h.slots, gi);
        const int gs = p.stream(gi);
        w.kernel(gs); w.access(HEIGHTS, false, gs); w.access(SEL0 + gi, true, gs); geoslots_selected(h.slots, gi);
        p.select_end(gi);
        geoslots_current(h.slots, gi);
    }
    void update_heights()                                     // vr_terrain_update_heights
    {
        geoslots_invalidate(h.slots);
        p.heights_begin();
        w.kernel(h.main); w.access(HEIGHTS, true, h.main);
        p.heights_end();
    }
    // ---- the editing path.  Every kernel runs on the context's stream.  Not modelled: a refusal; a growth of the staging or of a
    // brush buffer (its quiesce is the stream synchronise / the order_side_idle that the call makes anyway); a pending G-buffer frame.
    template <class Write> void level0_write(int which, Write&& write)      // vr_derive_level0_write
    {
        const int s = h.main, map = which ? AMAP : HMAP;
        p.maps_begin();
        geoslots_invalidate(h.slots);
        write();
        w.kernel(s); w.access(map, true, s);                                // levels 1 .. and the tables
        if (which == 0) { w.kernel(s); w.access(HMAP, false, s); w.access(HEIGHTS, true, s); }
        if (which == 0 && h.pyramid_built) {
            p.pyramid_begin(true);
            w.kernel(s); w.access(HMAP, false, s); w.access(PYRAMID, true, s);
            p.pyramid_end();
        }
        p.maps_end();
    }
    void capture(int which)                                   // vr_history_capture: every call is one committed step here
    {
        if (!h.history_on) return;
        const int s = h.main;
        p.journal_begin();
        w.kernel(s); w.access(which ? AMAP : HMAP, false, s); w.access(JOURNAL, true, s);
        p.journal_end();
        h.undo.push_back(which); h.redo.clear();
    }
    void edit(int which, bool host_pointer)                   // vr_terrain_edit
    {
        const int s = h.main;
        level0_write(which, [&]() {
            capture(which);
            if (host_pointer) { w.kernel(s); w.access(STAGE, true, s); }
            w.kernel(s); if (host_pointer) w.access(STAGE, false, s); w.access(which ? AMAP : HMAP, true, s);
        });
        if (host_pointer) w.sync_stream(s);
    }
    void brush()                                              // vr_brush_call: vr_terrain_brush (a sculpting op), vr_terrain_erode, _erode_hydraulic
    {
        const int s = h.main;
        p.brush_idle();
        w.host_touch(BRUSHBUF);                               // the pinned dab list is written; a buffer that grows is freed
        level0_write(0, [&]() {
            capture(0);
            w.kernel(s); w.access(BRUSHBUF, true, s);         // the upload, the snapshot, the block's planes
            w.kernel(s); w.access(BRUSHBUF, false, s); w.access(HMAP, true, s);
            p.brush_end();
        });
        h.sweep_left = true;
    }
    void undo_redo()                                          // history_apply: undo if there is a step to undo, else redo
    {
        const bool undo = !h.undo.empty();
        if (!undo && h.redo.empty()) return;                  // queues nothing
        std::vector<int>& from = undo ? h.undo : h.redo;
        const int which = from.back(), s = h.main;
        from.pop_back(); (undo ? h.redo : h.undo).push_back(which);
        level0_write(which, [&]() {
            p.journal_begin();
            w.kernel(s); w.access(JOURNAL, true, s); w.access(which ? AMAP : HMAP, true, s);
            p.journal_end();
        });
    }
    void history_enable()                                     // vr_terrain_history_enable with another budget: a new arena replaces the old one
    {
        if (h.history_on) { p.journal_idle(); w.host_touch(JOURNAL); }
        h.history_on = true; h.undo.clear(); h.redo.clear();
    }
    void cast(bool host_pointers)                             // vr_terrain_cast_rays; the first one builds the pyramid (ensure_pyramid)
    {
        const int s = h.main;
        if (h.pyramid_built) p.pyramid_begin(false);
        else { w.kernel(s); w.access(HMAP, false, s); w.access(PYRAMID, true, s); p.pyramid_end(); h.pyramid_built = true; }
        if (host_pointers) { w.kernel(s); w.access(STAGE, true, s); }
        w.kernel(s); w.access(HMAP, false, s); w.access(PYRAMID, false, s);
        if (host_pointers) { w.access(STAGE, true, s); w.kernel(s); w.access(STAGE, false, s); w.sync_stream(s); }
    }
    void query_device() { w.kernel(h.main); w.access(HMAP, false, h.main); }      // vr_terrain_query_heights, nothing waited for
    void sweep_state()                                        // vr_debug_terrain_sweep_state
    {
        if (!h.sweep_left) return;
        p.sweep_begin();
        w.kernel(h.main); w.access(BRUSHBUF, false, h.main);
        w.sync_stream(h.main);
    }
    void query_pyramid()                                      // vr_debug_terrain_query_pyramid: builds nothing; the copy is a reader, like the walk
    {
        if (!h.pyramid_built) return;
        p.pyramid_begin(false);
        w.kernel(h.main); w.access(PYRAMID, false, h.main);
        w.sync_stream(h.main);
    }
    void timing(int level) { events_timing_enable(h.events, Host::EvOps{ &w, &h }, h.main, level); }      // vr_timing_enable / vr_timing_collect
    // a frame of ANOTHER terrain of the same context, unfused: its tile pass and its lighting pass take ring slots (all four of this
    // ring) and touch nothing of this terrain's; its chains run on its own geometry streams
    void other_terrain_frame() { h.stamped_launch(w); h.stamped_launch(w); }
    void submit(int im, bool tm_cross)                        // vr_frame_submit: view n, the next two prepared ahead
    {
        const int view = h.frame_no % 3;
        const bool fused = h.frame_fusion;                    // (where the tile pass's G-buffer-keeping flavour applies)
        const EventRef<int> fused_stop = render(view, false, fused ? im : -1);
        prepare((view + 1) % 3); prepare((view + 2) % 3);
        EventRef<int> light_stop;
        if (!fused) {
            p.light_writer_begins(im);
            light_stop = h.stamped_launch(w);
            w.access(IMG0 + im, true, h.main);
        }
        const int reader = tm_cross ? TM : h.main;
        const bool cross = reader != h.main;
        if (cross) p.image_written(im, fused, fused_stop, light_stop, reader);
        w.kernel(reader); w.access(IMG0 + im, false, reader);
        if (cross) p.reader_done(im, reader);
        h.frame_no++;
    }
    void call(int c)
    {
        h.launched = false;
        switch (c) {
        case RENDER0: case RENDER1: case RENDER2: render(c - RENDER0, false, -1); break;
        case PREPARE0: case PREPARE1: case PREPARE2: prepare(c - PREPARE0); break;
        case RENDER_LOCKED: render(0, true, -1); break;
        case SELECT: select(); break;
        case HEIGHTS_UPDATE: update_heights(); break;
        case SET_STREAM: { const int to = h.main == M0 ? M1 : M0; w.host_orders(to, h.main); h.main = to; } break;     // (test_context_stream_changed_...: "what the host owes")
        case ASYNC_TOGGLE: h.async_geometry = !h.async_geometry; break;
        case DISPATCH_TOGGLE: events_set_dispatch(h.events, Host::EvOps{ &w, &h }, h.main, !h.events.dispatch_events); break;   // vr_context_set_option
        case FUSION_TOGGLE: h.frame_fusion = !h.frame_fusion; break;
        case NOT_STAMPED_1ST: h.not_stamped = 1u; break;
        case NOT_STAMPED_2ND: h.not_stamped = 2u; break;
        case TIMING_ON: timing(2); break;
        case TIMING_OFF: timing(0); break;
        case SUBMIT_A_CROSS: submit(0, true); break;
        case SUBMIT_A_SAME: submit(0, false); break;
        case SUBMIT_B_CROSS: submit(1, true); break;
        case SUBMIT_B_SAME: submit(1, false); break;
        case EDIT_HOST: edit(0, true); break;
        case EDIT_DEVICE: edit(0, false); break;
        case EDIT_ALBEDO_DEVICE: edit(1, false); break;
        case BRUSH: brush(); break;
        case UNDO_REDO: undo_redo(); break;
        case HISTORY_ENABLE: history_enable(); break;
        case CAST_HOST: cast(true); break;
        case CAST_DEVICE: cast(false); break;
        case QUERY_DEVICE: query_device(); break;
        case SWEEP_STATE: sweep_state(); break;
        case QUERY_PYRAMID: query_pyramid(); break;
        case OTHER_TERRAIN_FRAME: other_terrain_frame(); break;
        }
        if (h.launched) h.not_stamped = 0;                    // the marker covers the next call that launches, no more
    }
};

struct Outcome { std::vector<Op> trace; int unordered; std::string first; };
static World g_world;
static Outcome run_parent(const int* seq, int n, Intended in, int drop)
{
    g_world.reset(drop);
    Host h; Parent p(g_world, h, in); Driver<Parent> d{ g_world, h, p };
    for (int i = 0; i < n; i++) d.call(seq[i]);
    return { g_world.trace, g_world.unordered, g_world.first };
}
static Outcome run_protocol(const int* seq, int n)
{
    g_world.reset(0);
    Host h; Protocol p(g_world, h); Driver<Protocol> d{ g_world, h, p };
    for (int i = 0; i < n; i++) d.call(seq[i]);
    return { g_world.trace, g_world.unordered, g_world.first };
}
static bool same(const std::vector<Op>& a, const std::vector<Op>& b) { return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(Op)) == 0); }
static std::string show(const int* seq, int n) { std::string s; for (int i = 0; i < n; i++) { if (i) s += "; "; s += kCallName[seq[i]]; } return s; }
static std::string show(const std::vector<Op>& t)
{
    std::string s;
    for (const Op& o : t) { char b[64]; snprintf(b, sizeof(b), " %s(%s,e%d)", o.wait == 2 ? "sync" : o.wait ? "wait" : "record", kStreamName[o.stream], o.event); s += b; }
    return s;
}

// ---- (c) the sequences ------------------------------------------------------------------------------------
constexpr int kExhaustive = 4, kRandom = 200000, kRandomMax = 14;
static const Intended kPlain = { false, false, false, false, false }, kAll = { true, true, true, true, true };
static long sequences = 0, failures = 0;
// the parent's own unordered pairs, by the one intended difference that repairs them
struct Finding { const char* name; Intended only; long count; int shortest[kRandomMax], shortest_n; std::string pair; };
static Finding findings[2] = {
    { "vr_frame_submit took ctx->last_stop for a lighting pass that was not stamped", { true, false, false, false, false }, 0, {}, 0, "" },
    { "the node-height update did not wait for chains that still read the heights", { false, true, false, false, false }, 0, {}, 0, "" },
};
static long drop_reported[N_SITES];

static void check(const int* seq, int n)
{
    sequences++;
    const Outcome now = run_protocol(seq, n);
    if (now.unordered) { if (failures++ < 10) printf("FAIL (b) protocol: %s\n    %s\n", show(seq, n).c_str(), now.first.c_str()); }
    const Outcome spec = run_parent(seq, n, kAll, 0);
    if (!same(now.trace, spec.trace)) {
        if (failures++ < 10) printf("FAIL (a) traces differ: %s\n    parent  :%s\n    protocol:%s\n", show(seq, n).c_str(), show(spec.trace).c_str(), show(now.trace).c_str());
    }
    const Outcome plain = run_parent(seq, n, kPlain, 0);
    if (plain.unordered) {
        // a finding about the parent: one of the two differences alone must repair it, or both together (two findings in one sequence)
        bool explained = false;
        for (Finding& f : findings) {
            if (run_parent(seq, n, f.only, 0).unordered) continue;
            explained = true; f.count++;
            if (!f.shortest_n || n < f.shortest_n) { f.shortest_n = n; memcpy(f.shortest, seq, n * sizeof(int)); f.pair = plain.first; }
        }
        if (!explained && run_parent(seq, n, { true, true, false, false, false }, 0).unordered) {
            if (failures++ < 10) printf("FAIL (b) parent, not repaired by the intended differences: %s\n    %s\n", show(seq, n).c_str(), plain.first.c_str());
        }
    }
}
static void check_drops(const int* seq, int n)
{
    sequences++;
    // (the dead wait that Intended::sweep_dead_wait drops exists only with that switch off)
    static const Intended kWithDead = { true, true, true, false, true };
    for (int site = 1; site < N_SITES; site++) if (run_parent(seq, n, site == W_SWEEP_DEAD ? kWithDead : kAll, site).unordered) drop_reported[site]++;
}

template <class F> static void all_sequences(int longest, long random, F&& f)
{
    int seq[kRandomMax];
    for (int n = 1; n <= longest; n++) {
        long total = 1;
        for (int i = 0; i < n; i++) total *= N_CALLS;
        for (long k = 0; k < total; k++) { long v = k; for (int i = 0; i < n; i++) { seq[i] = (int)(v % N_CALLS); v /= N_CALLS; } f(seq, n); }
    }
    uint64_t x = 0x9E3779B97F4A7C15ull;                           // xorshift64, fixed seed
    auto next = [&x]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    for (long k = 0; k < random; k++) {
        const int n = longest + 1 + (int)(next() % (uint64_t)(kRandomMax - longest));
        for (int i = 0; i < n; i++) seq[i] = (int)(next() % N_CALLS);
        f(seq, n);
    }
}

// a sequence on which the plain transcription must fail (b) and the protocol must pass
static void known(const char* what, std::vector<int> seq)
{
    const Outcome plain = run_parent(seq.data(), (int)seq.size(), kPlain, 0), now = run_protocol(seq.data(), (int)seq.size());
    printf("known: %s\n    %s\n    parent: %s\n    protocol: %s\n", what, show(seq.data(), (int)seq.size()).c_str(),
           plain.unordered ? plain.first.c_str() : "ordered", now.unordered ? now.first.c_str() : "ordered");
    if (!plain.unordered || now.unordered) { failures++; printf("FAIL: expected the parent unordered and the protocol ordered\n"); }
}

// The rule of vr_events.h for a ring handle that is no longer live, pinned: set 1's tile pass is stamped on main0; the context moves
// to main1, where another terrain's frame takes all four slots; two renders later set 1's next chain waits on the mark - for the
// slot's new occupant, stamped on ANOTHER stream, and that orders the chain behind the tile pass all the same.
static void pinned_ring_reuse()
{
    const std::vector<int> seq = { RENDER0, SET_STREAM, OTHER_TERRAIN_FRAME, RENDER1, RENDER2 };
    g_world.reset(0);
    Host h; Protocol p(g_world, h); Driver<Protocol> d{ g_world, h, p };
    for (size_t i = 0; i + 1 < seq.size(); i++) d.call(seq[i]);
    const EventRef<int> mark = p.sets[1].tile_pass.at;
    const bool stale = mark.slot != 0 && !events_live(h.events, mark) && events_wait_needed(h.events, mark);
    const size_t before = g_world.trace.size();
    d.call(seq.back());
    bool waited = false;
    for (size_t i = before; i < g_world.trace.size(); i++) waited |= g_world.trace[i].wait == 1 && g_world.trace[i].event == mark.ev && g_world.trace[i].stream == p.stream(1);
    printf("pinned: a wait on a reissued ring slot is a wait for its new occupant, queued behind the old one\n    %s\n    handle %s, %s, %s\n",
           show(seq.data(), (int)seq.size()).c_str(), stale ? "no longer live" : "LIVE", waited ? "waited for" : "NOT waited for", g_world.unordered ? g_world.first.c_str() : "ordered");
    if (!stale || !waited || g_world.unordered) { failures++; printf("FAIL: expected a stale ring handle, a wait on it and no unordered pair\n"); }
}

int main(int argc, char** argv)
{
    if (argc > 1 && !strcmp(argv[1], "--drop-each")) {
        all_sequences(3, 20000, check_drops);
        printf("%ld sequences, the transcription (intended differences on) less one wait site at a time:\n", sequences);
        int reported = 0, bad = 0;
        for (int site = 1; site < N_SITES; site++) {
            printf("  %-72s %s (%ld sequences)\n", kSiteName[site], drop_reported[site] ? "reported" : "NOT reported", drop_reported[site]);
            if (!drop_reported[site] && dead_reason(site)) printf("      orders nothing: %s\n", dead_reason(site));
            reported += drop_reported[site] != 0;
            // every wait is needed somewhere, or is named with the reason it orders nothing
            bad += (drop_reported[site] != 0) == (dead_reason(site) != nullptr);
        }
        printf("%d of %d wait sites reported, %d unexpected\n", reported, N_SITES - 1, bad);
        return bad ? 1 : 0;
    }
    // intended difference 1 (known before): the tile pass is stamped, the lighting launch is not - ctx->last_stop is the tile pass's
    // stop event and the tone-map stage reads the image while the lighting pass writes it
    known(findings[0].name, { FUSION_TOGGLE, NOT_STAMPED_2ND, SUBMIT_A_CROSS });
    // intended difference 2 (found by (b)): a select's chain is consumed by nothing on the context's stream, which then rewrites the heights
    known(findings[1].name, { SELECT, HEIGHTS_UPDATE });
    pinned_ring_reuse();
    all_sequences(kExhaustive, kRandom, check);
    for (const Finding& f : findings) {
        printf("finding: %s: %ld sequences; shortest: %s\n    %s\n", f.name, f.count, show(f.shortest, f.shortest_n).c_str(), f.pair.c_str());
        if (!f.count) { failures++; printf("FAIL: the finding was not seen\n"); }
    }
    printf("dead wait dropped: vr_debug_terrain_sweep_state waits for the erosion only where it ran on another stream (Intended::sweep_dead_wait)\n");
    printf("wait kept: a mark that holds a ring event outlives a recycled timing epoch; its launch is complete by then (Intended::ring_handles)\n");
    printf("permitted reorder: vr_terrain_select queues the main-dependency wait last, as launch_geometry does (Intended::common_order)\n");
    printf("%ld sequences (all up to %d calls of %d, %d random up to %d), %ld failures\n", sequences, kExhaustive, (int)N_CALLS, kRandom, kRandomMax, failures);
    return failures ? 1 : 0;
}
