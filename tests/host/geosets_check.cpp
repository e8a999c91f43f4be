// vr_geosets.h against a transcription of the code it replaced, and against the invariants it states.
//
// (a) The transcription ("Old") is the slot policy as it stood inline in vr_raster.hip (prepared_matches, vr_terrain_prepare,
//     launch_geometry's have_selection, terrain_render_impl, vr_gbuffer_materialise_planes), vr_select.hip (vr_terrain_pick_set,
//     vr_terrain_select, vr_select_launch, the invalidation loops of vr_terrain_update_heights and alloc_scratch) and vr_derive.hip
//     (vr_derive_level0_write's loop), over the loose fields GeoSet and vr_terrain had for it.  The HIP calls, the ordering calls and
//     launch_geometry's kernels are one thing here: a fallible step, which a script may make fail.  The other side ("New") is what
//     the .hip files do now around the header's transitions, with the same fallible steps at the same places.  After every event
//     of every sequence both sides agree on the return code, the set chosen, whether a build was started, the selection source,
//     what order_prepare_wait was told, and the whole state.
// (b) The invariants, on the New side after every event: check_invariants().
//
// Events: prepare(key), render(key, lock_view), select, invalidate (vr_terrain_update_heights, vr_derive_level0_write and
// alloc_scratch alike), materialise(key) and "the k-th fallible step from now fails".  Six keys: a base frame; the same with
// assume_cleared and depth_ranges set (the equality ignores both); with 64-pixel raster tiles; from another camera; wireframe = 1
// and wireframe = 2 (one truth value).
//
//   geosets_check                is the header right?
//   geosets_check --break-each   is the check alive?  One rule at a time is weakened in a copy of the policy kept here (pol_*: the
//                                product header has no switches); each must be reported.
//
// g++ -std=c++17 -O1 -Wall -Werror -I vrenderer_amd/csrc tests/host/geosets_check.cpp
#include "vr_geosets.h"

#include <stdio.h>
#include <string.h>
#include <string>

// ---- the events --------------------------------------------------------------------------------------------------------------------
struct In { vr_view view; vr_render_params rp; int w, h, rank, world, tile_shift; };
enum { K_BASE, K_IGNORED, K_TILE64, K_VIEW, K_WIRE1, K_WIRE2, N_KEYS };
static const char* const kKeyName[N_KEYS] = { "base", "base+assume_cleared+depth_ranges", "base, 64-pixel tiles", "other camera", "wireframe=1", "wireframe=2" };
static In g_keys[N_KEYS];
static void make_keys()
{
    In b;
    memset(&b, 0, sizeof b);
    for (int i = 0; i < 16; i++) b.view.world_to_view[i] = b.view.view_to_clip[i] = (float)(i % 5 == 0);
    b.view.camera_pos[0] = 1.0f; b.view.viewport_w = 320; b.view.viewport_h = 180;
    b.rp.max_height = 400.0f;
    b.w = 320; b.h = 180; b.rank = 0; b.world = 1; b.tile_shift = 5;
    for (In& k : g_keys) k = b;
    g_keys[K_IGNORED].rp.assume_cleared = 1; g_keys[K_IGNORED].rp.depth_ranges = 1;
    g_keys[K_TILE64].tile_shift = 6;
    g_keys[K_VIEW].view.camera_pos[0] = 2.0f;
    g_keys[K_WIRE1].rp.wireframe = 1;
    g_keys[K_WIRE2].rp.wireframe = 2;
}
enum Kind { E_PREPARE, E_RENDER, E_RENDER_LOCKED, E_SELECT, E_INVALIDATE, E_MATERIALISE, E_FAIL };
struct Ev { int kind, arg; };                      // arg: the key, or k of E_FAIL
constexpr int kMaxFail = 6;                        // a prepare has six fallible steps, a render five
constexpr int N_EVENTS = 4 * N_KEYS + 2 + kMaxFail;
static Ev g_events[N_EVENTS];
static void make_events()
{
    int n = 0;
    for (int kind : { E_PREPARE, E_RENDER, E_RENDER_LOCKED, E_MATERIALISE }) for (int k = 0; k < N_KEYS; k++) g_events[n++] = { kind, k };
    g_events[n++] = { E_SELECT, 0 }; g_events[n++] = { E_INVALIDATE, 0 };
    for (int k = 1; k <= kMaxFail; k++) g_events[n++] = { E_FAIL, k };
}
static std::string show(const Ev& e)
{
    static const char* const kinds[] = { "prepare", "render", "render_locked", "select", "invalidate", "materialise", "fail_step" };
    char b[96];
    if (e.kind == E_SELECT || e.kind == E_INVALIDATE) return kinds[e.kind];
    if (e.kind == E_FAIL) snprintf(b, sizeof b, "fail_step(%d)", e.arg);
    else snprintf(b, sizeof b, "%s(%s)", kinds[e.kind], kKeyName[e.arg]);
    return b;
}

// the k-th fallible step from now fails (0: none does)
struct Script { int fail_in = 0; bool fails() { return fail_in > 0 && --fail_in == 0; } };
// what a call chose and answered
struct Out { int rc = 0, set = -1, built = 0, source = -2, other = -1; };
static bool same(const Out& a, const Out& b) { return a.rc == b.rc && a.set == b.set && a.built == b.built && a.source == b.source && a.other == b.other; }

// ---- (a) the transcription ---------------------------------------------------------------------------------------------------------
struct Old {
    struct Set {
        bool have_selection = false, prepared = false;
        uint64_t prep_serial = 0;
        vr_view prep_view; vr_render_params prep_rp; int prep_w = 0, prep_h = 0, prep_rank = 0, prep_world = 0, prep_tile_shift = 0;
    } sets[3];
    int cur = 0;
    uint64_t prep_counter = 0;
    Script script;
    Old() { for (Set& g : sets) { memset(&g.prep_view, 0, sizeof g.prep_view); memset(&g.prep_rp, 0, sizeof g.prep_rp); } }

    static bool prepared_matches(const Set& g, const In& k)
    {
        return memcmp(&g.prep_view, &k.view, sizeof(vr_view)) == 0 && g.prep_rp.max_height == k.rp.max_height && g.prep_rp.depth_only == k.rp.depth_only
            && !g.prep_rp.wireframe == !k.rp.wireframe && g.prep_w == k.w && g.prep_h == k.h && g.prep_rank == k.rank && g.prep_world == k.world
            && g.prep_tile_shift == k.tile_shift;
    }
    int pick_set() const
    {
        int best = -1;
        for (int i = 0; i < 3; i++) {
            if (i == cur) continue;
            if (!sets[i].prepared) return i;
            if (best < 0 || sets[i].prep_serial < sets[best].prep_serial) best = i;
        }
        return best;
    }
    int select_launch(Set& g)
    {
        if (script.fails()) return 1;                                  // the launch's hipGetLastError
        g.have_selection = true;
        return 0;
    }
    int launch_geometry(Set& g, Set* selection_from, Out& o)
    {
        o.built = 1; o.source = selection_from ? (int)(selection_from - sets) : -1;
        if (script.fails()) return 1;                                  // order_begin_chain
        if (selection_from == nullptr) { if (select_launch(g)) return 1; }
        else if (selection_from != &g) {
            if (script.fails()) return 1;                              // order_copy_selection
            g.have_selection = true;
        }
        if (script.fails()) return 1;                                  // the tile buffers' growth, order_end_chain, hipGetLastError
        return 0;
    }
    int prepare(const In& k, Out& o)
    {
        if (script.fails()) return 1;                                  // vr_terrain_frame_scratch, vr_partition_tables
        for (Set& p : sets)
            if (p.prepared && prepared_matches(p, k)) return 0;
        Set& g = sets[pick_set()];
        o.set = (int)(&g - sets);
        g.prepared = false;
        if (script.fails()) return 1;                                  // order_prepare_start
        if (launch_geometry(g, nullptr, o)) return 1;
        bool other_prepared = false;
        for (const Set& p : sets) other_prepared |= (&p != &g) && p.prepared;
        o.other = other_prepared;
        if (script.fails()) return 1;                                  // order_prepare_wait
        g.prepared = true; g.prep_view = k.view; g.prep_rp = k.rp; g.prep_w = k.w; g.prep_h = k.h; g.prep_rank = k.rank; g.prep_world = k.world; g.prep_tile_shift = k.tile_shift;
        g.prep_serial = ++prep_counter;
        return 0;
    }
    int render(const In& k, Out& o)
    {
        if (script.fails()) return 1;                                  // everything in front of the set's choice: scratch, plan, pending planes
        int gi = -1;
        if (!k.rp.lock_view)
            for (int i = 0; i < 3; i++)
                if (i != cur && sets[i].prepared && prepared_matches(sets[i], k)) { gi = i; break; }
        const bool use_prepared = gi >= 0;
        if (!use_prepared) gi = pick_set();
        Set& g = sets[gi];
        Set& last = sets[cur];
        o.set = gi;
        g.prepared = false;
        if (!use_prepared) {
            Set* sel = (k.rp.lock_view && last.have_selection) ? &last : nullptr;
            if (launch_geometry(g, sel, o)) return 1;
        }
        cur = gi;
        if (script.fails()) return 1;                                  // order_tile_pass_begin and everything behind it
        return 0;
    }
    int materialise(const In& k, Out& o)
    {
        const int c = cur;
        const int rc = render(k, o);
        cur = c;
        return rc;
    }
    int select(Out& o)
    {
        if (script.fails()) return 1;                                  // terrain_poll
        const int gi = pick_set();
        Set& g = sets[gi];
        o.set = gi;
        if (script.fails()) return 1;                                  // order_begin_chain
        g.prepared = false;
        if (select_launch(g)) return 1;
        if (script.fails()) return 1;                                  // order_end_chain
        cur = gi;
        return 0;
    }
    int invalidate()
    {
        if (script.fails()) return 1;                                  // vr_terrain_materialise_pending, the ordering calls; vr_grow_group
        for (Set& g : sets) g.prepared = false;
        return 0;
    }
};

// ---- the policy the New side calls: the header's, or under --break-each a copy with one rule weakened -----------------------------
static const char* const kBreakNames[] = {
    "none", "the pick may return cur", "eviction takes the newest", "wireframe is compared by value", "tile_shift is left out of the key",
    "invalidate clears selections", "materialise moves cur", "a render's claim comes behind its build", "the serial is taken in front of order_prepare_wait" };
enum { BRK_NONE = 0, BRK_PICK_CUR, BRK_EVICT_NEWEST, BRK_WIRE_VALUE, BRK_NO_TILE_SHIFT, BRK_INVALIDATE_SELECTIONS, BRK_MATERIALISE_CUR, BRK_CLAIM_LATE,
       BRK_SERIAL_EARLY, N_BREAKS };
static int g_break = BRK_NONE;
typedef GeoSlots<GeoKey> Slots;

static int pol_pick(const Slots& s)
{
    if (g_break != BRK_PICK_CUR && g_break != BRK_EVICT_NEWEST) return geoslots_pick(s);
    int best = -1;
    for (int i = 0; i < kGeoSets; i++) {
        if (i == s.cur && g_break != BRK_PICK_CUR) continue;
        if (!s.slot[i].prepared) return i;
        if (best < 0 || (g_break == BRK_EVICT_NEWEST ? s.slot[i].serial > s.slot[best].serial : s.slot[i].serial < s.slot[best].serial)) best = i;
    }
    return best;
}
static int pol_find(const Slots& s, const GeoKey& key)
{
    if (g_break != BRK_WIRE_VALUE && g_break != BRK_NO_TILE_SHIFT) return geoslots_find(s, key);
    for (int i = 0; i < kGeoSets; i++) {
        const GeoKey& a = s.slot[i].key;
        if (s.slot[i].prepared && memcmp(&a.view, &key.view, sizeof(vr_view)) == 0 && a.max_height == key.max_height && a.depth_only == key.depth_only
            && (g_break == BRK_WIRE_VALUE ? a.wireframe == key.wireframe : !a.wireframe == !key.wireframe) && a.w == key.w && a.h == key.h && a.rank == key.rank
            && a.world == key.world && (g_break == BRK_NO_TILE_SHIFT || a.tile_shift == key.tile_shift)) return i;
    }
    return -1;
}
static void pol_invalidate(Slots& s)
{
    geoslots_invalidate(s);
    if (g_break == BRK_INVALIDATE_SELECTIONS) for (Slots::Slot& p : s.slot) p.have_selection = false;
}

static long failures = 0;
static bool g_quiet = false;
static const Ev* g_seq[32]; static int g_len = 0;
static void fail(const char* what)
{
    if (failures++ < 10 && !g_quiet) {
        printf("FAIL %s\n   ", what);
        for (int i = 0; i < g_len; i++) printf(" %s;", show(*g_seq[i]).c_str());
        printf("\n");
    }
}

// ---- what the .hip files do around the header --------------------------------------------------------------------------------------
struct New {
    Slots st;
    Script script;
    static GeoKey key_of(const In& k) { return geo_key(k.view, k.rp, k.w, k.h, k.rank, k.world, k.tile_shift); }
    int found(const GeoKey& key) const
    {
        const int gi = pol_find(st, key);
        if (gi >= 0 && !(st.slot[gi].key == key)) fail("(b) a set was found whose key is not equal");
        return gi;
    }
    int select_launch(int gi)                                          // vr_select_launch
    {
        if (script.fails()) return 1;
        geoslots_selected(st, gi);
        return 0;
    }
    int launch_geometry(int gi, int from, Out& o)                      // launch_geometry
    {
        o.built = 1; o.source = from;
        if (script.fails()) return 1;
        if (from < 0) { if (select_launch(gi)) return 1; }
        else if (from != gi) {
            if (script.fails()) return 1;
            geoslots_selected(st, gi);
        }
        if (script.fails()) return 1;
        return 0;
    }
    int prepare(const In& k, Out& o)                                   // vr_terrain_prepare
    {
        if (script.fails()) return 1;
        const GeoKey key = key_of(k);
        if (found(key) >= 0) return 0;
        const int gi = pol_pick(st);
        o.set = gi;
        geoslots_claim(st, gi);
        if (script.fails()) return 1;
        if (launch_geometry(gi, -1, o)) return 1;
        o.other = geoslots_other_prepared(st, gi);
        if (g_break == BRK_SERIAL_EARLY) st.counter++;
        if (script.fails()) return 1;
        if (g_break == BRK_SERIAL_EARLY) st.counter--;
        geoslots_prepared(st, gi, key);
        return 0;
    }
    int render(const In& k, Out& o)                                    // terrain_render_impl
    {
        if (script.fails()) return 1;
        int gi = k.rp.lock_view ? -1 : found(key_of(k));
        const bool use_prepared = gi >= 0;
        if (!use_prepared) gi = pol_pick(st);
        o.set = gi;
        if (g_break != BRK_CLAIM_LATE) geoslots_claim(st, gi);
        if (!use_prepared) {
            const int from = geoslots_selection_source(st, k.rp.lock_view != 0);
            if (launch_geometry(gi, from, o)) return 1;
        }
        if (g_break == BRK_CLAIM_LATE) geoslots_claim(st, gi);
        geoslots_current(st, gi);
        if (script.fails()) return 1;
        return 0;
    }
    int materialise(const In& k, Out& o)                               // vr_gbuffer_materialise_planes
    {
        int rc;
        { const GeoBorrow<GeoKey> borrowed(st); rc = render(k, o); }
        if (g_break == BRK_MATERIALISE_CUR && !rc) st.cur = o.set;
        return rc;
    }
    int select(Out& o)                                                 // vr_terrain_select
    {
        if (script.fails()) return 1;
        const int gi = pol_pick(st);
        o.set = gi;
        if (script.fails()) return 1;
        geoslots_claim(st, gi);
        if (select_launch(gi)) return 1;
        if (script.fails()) return 1;
        geoslots_current(st, gi);
        return 0;
    }
    int invalidate()                                                   // vr_terrain_update_heights, vr_derive_level0_write, alloc_scratch
    {
        if (script.fails()) return 1;
        pol_invalidate(st);
        return 0;
    }
};

static bool same_state(const Old& o, const New& n)
{
    if (o.cur != n.st.cur || o.prep_counter != n.st.counter || o.script.fail_in != n.script.fail_in) return false;
    for (int i = 0; i < kGeoSets; i++) {
        const Old::Set& g = o.sets[i]; const Slots::Slot& p = n.st.slot[i]; const GeoKey& k = p.key;
        if (g.prepared != p.prepared || g.have_selection != p.have_selection || g.prep_serial != p.serial) return false;
        if (memcmp(&g.prep_view, &k.view, sizeof(vr_view)) != 0 || g.prep_rp.max_height != k.max_height || g.prep_rp.depth_only != k.depth_only
            || g.prep_rp.wireframe != k.wireframe || g.prep_w != k.w || g.prep_h != k.h || g.prep_rank != k.rank || g.prep_world != k.world
            || g.prep_tile_shift != k.tile_shift) return false;
    }
    return true;
}

// ---- (b) the invariants, after every event -----------------------------------------------------------------------------------------
//   1  the current set holds no prepared frame
//   2  the pick is never the current set; it is an unprepared set if another set than the current one is unprepared, else the
//      prepared set with the smallest serial
//   3  at most kGeoSets - 1 sets are prepared
//   4  the serials of prepared sets are distinct
//   5  a found set's key is equal to the one asked for (New::found)
//   6  no set is prepared after an invalidate that was not refused
//   7  the current set is the same after a materialise as before it, whatever it returned
//   8  have_selection never falls
static void check_invariants(const Slots& before, const Slots& s, const Ev& e, int rc)
{
    if (s.slot[s.cur].prepared) fail("(b) 1: the current set holds a prepared frame");
    const int pick = pol_pick(s);
    int prepared = 0;
    bool free_other = false;
    for (int i = 0; i < kGeoSets; i++) { prepared += s.slot[i].prepared; free_other |= i != s.cur && !s.slot[i].prepared; }
    if (pick < 0 || pick >= kGeoSets || pick == s.cur) fail("(b) 2: the pick is the current set, or no set");
    else if (free_other && s.slot[pick].prepared) fail("(b) 2: the pick evicts a prepared frame while a set is free");
    else if (!free_other)
        for (int i = 0; i < kGeoSets; i++) if (i != s.cur && s.slot[i].serial < s.slot[pick].serial) { fail("(b) 2: the pick evicts a frame that is not the oldest"); break; }
    if (prepared > kGeoSets - 1) fail("(b) 3: every set is prepared");
    for (int i = 0; i < kGeoSets; i++) for (int j = i + 1; j < kGeoSets; j++)
        if (s.slot[i].prepared && s.slot[j].prepared && s.slot[i].serial == s.slot[j].serial) fail("(b) 4: two prepared sets share a serial");
    if (e.kind == E_INVALIDATE && !rc && prepared) fail("(b) 6: a set is prepared after an invalidate");
    if (e.kind == E_MATERIALISE && s.cur != before.cur) fail("(b) 7: a materialise moved the current set");
    for (int i = 0; i < kGeoSets; i++) if (before.slot[i].have_selection && !s.slot[i].have_selection) fail("(b) 8: a selection was lost");
}

struct Sim { Old old; New lib; };
static long sequences = 0, events_run = 0;
static void step(Sim& s, const Ev& e)
{
    events_run++;
    Out oo, on;
    const Slots before = s.lib.st;
    In k = g_keys[e.kind == E_SELECT || e.kind == E_INVALIDATE || e.kind == E_FAIL ? 0 : e.arg];
    switch (e.kind) {
    case E_PREPARE: oo.rc = s.old.prepare(k, oo); on.rc = s.lib.prepare(k, on); break;
    case E_RENDER_LOCKED: k.rp.lock_view = 1;       // falls through
    case E_RENDER: oo.rc = s.old.render(k, oo); on.rc = s.lib.render(k, on); break;
    case E_SELECT: oo.rc = s.old.select(oo); on.rc = s.lib.select(on); break;
    case E_INVALIDATE: oo.rc = s.old.invalidate(); on.rc = s.lib.invalidate(); break;
    case E_MATERIALISE: oo.rc = s.old.materialise(k, oo); on.rc = s.lib.materialise(k, on); break;
    case E_FAIL: s.old.script.fail_in = s.lib.script.fail_in = e.arg; break;
    }
    if (!same(oo, on)) fail("(a) the header and the transcription chose or answered differently");
    if (!same_state(s.old, s.lib)) fail("(a) the header and the transcription left different states");
    check_invariants(before, s.lib.st, e, on.rc);
}

static void enumerate(const Sim& s, int depth)
{
    for (const Ev& e : g_events) {
        Sim t = s;
        g_seq[g_len++] = &e;
        step(t, e);
        sequences++;
        if (depth > 1) enumerate(t, depth - 1);
        g_len--;
    }
}
static uint64_t g_rng;
static uint32_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return (uint32_t)(g_rng >> 32); }
constexpr int kRandomMax = 24;
static void run_all(int depth, long random_sequences)
{
    enumerate(Sim(), depth);
    g_rng = 0x9e3779b97f4a7c15ull;
    for (long i = 0; i < random_sequences; i++) {
        Sim s;
        const int n = depth + 1 + (int)(rnd() % (uint32_t)(kRandomMax - depth));
        g_len = 0;
        for (int k = 0; k < n; k++) {
            const Ev& e = g_events[rnd() % N_EVENTS];
            g_seq[g_len++] = &e;
            step(s, e);
        }
        sequences++;
    }
    g_len = 0;
}

int main(int argc, char** argv)
{
    make_keys(); make_events();
    if (argc > 1 && !strcmp(argv[1], "--break-each")) {
        int reported = 0;
        g_quiet = true;
        for (int b = 1; b < N_BREAKS; b++) {
            g_break = b; failures = 0;
            run_all(3, 20000);
            printf("  %-56s %s (%ld checks failed)\n", kBreakNames[b], failures ? "reported" : "NOT REPORTED", failures);
            reported += failures ? 1 : 0;
        }
        printf("%d of %d weakenings reported\n", reported, N_BREAKS - 1);
        return reported == N_BREAKS - 1 ? 0 : 1;
    }
    constexpr int kExhaustive = 4;
    constexpr long kRandom = 200000;
    run_all(kExhaustive, kRandom);
    printf("%ld sequences (all up to %d events of %d, %ld random up to %d), %ld events run, %ld failures\n", sequences, kExhaustive, N_EVENTS, kRandom, kRandomMax,
           events_run, failures);
    return failures ? 1 : 0;
}
