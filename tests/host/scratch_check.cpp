// vr_scratch.h against a transcription of the code it replaced, and against invariants of its own.
//
// The transcription ("old_*") is vr_select.hip's vr_terrain_poll, read_counters, vr_terrain_reserve_bins and the bin arithmetic
// of alloc_scratch as they were when the policy lived there, with the HIP calls replaced by a script: a chain "completes" when
// the sequence says so, and the allocator answers what the sequence last told it to.  The other side ("new_*") is what
// vr_select.hip does now - the mechanism around the header's functions - on the same script.  After every event the state, the
// return code, the allocation requested (node capacity, bins) and the message that would be set are compared.
//
// Events: a chain on set i completes with status words W; poll with / without report; the synchronous read with / without
// selection_only; reserve for N raster tiles; the allocator grants / refuses from now on.  W: flags x wanted nodes x bin total
// from the boundary values of the rules, relative to the capacities of the moment.  Every sequence of one and two events and a
// fixed-seed sample of longer ones, for every configuration (max_instances, initial capacity, bins override).
//
// g++ -std=c++17 -O1 -Wall -Werror -I vrenderer_amd/csrc tests/host/scratch_check.cpp
#include "vr_scratch.h"

#include <stdio.h>
#include <string.h>

// ---- the script both sides run on ----------------------------------------------------------------------------------------------
enum Msg { M_NONE, M_NO_MEMORY, M_EARLIER_TOO_MANY, M_EARLIER_OVERFLOW, M_READ_TOO_MANY, M_READ_LIST_FULL, M_READ_SHORT };
struct Outcome {
    int rc = 0;
    int n_alloc = 0; int alloc_cap[2] = { 0, 0 }; size_t alloc_bins[2] = { 0, 0 };
    int msg = M_NONE; size_t msg_a = 0, msg_b = 0;          // the last message set, with its figures
    void say(int m, size_t a = 0, size_t b = 0) { msg = m; msg_a = a; msg_b = b; }
};
struct Config { int max_instances, initial; long override_bins; };     // override_bins 0: VR_SCRATCH_INITIAL_BINS is not set
struct Env {
    Config cfg;
    bool alloc_ok = true;
    uint32_t mirror[kScratchSets][kStatusWords] = {};      // h_status
    uint32_t counters[kScratchSets][kStatusWords] = {};    // d_counters
    bool completed[kScratchSets] = { false, false, false };    // hipEventQuery(chain) == hipSuccess
    int cur = 0;
};
static bool allocate(const Env& e, Outcome& o, int cap, size_t bins)
{
    if (o.n_alloc < 2) { o.alloc_cap[o.n_alloc] = cap; o.alloc_bins[o.n_alloc] = bins; }
    o.n_alloc++;
    if (!e.alloc_ok) o.say(M_NO_MEMORY);
    return e.alloc_ok;
}

// ---- the transcription -----------------------------------------------------------------------------------------------------------
struct Old {
    int cap_instances = 0; size_t bin_capacity = 0;
    uint32_t high_water = 0; size_t bin_high_water = 0, bin_want = 0;
    int sticky_error = 0; uint32_t sticky_count = 0;
    bool status_pending[kScratchSets] = { false, false, false };
};
static int old_alloc_scratch(Old* t, const Env& env, Outcome& o, int cap, size_t bin_want)
{
    const size_t mi = (size_t)cap;
    size_t bins = ((size_t)1 << 20) * ((mi + 1023) / 1024);
    if (env.cfg.override_bins) { const long v = env.cfg.override_bins; if (v >= 1024) bins = (size_t)v; }
    if (bin_want > bins) bins = bin_want;
    if (!allocate(env, o, cap, bins)) return VR_ERR_OUT_OF_MEMORY;
    t->cap_instances = cap; t->bin_capacity = bins; t->bin_want = bin_want;
    return VR_OK;
}
static int old_reserve_bins(Old* t, const Env& env, Outcome& o, size_t tiles)
{
    const size_t est = tiles * 8;
    if (est <= t->bin_capacity) return VR_OK;
    size_t b = t->bin_capacity ? t->bin_capacity : ((size_t)1 << 20);
    while (b < est) b *= 2;
    return old_alloc_scratch(t, env, o, t->cap_instances, b);
}
static int old_poll(Old* t, const Env& env, Outcome& o, bool report)
{
    uint32_t seen = 0;
    for (int i = 0; i < kScratchSets; i++) {
        if (!t->status_pending[i] || !env.completed[i]) continue;
        t->status_pending[i] = false;
        const uint32_t* st = env.mirror[i];
        const uint32_t flags = st[1], wanted = st[6];
        if (wanted > seen) seen = wanted;
        if ((size_t)st[5] > t->bin_high_water) t->bin_high_water = (size_t)st[5];
        if (flags & 1u) { t->sticky_error = VR_ERR_TOO_MANY_INSTANCES; t->sticky_count = wanted; }
        else if (flags & 6u) { if (!t->sticky_error) t->sticky_error = VR_ERR_OVERFLOW; t->sticky_count = wanted; }
    }
    if (seen > t->high_water) t->high_water = seen;
    const int max_i = env.cfg.max_instances;
    const bool grow_nodes = t->cap_instances < max_i && (size_t)t->high_water * 2 > (size_t)t->cap_instances;
    const bool grow_bins = t->bin_high_water * 2 > t->bin_capacity;
    if (grow_nodes || grow_bins) {
        int want = t->cap_instances;
        while (want < max_i && (size_t)t->high_water * 2 > (size_t)want) want *= 2;
        if (want > max_i) want = max_i;
        size_t bin_want = t->bin_want;
        if (grow_bins) { bin_want = t->bin_capacity; while (bin_want < t->bin_high_water * 2) bin_want *= 2; }
        const int rc = old_alloc_scratch(t, env, o, want, bin_want);
        if (rc) {
            t->bin_want = 0; t->high_water = 0; t->bin_high_water = 0;
            return rc;
        }
    }
    if (report && t->sticky_error) {
        const int e = t->sticky_error;
        t->sticky_error = VR_OK;
        if (e == VR_ERR_TOO_MANY_INSTANCES) o.say(M_EARLIER_TOO_MANY, t->sticky_count);
        else o.say(M_EARLIER_OVERFLOW, t->sticky_count, (size_t)t->cap_instances);
        return e;
    }
    return VR_OK;
}
static int old_read_counters(Old* t, const Env& env, Outcome& o, bool selection_only)
{
    uint32_t c[8];
    memcpy(c, env.counters[env.cur], sizeof(c));
    t->status_pending[env.cur] = false;
    if (c[1] & 1u) { o.say(M_READ_TOO_MANY); return VR_ERR_TOO_MANY_INSTANCES; }
    if ((size_t)c[5] > t->bin_high_water) t->bin_high_water = (size_t)c[5];
    if (c[1] & 2u) {
        (void)old_poll(t, env, o, false);
        o.say(M_READ_LIST_FULL, c[5], t->bin_capacity);
        return VR_ERR_OVERFLOW;
    }
    if (c[1] & 4u) {
        if (c[6] > t->high_water) t->high_water = c[6];
        (void)old_poll(t, env, o, false);
        if (selection_only) return VR_OK;
        t->sticky_error = VR_OK;
        o.say(M_READ_SHORT, (size_t)t->cap_instances);
        return VR_ERR_OVERFLOW;
    }
    return VR_OK;
}

// ---- the header, with vr_select.hip's mechanism around it, and the invariants ----------------------------------------------------
static long g_failures = 0, g_bins_shrank = 0;
static const char* g_where = "";
static void fail(const char* what)
{
    if (g_failures++ < 20) printf("FAIL %s: %s\n", g_where, what);
}
struct Track {
    bool ever_refused = false;      // a poll's growth has been refused at some point of the sequence
    bool outstanding = false;       // a condition has been observed and not reported yet
    bool quiet = false;             // a growth was refused and nothing has been observed, read or reserved since
};
static int new_alloc_scratch(ScratchState& s, Track& k, const Env& env, Outcome& o, int cap, size_t bin_want)
{
    const size_t bins = scratch_bins(cap, env.cfg.override_bins, bin_want);
    if (k.quiet) fail("an allocation was requested after a refusal with nothing new observed");
    if (!allocate(env, o, cap, bins)) return VR_ERR_OUT_OF_MEMORY;
    scratch_allocated(s, cap, bins, bin_want);
    return VR_OK;
}
static int new_poll(ScratchState& s, Track& k, const Env& env, Outcome& o, bool report)
{
    uint32_t needed = 0;            // most nodes, of the frames observed here that stayed within max_instances
    for (int i = 0; i < kScratchSets; i++)
        if (s.pending[i] && env.completed[i]) {
            scratch_observe(s, i, env.mirror[i]);
            k.quiet = false;
            if (env.mirror[i][C_FLAGS] & (kStTooMany | kStListFull | kStScratchShort)) k.outstanding = true;
            if (env.mirror[i][C_WANTED] <= (uint32_t)env.cfg.max_instances && env.mirror[i][C_WANTED] > needed) needed = env.mirror[i][C_WANTED];
        }
    const ScratchGrowth grow = scratch_growth(s, env.cfg.max_instances);
    if (grow.due) {
        const int rc = new_alloc_scratch(s, k, env, o, grow.cap, grow.bin_want);
        if (rc) { scratch_refused(s); k.quiet = k.ever_refused = true; return rc; }
    }
    if ((uint32_t)s.cap_instances < needed) fail("a frame within max_instances was observed and the scratch holds fewer nodes");
    if (!report) return VR_OK;
    const ScratchReport r = scratch_take_report(s);
    if ((r.code != 0) != k.outstanding) fail(r.code ? "a condition was reported a second time" : "an observed condition was not reported");
    k.outstanding = false;
    if (r.code == VR_ERR_TOO_MANY_INSTANCES) o.say(M_EARLIER_TOO_MANY, r.count);
    else if (r.code) o.say(M_EARLIER_OVERFLOW, r.count, (size_t)s.cap_instances);
    return r.code;
}
static int new_read_counters(ScratchState& s, Track& k, const Env& env, Outcome& o, bool selection_only)
{
    const uint32_t* c = env.counters[env.cur];
    const ScratchRead r = scratch_read(s, env.cur, c, selection_only);
    k.quiet = false;
    if (r.poll) (void)new_poll(s, k, env, o, false);
    if (r.drop_report) { (void)scratch_take_report(s); k.outstanding = false; }
    if (r.kind == SCRATCH_READ_TOO_MANY) o.say(M_READ_TOO_MANY);
    else if (r.kind == SCRATCH_READ_LIST_FULL) o.say(M_READ_LIST_FULL, c[C_BINTOTAL], s.bin_capacity);
    else if (r.kind == SCRATCH_READ_SHORT) o.say(M_READ_SHORT, (size_t)s.cap_instances);
    // the read returns its own frame's condition itself - but for a selection alone, which needs no scratch
    const bool own = (c[C_FLAGS] & (kStTooMany | kStListFull)) || ((c[C_FLAGS] & kStScratchShort) && !selection_only);
    if ((r.code != 0) != own) fail("the synchronous read's code does not follow its own status words");
    return r.code;
}
static int new_reserve(ScratchState& s, Track& k, const Env& env, Outcome& o, size_t tiles)
{
    k.quiet = false;
    if (const size_t bins = scratch_reserve(s, tiles)) return new_alloc_scratch(s, k, env, o, s.cap_instances, bins);
    return VR_OK;
}

// ---- events ----------------------------------------------------------------------------------------------------------------------
struct World { Env env; Old o; ScratchState n; Track k; };
constexpr int kFlagValues = 6, kWantedValues = 8, kBinValues = 5, kWords = kFlagValues * kWantedValues * kBinValues;
constexpr int kEvComplete = 0, kEvPoll = kScratchSets * kWords, kEvRead = kEvPoll + 2, kEvReserve = kEvRead + 2, kEvAllocator = kEvReserve + 4,
              kEvents = kEvAllocator + 2;

static void same(const World& w, const Outcome& a, const Outcome& b)
{
    const Old& o = w.o; const ScratchState& n = w.n;
    if (o.cap_instances != n.cap_instances || o.bin_capacity != n.bin_capacity || o.bin_want != n.bin_want || o.high_water != n.high_water
        || o.bin_high_water != n.bin_high_water || o.sticky_error != n.sticky_error || o.sticky_count != n.sticky_count
        || memcmp(o.status_pending, n.pending, sizeof(n.pending)) != 0) fail("the states differ");
    if (a.rc != b.rc) fail("the return codes differ");
    if (a.n_alloc != b.n_alloc || memcmp(a.alloc_cap, b.alloc_cap, sizeof(a.alloc_cap)) != 0 || memcmp(a.alloc_bins, b.alloc_bins, sizeof(a.alloc_bins)) != 0)
        fail("the allocations requested differ");
    if (a.msg != b.msg || a.msg_a != b.msg_a || a.msg_b != b.msg_b) fail("the messages differ");
}

static void apply(World& w, int ev)
{
    Env& env = w.env;
    Outcome a, b;
    const int cap0 = w.n.cap_instances; const size_t bins0 = w.n.bin_capacity;
    if (ev < kEvPoll) {
        // a chain on `set` is queued and completes: its words in the mirror and in the set's counters; it is the current set
        const int set = ev / kWords, r = ev % kWords;
        const uint32_t cap = (uint32_t)w.o.cap_instances, mx = (uint32_t)env.cfg.max_instances;
        const uint64_t bins = w.o.bin_capacity;
        const uint32_t flag_values[kFlagValues] = { 0u, 1u, 2u, 4u, 1u | 2u, 2u | 4u };
        const uint32_t wanted_values[kWantedValues] = { 0u, cap / 2, cap / 2 + 1, cap, cap + 1, 2 * cap + 1, mx, mx + 1 };
        const uint64_t bin_values[kBinValues] = { 0u, bins / 2, bins / 2 + 1, bins + 1, 4 * bins };
        const uint32_t wanted = wanted_values[(r / kBinValues) % kWantedValues];
        const uint64_t total = bin_values[r % kBinValues];
        uint32_t words[kStatusWords] = {};
        words[C_FLAGS] = flag_values[r / (kBinValues * kWantedValues)];
        words[C_WANTED] = wanted; words[C_SELECTED] = wanted < mx ? wanted : mx; words[C_COUNT] = words[C_SELECTED] < cap ? words[C_SELECTED] : cap;
        words[C_BINTOTAL] = total > 0xffffffffull ? 0xffffffffu : (uint32_t)total;        // (the device's counter is a 32-bit word)
        memcpy(env.mirror[set], words, sizeof(words)); memcpy(env.counters[set], words, sizeof(words));
        env.completed[set] = true; env.cur = set;
        w.o.status_pending[set] = true;
        scratch_chain_queued(w.n, set);
    } else if (ev < kEvRead) {
        a.rc = old_poll(&w.o, env, a, ev - kEvPoll != 0);
        b.rc = new_poll(w.n, w.k, env, b, ev - kEvPoll != 0);
    } else if (ev < kEvReserve) {
        a.rc = old_read_counters(&w.o, env, a, ev - kEvRead != 0);
        b.rc = new_read_counters(w.n, w.k, env, b, ev - kEvRead != 0);
    } else if (ev < kEvAllocator) {
        const size_t per8 = w.o.bin_capacity / 8, tile_values[4] = { 0, per8, per8 + 1, w.o.bin_capacity };
        a.rc = old_reserve_bins(&w.o, env, a, tile_values[ev - kEvReserve]);
        b.rc = new_reserve(w.n, w.k, env, b, tile_values[ev - kEvReserve]);
    } else env.alloc_ok = ev - kEvAllocator == 0;
    same(w, a, b);
    // the capacities, on the header's side alone
    const bool refused = b.n_alloc > 0 && !env.alloc_ok;
    if (w.n.cap_instances < cap0 || w.n.cap_instances > env.cfg.max_instances) fail("the node capacity fell, or passed max_instances");
    if (refused && (w.n.cap_instances != cap0 || w.n.bin_capacity != bins0)) fail("a refused growth changed a capacity");
    if (w.n.bin_capacity < bins0) {
        // FINDING (the transcription does the same): a refusal forgets the bin request, so the next growth of the nodes allocates
        // the floor again even where the bins had grown beyond it - the next reserve or bin high-water mark grows them back
        if (w.k.ever_refused) g_bins_shrank++; else fail("the bin capacity fell without a refusal before it");
    }
}

static World start(const Config& cfg)
{
    World w;
    w.env.cfg = cfg;
    Outcome a, b;                   // vr_terrain_create: alloc_scratch(initial, 0)
    (void)old_alloc_scratch(&w.o, w.env, a, cfg.initial, 0);
    (void)new_alloc_scratch(w.n, w.k, w.env, b, cfg.initial, 0);
    same(w, a, b);
    return w;
}

int main()
{
    // max_instances 1, a maximum that is no power of two, 4096; from one node, from the maximum, from the default 1024 (which create
    // clamps to the maximum: distinct only under 4096); without and with VR_SCRATCH_INITIAL_BINS
    const int shapes[6][2] = { { 1, 1 }, { 1000, 1 }, { 1000, 1000 }, { 4096, 1 }, { 4096, 4096 }, { 4096, 1024 } };
    long sequences = 0;
    char where[256];
    g_where = where;
    uint64_t rng = 0x9e3779b97f4a7c15ull;
    auto next = [&rng](uint32_t n) { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return (uint32_t)((rng >> 33) % n); };
    for (const auto& shape : shapes)
        for (int with_override = 0; with_override < 2; with_override++) {
            const long override_bins = with_override ? 4096 : 0;
            const Config cfg = { shape[0], shape[1], override_bins };
            const World w0 = start(cfg);
            // every sequence of one and of two events
            for (int e1 = 0; e1 < kEvents; e1++) {
                World w1 = w0;
                snprintf(where, sizeof(where), "max %d initial %d bins %ld: event %d", cfg.max_instances, cfg.initial, cfg.override_bins, e1);
                apply(w1, e1); sequences++;
                for (int e2 = 0; e2 < kEvents; e2++) {
                    World w2 = w1;
                    snprintf(where, sizeof(where), "max %d initial %d bins %ld: events %d %d", cfg.max_instances, cfg.initial, cfg.override_bins, e1, e2);
                    apply(w2, e2); sequences++;
                }
            }
            // longer ones: 3..16 events, the kind of event drawn first so that polls, reads and refusals are as frequent as chains
            for (int q = 0; q < 20000; q++) {
                World w = w0;
                const int len = 3 + (int)next(14);
                int n = snprintf(where, sizeof(where), "max %d initial %d bins %ld: events", cfg.max_instances, cfg.initial, cfg.override_bins);
                for (int i = 0; i < len; i++) {
                    const int first[5] = { kEvComplete, kEvPoll, kEvRead, kEvReserve, kEvAllocator }, count[5] = { kEvPoll, 2, 2, 4, 2 };
                    const uint32_t kind = next(5);
                    const int ev = first[kind] + (int)next((uint32_t)count[kind]);
                    if (n < (int)sizeof(where) - 8) n += snprintf(where + n, sizeof(where) - (size_t)n, " %d", ev);
                    apply(w, ev);
                }
                sequences++;
            }
        }
    printf("bin capacity fell after an earlier refusal (finding, as transcribed): %ld times\n", g_bins_shrank);
    printf("%ld sequences, %ld failures\n", sequences, g_failures);
    return g_failures ? 1 : 0;
}
