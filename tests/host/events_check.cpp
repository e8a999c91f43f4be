// Check of the launch-event supplier (vrenderer_amd/csrc/vr_events.h) against a counting fake of its ops, over fixed-seed random
// sequences of its transitions - a scope taken (recorded around the launch or stamped by its dispatch, on the context's stream
// or another), launched, ended; timing enabled at every level the API accepts; collect; VR_OPT_DISPATCH_EVENTS toggled; the
// context's stream changed - with creations, stream synchronisations and elapsed-time queries that fail now and then.  A ring
// of 4 and pools made ahead of 3 / 2 events, so that reuse, recycling and creation on demand all happen within a few steps.
// Held after every step:
//   - no event is in two places at once among the pool, the ring and (the recorded pairs + the live scopes' pooled pairs), and
//     every event ever created is in one of them;
//   - a recorded pair, once no scope is live, has been recorded or stamped since the last recycle (a scope that ends without a
//     launch leaves no never-recorded pair);
//   - a failed creation leaves the launch without events and the places as they were;
//   - collect returns exactly the pairs committed since the last recycle, less the ones whose query failed, and recycles on that
//     path too; a failed stream synchronisation changes nothing;
//   - a handle is live exactly until the pool is recycled (pooled) or its event is handed to another launch (ring).
// At the end of a sequence every event created is destroyed exactly once.
// Plain C++17, no GPU: g++ -std=c++17 -Wall -Werror -I vrenderer_amd/csrc tests/host/events_check.cpp
#include "vr_events.h"

#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>

static long cases = 0, failures = 0;
#define EXPECT(cond, what) do { if (!(cond)) { if (failures++ < 10) printf("FAIL: %s (%s:%d), sequence %ld\n", what, __FILE__, __LINE__, cases); } } while (0)

constexpr int kIds = 5;
struct Fake {
    int next = 1, fail_create_in = -1, fail_elapsed_in = -1;
    bool fail_sync = false;
    long now = 1;
    std::map<int, int> created, destroyed;
    std::map<int, long> stamped_at;
    bool create(int* e) { if (fail_create_in >= 0 && fail_create_in-- == 0) return false; *e = next++; created[*e]++; return true; }
    void destroy(int e) { destroyed[e]++; }
    void record(int e, int) { stamped_at[e] = now; }
    int sync_stream(int) { return fail_sync ? 7 : 0; }
    int sync_event(int) { return 0; }
    int elapsed(float* ms, int, int) { if (fail_elapsed_in >= 0 && fail_elapsed_in-- == 0) return 9; *ms = 1.0f; return 0; }
};
struct Ops { Fake* f;
    bool create(int* e) const { return f->create(e); } void destroy(int e) const { f->destroy(e); } void record(int e, int s) const { f->record(e, s); }
    int sync_stream(int s) const { return f->sync_stream(s); } int sync_event(int e) const { return f->sync_event(e); }
    int elapsed(float* ms, int a, int b) const { return f->elapsed(ms, a, b); } };

struct Handle { EventRef<int> ref; long recycles; long tag; };
struct Run {
    Fake f; Ops ops{ &f };
    EventSupply<int> s;
    std::vector<EventPair<int, int>> live;
    std::vector<Handle> handles;
    std::map<int, long> owner;            // event -> tag of the take that last handed it out
    long tags = 0, recycles = 0, last_recycle_at = 0;
    int expected[kIds] = {};              // pairs committed since the last recycle, per id
    int main = 1;
    uint64_t x;
    uint64_t rnd() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; }

    std::map<int, int> places() const
    {
        std::map<int, int> n;
        for (int e : s.pool) n[e]++;
        for (const auto& sl : s.ring) n[sl.ev]++;
        std::map<int, int> held;
        for (const auto& p : s.recorded) { held[p.begin] = 1; held[p.end] = 1; }
        for (const auto& p : live) if (p.from == p.POOL) { held[p.begin] = 1; held[p.end] = 1; }
        for (const auto& h : held) n[h.first]++;
        return n;
    }
    void invariants()
    {
        const std::map<int, int> n = places();
        for (const auto& c : f.created) {
            const auto it = n.find(c.first);
            EXPECT(it != n.end(), "an event is in no place");
            EXPECT(it == n.end() || it->second == 1, "an event is in two places at once");
        }
        EXPECT(n.size() == f.created.size(), "a place holds an event that was never created");
        for (const auto& p : s.recorded) {
            EXPECT(p.begin != p.end && p.id >= 0 && p.id < kIds, "a recorded pair is malformed");
            bool scope_live = false;
            for (const auto& l : live) scope_live |= l.from == l.POOL && l.end == p.end;
            if (!scope_live) EXPECT(f.stamped_at[p.begin] > last_recycle_at && f.stamped_at[p.end] > last_recycle_at, "a never-recorded pair in the collect list");
        }
        for (const Handle& h : handles) {
            const bool want = h.ref.slot == 0 ? h.recycles == recycles : owner[h.ref.ev] == h.tag;
            EXPECT(events_live(s, h.ref) == want, "a handle's liveness");
            EXPECT(events_wait_needed(s, h.ref) == (h.ref.slot != 0 || want), "what a wait on a handle does");
        }
        const EventRef<int> own{ 1000, 0, 0 };
        EXPECT(events_live(s, own) && events_wait_needed(s, own), "an own event is always live");
        EXPECT(s.last_stop.ev == 0 || events_live(s, s.last_stop) || s.last_stop.slot != 0, "the start hint outlived a recycle");
    }
    void recycled() { recycles++; last_recycle_at = f.now; for (int& e : expected) e = 0; }

    void take()
    {
        // (at most one scope whose dispatch stamps its pair is open at a time, as in the library: a ring of 4 is two such launches)
        bool dispatch_open = false;
        for (const auto& l : live) dispatch_open |= l.by_dispatch;
        const bool by_dispatch = (rnd() & 1) && !dispatch_open, fail = rnd() % 8 == 0;
        const int stream = rnd() % 4 ? main : 3, id = (int)(rnd() % kIds);
        const std::map<int, int> before = places();
        const size_t recorded_before = s.recorded.size();
        if (fail) f.fail_create_in = (int)(rnd() % 2);
        const long created_before = (long)f.created.size();
        EventPair<int, int> p = events_take(s, ops, id, stream, by_dispatch);
        const bool create_failed = f.fail_create_in == -1 && fail;       // the armed failure was consumed
        f.fail_create_in = -1;
        if (create_failed) {
            EXPECT(p.from == p.NONE && !p.stamps() && p.begin == 0 && p.end == 0, "a failed creation left the launch with events");
            EXPECT(s.recorded.size() == recorded_before, "a failed creation committed a pair");
            std::map<int, int> after = places();
            for (const auto& b : before) EXPECT(after[b.first] == b.second, "a failed creation moved an event");
            EXPECT((long)after.size() - (long)before.size() == (long)f.created.size() - created_before, "a failed creation lost an event");
        }
        const bool pooled = s.timing == 1 || (s.timing == 2 && by_dispatch);
        if (!create_failed) EXPECT((p.from == p.POOL) == pooled && (p.from == p.RING) == (!pooled && by_dispatch && s.dispatch_events), "the source of a pair");
        if (p.from != p.NONE) {
            const long tag = ++tags;
            owner[p.begin] = tag; owner[p.end] = tag;
            if (p.from == p.POOL && !by_dispatch) expected[id]++;
            EXPECT(p.stop.ev == p.end, "the stop handle is not the end event");
        }
        live.push_back(p);
    }
    void launch()
    {
        if (live.empty()) return;
        EventPair<int, int>& p = live[rnd() % live.size()];
        if (!p.stamps() || p.launched) return;
        f.stamped_at[p.begin] = f.stamped_at[p.end] = f.now;              // the dispatch stamps both
        events_launched(s, p, main);
        if (p.from == p.POOL) expected[p.id]++;
        const EventRef<int> stop = events_stop(s, p);
        EXPECT((stop.ev != 0) == s.dispatch_events, "a launched scope's stop event");
        if (stop.ev) handles.push_back({ stop, recycles, owner[stop.ev] });
        if (p.stream == main) EXPECT(s.last_stop.ev == p.end, "the start hint is not the last stamped launch on the context's stream");
    }
    void release(size_t i)
    {
        EXPECT(events_stop(s, live[i]).ev == 0 || live[i].launched, "a stop event without a launch");
        events_release(s, ops, live[i]);
        live.erase(live.begin() + (long)i);
    }
    void enable()
    {
        const int level = (int)(rnd() % 5) - 1;
        f.fail_sync = rnd() % 8 == 0;
        const uint64_t epoch = s.epoch; const size_t n = s.recorded.size(); const int timing = s.timing;
        const int rc = events_timing_enable(s, ops, main, level);
        if (f.fail_sync) EXPECT(rc == 7 && s.epoch == epoch && s.recorded.size() == n && s.timing == timing, "a failed synchronise changed the state (enable)");
        else {
            EXPECT(rc == 0 && s.epoch == epoch + 1 && s.recorded.empty() && s.last_stop.ev == 0, "enable did not recycle");
            EXPECT(s.timing == (level < 0 ? 0 : level > 2 ? 1 : level), "the timing level");
            EXPECT(s.pool.size() >= s.precreate[s.timing], "the pool was not made ahead");
            recycled();
        }
        f.fail_sync = false;
    }
    void collect()
    {
        float ms[kIds]; int32_t launches[kIds];
        for (int i = 0; i < kIds; i++) { ms[i] = -1.0f; launches[i] = -1; }
        f.fail_sync = rnd() % 8 == 0;
        const bool fail_query = !f.fail_sync && !s.recorded.empty() && rnd() % 4 == 0;
        int failed_id = -1;
        if (fail_query) { f.fail_elapsed_in = (int)(rnd() % s.recorded.size()); failed_id = s.recorded[(size_t)f.fail_elapsed_in].id; }
        const uint64_t epoch = s.epoch; const size_t n = s.recorded.size();
        const int rc = events_collect(s, ops, main, ms, launches, kIds);
        f.fail_elapsed_in = -1;
        if (f.fail_sync) EXPECT(rc == 7 && s.epoch == epoch && s.recorded.size() == n && launches[0] == -1, "a failed synchronise changed the state (collect)");
        else {
            EXPECT(rc == (fail_query ? 9 : 0), "collect's code");
            for (int i = 0; i < kIds; i++) {
                EXPECT(launches[i] == expected[i] - (i == failed_id), "collect's launch counts are not the pairs committed since the last recycle");
                EXPECT(ms[i] == (float)launches[i], "collect's sums");
            }
            EXPECT(s.epoch == epoch + 1 && s.recorded.empty() && s.last_stop.ev == 0, "collect did not recycle");
            recycled();
        }
        f.fail_sync = false;
    }
    void dispatch_toggle()
    {
        f.fail_sync = rnd() % 8 == 0;
        const bool was = s.dispatch_events;
        const int rc = events_set_dispatch(s, ops, main, !was);
        if (f.fail_sync) EXPECT(rc == 7 && s.dispatch_events == was, "a failed synchronise changed the state (option)");
        else EXPECT(rc == 0 && s.dispatch_events == !was && s.last_stop.ev == 0 && events_start_hint(s).ev == 0, "the option's toggle");
        f.fail_sync = false;
    }
    void run(uint64_t seed, int steps)
    {
        x = seed * 0x9E3779B97F4A7C15ull + 1;
        s.ring_size = 4; s.precreate[1] = 3; s.precreate[2] = 2;
        for (int k = 0; k < steps; k++) {
            f.now++;
            const unsigned r = (unsigned)(rnd() % 16);
            if (r < 5 && live.size() < 3) take();
            else if (r < 9) launch();
            else if (r < 13) { if (!live.empty()) release(rnd() % live.size()); }
            else if (!live.empty()) release(0);                       // the calls below are API calls: no scope is open across one
            else if (r == 13) enable();
            else if (r == 14) collect();
            else if (rnd() & 1) dispatch_toggle();
            else main = main == 1 ? 2 : 1;
            invariants();
        }
        while (!live.empty()) release(0);
        invariants();
        events_destroy(s, ops);
        EXPECT(s.pool.empty() && s.ring.empty() && s.recorded.empty(), "teardown left events behind");
        for (const auto& c : f.created) EXPECT(c.second == 1 && f.destroyed[c.first] == 1, "an event was not destroyed exactly once");
        EXPECT(f.destroyed.size() == f.created.size(), "teardown destroyed an event that was never created");
    }
};

int main()
{
    for (int k = 0; k < 20000; k++) { cases++; Run r; r.run((uint64_t)k + 1, 60); }
    printf("%ld cases, %ld failures\n", cases, failures);
    return failures ? 1 : 0;
}
