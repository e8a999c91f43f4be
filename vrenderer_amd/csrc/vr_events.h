// Where a launch's start / stop events come from, and for how long a handle to one denotes its launch.  Plain C++17, no HIP:
// tests/host/events_check.cpp drives the transitions against a counting fake of the ops, and tests/host/order_check.cpp takes
// its events from here with a ring of 4.  Event and Stream are opaque handles (Event{} = none); the HIP work goes through
// the caller's `ops` (vr_host.hip): create(Event*) -> bool (false leaves *out alone), destroy(event), record(event, stream),
// and sync_stream(stream), sync_event(event), elapsed(float* ms, begin, end) -> int, non-zero being the code to return.
//
// TWO SOURCES.  While timing is on (level 1: every launch, a record on either side; level 2: only the launches whose dispatch
// stamps its own events) a pair comes from the POOL and, once something will stamp it, enters the list that collect reads.
// Otherwise a stamped launch takes two slots of the RING if its stop event serves as a dependency (dispatch_events), and an
// unstamped one takes nothing.  (One dispatch-stamped scope is open at a time: a ring holds ring_size / 2 launches.)
//
// ONE HANDLE, ONE RULE.  A stop event that leaves here as a dependency is an EventRef.  It is LIVE - it denotes the launch it was
// handed out for - until its source gives the event to another launch: a pooled one until the epoch advances (the pool is
// recycled), a ring one until its slot is issued again.  A wait on a handle that is no longer live (events_wait_needed):
//   pooled  does nothing.  Both recyclers synchronise the context's stream and every recorded end first: the launch is complete.
//   ring    waits, for the slot's new occupant.  That is never too little: only launches on the context's stream are stamped, and
//           a host that moves the context to another stream orders that stream behind the old one (the contract of
//           vr_context_set_stream), so the new occupant was queued behind the old one.  order_check holds every reissue to
//           that and pins a sequence with such a wait across a stream change.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <vector>

// serial 0: the holder's own event, always live.  slot 0: pooled, serial = its epoch.  Else ring slot `slot - 1` and its issue serial.
template <class Event> struct EventRef {
    Event ev{};
    uint32_t slot = 0;
    uint64_t serial = 0;
};

template <class Event> struct EventSupply {
    size_t ring_size = 64;               // events, two per stamped launch
    size_t precreate[3] = { 0, 8192, 2048 };   // pool size events_timing_enable fills up to, by level
    int timing = 0;                      // 0 off, 1 every kernel (two event records each), 2 only the launches whose events the dispatch stamps
    // VR_OPT_DISPATCH_EVENTS: the stop events of stamped launches double as the cross-stream dependencies (tile pass done -> its set
    // is free; lighting pass done -> the next frame's geometry may start): no event-record packets between a frame's two big kernels
    bool dispatch_events = true;
    std::vector<Event> pool;             // reusable events
    struct Slot { Event ev{}; uint64_t serial = 0; };
    std::vector<Slot> ring; size_t ring_pos = 0; uint64_t ring_serial = 0;
    struct Pair { Event begin{}, end{}; int id = 0; };
    std::vector<Pair> recorded;          // what collect reads: every pair something stamps or has stamped, since the last recycle
    uint64_t epoch = 1;                  // advanced whenever the pool is recycled
    EventRef<Event> last_stop;           // events_start_hint
};

// One launch's pair, between events_take and events_release.
template <class Event, class Stream> struct EventPair {
    enum From : uint8_t { NONE, POOL, RING };
    Event begin{}, end{};
    EventRef<Event> stop;                // `end` as a dependency
    Stream stream{};
    int id = 0;
    From from = NONE;
    bool by_dispatch = false, committed = false, launched = false;
    bool stamps() const { return from != NONE && by_dispatch; }    // the launch passes begin / end to the dispatch
};

template <class Event> bool events_live(const EventSupply<Event>& s, const EventRef<Event>& r)
{
    if (r.serial == 0) return true;
    return r.slot == 0 ? r.serial == s.epoch : s.ring[r.slot - 1].serial == r.serial;
}
// (the rule at the top)
template <class Event> bool events_wait_needed(const EventSupply<Event>& s, const EventRef<Event>& r) { return r.slot != 0 || events_live(s, r); }

template <class Event, class Ops> Event events_pool_take(EventSupply<Event>& s, const Ops& ops)
{
    Event e{};
    if (!s.pool.empty()) { e = s.pool.back(); s.pool.pop_back(); }
    else if (!ops.create(&e)) return Event{};
    return e;
}
template <class Event, class Ops> EventRef<Event> events_ring_take(EventSupply<Event>& s, const Ops& ops)
{
    size_t at = s.ring.size();
    if (at < s.ring_size) {
        Event e{};
        if (!ops.create(&e)) return {};
        s.ring.push_back({ e, 0 });
    } else { at = s.ring_pos; s.ring_pos = (s.ring_pos + 1) % s.ring_size; }
    s.ring[at].serial = ++s.ring_serial;
    return { s.ring[at].ev, (uint32_t)at + 1, s.ring_serial };
}

// A pair for launch `id` on `stream`.  by_dispatch: the launch hands the pair to the dispatch, which stamps it - no extra packets
// between two dependent kernels on the stream; else the begin event is recorded here and the end event by events_release, at
// level 1 alone: two records around each of a frame's dozen small kernels make a loop with a ~110 us frame period host-bound.
// A failed creation leaves the launch without events (from == NONE).
template <class Event, class Stream, class Ops>
EventPair<Event, Stream> events_take(EventSupply<Event>& s, const Ops& ops, int id, Stream stream, bool by_dispatch)
{
    EventPair<Event, Stream> p;
    p.stream = stream; p.id = id; p.by_dispatch = by_dispatch;
    if (s.timing == 1 || (s.timing == 2 && by_dispatch)) {
        p.begin = events_pool_take(s, ops); p.end = events_pool_take(s, ops);
        if (p.begin == Event{} || p.end == Event{}) {
            if (p.begin != Event{}) s.pool.push_back(p.begin);
            if (p.end != Event{}) s.pool.push_back(p.end);
            p.begin = p.end = Event{};
            return p;
        }
        p.from = p.POOL; p.stop = { p.end, 0, s.epoch };
        // the pair enters the list only once something will stamp it: here, or when the dispatch has been issued
        if (!by_dispatch) { ops.record(p.begin, stream); s.recorded.push_back({ p.begin, p.end, id }); p.committed = true; }
    } else if (by_dispatch && s.dispatch_events) {
        const EventRef<Event> b = events_ring_take(s, ops), e = events_ring_take(s, ops);
        if (b.ev == Event{} || e.ev == Event{}) return p;
        p.from = p.RING; p.begin = b.ev; p.end = e.ev; p.stop = e;
    }
    return p;
}
// the dispatch that stamps the pair has been issued; `main`: the context's stream of the moment
template <class Event, class Stream> void events_launched(EventSupply<Event>& s, EventPair<Event, Stream>& p, Stream main)
{
    if (p.from == p.POOL && !p.committed) { s.recorded.push_back({ p.begin, p.end, p.id }); p.committed = true; }
    p.launched = true;
    if (p.stream == main) s.last_stop = p.stop;
}
// the scope ends: the closing record, or - the dispatch was never issued - the pair goes back instead of staying a never-recorded one
template <class Event, class Stream, class Ops> void events_release(EventSupply<Event>& s, const Ops& ops, EventPair<Event, Stream>& p)
{
    if (p.from == p.POOL) {
        if (!p.by_dispatch) ops.record(p.end, p.stream);
        else if (!p.committed) { s.pool.push_back(p.begin); s.pool.push_back(p.end); }
    }
    p.from = p.NONE;
}
// this launch's own stop event where such events serve as dependencies; none: not stamped, or no launch
template <class Event, class Stream> EventRef<Event> events_stop(const EventSupply<Event>& s, const EventPair<Event, Stream>& p)
{ return p.launched && s.dispatch_events ? p.stop : EventRef<Event>{}; }
// The stop event of the most recent stamped launch on the context's stream.  ONE permitted use: the start hint of the next prepared
// chain (order_tile_pass_begin), where a wrong event costs time and not correctness.  It says nothing about which launch it
// belongs to: a pass that others must wait for hands out its own stop event (events_stop).
template <class Event> EventRef<Event> events_start_hint(const EventSupply<Event>& s) { return s.dispatch_events ? s.last_stop : EventRef<Event>{}; }

// every handle to a pooled event taken before this point is stale now
template <class Event> void events_recycle(EventSupply<Event>& s)
{
    s.epoch++;
    s.last_stop = {};
    for (const auto& p : s.recorded) { s.pool.push_back(p.begin); s.pool.push_back(p.end); }
    s.recorded.clear();
}
// `level` as the caller gave it: below 0 is off, above 2 is 1
template <class Event, class Stream, class Ops> int events_timing_enable(EventSupply<Event>& s, const Ops& ops, Stream main, int level)
{
    if (const int rc = ops.sync_stream(main)) return rc;
    // pairs recorded on a terrain's geometry stream may still be pending: wait for each before its events are recycled
    for (const auto& p : s.recorded) (void)ops.sync_event(p.end);
    events_recycle(s);
    s.timing = level < 0 ? 0 : (level > 2 ? 1 : level);
    // events for the launches to come are made HERE, not one by one inside the host's frame loop (a creation per stamped
    // launch was ~20 us of a rank's ~100 us of host time per frame): enough for a few hundred frames, more are made on demand
    while (s.pool.size() < s.precreate[s.timing]) {
        Event e{};
        if (!ops.create(&e)) break;
        s.pool.push_back(e);
    }
    return 0;
}
// ms_sum[id], launches[id] (n_ids each) over every pair committed since the last recycle.  A failing query's code is returned behind
// the rest, and the list is recycled on that path too: a bad pair must not persist
template <class Event, class Stream, class Ops>
int events_collect(EventSupply<Event>& s, const Ops& ops, Stream main, float* ms_sum, int32_t* launches, int n_ids)
{
    if (const int rc = ops.sync_stream(main)) return rc;
    for (int i = 0; i < n_ids; i++) { ms_sum[i] = 0.0f; launches[i] = 0; }
    int rc = 0;
    for (const auto& p : s.recorded) {
        float ms = 0.0f;
        int e = ops.sync_event(p.end);                   // may have been recorded on a terrain's geometry stream
        if (!e) e = ops.elapsed(&ms, p.begin, p.end);
        if (e) { rc = e; continue; }
        ms_sum[p.id] += ms; launches[p.id]++;
    }
    events_recycle(s);
    return rc;
}
template <class Event, class Stream, class Ops> int events_set_dispatch(EventSupply<Event>& s, const Ops& ops, Stream main, bool on)
{
    if (const int rc = ops.sync_stream(main)) return rc;
    s.dispatch_events = on; s.last_stop = {};
    return 0;
}
template <class Event, class Ops> void events_destroy(EventSupply<Event>& s, const Ops& ops)
{
    events_recycle(s);
    for (Event e : s.pool) ops.destroy(e);
    for (const auto& sl : s.ring) ops.destroy(sl.ev);
    s.pool.clear(); s.ring.clear(); s.ring_pos = 0;
}
