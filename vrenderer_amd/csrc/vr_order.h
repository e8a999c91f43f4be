// Who waits for whom between a terrain's two geometry streams, the context's stream and a tone mapper's stream.  Plain C++17:
// no HIP, no library types - a CPU program replays every short sequence of API calls against a transcription of the code this
// replaced and against a happens-before model of the streams (tests/host/order_check.cpp).  Stream and Event are opaque
// handles (Event{} = none); every operation on them goes through the caller's `ops` (vr_internal.h wraps HIP's three calls):
//
//   ops.record(event, stream) -> int      the event completes once everything queued on the stream so far has
//   ops.wait(stream, event)   -> int      what is queued on the stream from now on runs behind the event's last record
//   ops.sync(event)           -> int      the HOST waits for the event's last record (the side resources alone, below)
//
// A non-zero result ends the step and is returned; 0 otherwise.
//
// What is ordered.  A geometry set (three rotate) is written by a CHAIN on a geometry stream - select or a lock_view copy of
// another set's selection, then vertices and bins - and read by one TILE PASS on the context's stream.  A stand-alone select
// is a chain that writes the selection only.  Every select reads the node heights, which the context's stream writes.  An HDR
// image is written by the lighting pass (or the fused tile pass) on the context's stream and read by a tone-map stage that
// may run on another stream.  The steps, in the order a frame takes them:
//
//   order_begin_chain       a new writer of a set: takes the next geometry stream (the two take turns) and queues on it the waits
//                           for everything that still uses the set - its previous chain (which may have run on the other stream
//                           and may never have been consumed), a lock_view copy out of it, the tile pass that last read it, and
//                           what the context's stream did to the terrain.  Single-stream mode (VR_OPT_ASYNC_GEOMETRY off) first
//                           records that last dependency, so the chain runs behind everything queued so far.
//   order_copy_selection    lock_view: the chain takes its selection from the set of the last unlocked frame, whose select ran
//                           on that set's stream; the source's next writer must not overtake the copies.
//   order_end_chain         the set's chain mark.
//   order_prepare_start,    vr_terrain_prepare: the chain starts behind the start hint (below); afterwards the context's stream
//   order_prepare_wait      waits for it NOW if it is the only prepared one, else behind the next tile pass (order_wait_ahead) -
//                           never in front of the tile pass that consumes it, never earlier than it has to.
//   order_tile_pass_begin   the tile pass waits for the set's chain unless a wait queued at prepare time sits on this very
//                           stream (a host may change the context's stream in between), and leaves the start hint: "the
//                           context's stream has reached this tile pass" - the stop event of whatever was stamped last on the
//                           stream, or an explicit record.  A HINT: it says when a chain becomes runnable; a wrong event there
//                           costs time, never correctness.
//   order_tile_pass_launched, order_wait_ahead
//                           the set's tile-pass mark (what its next chain waits for), then the waits that prepare deferred.
//   order_terrain_changing, order_terrain_changed
//                           around a write of the node heights on the context's stream: behind every chain queued so far (a
//                           select may still be reading them), and every set's next chain behind the write.
//   order_terrain_tables_changing
//                           in front of a write of the maps themselves (vr_terrain_edit), with order_terrain_changing: behind
//                           every set's tile pass, which reads the maps' tables.
//   order_image_writer_begins / _written / _reader_done
//                           the pass that writes an image waits for the stage that still reads it; the stage on another stream
//                           waits for the pass's own stop event (or an explicit record); the image remembers the stage.
//
// SIDE RESOURCES.  Memory a terrain keeps beside its maps, whose kernels all run on the context's stream of the moment - the
// query pyramid, the history journal's arena, the brush's and the erosions' buffers (dab lists, snapshot, block of planes).  One
// event and the stream of its last record each (OrderSide); three steps:
//
//   order_side_begin        in front of a kernel that touches the resource: behind its last user if that ran on another stream
//                           (the host changed the context's stream in between; on the same stream the stream orders it)
//   order_side_end          behind the kernel: the event moves there
//   order_side_idle         the one wait on the HOST: nothing queued can still touch the resource - in front of a free or a
//                           growth, or of the host's next write into pinned memory a queued copy reads
#pragma once

#include "vr_events.h"

#include <stddef.h>
#include <stdint.h>

#define VR_ORDER_TRY(expr) do { const int rc_ = (expr); if (rc_) return rc_; } while (0)

// A point on a stream that others may wait for: the stop event a launch's dispatch stamped, as the handle vr_events.h gave out
// for it (such a handle denotes its launch only until the event's source reissues it; what a wait does afterwards is that
// header's rule, events_wait_needed), or this mark's own event, recorded explicitly (always valid).  Unset until the first of either.
template <class Event> struct OrderMark {
    Event own{};             // created and destroyed by the owner of the mark
    EventRef<Event> at;
    bool set = false;
};
template <class Event> void order_mark_stamped(OrderMark<Event>& m, const EventRef<Event>& stop) { m.at = stop; m.set = true; }
template <class Event, class Stream, class Ops> int order_mark_record(OrderMark<Event>& m, const Ops& ops, Stream s)
{
    VR_ORDER_TRY(ops.record(m.own, s));
    m.at = { m.own, 0, 0 }; m.set = true;
    return 0;
}
// the stamped stop event if there is one, else a record
template <class Event, class Stream, class Ops> int order_mark_here(OrderMark<Event>& m, const Ops& ops, Stream s, const EventRef<Event>& stop)
{
    if (stop.ev != Event{}) { order_mark_stamped(m, stop); return 0; }
    return order_mark_record(m, ops, s);
}
template <class Event, class Stream, class Ops> int order_mark_wait(const OrderMark<Event>& m, const Ops& ops, Stream s, const EventSupply<Event>& events)
{
    if (!m.set || !events_wait_needed(events, m.at)) return 0;
    return ops.wait(s, m.at.ev);
}

// A reader that nobody has waited for yet.
template <class Event> struct OrderPending {
    Event ev{};
    bool pending = false;
};
template <class Event, class Stream, class Ops> int order_pending_record(OrderPending<Event>& p, const Ops& ops, Stream s)
{
    VR_ORDER_TRY(ops.record(p.ev, s));
    p.pending = true;
    return 0;
}
template <class Event, class Stream, class Ops> int order_pending_wait(OrderPending<Event>& p, const Ops& ops, Stream s)
{
    if (!p.pending) return 0;
    VR_ORDER_TRY(ops.wait(s, p.ev));
    p.pending = false;
    return 0;
}

template <class Stream, class Event> struct OrderSet {
    Stream stream{};                    // the geometry stream the set's last chain ran on
    OrderMark<Event> chain;             // the last chain (always this set's own event)
    OrderMark<Event> tile_pass;         // the tile pass that last read the set
    OrderPending<Event> sel_read;       // a lock_view copy OUT of this set, on the copying set's stream
    OrderPending<Event> main_dep;       // the context's stream changed the terrain; `ev` is the terrain's one event (OrderTerrain::ev_changed)
    bool main_waited = false;           // the context's stream already waits for the chain (order_prepare_wait, order_wait_ahead) ...
    Stream main_wait_stream{};          // ... on this stream; the wait only counts for the stream that holds it
};
template <class Event> struct OrderTerrain {
    Event ev_changed{};                 // the context's stream changed the terrain (shared by the sets' main_dep)
    Event ev_sel_ready{};               // lock_view: the source set's selection is complete
    OrderMark<Event> hint;              // the start hint: the context's stream reached the last tile pass
};
template <class Event> struct OrderImage {
    OrderMark<Event> written;           // (own event: made by the first frame that needs it)
    OrderPending<Event> read_done;
};

// `single_stream`: the chain is part of a frame and VR_OPT_ASYNC_GEOMETRY is off.  (A set whose status slot the host has not read
// yet - ScratchState::pending - would be waited for here, too.)
template <class Stream, class Event, class Ops>
int order_begin_chain(OrderTerrain<Event>& t, OrderSet<Stream, Event>& g, const Ops& ops, const Stream (&geo_streams)[2], unsigned& turn,
                      Stream main, bool single_stream, const EventSupply<Event>& events)
{
    g.stream = geo_streams[turn++ & 1u];
    g.main_waited = false;
    if (single_stream) {
        VR_ORDER_TRY(ops.record(t.ev_changed, main));
        g.main_dep.pending = true;
    }
    VR_ORDER_TRY(order_mark_wait(g.chain, ops, g.stream, events));
    VR_ORDER_TRY(order_pending_wait(g.sel_read, ops, g.stream));
    VR_ORDER_TRY(order_mark_wait(g.tile_pass, ops, g.stream, events));
    return order_pending_wait(g.main_dep, ops, g.stream);
}

// copy() -> int queues the copies on dst's stream
template <class Stream, class Event, class Ops, class Copy>
int order_copy_selection(OrderTerrain<Event>& t, OrderSet<Stream, Event>& dst, OrderSet<Stream, Event>& src, const Ops& ops, Copy&& copy)
{
    VR_ORDER_TRY(ops.record(t.ev_sel_ready, src.stream));
    VR_ORDER_TRY(ops.wait(dst.stream, t.ev_sel_ready));
    VR_ORDER_TRY(copy());
    return order_pending_record(src.sel_read, ops, dst.stream);
}

template <class Stream, class Event, class Ops> int order_end_chain(OrderSet<Stream, Event>& g, const Ops& ops)
{
    return order_mark_record(g.chain, ops, g.stream);
}

// in front of order_begin_chain: on the stream it takes next
template <class Stream, class Event, class Ops>
int order_prepare_start(const OrderTerrain<Event>& t, const Ops& ops, const Stream (&geo_streams)[2], unsigned turn, const EventSupply<Event>& events)
{
    return order_mark_wait(t.hint, ops, geo_streams[turn & 1u], events);
}
template <class Stream, class Event, class Ops>
int order_prepare_wait(OrderSet<Stream, Event>& g, const Ops& ops, Stream main, bool other_prepared)
{
    g.main_waited = false;
    if (other_prepared) return 0;
    VR_ORDER_TRY(ops.wait(main, g.chain.own));
    g.main_waited = true; g.main_wait_stream = main;
    return 0;
}

// `prepared`: the set's chain was built ahead by vr_terrain_prepare; `hint`: events_start_hint - the stop event of the most recent
// stamped launch on the stream if such events serve as dependencies (VR_OPT_DISPATCH_EVENTS) and there is one, else none
template <class Stream, class Event, class Ops>
int order_tile_pass_begin(OrderTerrain<Event>& t, OrderSet<Stream, Event>& g, const Ops& ops, Stream main, bool prepared, const EventRef<Event>& hint)
{
    if (!(prepared && g.main_waited && g.main_wait_stream == main)) VR_ORDER_TRY(ops.wait(main, g.chain.own));
    g.main_waited = false;
    return order_mark_here(t.hint, ops, main, hint);
}
// `stop`: the pass's own dispatch-stamped stop event (events_stop), none if it was not stamped (or nothing was launched)
template <class Stream, class Event, class Ops>
int order_tile_pass_launched(OrderSet<Stream, Event>& g, const Ops& ops, Stream main, const EventRef<Event>& stop)
{
    return order_mark_here(g.tile_pass, ops, main, stop);
}
// for every OTHER set that holds a prepared frame, behind the tile pass
template <class Stream, class Event, class Ops> int order_wait_ahead(OrderSet<Stream, Event>& p, const Ops& ops, Stream main)
{
    if ((p.main_waited && p.main_wait_stream == main) || !p.chain.set) return 0;
    VR_ORDER_TRY(ops.wait(main, p.chain.own));
    p.main_waited = true; p.main_wait_stream = main;
    return 0;
}

template <class Stream, class Event, class Ops, size_t N>
int order_terrain_changing(OrderSet<Stream, Event>* const (&sets)[N], const Ops& ops, Stream main)
{
    for (OrderSet<Stream, Event>* g : sets) if (g->chain.set) VR_ORDER_TRY(ops.wait(main, g->chain.own));
    return 0;
}
template <class Stream, class Event, class Ops, size_t N>
int order_terrain_changed(OrderTerrain<Event>& t, OrderSet<Stream, Event>* const (&sets)[N], const Ops& ops, Stream main)
{
    VR_ORDER_TRY(ops.record(t.ev_changed, main));
    for (OrderSet<Stream, Event>* g : sets) g->main_dep.pending = true;
    return 0;
}

// A write of the maps' tables on the context's stream (vr_terrain_edit), next to order_terrain_changing: behind every set's tile
// pass, which reads them - on whatever stream the context had when that pass was queued.
template <class Stream, class Event, class Ops, size_t N>
int order_terrain_tables_changing(OrderSet<Stream, Event>* const (&sets)[N], const Ops& ops, Stream main, const EventSupply<Event>& events)
{
    for (OrderSet<Stream, Event>* g : sets) VR_ORDER_TRY(order_mark_wait(g->tile_pass, ops, main, events));
    return 0;
}

template <class Stream, class Event, class Ops> int order_image_writer_begins(OrderImage<Event>& im, const Ops& ops, Stream writer)
{
    return order_pending_wait(im.read_done, ops, writer);
}
// the writing pass has been launched on `writer` and a stage on ANOTHER stream reads next; `stop` as in order_tile_pass_launched
template <class Stream, class Event, class Ops>
int order_image_written(OrderImage<Event>& im, const Ops& ops, Stream writer, Stream reader, const EventRef<Event>& stop, const EventSupply<Event>& events)
{
    VR_ORDER_TRY(order_mark_here(im.written, ops, writer, stop));
    return order_mark_wait(im.written, ops, reader, events);
}
template <class Stream, class Event, class Ops> int order_image_reader_done(OrderImage<Event>& im, const Ops& ops, Stream reader)
{
    return order_pending_record(im.read_done, ops, reader);
}

template <class Stream, class Event> struct OrderSide {
    Event ev{};              // created and destroyed by the owner of the resource
    Stream stream{};         // where `ev` was last recorded
    bool queued = false;     // a record of `ev` that the host has not waited for
};
template <class Stream, class Event, class Ops> int order_side_begin(const OrderSide<Stream, Event>& r, const Ops& ops, Stream s)
{
    return r.queued && s != r.stream ? ops.wait(s, r.ev) : 0;
}
template <class Stream, class Event, class Ops> int order_side_end(OrderSide<Stream, Event>& r, const Ops& ops, Stream s)
{
    VR_ORDER_TRY(ops.record(r.ev, s));
    r.stream = s; r.queued = true;
    return 0;
}
template <class Stream, class Event, class Ops> int order_side_idle(OrderSide<Stream, Event>& r, const Ops& ops)
{
    if (r.queued) VR_ORDER_TRY(ops.sync(r.ev));
    r.queued = false;
    return 0;
}
