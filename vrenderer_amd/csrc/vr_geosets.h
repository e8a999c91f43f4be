// A terrain's three geometry sets: which set a call gets.  Plain C++17: no HIP - a CPU program drives these transitions and a
// transcription of the code they replaced through the same event sequences (tests/host/geosets_check.cpp), and the model of the
// sets' stream order takes its slot policy from here (tests/host/order_check.cpp).  The .hip files keep the mechanism - the
// chains, the tile pass, the ordering calls around each transition - and only read this state; every write is a function below.
//
// One set is CURRENT: the set of the most recent select or render.  A tile pass in flight may be reading it and lock_view copies
// its selection, so no build ever goes to it.  The other two are built ahead by vr_terrain_prepare (PREPARED: geometry for
// exactly one key, waiting for the render that names that key), rebuilt by a render that found nothing prepared, or taken by a
// stand-alone select.
//
// INVARIANT: !slot[cur].prepared.  A set becomes prepared only through geoslots_prepared, on a set geoslots_pick chose, and the
// pick is never `cur`; a set becomes current only through geoslots_current, behind the geoslots_claim that took its prepared
// frame; GeoBorrow puts back a `cur` that was current before, and the borrowed pass - a render - prepares nothing.  So there is
// ONE find rule, over all sets: vr_terrain_prepare (is this frame prepared already?) and the render (is there a set prepared for
// this frame, other than the one the last tile pass reads?) ask the same question.
//
// have_selection only rises: a selection lives in the part of a set that no invalidation and no regrowth of the scratch touches.
#pragma once

#include <stdint.h>
#include <string.h>

#include "../../include/vrterrain.h"

constexpr int kGeoSets = 3;

// Key: what a prepared frame was built for (the product's is GeoKey; a model may use an int)
template <class Key> struct GeoSlots {
    struct Slot {
        bool prepared = false;           // holds geometry built ahead for exactly `key`
        bool have_selection = false;
        uint64_t serial = 0;             // order of the geoslots_prepared calls (the oldest prepared set is evicted first)
        Key key{};
    };
    Slot slot[kGeoSets];
    int cur = 0;                         // set of the most recent select / render
    uint64_t counter = 0;
};

// "Prepared for exactly this frame": everything the geometry chain's output depends on.  The whole view bytewise, of the render
// parameters max_height, depth_only and wireframe as a truth value - assume_cleared, depth_ranges and lock_view change the tile
// pass alone - and the target, the partition and the raster tile edge (VR_OPT_RASTER_TILE may change in between: the bins are
// per tile size).
struct GeoKey {
    vr_view view;
    float max_height;
    int32_t depth_only, wireframe;
    int w, h, rank, world, tile_shift;
};
inline GeoKey geo_key(const vr_view& view, const vr_render_params& rp, int w, int h, int rank, int world, int tile_shift)
{
    return { view, rp.max_height, rp.depth_only, rp.wireframe, w, h, rank, world, tile_shift };
}
inline bool operator==(const GeoKey& a, const GeoKey& b)
{
    return memcmp(&a.view, &b.view, sizeof(vr_view)) == 0 && a.max_height == b.max_height && a.depth_only == b.depth_only
        && !a.wireframe == !b.wireframe && a.w == b.w && a.h == b.h && a.rank == b.rank && a.world == b.world && a.tile_shift == b.tile_shift;
}

// The set the next select / geometry build goes to: never the current one; among the others one that holds no prepared frame,
// else the one prepared longest ago.
template <class Key> int geoslots_pick(const GeoSlots<Key>& s)
{
    int best = -1;
    for (int i = 0; i < kGeoSets; i++) {
        if (i == s.cur) continue;
        if (!s.slot[i].prepared) return i;
        if (best < 0 || s.slot[i].serial < s.slot[best].serial) best = i;
    }
    return best;
}
// the set prepared for `key`, or -1
template <class Key> int geoslots_find(const GeoSlots<Key>& s, const Key& key)
{
    for (int i = 0; i < kGeoSets; i++)
        if (s.slot[i].prepared && s.slot[i].key == key) return i;
    return -1;
}
// set i is taken - a build into it begins, or a tile pass consumes what was prepared in it: its prepared frame is gone
template <class Key> void geoslots_claim(GeoSlots<Key>& s, int i) { s.slot[i].prepared = false; }
// set i holds a prepared frame for `key` (the one place the counter moves)
template <class Key> void geoslots_prepared(GeoSlots<Key>& s, int i, const Key& key)
{
    s.slot[i].prepared = true; s.slot[i].key = key; s.slot[i].serial = ++s.counter;
}
template <class Key> void geoslots_selected(GeoSlots<Key>& s, int i) { s.slot[i].have_selection = true; }
template <class Key> void geoslots_current(GeoSlots<Key>& s, int i) { s.cur = i; }
// is a frame prepared in any set but i (what order_prepare_wait is told)
template <class Key> bool geoslots_other_prepared(const GeoSlots<Key>& s, int i)
{
    bool other = false;
    for (int p = 0; p < kGeoSets; p++) other |= p != i && s.slot[p].prepared;
    return other;
}
// where a render's build takes its selection from: the current set under lock_view if it holds one, else -1 (a new select)
template <class Key> int geoslots_selection_source(const GeoSlots<Key>& s, bool lock_view)
{
    return lock_view && s.slot[s.cur].have_selection ? s.cur : -1;
}
// every prepared frame is stale (the maps, the node heights or the scratch changed); selections and `cur` stay
template <class Key> void geoslots_invalidate(GeoSlots<Key>& s)
{
    for (int i = 0; i < kGeoSets; i++) s.slot[i].prepared = false;
}
// A borrowed pass: the render that vr_gbuffer_materialise_planes runs for a frame of the past.  It picks and claims a set like
// any render - the oldest prepared frame may be evicted for it - but the terrain's current set stays the one it was, whatever the
// pass returned, and the set it borrowed is left unprepared.
template <class Key> struct GeoBorrow {
    GeoSlots<Key>& s; const int cur;
    explicit GeoBorrow(GeoSlots<Key>& slots) : s(slots), cur(slots.cur) {}
    ~GeoBorrow() { s.cur = cur; }
    GeoBorrow(const GeoBorrow&) = delete;
    GeoBorrow& operator=(const GeoBorrow&) = delete;
};
