// A terrain's per-frame scratch: how large it is, when it grows and how a frame that outgrew it is reported.  Plain C++17: no HIP,
// no getenv, no error strings - a CPU program drives these functions and a transcription of the code they replaced through the
// same event sequences (tests/host/scratch_check.cpp).  vr_select.hip keeps the mechanism: event queries, the allocation
// (alloc_scratch -> vr_grow_group), the environment reads and the messages.
//
// Vertices, triangle records and bins are sized for cap_instances nodes, not for max_instances (4096: 1.7 GB per geometry set,
// of which an 8K frame's ~300 nodes use a few percent).  Every chain leaves its status words in a pinned host mirror (k_fill's
// first act); the next API call observes the mirrors of the chains that have completed and grows the scratch BEFORE a frame can
// exceed it.  A frame that does exceed it - the count more than doubled within three frames - is drawn without the excess and
// reported like the other device-side conditions: once, by the next vr_terrain_render.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/vrterrain.h"

// ---- status words: the contract between k_select, k_scan, k_fill and the host ------------------------------------------------
// A geometry set's counters[]; the first kStatusWords are what k_fill mirrors to the host.  C_HARDTRIS..C_BINTOTAL and the
// classes are reset by k_vertex, the first kernel of a chain that uses them; C_COUNT, C_FLAGS, C_WANTED and C_SELECTED are k_select's.
enum {
    C_COUNT = 0,        // nodes the chain draws: min(C_SELECTED, the scratch's capacity)
    C_FLAGS = 1,        // kSt* bits
    C_HARDTRIS = 2,     // the clipper's sub-triangles
    C_XVERTS = 3,       // the clipper's extra vertices
    C_HARDLIST = 4,     // triangles handed to the clipper
    C_BINTOTAL = 5,     // (triangle, tile) pairs the frame wanted
    C_WANTED = 6,       // nodes selected before any truncation
    C_SELECTED = 7,     // what NodeSelect returns: min(C_WANTED, max_instances)
    C_CLASS0 = 8,       // 8..15: raster tiles per bin-length class (k_scan)
    C_END = 16
};
constexpr int kStatusWords = 8;
constexpr uint32_t kStTooMany = 1u;        // more than max_instances nodes selected
constexpr uint32_t kStListFull = 2u;       // a work list (frontier, clipper, bins) was full: triangles or nodes were dropped
constexpr uint32_t kStScratchShort = 4u;   // more nodes than the scratch held (and no more than max_instances)

constexpr int kScratchSets = 3;            // == kGeoSets (vr_geosets.h)

struct ScratchState {
    int cap_instances = 0;                 // nodes the scratch holds (<= max_instances)
    size_t bin_capacity = 0;               // bin entries it holds
    size_t bin_want = 0;                   // the bin request of the last allocation: kept across a growth of the nodes alone
    uint32_t high_water = 0;               // most nodes an observed frame selected
    size_t bin_high_water = 0;             // most bin entries an observed frame wanted
    int sticky_error = 0;                  // VR_ERR_* of an observed frame, not yet reported
    uint32_t sticky_count = 0;             // that frame's C_WANTED
    bool pending[kScratchSets] = { false, false, false };   // the set's last chain has not been observed yet
};

inline void scratch_chain_queued(ScratchState& s, int set) { s.pending[set] = true; }

// The status words of a completed chain (the mirror, or a copy).  kStTooMany replaces whatever is waiting to be reported; the two
// overflow bits set the code only if none is waiting, and the count either way.
inline void scratch_observe(ScratchState& s, int set, const volatile uint32_t* w)
{
    s.pending[set] = false;
    const uint32_t flags = w[C_FLAGS], wanted = w[C_WANTED];
    if (wanted > s.high_water) s.high_water = wanted;
    if ((size_t)w[C_BINTOTAL] > s.bin_high_water) s.bin_high_water = (size_t)w[C_BINTOTAL];
    if (flags & kStTooMany) { s.sticky_error = VR_ERR_TOO_MANY_INSTANCES; s.sticky_count = wanted; }
    else if (flags & (kStListFull | kStScratchShort)) { if (!s.sticky_error) s.sticky_error = VR_ERR_OVERFLOW; s.sticky_count = wanted; }
}

// Grow before a frame can outgrow the scratch: nodes and bins alike to twice the largest figure seen, once that passes half the
// capacity.  (A scratch never has zero nodes or bins: scratch_bins.)
struct ScratchGrowth { bool due; int cap; size_t bin_want; };
inline ScratchGrowth scratch_growth(const ScratchState& s, int max_instances)
{
    const bool grow_nodes = s.cap_instances < max_instances && (size_t)s.high_water * 2 > (size_t)s.cap_instances;
    const bool grow_bins = s.bin_high_water * 2 > s.bin_capacity;
    if (!grow_nodes && !grow_bins) return { false, s.cap_instances, s.bin_want };
    int cap = s.cap_instances;
    while (cap < max_instances && (size_t)s.high_water * 2 > (size_t)cap) cap *= 2;
    if (cap > max_instances) cap = max_instances;
    size_t bin_want = s.bin_want;
    if (grow_bins) { bin_want = s.bin_capacity; while (bin_want < s.bin_high_water * 2) bin_want *= 2; }
    return { true, cap, bin_want };
}

// Bin entries of an allocation for `cap` nodes.  (triangle, tile) pairs: an 8K frame of ~300 nodes has ~0.3 M, a 1080p frame
// ~0.6 M; 1 M per 1024 nodes and never fewer - or `override_bins` (VR_SCRATCH_INITIAL_BINS; tests force the growth path with it),
// or what the frames seen so far asked for (a large target on 32-pixel tiles: every triangle lands in more bins).
inline size_t scratch_bins(int cap, long override_bins, size_t bin_want)
{
    size_t bins = ((size_t)1 << 20) * (((size_t)cap + 1023) / 1024);
    if (override_bins >= 1024) bins = (size_t)override_bins;
    return bin_want > bins ? bin_want : bins;
}

inline void scratch_allocated(ScratchState& s, int cap, size_t bins, size_t bin_want)
{
    s.cap_instances = cap; s.bin_capacity = bins; s.bin_want = bin_want;
}
// scratch_growth's request did not fit: the old scratch is still there (frames that need more stay truncated and reported), and
// nothing is asked for again until a new frame has been observed.
inline void scratch_refused(ScratchState& s) { s.bin_want = 0; s.high_water = 0; s.bin_high_water = 0; }

// A target of `tiles` raster tiles is about to be drawn: room for ~8 bin entries per tile up front (measured: 9.3 per tile at 8K,
// 5.9 at 15360x8640, 4.7 at 16384^2 - the terrain's triangles grow with the frame, the tiles do not), so that the first frame on
// a very large target does not have to overflow before the bins grow.  0: it fits; else the bin request of an allocation for
// cap_instances nodes.  (A refusal of that one changes nothing here: the next frame asks again.)
inline size_t scratch_reserve(const ScratchState& s, size_t tiles)
{
    const size_t est = tiles * 8;
    if (est <= s.bin_capacity) return 0;
    size_t b = s.bin_capacity ? s.bin_capacity : ((size_t)1 << 20);
    while (b < est) b *= 2;
    return b;
}

// What is waiting to be reported (code 0: nothing), taken: it is not reported again.
struct ScratchReport { int code; uint32_t count; };
inline ScratchReport scratch_take_report(ScratchState& s)
{
    const ScratchReport r = { s.sticky_error, s.sticky_count };
    s.sticky_error = VR_OK;
    return r;
}

// The current set's counters as a synchronous copy shows them (vr_terrain_num_chunks, vr_terrain_select with outputs).  The
// caller then, in this order: polls if `poll` (the growth happens now, so that rendering the frame again is complete), takes and
// drops the pending report if `drop_report`, sets the message of `kind`, returns `code`.  Where this differs from
// scratch_observe of the same words - all three as the code it replaced:
//   - the set counts as observed BEFORE that poll, which therefore does not see these words a second time: a condition this read
//     returns is not also made sticky;
//   - kStTooMany returns at once and moves no mark (scratch_observe raises high_water even then);
//   - the pending report is dropped only for kStScratchShort outside selection_only - after the poll, so another set's condition
//     observed by it goes too; a full work list leaves it, and so does selection_only, which returns VR_OK (a selection alone
//     needs no scratch) and whose condition is reported by nobody.
enum ScratchReadKind { SCRATCH_READ_OK, SCRATCH_READ_TOO_MANY, SCRATCH_READ_LIST_FULL, SCRATCH_READ_SHORT };
struct ScratchRead { ScratchReadKind kind; int code; bool poll, drop_report; };
inline ScratchRead scratch_read(ScratchState& s, int set, const uint32_t* w, bool selection_only)
{
    s.pending[set] = false;
    if (w[C_FLAGS] & kStTooMany) return { SCRATCH_READ_TOO_MANY, VR_ERR_TOO_MANY_INSTANCES, false, false };
    if ((size_t)w[C_BINTOTAL] > s.bin_high_water) s.bin_high_water = (size_t)w[C_BINTOTAL];
    if (w[C_FLAGS] & kStListFull) return { SCRATCH_READ_LIST_FULL, VR_ERR_OVERFLOW, true, false };
    if (w[C_FLAGS] & kStScratchShort) {
        if (w[C_WANTED] > s.high_water) s.high_water = w[C_WANTED];
        if (selection_only) return { SCRATCH_READ_OK, VR_OK, true, false };
        return { SCRATCH_READ_SHORT, VR_ERR_OVERFLOW, true, true };
    }
    return { SCRATCH_READ_OK, VR_OK, false, false };
}
