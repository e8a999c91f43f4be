// The journal behind vr_terrain_undo / vr_terrain_redo: where a record lies in the device arena, how its rows are laid out, which
// records form a step, and what is given up when the budget is short.  Plain C++17: no HIP, no library types - a CPU program drives
// these functions with random operation sequences against a model that keeps whole copies of the maps and places records by an
// occupancy map of its own (tests/host/history_check.cpp).  vr_history.hip keeps the mechanism: the arena, the two kernels, the
// event behind them and the refresh (vr_derive_level0_write); it takes every offset, pitch and range from here.
//
//   record   one write of a rectangle of level 0 of a map (vr_terrain_edit, vr_terrain_brush): (which, rectangle) and the
//            rectangle's bytes as they were before the write - after an undo, as they were after it (the swap kernel exchanges
//            record and map, so one copy serves both directions).
//   layout   rows `pitch` bytes apart, pitch a multiple of 16; a row's first byte lies `head` = (x0 * texel_bytes) mod 16 bytes
//            into its pitch.  Record offsets are multiples of 16 and the arena is aligned far beyond that, so a record byte and the
//            map byte it mirrors have the same address modulo 16 whenever the map's row pitch is a multiple of 16 (every map of a
//            power-of-two width): the interior of a row then moves as aligned 16-byte vectors on both sides.  Any other map row is
//            moved element by element (vr_history.hip decides per row, from the addresses).
//   ring     records lie in the arena in the order they were made, each contiguous; one that does not fit behind the newest starts
//            again at offset 0 (the bytes behind the newest stay unused until the records in front of them have gone).
//   steps    records join the open step; commit closes it.  The cursor `cur` divides the closed steps into those undo can apply
//            (in front, pre-images) and those redo can apply (behind, post-images).  A new record discards everything behind the
//            cursor.
//   budget   room is made by dropping the oldest closed steps whole.  If that is not enough - the open step alone fills the arena
//            or the record table, or the record is larger than the arena - nothing can be restored across the change that is about
//            to happen unrecorded: every step is dropped, the open step is lost and records nothing more until commit.
//            dropped_steps counts every step given up, the lost one included.
//   cap      the record table holds kHistoryMaxRecords records, reserved at enable; a full table is treated like a full arena.
#pragma once

#include <stdint.h>

#include "vr_dirty.h"

constexpr uint32_t kHistoryMaxRecords = 4096;
constexpr uint32_t kHistoryAlign = 16;

// ---- record layout ----
inline uint32_t history_row_head(int x0, int texel_bytes) { return (uint32_t)(((uint64_t)x0 * (uint64_t)texel_bytes) & (kHistoryAlign - 1)); }
inline uint64_t history_row_pitch(int x0, int w, int texel_bytes)
{
    const uint64_t end = history_row_head(x0, texel_bytes) + (uint64_t)w * (uint64_t)texel_bytes;
    return (end + (kHistoryAlign - 1)) & ~(uint64_t)(kHistoryAlign - 1);
}
inline uint64_t history_record_bytes(const DirtyRect& r, int texel_bytes)
{
    return dirty_empty(r) ? 0 : history_row_pitch(r.x0, r.x1 - r.x0, texel_bytes) * (uint64_t)(r.y1 - r.y0);
}

struct HistoryRecord {
    DirtyRect r;                 // of level 0
    uint64_t off = 0, bytes = 0; // in the arena; both multiples of 16
    uint32_t pitch = 0;          // bytes between two rows
    uint8_t which = 0;           // 0 heightmap, 1 albedo
    uint8_t texel_bytes = 1;
    uint8_t head = 0;            // a row's first byte inside its pitch
    uint8_t step_first = 0;      // the first record of its step
};

struct HistoryState {
    uint64_t budget = 0;                 // bytes of the arena (0: history is off)
    HistoryRecord* rec = nullptr;        // table of `cap` records, a ring addressed by the counters below modulo cap
    uint32_t cap = 0;
    uint64_t first = 0, cur = 0, last = 0;      // live records: [first, last); applied: [first, cur); undone: [cur, last)
    uint32_t undo_steps = 0, redo_steps = 0;    // closed steps in front of / behind the cursor
    uint32_t open_records = 0;                  // the open step: the last open_records of [first, cur) (then cur == last)
    uint32_t dropped_steps = 0;
    bool open_lost = false;                     // the open step could not be kept: nothing is recorded until commit
    uint64_t bytes_used = 0;                    // sum of the live records' bytes
};

inline HistoryRecord& history_at(const HistoryState& s, uint64_t i) { return s.rec[i % s.cap]; }

// enable: an empty journal over `budget` bytes and a table of `cap` records (budget == 0: off)
inline void history_reset(HistoryState& s, uint64_t budget, HistoryRecord* table, uint32_t cap)
{
    s = HistoryState();
    s.budget = budget; s.rec = table; s.cap = budget ? cap : 0;
}

// where a record of n bytes (a multiple of 16) can go without touching a live one; the live records are left alone
inline bool history_place(const HistoryState& s, uint64_t n, uint64_t* off)
{
    if (n > s.budget || s.last - s.first >= s.cap) return false;
    if (s.first == s.last) { *off = 0; return true; }
    const HistoryRecord& oldest = history_at(s, s.first), & newest = history_at(s, s.last - 1);
    const uint64_t tail = oldest.off, head = newest.off + newest.bytes;
    if (newest.off >= oldest.off) {                  // the live bytes are [tail, head)
        if (n <= s.budget - head) { *off = head; return true; }
        if (n <= tail) { *off = 0; return true; }    // wrap
        return false;
    }
    if (n <= tail - head) { *off = head; return true; }      // wrapped already: the free bytes are [head, tail)
    return false;
}

inline void history_discard_redo(HistoryState& s)
{
    while (s.last > s.cur) { s.last--; s.bytes_used -= history_at(s, s.last).bytes; }
    s.redo_steps = 0;
}
// the oldest closed step in front of the cursor (undo_steps > 0)
inline void history_drop_oldest(HistoryState& s)
{
    do { s.bytes_used -= history_at(s, s.first).bytes; s.first++; } while (s.first < s.cur && !history_at(s, s.first).step_first);
    s.undo_steps--; s.dropped_steps++;
}
inline void history_lose_open(HistoryState& s)
{
    while (s.undo_steps) history_drop_oldest(s);
    while (s.last > s.first) { s.last--; s.bytes_used -= history_at(s, s.last).bytes; }
    s.cur = s.last; s.open_records = 0; s.open_lost = true; s.dropped_steps++;
}

// A write of `r` (not empty) is about to happen.  true: *out is the record that must capture the rectangle first.  false: the
// write goes unrecorded (history off, or the open step is lost).
inline bool history_append(HistoryState& s, int which, const DirtyRect& r, int texel_bytes, HistoryRecord* out)
{
    if (!s.budget) return false;
    history_discard_redo(s);
    if (s.open_lost) return false;
    const uint64_t n = history_record_bytes(r, texel_bytes);
    uint64_t off = 0;
    while (!history_place(s, n, &off)) {
        if (n <= s.budget && s.undo_steps) { history_drop_oldest(s); continue; }
        history_lose_open(s);
        return false;
    }
    HistoryRecord& e = history_at(s, s.last);
    e.r = r; e.off = off; e.bytes = n; e.pitch = (uint32_t)history_row_pitch(r.x0, r.x1 - r.x0, texel_bytes);
    e.which = (uint8_t)which; e.texel_bytes = (uint8_t)texel_bytes; e.head = (uint8_t)history_row_head(r.x0, texel_bytes);
    e.step_first = s.open_records == 0;
    s.last++; s.cur = s.last; s.open_records++; s.bytes_used += n;
    *out = e;
    return true;
}

inline void history_commit(HistoryState& s)
{
    if (s.open_records) { s.undo_steps++; s.open_records = 0; }
    s.open_lost = false;
}

// The newest closed step in front of the cursor: its records are [*lo, *hi), to be swapped NEWEST FIRST (hi - 1 down to lo).
inline bool history_undo(HistoryState& s, uint64_t* lo, uint64_t* hi)
{
    history_commit(s);
    if (!s.undo_steps) return false;
    uint64_t a = s.cur - 1;
    while (!history_at(s, a).step_first) a--;
    *lo = a; *hi = s.cur;
    s.cur = a; s.undo_steps--; s.redo_steps++;
    return true;
}
// The oldest step behind the cursor: its records are [*lo, *hi), to be swapped OLDEST FIRST.
inline bool history_redo(HistoryState& s, uint64_t* lo, uint64_t* hi)
{
    history_commit(s);
    if (!s.redo_steps) return false;
    uint64_t b = s.cur + 1;
    while (b < s.last && !history_at(s, b).step_first) b++;
    *lo = s.cur; *hi = b;
    s.cur = b; s.undo_steps++; s.redo_steps--;
    return true;
}
