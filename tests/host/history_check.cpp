// vr_history.h against a naive model, on the CPU.  The model is a list of steps; every step keeps WHOLE copies of both maps from
// before and after it, and places its records by an occupancy map of the arena (try behind the newest record, then offset 0, else
// give up the oldest step).  The header's records are played through a byte array that stands for the device arena: capture and
// swap are the obvious loops over the layout the header hands out (offset, pitch, head).  Random sequences of append / commit /
// undo / redo / enable over a 4 KB arena (and a 24-record table, so that the cap is reached), rectangles from 1 x 1 to a whole map
// of 4800 bytes - larger than the arena.  After every operation:
//   - live records lie inside the arena (none straddles its end), are 16-byte aligned and do not overlap;
//   - pitch is a multiple of 16, head == x0 * tb mod 16, the row fits its pitch, bytes == pitch * rows;
//   - the header's record list is the model's (which, rectangle, offset, in order) and bytes_used, undo_steps, redo_steps,
//     open_records and dropped_steps equal the model's;
//   - after undo / redo the two maps equal the model's whole copies, byte for byte.
// Prints the counts of the paths reached (each must be non-zero), the case count and "N failures".
//
//   history_check            the run above
//   history_check size x0 w h tb     prints history_record_bytes of that rectangle (the GPU tests size their arenas with it)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "vr_history.h"

static int failures = 0;
static long cases = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures < 20) { printf("FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } failures++; } } while (0)

struct Rng {
    uint64_t s;
    uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
    int below(int n) { return (int)(next() % (uint32_t)n); }
};

constexpr int kMapW[2] = { 80, 40 }, kMapH[2] = { 60, 30 }, kTb[2] = { 1, 4 };
constexpr uint32_t kTable = 24;
struct Maps { std::vector<uint8_t> m[2]; bool operator==(const Maps& o) const { return m[0] == o.m[0] && m[1] == o.m[1]; } };

struct MRec { int which; DirtyRect r; uint64_t off, bytes; };
struct MStep { std::vector<MRec> recs; Maps before, after; };
struct Model {
    uint64_t budget = 0;
    std::vector<MStep> steps; size_t cursor = 0;      // steps[0, cursor) can be undone, steps[cursor, ..) redone
    MStep open; bool lost = false;
    uint32_t dropped = 0;
    std::vector<MRec> live() const
    {
        std::vector<MRec> v;
        for (const MStep& s : steps) v.insert(v.end(), s.recs.begin(), s.recs.end());
        v.insert(v.end(), open.recs.begin(), open.recs.end());
        return v;
    }
};
struct Reached { long wraps = 0, drops = 0, redo_discards = 0, lost = 0, oversize = 0, table_full = 0, undos = 0, redos = 0, recorded = 0; };

static uint64_t model_bytes(const DirtyRect& r, int tb)
{
    const uint64_t head = ((uint64_t)r.x0 * tb) % 16, row = head + (uint64_t)(r.x1 - r.x0) * tb;
    return (row + 15) / 16 * 16 * (uint64_t)(r.y1 - r.y0);
}
// the model's placement: an occupancy map, behind the newest record first, offset 0 second
static bool model_place(const Model& m, uint64_t n, uint64_t* off, bool* wrapped, bool* table_full)
{
    const std::vector<MRec> lv = m.live();
    *table_full = lv.size() >= kTable;
    if (*table_full) return false;
    std::vector<uint8_t> used(m.budget, 0);
    for (const MRec& e : lv) for (uint64_t b = e.off; b < e.off + e.bytes; b++) used[b] = 1;
    const uint64_t head = lv.empty() ? 0 : lv.back().off + lv.back().bytes;
    const uint64_t cand[2] = { head, 0 };
    for (int c = 0; c < 2; c++) {
        if (cand[c] + n > m.budget) continue;
        bool free_ = true;
        for (uint64_t b = cand[c]; b < cand[c] + n && free_; b++) free_ = !used[b];
        if (free_) { *off = cand[c]; *wrapped = c == 1 && !lv.empty() && head != 0; return true; }
    }
    return false;
}

// the device's two kernels as loops over the arena
static void move_rect(const HistoryRecord& e, std::vector<uint8_t>& arena, Maps& maps, bool swap)
{
    const int tb = e.texel_bytes, mw = kMapW[e.which];
    const size_t row_bytes = (size_t)(e.r.x1 - e.r.x0) * tb;
    for (int y = e.r.y0; y < e.r.y1; y++)
        for (size_t b = 0; b < row_bytes; b++) {
            const size_t a = e.off + (size_t)(y - e.r.y0) * e.pitch + e.head + b;
            CHECK(a < arena.size(), "arena index %zu of %zu", a, arena.size());
            if (a >= arena.size()) return;
            uint8_t& mb = maps.m[e.which][((size_t)y * mw + e.r.x0) * tb + b];
            const uint8_t was = mb;
            if (swap) mb = arena[a];
            arena[a] = was;
        }
}

static void check_state(const HistoryState& s, const Model& m, const char* op)
{
    const std::vector<MRec> lv = m.live();
    CHECK(s.last - s.first == lv.size(), "%s: %llu live records, the model has %zu", op, (unsigned long long)(s.last - s.first), lv.size());
    uint64_t used = 0;
    for (const MRec& e : lv) used += e.bytes;
    CHECK(s.bytes_used == used, "%s: bytes_used %llu, model %llu", op, (unsigned long long)s.bytes_used, (unsigned long long)used);
    CHECK(s.undo_steps == m.cursor, "%s: undo_steps %u, model %zu", op, s.undo_steps, m.cursor);
    CHECK(s.redo_steps == m.steps.size() - m.cursor, "%s: redo_steps %u, model %zu", op, s.redo_steps, m.steps.size() - m.cursor);
    CHECK(s.open_records == m.open.recs.size(), "%s: open_records %u, model %zu", op, s.open_records, m.open.recs.size());
    CHECK(s.dropped_steps == m.dropped, "%s: dropped_steps %u, model %u", op, s.dropped_steps, m.dropped);
    CHECK(s.open_lost == m.lost, "%s: open_lost %d, model %d", op, (int)s.open_lost, (int)m.lost);
    if (s.last - s.first != lv.size()) return;
    for (uint64_t i = s.first; i < s.last; i++) {
        const HistoryRecord& e = history_at(s, i);
        const MRec& w = lv[i - s.first];
        const int tb = kTb[e.which];
        CHECK(e.which == w.which && e.r.x0 == w.r.x0 && e.r.y0 == w.r.y0 && e.r.x1 == w.r.x1 && e.r.y1 == w.r.y1 && e.off == w.off && e.bytes == w.bytes,
              "%s: record %llu is not the model's (offset %llu / %llu)", op, (unsigned long long)i, (unsigned long long)e.off, (unsigned long long)w.off);
        CHECK(e.off % 16 == 0 && e.bytes % 16 == 0 && e.off + e.bytes <= s.budget, "%s: record [%llu, +%llu) of %llu", op, (unsigned long long)e.off, (unsigned long long)e.bytes, (unsigned long long)s.budget);
        CHECK(e.pitch % 16 == 0 && e.head == ((uint64_t)e.r.x0 * tb) % 16 && e.texel_bytes == tb, "%s: pitch %u head %u", op, e.pitch, e.head);
        CHECK((uint64_t)e.head + (uint64_t)(e.r.x1 - e.r.x0) * tb <= e.pitch && e.bytes == (uint64_t)e.pitch * (e.r.y1 - e.r.y0), "%s: a row does not fit its pitch", op);
        for (uint64_t k = i + 1; k < s.last; k++) {
            const HistoryRecord& o = history_at(s, k);
            CHECK(e.off + e.bytes <= o.off || o.off + o.bytes <= e.off, "%s: records %llu and %llu overlap", op, (unsigned long long)i, (unsigned long long)k);
        }
    }
}

static void run(uint64_t seed, long ops, Reached& hit)
{
    Rng rng{ seed };
    Maps maps;
    for (int k = 0; k < 2; k++) { maps.m[k].resize((size_t)kMapW[k] * kMapH[k] * kTb[k]); for (uint8_t& b : maps.m[k]) b = (uint8_t)rng.next(); }
    std::vector<HistoryRecord> table(kTable);
    std::vector<uint8_t> arena;
    HistoryState s;
    Model m;
    auto enable = [&](uint64_t budget) {
        history_reset(s, budget, table.data(), kTable);
        arena.assign(budget, 0xEE);
        m = Model(); m.budget = budget;
    };
    auto model_commit = [&]() {
        if (!m.open.recs.empty()) { m.open.after = maps; m.steps.push_back(m.open); m.cursor++; m.open = MStep(); }
        m.lost = false;
    };
    enable(4096);
    for (long i = 0; i < ops; i++, cases++) {
        const int p = rng.below(100);
        const char* op = "append";
        if (p < 56) {
            const int which = rng.below(2), mw = kMapW[which], mh = kMapH[which], tb = kTb[which];
            int w, h;
            const int kind = rng.below(40);
            if (kind == 0) { w = mw; h = mh; }                                           // the whole map: larger than the arena
            else if (kind < 4) { w = 1 + rng.below(mw); h = 1 + rng.below(mh); }
            else { w = 1 + rng.below(which ? 9 : 30); h = 1 + rng.below(9); }
            DirtyRect r; r.x0 = rng.below(mw - w + 1); r.y0 = rng.below(mh - h + 1); r.x1 = r.x0 + w; r.y1 = r.y0 + h;
            // the model first
            bool recorded = false; uint64_t off = 0;
            if (m.budget) {
                if (m.cursor < m.steps.size()) { hit.redo_discards++; m.steps.resize(m.cursor); }
                if (!m.lost) {
                    const uint64_t n = model_bytes(r, tb);
                    if (n > m.budget) hit.oversize++;
                    for (;;) {
                        bool wrapped = false, full = false;
                        if (m.open.recs.empty()) m.open.before = maps;
                        if (n <= m.budget && model_place(m, n, &off, &wrapped, &full)) { recorded = true; hit.wraps += wrapped; break; }
                        hit.table_full += full;
                        if (n <= m.budget && m.cursor > 0) { m.steps.erase(m.steps.begin()); m.cursor--; m.dropped++; hit.drops++; continue; }
                        m.dropped += (uint32_t)m.cursor + 1; m.steps.clear(); m.cursor = 0; m.open = MStep(); m.lost = true; hit.lost++;
                        break;
                    }
                    if (recorded) { MRec e; e.which = which; e.r = r; e.off = off; e.bytes = n; m.open.recs.push_back(e); hit.recorded++; }
                }
            }
            HistoryRecord e;
            const bool got = history_append(s, which, r, tb, &e);
            CHECK(got == recorded, "append: recorded %d, model %d", (int)got, (int)recorded);
            if (got) move_rect(e, arena, maps, false);
            for (int y = r.y0; y < r.y1; y++)                                             // the write itself
                for (int b = 0; b < w * tb; b++) maps.m[which][((size_t)y * mw + r.x0) * tb + b] = (uint8_t)rng.next();
        } else if (p < 72) {
            op = "commit";
            history_commit(s); model_commit();
        } else if (p < 86) {
            op = "undo";
            model_commit();
            uint64_t lo = 0, hi = 0;
            const bool got = history_undo(s, &lo, &hi);
            CHECK(got == (m.cursor > 0), "undo: applied %d, model has %zu steps", (int)got, m.cursor);
            if (got && m.cursor > 0) {
                for (uint64_t k = hi; k-- > lo;) move_rect(history_at(s, k), arena, maps, true);
                m.cursor--; hit.undos++;
                CHECK(maps == m.steps[m.cursor].before, "undo: the maps are not those from before the step");
                CHECK(hi - lo == m.steps[m.cursor].recs.size(), "undo: %llu records, the step has %zu", (unsigned long long)(hi - lo), m.steps[m.cursor].recs.size());
            }
        } else if (p < 98) {
            op = "redo";
            model_commit();
            uint64_t lo = 0, hi = 0;
            const bool got = history_redo(s, &lo, &hi);
            CHECK(got == (m.cursor < m.steps.size()), "redo: applied %d", (int)got);
            if (got && m.cursor < m.steps.size()) {
                for (uint64_t k = lo; k < hi; k++) move_rect(history_at(s, k), arena, maps, true);
                CHECK(maps == m.steps[m.cursor].after, "redo: the maps are not those from after the step");
                CHECK(hi - lo == m.steps[m.cursor].recs.size(), "redo: %llu records, the step has %zu", (unsigned long long)(hi - lo), m.steps[m.cursor].recs.size());
                m.cursor++; hit.redos++;
            }
        } else {
            op = "enable";
            const uint64_t budgets[4] = { 4096, 3008, 0, 4096 };
            enable(budgets[rng.below(4)]);
        }
        check_state(s, m, op);
    }
}

int main(int argc, char** argv)
{
    if (argc == 6 && !strcmp(argv[1], "size")) {
        DirtyRect r; r.x0 = atoi(argv[2]); r.y0 = 0; r.x1 = r.x0 + atoi(argv[3]); r.y1 = atoi(argv[4]);
        printf("%llu\n", (unsigned long long)history_record_bytes(r, atoi(argv[5])));
        return 0;
    }
    Reached hit;
    const uint64_t seeds[4] = { 1, 20240917, 77, 0xC0FFEE };
    for (uint64_t seed : seeds) run(seed, 10000, hit);
    printf("recorded %ld wraps %ld drops %ld redo_discards %ld lost %ld oversize %ld table_full %ld undos %ld redos %ld\n",
           hit.recorded, hit.wraps, hit.drops, hit.redo_discards, hit.lost, hit.oversize, hit.table_full, hit.undos, hit.redos);
    const long reached[] = { hit.recorded, hit.wraps, hit.drops, hit.redo_discards, hit.lost, hit.oversize, hit.table_full, hit.undos, hit.redos };
    for (long v : reached) CHECK(v > 0, "a path was never reached");
    printf("%ld cases, %d failures\n", cases, failures);
    return failures ? 1 : 0;
}
