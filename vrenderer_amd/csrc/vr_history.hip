// vr_terrain_undo / vr_terrain_redo: a journal of level-0 rectangles in one device arena.  What is recorded, where it lies and what
// is given up when the budget is short is vr_history.h; this file holds the arena, the two kernels that move a rectangle between
// a map and its record, the event behind them and the entry points.
//
//   k_history_capture<T>   map -> record, queued by vr_level0_call (vr_level0.h) in front of every edit's write of level 0
//   k_history_swap<T>      map <-> record, queued by undo and redo as the write of vr_derive_level0_write, whose refresh follows
//
// Both are one launch per record, one lane per 16-byte chunk of a record row (pitch / 16 chunks per row, rows x chunks lanes in
// all, 256 to a workgroup).  A chunk that lies wholly inside the row's bytes moves as one 16-byte vector on both sides where the
// map address is 16-byte aligned too - which vr_history.h's layout arranges for every row of a map whose row pitch is a multiple
// of 16.  The chunks at a row's ragged ends, and every chunk of a row whose map address is not congruent, move texel by texel
// (T = uint8_t / uint32_t).  Only the bytes of the rectangle are read or written, in the map and in the record alike: the padding of
// a record row is never touched, and nothing is ever written into the map from it.  Every byte belongs to exactly one lane, so the
// swap needs no order between lanes.  The kernels are untimed, like the brush and the mip kernels.
#include "vr_internal.h"
#include "vr_dirty.h"
#include "vr_history.h"

#include <new>

// `map`: the first byte of the rectangle's first row; map_pitch: bytes between two rows of the map.  `rec`: the record's first byte
// (16-byte aligned); rows rec_pitch apart, the row's bytes are [head, head + row_bytes) of its pitch.
struct HistoryMove {
    uint8_t* map; uint8_t* rec;
    uint64_t map_pitch;
    uint32_t rec_pitch, head, row_bytes, rows, chunks;      // chunks = rec_pitch / 16
};

template <class T, bool SWAP>
__device__ __forceinline__ void history_move(const HistoryMove& m)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= m.rows * m.chunks) return;
    const uint32_t row = i / m.chunks, c0 = (i - row * m.chunks) * 16u;     // the chunk is [c0, c0 + 16) of the row's pitch
    uint8_t* rec_row = m.rec + (size_t)row * m.rec_pitch;
    uint8_t* map_row = m.map + (size_t)row * m.map_pitch - m.head;          // byte j of the pitch mirrors map_row[j] (j >= head)
    const uint32_t lo = c0 > m.head ? c0 : m.head, end = m.head + m.row_bytes, hi = c0 + 16u < end ? c0 + 16u : end;
    if (lo >= hi) return;                                                    // (a chunk of padding alone cannot occur; kept as a bound)
    if (hi - lo == 16u && (((uintptr_t)(map_row + c0)) & 15u) == 0) {
        uint4* pm = reinterpret_cast<uint4*>(map_row + c0);
        uint4* pr = reinterpret_cast<uint4*>(rec_row + c0);
        const uint4 vm = *pm;
        if (SWAP) { const uint4 vr = *pr; *pm = vr; }
        *pr = vm;
        return;
    }
    for (uint32_t j = lo; j < hi; j += (uint32_t)sizeof(T)) {               // head, row_bytes and the map address are multiples of sizeof(T)
        T* pm = reinterpret_cast<T*>(map_row + j);
        T* pr = reinterpret_cast<T*>(rec_row + j);
        const T vm = *pm;
        if (SWAP) { const T vr = *pr; *pm = vr; }
        *pr = vm;
    }
}
template <class T> __global__ __launch_bounds__(256) void k_history_capture(HistoryMove m) { history_move<T, false>(m); }
template <class T> __global__ __launch_bounds__(256) void k_history_swap(HistoryMove m) { history_move<T, true>(m); }

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
static HistoryMove history_move_of(const vr_terrain* t, const HistoryRecord& e)
{
    const DevTex& tex = vr_terrain_map(t, e.which);
    HistoryMove m;
    m.map_pitch = (uint64_t)tex.w0 * e.texel_bytes;
    m.map = const_cast<uint8_t*>(tex.base) + (size_t)e.r.y0 * m.map_pitch + (size_t)e.r.x0 * e.texel_bytes;
    m.rec = t->d_history + e.off;
    m.rec_pitch = e.pitch; m.head = e.head; m.row_bytes = (uint32_t)(e.r.x1 - e.r.x0) * e.texel_bytes;
    m.rows = (uint32_t)(e.r.y1 - e.r.y0); m.chunks = e.pitch / kHistoryAlign;
    return m;
}
// one lane per chunk: at most 2^26 texels x 4 bytes / 16 + one chunk per row = 2^24 + 2^14 lanes, 65600 workgroups
static dim3 history_grid(const HistoryMove& m) { return dim3((unsigned)(((uint64_t)m.rows * m.chunks + 255) / 256)); }

// One journal kernel on `s`, between the journal's order_side_begin and order_side_end.
template <bool SWAP>
static int history_queue(vr_terrain* t, const HistoryRecord& e, hipStream_t s)
{
    { const int rc = order_side_begin(t->ord_journal, VrOrderOps(), s); if (rc) return rc; }
    const HistoryMove m = history_move_of(t, e);
    const dim3 grid = history_grid(m);
    if (SWAP) {
        if (e.texel_bytes == 1) hipLaunchKernelGGL(k_history_swap<uint8_t>, grid, dim3(256), 0, s, m);
        else hipLaunchKernelGGL(k_history_swap<uint32_t>, grid, dim3(256), 0, s, m);
    } else {
        if (e.texel_bytes == 1) hipLaunchKernelGGL(k_history_capture<uint8_t>, grid, dim3(256), 0, s, m);
        else hipLaunchKernelGGL(k_history_capture<uint32_t>, grid, dim3(256), 0, s, m);
    }
    VR_HIP(hipGetLastError());
    return order_side_end(t->ord_journal, VrOrderOps(), s);
}

int vr_history_capture(vr_terrain* t, int which, const DirtyRect& dirty, hipStream_t s)
{
    HistoryRecord e;
    if (!history_append(t->history, which, dirty, which == 0 ? 1 : 4, &e)) return VR_OK;      // off, or the open step is lost
    return history_queue<false>(t, e, s);
}

void vr_history_release(vr_terrain* t)
{
    (void)order_side_idle(t->ord_journal, VrOrderOps());
    if (t->ord_journal.ev) (void)hipEventDestroy(t->ord_journal.ev);
    t->ord_journal = VrOrderSide();
    (void)hipFree(t->d_history); t->d_history = nullptr;
    history_reset(t->history, 0, nullptr, 0);
}

extern "C" VR_API int vr_terrain_history_enable(vr_terrain* t, size_t budget_bytes)
{
    static_assert(sizeof(vr_history_status) == 32, "vr_history_status layout");
    static_assert(VR_HISTORY_MAX_RECORDS == kHistoryMaxRecords, "vr_history.h's cap");
    VR_REQUIRE(t != nullptr, "terrain is NULL");
    if ((uint64_t)budget_bytes == t->history.budget) return VR_OK;               // as it is: the steps stay
    VR_HIP(hipSetDevice(t->ctx->device));
    if (budget_bytes == 0) { vr_history_release(t); return VR_OK; }
    // everything the journal will ever need, before the old arena goes: the record table, the event, then the arena itself
    try { t->history_table.resize(kHistoryMaxRecords); }
    catch (const std::bad_alloc&) { vr_set_error("terrain history: %zu bytes for the record table", (size_t)kHistoryMaxRecords * sizeof(HistoryRecord)); return VR_ERR_OUT_OF_MEMORY; }
    if (!t->ord_journal.ev) VR_HIP(hipEventCreateWithFlags(&t->ord_journal.ev, hipEventDisableTiming));
    void** const slot[1] = { (void**)&t->d_history };
    const size_t want[1] = { budget_bytes };
    const int rc = vr_grow_group(slot, want, [t]() -> int { return order_side_idle(t->ord_journal, VrOrderOps()); });
    if (rc) { if (rc == VR_ERR_OUT_OF_MEMORY) vr_set_error("terrain history: %zu bytes for the arena", budget_bytes); return rc; }
    history_reset(t->history, budget_bytes, t->history_table.data(), kHistoryMaxRecords);
    return VR_OK;
}

extern "C" VR_API int vr_terrain_history_commit(vr_terrain* t)
{
    VR_REQUIRE(t != nullptr, "terrain is NULL");
    history_commit(t->history);
    return VR_OK;
}

static int history_apply(vr_terrain* t, bool undo, int32_t* applied)
{
    if (applied) *applied = 0;
    uint64_t lo = 0, hi = 0;
    // A frame recorded for a target's pending colour planes draws the map as it is now: where a step will be applied its pass is
    // queued first, in front of the journal's own move - a refusal there leaves the journal where it was.  (Asked of a copy of the
    // bookkeeping: a call that applies nothing queues nothing.)
    if (t->pending_target) {
        HistoryState probe = t->history;
        if (undo ? history_undo(probe, &lo, &hi) : history_redo(probe, &lo, &hi)) {
            VR_HIP(hipSetDevice(t->ctx->device));
            const int rc = vr_terrain_materialise_pending(t);
            if (rc) return rc;
        }
    }
    if (!(undo ? history_undo(t->history, &lo, &hi) : history_redo(t->history, &lo, &hi))) return VR_OK;      // queues nothing
    VR_HIP(hipSetDevice(t->ctx->device));
    for (uint64_t k = 0; k < hi - lo; k++) {
        const HistoryRecord e = history_at(t->history, undo ? hi - 1 - k : lo + k);
        // (not vr_level0_call: applying a record captures nothing, so the write is the swap alone)
        const int rc = vr_derive_level0_write(t, e.which, e.r, [&](hipStream_t s) -> int { return history_queue<true>(t, e, s); });
        if (rc) return rc;
    }
    if (applied) *applied = 1;
    return VR_OK;
}

extern "C" VR_API int vr_terrain_undo(vr_terrain* t, int32_t* applied)
{
    VR_REQUIRE(t != nullptr, "terrain is NULL");
    return history_apply(t, true, applied);
}

extern "C" VR_API int vr_terrain_redo(vr_terrain* t, int32_t* applied)
{
    VR_REQUIRE(t != nullptr, "terrain is NULL");
    return history_apply(t, false, applied);
}

extern "C" VR_API int vr_terrain_history_status(const vr_terrain* t, vr_history_status* out)
{
    VR_REQUIRE(t != nullptr, "terrain is NULL");
    VR_REQUIRE(out != nullptr, "out is NULL");
    const HistoryState& s = t->history;
    out->undo_steps = s.undo_steps; out->redo_steps = s.redo_steps; out->open_records = s.open_records; out->dropped_steps = s.dropped_steps;
    out->bytes_used = s.bytes_used; out->bytes_budget = s.budget;
    return VR_OK;
}
