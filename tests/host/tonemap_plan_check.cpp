// Exhaustive check of tm_refusal() and tm_plan() (vrenderer_amd/csrc/vr_tonemap_plan.h) against a flat transcription of the
// checks and launch sites the tone-map entry points and vr_frame_submit held before the plan existed (commit 86e1894; the line
// numbers are those of vrenderer_amd/csrc/vr_tonemap.hip, vr_frame.hip and vr_comm.hip there), written as that code wrote them,
// one function per entry point, and not as the header structures them - this is the specification.  A refusal is compared by
// its message text.  Plain C++17, no GPU: g++ -std=c++17 -Wall -Werror -I vrenderer_amd/csrc tests/host/tonemap_plan_check.cpp
#include "vr_tonemap_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

// the two refusals whose code and text come from a lookup (vr_partition_tables, rccl_load)
static const char* const kTables = "<vr_partition_tables>";
static const char* const kRccl = "<rccl_load>";

enum Entry { E_ADD, E_EXPOSURE, E_RENDER, E_SIMPLE, E_FRAME, E_COUNT };
static const unsigned kSteps[E_COUNT] = { TM_HISTOGRAM, TM_EXPOSURE, TM_RENDER, TM_RESET | TM_HISTOGRAM | TM_EXPOSURE | TM_RENDER,
                                          TM_RESET | TM_HISTOGRAM | TM_EXPOSURE | TM_RENDER };      // (E_FRAME: + TM_ALLREDUCE with a communicator)

// what the parent queued: the histogram kernel and the tone-map kernel of a call (family -1: none)
struct Launch { int family; unsigned grid; size_t num_blocks; };
struct Parent { const char* refusal; Launch hist, map; uint32_t q; bool effects_before_refusal; };

/* vr_tonemap.hip:39 */ static uint32_t parent_quantum(int w, int h)
{
    const uint64_t n = (uint64_t)w * (uint64_t)h;
    uint32_t q = 64u;
    while (q > 0u && (uint64_t)q * n > 0xffffffffull) q >>= 1;
    return q;
}
/* 381 */ static const char* parent_check_params(const TmPlanIn& in)
{
    /* 383 */ if (!in.have_params) return "NULL argument";
    /* 384 */ if (!(in.max_log > in.min_log)) return "max_log_luminance must exceed min_log_luminance";
    /* 385 */ if (!(in.white_point > 0.0f)) return "white_point must be positive";
    /* 386 */ if (!(in.min_adapted > 0.0f && in.max_adapted >= in.min_adapted)) return "bad adapted-luminance range";
    /* 387 */ if (!(in.low_percentile >= 0.0f && in.high_percentile <= 1.0f && in.high_percentile >= in.low_percentile)) return "bad histogram percentiles";
    return nullptr;
}
/* 406 */ static const char* parent_source_blocks(const TmPlanIn& in, size_t* blocks)
{
    const int w = in.w, h = in.h, kOwnerTile = 128;
    /* 408 */ if (!(w > 0 && h > 0)) return "bad frame size";
    if (in.packed) {
        /* 411 */ if (in.tables_failed) return kTables;
        /* 413 */ if (!((size_t)in.max_owned * kOwnerTile * kOwnerTile * 6 <= in.hdr_capacity)) return "hdr is smaller than vr_partition_packed_bytes()";
        /* 414 */ *blocks = (size_t)in.num_owned * 16;
    } else {
        /* 416 */ if (!((size_t)w * h * 8 <= in.hdr_capacity)) return "hdr is smaller than the frame";
        /* 417 */ *blocks = ((size_t)w * h / 4 + 255) / 256;
    }
    return nullptr;
}
/* 422 */ static const char* parent_add_frame(const TmPlanIn& in, Parent* r)
{
    const int w = in.w, h = in.h, kHistBlocks = 1024;
    /* 425 */ if (!(in.have_tm && in.have_hdr)) return "NULL argument";
    /* 426 */ if (const char* m = parent_check_params(in)) return m;
    /* 428 */ if (!in.device_same) return "image and tone-mapping pass live on different devices";
    size_t blocks = 0;
    /* 432 */ if (const char* m = parent_source_blocks(in, &blocks)) return m;
    /* 433 */ r->q = parent_quantum(w, h);
    /* 434 */ if (!(r->q != 0u)) return "frame has more than 2^32 - 1 pixels: the 32-bit histogram cannot count it";
    if (in.packed) {
        /* 437 */ if (blocks > 0) r->hist = { TM_PACKED, (unsigned)(blocks < (size_t)kHistBlocks ? blocks : (size_t)kHistBlocks), blocks };
    } else if (w % 4 == 0) {
        /* 441 */ r->hist = { TM_ROW, (unsigned)(blocks < (size_t)kHistBlocks ? blocks : (size_t)kHistBlocks), blocks };
    } else {
        /* 444 */ const size_t b = ((size_t)w * h + 255) / 256;
        /* 445 */ r->hist = { TM_SCALAR, (unsigned)(b < (size_t)kHistBlocks ? b : (size_t)kHistBlocks), 0 };
    }
    return nullptr;
}
/* 453 */ static const char* parent_exposure(const TmPlanIn& in)
{
    /* 455 */ if (!in.have_tm) return "NULL argument";
    /* 456 */ return parent_check_params(in);
}
/* 475 */ static const char* parent_render(const TmPlanIn& in, Parent* r)
{
    const int w = in.w, h = in.h, kOwnerTile = 128;
    /* 478 */ if (!(in.have_tm && in.have_hdr && in.have_ldr)) return "NULL argument";
    /* 479 */ if (const char* m = parent_check_params(in)) return m;
    /* 481 */ if (!in.device_same) return "image and tone-mapping pass live on different devices";
    size_t blocks = 0;
    /* 485 */ if (const char* m = parent_source_blocks(in, &blocks)) return m;
    /* 486 */ r->q = parent_quantum(w, h);
    if (in.packed) {
        /* 489 */ if (!((size_t)in.max_owned * kOwnerTile * kOwnerTile * 3 <= in.ldr_capacity)) return "ldr buffer is smaller than vr_partition_packed_bytes_ldr()";
        /* 490 */ if (blocks > 0) r->map = { TM_PACKED, (unsigned)blocks, 0 };
    } else {
        /* 494 */ if (!((size_t)w * h * 4 <= in.ldr_capacity)) return "ldr buffer is smaller than the frame";
        /* 495 */ if (w % 4 == 0) r->map = { TM_ROW, (unsigned)blocks, 0 };
        else {
            /* 499 */ const size_t b = ((size_t)w * h + 255) / 256;
            /* 500 */ r->map = { TM_SCALAR, (unsigned)b, 0 };
        }
    }
    return nullptr;
}
/* 508 */ static const char* parent_simple_render(const TmPlanIn& in, Parent* r)
{
    /* 511 */ if (!(in.have_tm && in.have_hdr)) return "NULL argument";
    /* 513 */ r->effects_before_refusal = true;                  // vr_tonemap_reset_histogram has zeroed the bins
    /* 514 */ if (const char* m = parent_add_frame(in, r)) return m;
    /* 515 */ if (const char* m = parent_exposure(in)) return m;
    /* 516 */ return parent_render(in, r);
}
/* vr_frame.hip:47 (f->tonemap set; :14-17 hold: t, gb, f, hdr_out present, the image on the terrain's device) */
static const char* parent_frame(const TmPlanIn& in, Parent* r)
{
    /* 50 */ if (!(in.have_params && in.have_ldr)) return "tone-map stage: params / ldr_out missing";
    /* 52 */ if (!in.frame_device_same) return "tone mapper lives on another device";
    /* 60 */ r->effects_before_refusal = true;
    /* 61 */ if (const char* m = parent_add_frame(in, r)) return m;
    /* 62; vr_comm.hip:116-117 */ if (in.have_comm) { if (!(in.have_tm && in.have_comm)) return "bad arguments"; if (in.rccl_missing) return kRccl; }
    /* 63 */ if (const char* m = parent_exposure(in)) return m;
    /* 64 */ if (const char* m = parent_render(in, r)) return m;
    /* 69 */ if (in.have_comm) {
        /* 70 */ if (!(in.have_part && in.have_gathered && in.have_ldr_frame)) return "exchange: partition / gathered / ldr_frame missing";
        /* 71; vr_comm.hip:105 (world >= 1: the tables exist) */ if (!(in.have_ldr && in.have_gathered && in.have_ldr_frame && in.w > 0 && in.h > 0)) return "bad arguments";
        /* vr_comm.hip:106 */ if (in.rccl_missing) return kRccl;
        /* vr_comm.hip:111; vr_tonemap.hip:531 */ if (!in.have_gathered || !in.have_ldr_frame) return "NULL argument";
        /* vr_tonemap.hip:532 */ if (!(in.w % 4 == 0 && in.w > 0 && in.h > 0)) return "frame width must be a multiple of 4";
    }
    return nullptr;
}

static long failures = 0;
static void fail(int entry, const TmPlanIn& in, const char* what)
{
    if (failures++ < 20)
        std::printf("FAIL %s: entry %d steps %u tm %d params %d hdr %d ldr %d log %g..%g wp %g adapted %g..%g pct %g..%g device %d %dx%d packed %d tables_failed %d "
                    "rccl_missing %d owned %d/%d hdr_cap %zu ldr_cap %zu frame %d comm %d part %d gathered %d ldr_frame %d frame_device %d\n",
                    what, entry, in.steps, in.have_tm, in.have_params, in.have_hdr, in.have_ldr, in.min_log, in.max_log, in.white_point, in.min_adapted, in.max_adapted,
                    in.low_percentile, in.high_percentile, in.device_same, in.w, in.h, in.packed, in.tables_failed, in.rccl_missing, in.num_owned, in.max_owned,
                    in.hdr_capacity, in.ldr_capacity, in.frame, in.have_comm, in.have_part, in.have_gathered, in.have_ldr_frame, in.frame_device_same);
}
#define CHECK(cond) do { if (!(cond)) fail(entry, in, #cond); } while (0)

int main()
{
    // widths of both classes x heights; pixel counts on both sides of 2^26 (Q 64 | 32) and of 2^32 - 1 (Q 1 | none); sizes that are none
    const int kWidths[7] = { 4, 6, 8, 1020, 1023, 7680, 16384 }, kHeights[4] = { 1, 36, 4200, 4320 };
    const int kMore[6][2] = { { 8191, 8192 }, { 8192, 8192 }, { 65535, 65537 }, { 65536, 65536 }, { 0, 36 }, { 4, -1 } };
    int sizes[34][2], ns = 0;
    for (int w : kWidths) for (int h : kHeights) { sizes[ns][0] = w; sizes[ns][1] = h; ns++; }
    for (const int* m : kMore) { sizes[ns][0] = m[0]; sizes[ns][1] = m[1]; ns++; }
    long cases = 0, accepted = 0, refusal_seen[TM_REFUSAL_COUNT] = {}, family_seen[3] = {};
    for (int entry = 0; entry < E_COUNT; entry++)
        for (int packed = 0; packed <= 1; packed++)
            for (int si = 0; si < ns; si++)
                for (int oi = 0; oi < 3; oi++)                       // num_owned: 0, 1, max_owned
                    for (int cap = 0; cap < 4; cap++)                // hdr, ldr: one byte under | exactly at the limit
                        for (int viol = 0; viol < 6; viol++)         // the parameters: fine | each of check_params's five conditions violated alone
                            for (unsigned bits = 0; bits < (entry == E_FRAME ? 1u << 7 : 1u << 5); bits++) {
                                TmPlanIn in{};
                                unsigned b = bits;
                                auto next = [&b]() { const bool v = b & 1u; b >>= 1; return v; };
                                const bool frame = entry == E_FRAME;
                                in.steps = kSteps[entry]; in.frame = frame; in.packed = packed != 0; in.have_part = in.packed;
                                in.w = sizes[si][0]; in.h = sizes[si][1];
                                in.have_ldr = next(); in.device_same = next(); in.tables_failed = next() && in.packed && in.w > 0 && in.h > 0;
                                // vr_frame_submit has checked its terrain, G-buffer and image, and the stage runs for a tone mapper only
                                in.have_tm = frame || next(); in.have_hdr = frame || next();
                                if (frame) {
                                    in.have_comm = next(); in.have_gathered = next(); in.have_ldr_frame = next(); in.rccl_missing = next() && in.have_comm;
                                    in.frame_device_same = in.device_same;      // (the image is on the terrain's device)
                                    if (in.have_comm) in.steps |= TM_ALLREDUCE;
                                }
                                // a two-rank split's larger share, as vr_partition_tables would count it
                                const size_t tiles = in.w > 0 && in.h > 0 ? (size_t)((in.w + 127) / 128) * (size_t)((in.h + 127) / 128) : 0;
                                in.max_owned = in.packed && !in.tables_failed ? (int)((tiles + 1) / 2) : 0;
                                in.num_owned = oi == 0 ? 0 : oi == 1 ? (in.max_owned < 1 ? in.max_owned : 1) : in.max_owned;
                                const size_t npx = in.w > 0 && in.h > 0 ? (size_t)in.w * (size_t)in.h : 0;
                                const size_t hdr_limit = in.packed ? (size_t)in.max_owned * 128 * 128 * 6 : npx * 8, ldr_limit = hdr_limit / 2;
                                in.hdr_capacity = hdr_limit - ((cap & 1) && hdr_limit ? 1 : 0); in.ldr_capacity = ldr_limit - ((cap & 2) && ldr_limit ? 1 : 0);
                                in.have_params = viol != 1;
                                in.min_log = -10.0f; in.max_log = viol == 2 ? -10.0f : 4.0f; in.white_point = viol == 3 ? 0.0f : 3.0f;
                                in.min_adapted = 0.02f; in.max_adapted = viol == 4 ? 0.01f : 0.5f; in.low_percentile = 0.8f; in.high_percentile = viol == 5 ? 0.7f : 0.95f;
                                cases++;

                                Parent q{};
                                q.hist.family = q.map.family = -1;
                                const char* want = entry == E_ADD ? parent_add_frame(in, &q) : entry == E_EXPOSURE ? parent_exposure(in)
                                                 : entry == E_RENDER ? parent_render(in, &q) : entry == E_SIMPLE ? parent_simple_render(in, &q) : parent_frame(in, &q);
                                const TmRefusal got = tm_refusal(in);
                                CHECK((int)got >= 0 && got < TM_REFUSAL_COUNT);
                                if ((int)got < 0 || got >= TM_REFUSAL_COUNT) continue;
                                refusal_seen[got]++;
                                const char* text = got == TM_NO_TABLES ? kTables : got == TM_NO_RCCL ? kRccl : tm_refusal_text(got);
                                CHECK((want == nullptr) == (got == TM_ACCEPTED));
                                if (want) CHECK(std::strcmp(want, text) == 0);
                                const TmPlan p = tm_plan(in);
                                if (got != TM_ACCEPTED) { CHECK(!p.launch); continue; }       // a refused call launches nothing
                                accepted++;
                                const bool hist = (in.steps & TM_HISTOGRAM) != 0, render = (in.steps & TM_RENDER) != 0;
                                if (!hist && !render) { CHECK(!p.launch); continue; }
                                CHECK(p.launch == !(in.packed && in.num_owned == 0));
                                CHECK(p.q == q.q);
                                if (hist) {
                                    CHECK(p.launch == (q.hist.family >= 0));
                                    if (p.launch) {
                                        CHECK((int)p.family == q.hist.family); CHECK(p.hist_grid == q.hist.grid); CHECK(p.hist_grid >= 1 && p.hist_grid <= (unsigned)kTmHistBlocks);
                                        if (p.family != TM_SCALAR) CHECK(p.blocks == q.hist.num_blocks);
                                    }
                                }
                                if (render) {
                                    CHECK(p.launch == (q.map.family >= 0));
                                    if (p.launch) { CHECK((int)p.family == q.map.family); CHECK(p.map_grid == q.map.grid); }
                                }
                                if (p.launch) family_seen[p.family]++;
                            }
    for (int r = 0; r < TM_REFUSAL_COUNT; r++)
        if (!refusal_seen[r]) { std::printf("FAIL refusal %d is never returned\n", r); failures++; }
    for (int f = 0; f < 3; f++)
        if (!family_seen[f]) { std::printf("FAIL kernel family %d is never chosen\n", f); failures++; }
    std::printf("tonemap_plan: %ld cases (%ld accepted), %ld failures\n", cases, accepted, failures);
    return failures ? EXIT_FAILURE : EXIT_SUCCESS;
}
