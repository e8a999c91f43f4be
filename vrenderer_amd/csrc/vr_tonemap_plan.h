// The tone-map stage's host decisions as two pure functions: tm_refusal() - does a call go ahead, and if not, which of the
// library's messages says why - and tm_plan() - which kernel family bins and maps an accepted frame, over which grids, with
// which bin quantum.  Plain C++17: no HIP, no library types - a CPU program enumerates every input
// (tests/host/tonemap_plan_check.cpp).  vr_tonemap_stage (vr_tonemap.hip) gathers the facts, asks both and acts afterwards; the
// four vr_tonemap_* entry points and vr_frame_submit are calls of it with a mask of steps.
//
// The refusals keep the order the entry points had: a call with several faults reports the one it always reported.  A step that
// is not asked for refuses nothing.  vr_frame_submit's stage adds its own in front (the descriptor's tone-map members, the tone
// mapper's device) and behind (the exchange's arguments and the LDR de-tile's width, when a communicator is given).
// The three families: packed tile-major tiles of a rank (a partition was given, even of one rank), row-major quads, and one
// pixel per lane for a row-major width that is no multiple of 4.  A packed source of such a width is accepted as it always was
// (the lighting pass refuses to produce one: light_width_ok, vr_light_plan.h).
#pragma once
#include <stddef.h>
#include <stdint.h>

constexpr int kTmOwnerTile = 128, kTmHistBlocks = 1024;      // VR_OWNER_TILE, kHistBlocks (vr_tonemap.hip asserts)

// Q = 64 >> s, s the smallest shift with Q * pixels <= 2^32 - 1 (pixels of the whole frame, also for a rank's share): no
// bin, LDS copy or per-workgroup sum can exceed Q * pixels, so the 32-bit bins never wrap, summed over the ranks included.
// 0 = more than 2^32 - 1 pixels.
inline uint32_t tm_bin_quantum(int w, int h)
{
    const uint64_t n = (uint64_t)w * (uint64_t)h;
    uint32_t q = 64u;
    while (q > 0u && (uint64_t)q * n > 0xffffffffull) q >>= 1;
    return q;
}

enum TmStep : unsigned { TM_RESET = 1u, TM_HISTOGRAM = 2u, TM_ALLREDUCE = 4u, TM_EXPOSURE = 8u, TM_RENDER = 16u };
enum TmFamily { TM_PACKED = 0, TM_ROW, TM_SCALAR };

// one value per message; TM_NO_TABLES and TM_NO_RCCL stand for the code and message of the lookup that failed
// (vr_partition_tables: "bad partition" or a HIP error; the RCCL loader: "RCCL not found ...")
enum TmRefusal {
    TM_ACCEPTED = 0,
    TM_STAGE_ARGS, TM_STAGE_DEVICE,                                        // vr_frame_submit, in front
    TM_NULL, TM_LOG_RANGE, TM_WHITE_POINT, TM_ADAPTED_RANGE, TM_PERCENTILES,
    TM_DEVICE, TM_FRAME_SIZE, TM_NO_TABLES, TM_HDR_PACKED, TM_HDR_FRAME, TM_PIXELS,
    TM_NO_RCCL,
    TM_LDR_PACKED, TM_LDR_FRAME,
    TM_EXCHANGE_ARGS, TM_DETILE_WIDTH,                                     // vr_frame_submit, behind
    TM_REFUSAL_COUNT
};
inline const char* tm_refusal_text(TmRefusal r)
{
    static const char* const kText[TM_REFUSAL_COUNT] = {
        "", "tone-map stage: params / ldr_out missing", "tone mapper lives on another device",
        "NULL argument", "max_log_luminance must exceed min_log_luminance", "white_point must be positive", "bad adapted-luminance range",
        "bad histogram percentiles",
        "image and tone-mapping pass live on different devices", "bad frame size", "", "hdr is smaller than vr_partition_packed_bytes()",
        "hdr is smaller than the frame", "frame has more than 2^32 - 1 pixels: the 32-bit histogram cannot count it",
        "",
        "ldr buffer is smaller than vr_partition_packed_bytes_ldr()", "ldr buffer is smaller than the frame",
        "exchange: partition / gathered / ldr_frame missing", "frame width must be a multiple of 4" };
    return kText[r];
}

struct TmPlanIn {
    unsigned steps;                // TmStep bits
    bool have_tm, have_params, have_hdr, have_ldr;
    float min_log, max_log, white_point, min_adapted, max_adapted, low_percentile, high_percentile;      // vr_tonemap_params, as given
    bool device_same;              // the image's device is the tone mapper's
    int w, h;
    bool packed;                   // a partition was given
    bool tables_failed, rccl_missing;      // the rank's tables (looked up for packed && w > 0 && h > 0) / the RCCL entry points (looked up for a communicator)
    int num_owned, max_owned;      // owner tiles of this rank / of the rank with the most (packed)
    size_t hdr_capacity, ldr_capacity;
    // vr_frame_submit's stage
    bool frame;
    bool have_comm, have_part, have_gathered, have_ldr_frame;
    bool frame_device_same;        // the tone mapper's device is the terrain's
};
struct TmPlan {
    bool launch;                   // false: this rank owns no tile - the steps run, the two streaming kernels are not launched
    TmFamily family;
    size_t blocks;                 // 256-lane blocks of work: 8 rows of an owner tile, 256 quads, or 256 pixels (TM_SCALAR)
    unsigned hist_grid, map_grid;  // k_tm_histogram*: at most kTmHistBlocks workgroups loop over the blocks; k_tonemap*: one per block
    uint32_t q;                    // tm_bin_quantum
};

inline TmRefusal tm_refusal(const TmPlanIn& in)
{
    const bool hist = in.steps & TM_HISTOGRAM, render = in.steps & TM_RENDER, source = hist || render;
    if (in.frame) {
        if (!in.have_params || !in.have_ldr) return TM_STAGE_ARGS;
        if (!in.frame_device_same) return TM_STAGE_DEVICE;
    }
    // (vr_tonemap_render looks at ldr first; behind a histogram step - vr_tonemap_simple_render - the histogram's refusals come first)
    if (!in.have_tm || (source && !in.have_hdr) || (render && !hist && !in.have_ldr) || !in.have_params) return TM_NULL;
    if (!(in.max_log > in.min_log)) return TM_LOG_RANGE;
    if (!(in.white_point > 0.0f)) return TM_WHITE_POINT;
    if (!(in.min_adapted > 0.0f && in.max_adapted >= in.min_adapted)) return TM_ADAPTED_RANGE;
    if (!(in.low_percentile >= 0.0f && in.high_percentile <= 1.0f && in.high_percentile >= in.low_percentile)) return TM_PERCENTILES;
    if (source) {
        if (!in.device_same) return TM_DEVICE;
        if (!(in.w > 0 && in.h > 0)) return TM_FRAME_SIZE;
        if (in.tables_failed) return TM_NO_TABLES;
        if (in.packed && (size_t)in.max_owned * kTmOwnerTile * kTmOwnerTile * 6 > in.hdr_capacity) return TM_HDR_PACKED;
        if (!in.packed && (size_t)in.w * in.h * 8 > in.hdr_capacity) return TM_HDR_FRAME;
        if (hist && tm_bin_quantum(in.w, in.h) == 0u) return TM_PIXELS;
    }
    if ((in.steps & TM_ALLREDUCE) && in.rccl_missing) return TM_NO_RCCL;
    if (render) {
        if (!in.have_ldr) return TM_NULL;
        if (in.packed && (size_t)in.max_owned * kTmOwnerTile * kTmOwnerTile * 3 > in.ldr_capacity) return TM_LDR_PACKED;
        if (!in.packed && (size_t)in.w * in.h * 4 > in.ldr_capacity) return TM_LDR_FRAME;
    }
    if (in.frame && in.have_comm) {
        if (!in.have_part || !in.have_gathered || !in.have_ldr_frame) return TM_EXCHANGE_ARGS;
        if (in.w % 4 != 0) return TM_DETILE_WIDTH;
    }
    return TM_ACCEPTED;
}

// What an accepted call with a source (TM_HISTOGRAM or TM_RENDER) launches; anything else launches neither streaming kernel.
inline TmPlan tm_plan(const TmPlanIn& in)
{
    TmPlan p{};
    if (!(in.steps & (TM_HISTOGRAM | TM_RENDER)) || tm_refusal(in) != TM_ACCEPTED) return p;
    const size_t npx = (size_t)in.w * (size_t)in.h;
    p.family = in.packed ? TM_PACKED : in.w % 4 == 0 ? TM_ROW : TM_SCALAR;
    p.launch = !in.packed || in.num_owned > 0;
    p.blocks = in.packed ? (size_t)in.num_owned * 16 : ((p.family == TM_ROW ? npx / 4 : npx) + 255) / 256;
    p.hist_grid = (unsigned)(p.blocks < (size_t)kTmHistBlocks ? p.blocks : (size_t)kTmHistBlocks);
    p.map_grid = (unsigned)p.blocks;
    p.q = tm_bin_quantum(in.w, in.h);
    return p;
}
