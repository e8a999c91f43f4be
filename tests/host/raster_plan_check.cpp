// Exhaustive check of raster_plan() (vrenderer_amd/csrc/vr_raster_plan.h): every combination of its inputs, against
//  (a) a flat transcription of the expressions terrain_render_impl held before the plan existed (commit 0e1e774,
//      vrenderer_amd/csrc/vr_raster.hip; line numbers are that file's), one line per decision, written as that code wrote
//      them and not as the header structures them - this is the specification;
//  (b) invariants that hold whatever the transcription says.
// Plain C++17, no GPU: g++ -std=c++17 -Wall -Werror -I vrenderer_amd/csrc tests/host/raster_plan_check.cpp
#include "vr_raster_plan.h"

#include <cstdio>
#include <cstdlib>

// what each variant's k_raster instantiation has compiled in: <WIRE, TILE, MODE, RANGES, NOEMI, LIT, KEEP> (MODE: 0 generic, 1 fast, 2 depth)
struct Flags { bool wire; int tile; int mode; bool ranges, noemi, lit, keep; };
static const Flags kFlags[RV_COUNT] = {
    /* RV_WIRE_32 */ { true, 32, 0, false, false, false, false },  /* RV_GENERIC_32 */ { false, 32, 0, false, false, false, false },
    /* RV_DEPTH_32 */ { false, 32, 2, false, false, false, false }, /* RV_FAST_32 */ { false, 32, 1, false, false, false, false },
    /* RV_FAST_NOEMI_32 */ { false, 32, 1, false, true, false, false }, /* RV_FAST_RANGES_32 */ { false, 32, 1, true, false, false, false },
    /* RV_FAST_RANGES_NOEMI_32 */ { false, 32, 1, true, true, false, false },
    /* RV_WIRE_64 */ { true, 64, 0, false, false, false, false },  /* RV_GENERIC_64 */ { false, 64, 0, false, false, false, false },
    /* RV_DEPTH_64 */ { false, 64, 2, false, false, false, false }, /* RV_FAST_64 */ { false, 64, 1, false, false, false, false },
    /* RV_FAST_NOEMI_64 */ { false, 64, 1, false, true, false, false }, /* RV_FAST_RANGES_64 */ { false, 64, 1, true, false, false, false },
    /* RV_FAST_RANGES_NOEMI_64 */ { false, 64, 1, true, true, false, false },
    /* RV_LIT_32 */ { false, 32, 1, false, true, true, false }, /* RV_LIT_64 */ { false, 64, 1, false, true, true, false },
    /* RV_KEEP_32 */ { false, 32, 1, false, true, true, true },
};

// (a) the parent's decisions, in the parent's order.  `part == nullptr` reads world == 1 (vr_terrain_render_keep passes no
// partition); rp-> and a. fields are the inputs of the same name; gb-> fields are the G-buffer's state as the parent's line saw it.
static RasterPlan parent_plan(const RasterPlanIn& in)
{
    RasterPlan p{};
    bool assume_cleared = in.assume_cleared, clear_pending = in.clear_pending, emissive_zero = in.emissive_zero;     // a.assume_cleared (1763), gb->
    int request = in.request;                                                                                         // lit_req
    /* 2013 */ const bool fast = in.tex_same && in.ws_pow2 && in.one_rsrc && !in.wireframe && !in.depth_only;
    /* 2019 */ bool keep = false;
    /* 2020 */ if (request == RASTER_REQ_KEEP) {
    /* 2021 */     const bool cleared = in.assume_cleared || clear_pending;
    /* 2022 */     keep = in.world == 1 && fast && in.tile_shift == 5 && cleared && !in.depth_ranges
    /* 2023 */         && in.plane_tracking && emissive_zero && !in.escaped
    /* 2024 */         && in.viewport_full && in.width_mult4
    /* 2025-2027 */    && in.lit_inputs_ok && in.hdr_fits;
    /* 2028-2032 */ if (keep) keep = in.lit_plain;
    /* 2034 */     if (!keep) request = RASTER_REQ_NONE;
               }
    /* 2036 */ if (clear_pending) {
    /* 2037 */     if (in.world <= 1 && !in.depth_only && (request == RASTER_REQ_NONE || keep)) { assume_cleared = true; clear_pending = false; p.consume_pending_clear = true; }
    /* 2038 */     else { p.materialise_first = true; emissive_zero = true; clear_pending = false; }          // gbuffer_clear_now, vr_host.hip:471-473
               }
    /* 2071 */ const bool depth = in.depth_only && !in.wireframe;
    /* 2073 */ const bool ranges = in.depth_ranges && fast && assume_cleared && !in.escaped;
    /* 2079 */ const bool noemi = fast && in.plane_tracking && emissive_zero && !in.escaped;
    /* 2082 */ bool fuse = keep;
    /* 2087 */ if (!keep && request != RASTER_REQ_NONE && fast && !ranges)
    /* 2093 */     fuse = in.lit_plain && in.width_mult4;          // (2090: !lit_plain is `extra` here - a refused list has left the function; 2091 refuses a partial viewport)
    /* 2106 */ p.track_regions = fast && (!fuse || keep) && in.tile_shift == 5 && in.plane_tracking && !in.escaped;
    const int e = in.tile_shift == 5 ? 0 : RV_WIRE_64 - RV_WIRE_32;
    /* 2113 */ if (fuse && keep) p.variant = RV_KEEP_32;
    /* 2114 */ else if (fuse && in.tile_shift == 5) p.variant = RV_LIT_32;
    /* 2115 */ else if (fuse) p.variant = RV_LIT_64;
    /* 2117, 2080 -> 1865 */ else if (in.wireframe) p.variant = (RasterVariant)(RV_WIRE_32 + e);
    /* 1866 */ else if (fast && ranges) p.variant = (RasterVariant)((noemi ? RV_FAST_RANGES_NOEMI_32 : RV_FAST_RANGES_32) + e);
    /* 1867 */ else if (fast) p.variant = (RasterVariant)((noemi ? RV_FAST_NOEMI_32 : RV_FAST_32) + e);
    /* 1868 */ else p.variant = (RasterVariant)((depth ? RV_DEPTH_32 : RV_GENERIC_32) + e);
    /* 2124 */ p.emissive_zero_after = !fuse && !noemi && !in.depth_only && assume_cleared && in.world <= 1;
    p.fast = fast; p.assume_cleared = assume_cleared; p.ranges = ranges; p.noemi = noemi; p.fuse = fuse; p.keep = keep;
    return p;
}

static long failures = 0;
static void fail(const RasterPlanIn& in, const char* what)
{
    if (failures++ < 20)
        std::printf("FAIL %s: wire %d depth_only %d assume_cleared %d depth_ranges %d world %d shift %d tex_same %d ws_pow2 %d one_rsrc %d tracking %d "
                    "clear_pending %d emissive_zero %d escaped %d viewport_full %d width_mult4 %d request %d inputs_ok %d plain %d hdr_fits %d\n",
                    what, in.wireframe, in.depth_only, in.assume_cleared, in.depth_ranges, in.world, in.tile_shift, in.tex_same, in.ws_pow2, in.one_rsrc,
                    in.plane_tracking, in.clear_pending, in.emissive_zero, in.escaped, in.viewport_full, in.width_mult4, (int)in.request, in.lit_inputs_ok,
                    in.lit_plain, in.hdr_fits);
}
#define CHECK(cond) do { if (!(cond)) fail(in, #cond); } while (0)
#define IMPLIES(a, b) CHECK(!(a) || (b))

int main()
{
    long cases = 0, reached[RV_COUNT] = {};
    for (unsigned bits = 0; bits < (1u << 16); bits++)
        for (int world = 1; world <= 2; world++)
            for (int shift = 5; shift <= 6; shift++)
                for (int req = RASTER_REQ_NONE; req <= RASTER_REQ_KEEP; req++) {
                    RasterPlanIn in{};
                    unsigned b = bits;
                    auto next = [&b]() { const bool v = b & 1u; b >>= 1; return v; };
                    in.wireframe = next(); in.depth_only = next(); in.assume_cleared = next(); in.depth_ranges = next();
                    in.tex_same = next(); in.ws_pow2 = next(); in.one_rsrc = next(); in.plane_tracking = next();
                    in.clear_pending = next(); in.emissive_zero = next(); in.escaped = next(); in.viewport_full = next();
                    in.width_mult4 = next(); in.lit_inputs_ok = next(); in.lit_plain = next(); in.hdr_fits = next();
                    in.world = world; in.tile_shift = shift; in.request = (RasterRequest)req;
                    const RasterPlan p = raster_plan(in);
                    cases++;
                    // (a)
                    const RasterPlan q = parent_plan(in);
                    CHECK(p.variant == q.variant); CHECK(p.fast == q.fast); CHECK(p.assume_cleared == q.assume_cleared);
                    CHECK(p.materialise_first == q.materialise_first); CHECK(p.consume_pending_clear == q.consume_pending_clear);
                    CHECK(p.ranges == q.ranges); CHECK(p.noemi == q.noemi); CHECK(p.fuse == q.fuse); CHECK(p.keep == q.keep);
                    CHECK(p.track_regions == q.track_regions); CHECK(p.emissive_zero_after == q.emissive_zero_after);
                    // (b)
                    const int v = (int)p.variant;
                    CHECK(v >= 0 && v < RV_COUNT);
                    if (v < 0 || v >= RV_COUNT) continue;
                    reached[p.variant]++;
                    const bool fast = in.tex_same && in.ws_pow2 && in.one_rsrc && !in.wireframe && !in.depth_only;
                    IMPLIES(p.keep, p.fuse && p.noemi && in.tile_shift == 5 && in.world == 1 && p.assume_cleared);
                    IMPLIES(p.keep, in.request == RASTER_REQ_KEEP && in.emissive_zero);
                    // the emissive plane is skipped only while it is known zero: the state said so, or the pass's own pending clear
                    // has just been written in front of it (which leaves it so)
                    IMPLIES(p.noemi, (in.emissive_zero || p.materialise_first) && in.plane_tracking && !in.escaped);
                    IMPLIES(p.noemi, fast);
                    IMPLIES(p.track_regions, fast && in.tile_shift == 5 && in.plane_tracking && !in.escaped);
                    IMPLIES(p.ranges, fast && p.assume_cleared && !in.escaped && in.depth_ranges);
                    IMPLIES(in.escaped, !p.noemi && !p.ranges && !p.track_regions && !p.keep);
                    CHECK(!(p.materialise_first && p.consume_pending_clear));
                    CHECK((p.materialise_first || p.consume_pending_clear) == in.clear_pending);
                    IMPLIES(p.consume_pending_clear, p.assume_cleared && in.world == 1 && !in.depth_only);
                    IMPLIES(p.assume_cleared, in.assume_cleared || p.consume_pending_clear);
                    IMPLIES(p.fuse, fast && in.request != RASTER_REQ_NONE && in.lit_plain && in.width_mult4 && !p.ranges);
                    IMPLIES(p.fuse && !p.keep, in.request == RASTER_REQ_LIT && p.materialise_first == in.clear_pending);   // LIT forces materialisation
                    IMPLIES(p.emissive_zero_after, !p.fuse && !p.noemi && !in.depth_only && p.assume_cleared && in.world == 1);
                    CHECK(p.fast == fast);
                    // the variant against the flags it has compiled in
                    const Flags& f = kFlags[p.variant];
                    CHECK(f.tile == (1 << in.tile_shift));
                    CHECK(f.keep == p.keep); CHECK(f.lit == p.fuse);
                    CHECK(f.ranges == p.ranges);
                    if (!f.lit) {
                        CHECK(f.wire == in.wireframe);
                        CHECK(f.noemi == p.noemi);
                        CHECK((f.mode == 1) == fast);
                        if (!f.wire && !fast) CHECK((f.mode == 2) == in.depth_only);
                        if (f.wire) CHECK(f.mode == 0);
                    } else {
                        CHECK(f.mode == 1 && fast);          // (LIT writes no emissive plane whatever is known of it; KEEP skips it: keep => noemi above)
                    }
                    const bool kernel_tracks = f.mode == 1 && f.tile == 32 && (!f.lit || f.keep) && !f.wire;      // k_raster's TRACK
                    IMPLIES(p.track_regions, kernel_tracks);
                    IMPLIES(kernel_tracks && in.plane_tracking && !in.escaped, p.track_regions);
                }
    for (int v = 0; v < RV_COUNT; v++)
        if (!reached[v]) { std::printf("FAIL variant %d is never chosen\n", v); failures++; }
    std::printf("raster_plan: %ld cases, %ld failures\n", cases, failures);
    return failures ? EXIT_FAILURE : EXIT_SUCCESS;
}
