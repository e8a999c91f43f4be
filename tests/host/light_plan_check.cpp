// Exhaustive check of light_plan() and light_width_ok() (vrenderer_amd/csrc/vr_light_plan.h): every combination of the boolean
// inputs and the three entry points, over a few light counts, owner-tile counts and frame sizes, against
//  (a) a flat transcription of the ternaries and launch sites deferred_light and deferred_light_tiled held before the plan
//      existed (commit 012f361, vrenderer_amd/csrc/vr_deferred.hip; line numbers are that file's), written as that code wrote
//      them and not as the header structures them - this is the specification;
//  (b) invariants that hold whatever the transcription says, against a table of what each variant has compiled in;
//  (c) the rule that is younger than that code, over the same inputs with sky_not_zero set (vr_light_domain.h could not show that
//      a cleared texel shades to +0): the tiled entry points are refused (light_sky_ok), the streaming pass gets the plan of the
//      same call with nothing known about the planes - k_deferred_stream or k_deferred_scalar, never k_deferred.  (a) and (b) run
//      with the flag clear, where the plan is the transcription's.
// Plain C++17, no GPU: g++ -std=c++17 -Wall -Werror -I vrenderer_amd/csrc tests/host/light_plan_check.cpp
#include "vr_light_plan.h"

#include <cstdio>
#include <cstdlib>

// what each variant's instantiation has compiled in.  k_deferred_stream / k_deferred: <PACKED, EXTRA, SHADOW, NT>;
// k_deferred_tiled: <PACKED, PXB, NT, EXTRA, SHADOW>; k_deferred_scalar: every light type, plain loads and stores, the shadow
// term by a run-time argument (shadow = -1)
enum Family { F_STREAM, F_HINTED, F_SCALAR, F_TILED };
struct Flags { Family family; bool packed, nt, extra; int shadow; };
static const Flags kFlags[LV_COUNT] = {
    /* LV_STREAM_ROW */ { F_STREAM, false, true, false, 0 }, /* _EXTRA */ { F_STREAM, false, true, true, 0 }, /* _SHADOW */ { F_STREAM, false, true, true, 1 },
    /* LV_STREAM_PACKED */ { F_STREAM, true, false, false, 0 }, /* _EXTRA */ { F_STREAM, true, false, true, 0 }, /* _SHADOW */ { F_STREAM, true, false, true, 1 },
    /* LV_HINTED_ROW */ { F_HINTED, false, true, false, 0 }, /* _EXTRA */ { F_HINTED, false, true, true, 0 }, /* _SHADOW */ { F_HINTED, false, true, true, 1 },
    /* LV_HINTED_PACKED */ { F_HINTED, true, false, false, 0 }, /* _EXTRA */ { F_HINTED, true, false, true, 0 }, /* _SHADOW */ { F_HINTED, true, false, true, 1 },
    /* LV_SCALAR */ { F_SCALAR, false, false, true, -1 },
    /* LV_TILED_ROW */ { F_TILED, false, true, false, 0 }, /* _EXTRA */ { F_TILED, false, true, true, 0 },
    /* _SHADOW */ { F_TILED, false, true, false, 1 }, /* _EXTRA_SHADOW */ { F_TILED, false, true, true, 1 },
    /* LV_TILED_PACKED */ { F_TILED, true, false, false, 0 }, /* _EXTRA */ { F_TILED, true, false, true, 0 },
    /* _SHADOW */ { F_TILED, true, false, false, 1 }, /* _EXTRA_SHADOW */ { F_TILED, true, false, true, 1 },
};
struct CullFlags { bool ranges, cone; };
static const CullFlags kCullFlags[LC_COUNT] = { { false, false }, { true, false }, { false, true }, { true, true } };

// an instantiation the parent compiled and could not launch (its `nt` constants were true): none of the plan's values
constexpr LightVariant LV_NEVER = LV_COUNT;

// (a) the parent's decisions, in the parent's order.  `refused`: one of its width refusals; the kernel template arguments are
// in the comments, the value is the plan's name for that instantiation.  Only what a call that reached the line could hold is
// transcribed: vr_deferred_light_tiled passed no binding and fill_light (line 237) had refused spot and spherical lights for it.
struct Parent { bool refused, launch; LightVariant shade; unsigned shade_grid; LightCull cull; unsigned cull_grid;
                int macro_x, tx, ty, stride; size_t words, scratch_words; bool use_ranges; };
static Parent parent_stream(const LightPlanIn& in)
{
    Parent r{};
    const bool shadow = in.shadow, extra = in.extra, hinted = in.hinted;
    /* 307 */ const size_t npx = (size_t)in.w * in.h;
    /* 308 */ const bool packed = in.packed;
    if (packed) {
        /* 319 */ if (!in.width_mult4) { r.refused = true; return r; }
        /* 321 */ if (in.num_owned > 0) {
            r.launch = true;
            /* 323 */ if (!hinted) r.shade = shadow ? LV_STREAM_PACKED_SHADOW /* <true, true, true> */ : (extra ? LV_STREAM_PACKED_EXTRA /* <true, true> */ : LV_STREAM_PACKED /* <true, false> */);
            /* 327 */ else r.shade = shadow ? LV_HINTED_PACKED_SHADOW /* <true, true, true> */ : (extra ? LV_HINTED_PACKED_EXTRA /* <true, true> */ : LV_HINTED_PACKED /* <true, false> */);
            /* 324, 328 */ r.shade_grid = (unsigned)in.num_owned * 16;
        }
    } else {
        r.launch = true;
        /* 334 */ if (in.width_mult4) {
            /* 335 */ const size_t quads = npx / 4;
            /* 337 */ const bool nt = true;
            /* 339 */ if (!hinted) r.shade = shadow ? LV_STREAM_ROW_SHADOW /* <false, true, true, true> */ : extra ? LV_STREAM_ROW_EXTRA /* <false, true, false, true> */
            /* 340 */                                                                                    : LV_STREAM_ROW /* <false, false, false, true> */;
            /* 344 */ else r.shade = shadow ? (nt ? LV_HINTED_ROW_SHADOW /* <false, true, true, true> */ : LV_NEVER /* <false, true, true, false> */)
            /* 345 */                : extra ? (nt ? LV_HINTED_ROW_EXTRA /* <false, true, false, true> */ : LV_NEVER /* <false, true, false, false> */)
            /* 346 */                        : (nt ? LV_HINTED_ROW /* <false, false, false, true> */ : LV_NEVER /* <false, false, false, false> */);
            /* 341, 347 */ r.shade_grid = (unsigned)((quads + 255) / 256);
        } else {
            /* 351 */ r.shade = LV_SCALAR; r.shade_grid = (unsigned)((npx + 255) / 256);          // (352: use_shadow = shadow ? 1 : 0)
        }
    }
    return r;
}
static Parent parent_tiled(const LightPlanIn& in)
{
    Parent r{};
    const bool shadow = in.shadow, extra = in.extra, cone = in.cone;       // (872-878: both false unless ex)
    const int num_lights = in.num_lights, kTileLightCap = 1024, kMacroTile = 128, kLightTile = 32, kSubTiles = 16;
    /* 879 */ const bool more = extra || shadow;
    /* 894 */ const bool packed = in.packed;
    /* 895 */ if (!in.width_mult4) { r.refused = true; return r; }
    /* 897 */ const int macro_x = (in.w + kMacroTile - 1) / kMacroTile, macro_y = (in.h + kMacroTile - 1) / kMacroTile;
    /* 898 */ const int tx = (in.w + kLightTile - 1) / kLightTile, ty = (in.h + kLightTile - 1) / kLightTile;
    /* 899 */ const int stride = (num_lights < kTileLightCap ? num_lights : kTileLightCap) + 1;
    /* 900 */ const size_t words = (size_t)tx * ty * stride;
    /* 903 */ const size_t scratch_words = (size_t)macro_x * macro_y * (size_t)(((num_lights + 3) / 4) * 4) + 4;
    /* 908 */ const bool use_ranges = in.ranges_usable;                     // vr_gbuffer_consume_ranges: CLEAN behind it if so
    /* 910 */ r.cull = cone ? (use_ranges ? LC_RANGES_CONE /* <true, true> */ : LC_DEPTH_CONE /* <false, true> */) : (use_ranges ? LC_RANGES /* <true> */ : LC_DEPTH /* <false> */);
    if (packed) {
        /* 919 */ if (in.num_owned > 0) {
            r.launch = true;
            /* 921 */ r.cull_grid = (unsigned)in.num_owned;
            /* 925 */ if (more)
            /* 926 */     r.shade = shadow ? (extra ? LV_TILED_PACKED_EXTRA_SHADOW /* <true, PXB, false, true, true> */ : LV_TILED_PACKED_SHADOW /* <true, PXB, false, false, true> */)
            /* 927 */                      : LV_TILED_PACKED_EXTRA /* <true, PXB, false, true, false> */;
            /* 932 */ else r.shade = LV_TILED_PACKED /* <true, PXB> */;
            /* 928, 932 */ r.shade_grid = (unsigned)in.num_owned * kSubTiles;
        }
    } else {
        r.launch = true;
        /* 940 */ r.cull_grid = (unsigned)(macro_x * macro_y);
        /* 944 */ const bool nt = true;
        /* 945 */ if (more)
        /* 946 */     r.shade = shadow ? (extra ? LV_TILED_ROW_EXTRA_SHADOW /* <false, PXB, true, true, true> */ : LV_TILED_ROW_SHADOW /* <false, PXB, true, false, true> */)
        /* 947 */                      : LV_TILED_ROW_EXTRA /* <false, PXB, true, true, false> */;
        /* 951 */ else if (nt) r.shade = LV_TILED_ROW /* <false, PXB, true> */;
        /* 954 */ else r.shade = LV_NEVER /* <false, PXB, false> */;
        /* 948-954 */ r.shade_grid = (unsigned)(tx * ty);
    }
    r.macro_x = macro_x; r.tx = tx; r.ty = ty; r.stride = stride; r.words = words; r.scratch_words = scratch_words; r.use_ranges = use_ranges;
    return r;
}

static long failures = 0;
static void fail(const LightPlanIn& in, const char* what)
{
    if (failures++ < 20)
        std::printf("FAIL %s: entry %d packed %d width_mult4 %d shadow %d extra %d cone %d hinted %d ranges_usable %d sky_not_zero %d lights %d %dx%d owned %d\n",
                    what, (int)in.entry, in.packed, in.width_mult4, in.shadow, in.extra, in.cone, in.hinted, in.ranges_usable, in.sky_not_zero, in.num_lights,
                    in.w, in.h, in.num_owned);
}
#define CHECK(cond) do { if (!(cond)) fail(in, #cond); } while (0)
#define IMPLIES(a, b) CHECK(!(a) || (b))

static bool same_plan(const LightPlan& a, const LightPlan& b)
{
    return a.launch == b.launch && a.shade == b.shade && a.shade_grid == b.shade_grid && a.macro_x == b.macro_x && a.cull == b.cull
        && a.cull_grid == b.cull_grid && a.tiles32_x == b.tiles32_x && a.tiles32_y == b.tiles32_y && a.list_stride == b.list_stride
        && a.list_words == b.list_words && a.scratch_words == b.scratch_words && a.consume_ranges == b.consume_ranges;
}

int main()
{
    const int kLights[5] = { 0, 1, kPlanTileLightCap, kPlanTileLightCap + 1, 65536 };
    // frame sizes by width class: the tests' frame, one whose edge tiles are partial in both directions, the 8K frame
    const int kSizes4[3][2] = { { 256, 144 }, { 132, 33 }, { 7680, 4320 } }, kSizesOdd[3][2] = { { 255, 144 }, { 1001, 77 }, { 7681, 4320 } };
    long cases = 0, refused = 0, unreachable = 0, reached[LV_COUNT] = {}, cull_reached[LC_COUNT] = {};
    for (int entry = LIGHT_STREAM; entry <= LIGHT_TILED_EX; entry++)
        for (unsigned bits = 0; bits < (1u << 7); bits++)
            for (int li = 0; li < 5; li++)
                for (int owned = 0; owned <= 1; owned++)
                    for (int si = 0; si < 3; si++) {
                        LightPlanIn in{};
                        unsigned b = bits;
                        auto next = [&b]() { const bool v = b & 1u; b >>= 1; return v; };
                        in.entry = (LightEntry)entry;
                        in.packed = next(); in.width_mult4 = next(); in.shadow = next(); in.extra = next(); in.cone = next();
                        in.hinted = next(); in.ranges_usable = next();
                        in.num_lights = kLights[li]; in.num_owned = owned;
                        const int* size = in.width_mult4 ? kSizes4[si] : kSizesOdd[si];
                        in.w = size[0]; in.h = size[1];
                        cases++;
                        const bool tiled = in.entry != LIGHT_STREAM;
                        // (a)
                        const Parent q = tiled ? parent_tiled(in) : parent_stream(in);
                        CHECK(light_width_ok(in) == !q.refused);
                        if (!light_width_ok(in)) { refused++; continue; }          // (the plan is asked for accepted widths only)
                        const LightPlan p = light_plan(in);
                        const bool parent_reaches = !(in.entry == LIGHT_TILED && (in.shadow || in.extra || in.cone));
                        if (!parent_reaches) unreachable++;
                        else {
                            CHECK(p.launch == q.launch);
                            if (q.launch) { CHECK(p.shade == q.shade); CHECK(p.shade_grid == q.shade_grid); }
                            if (tiled) {
                                CHECK(p.cull == q.cull); CHECK(p.consume_ranges == q.use_ranges);
                                if (q.launch) CHECK(p.cull_grid == q.cull_grid);
                                CHECK(p.macro_x == q.macro_x); CHECK(p.tiles32_x == q.tx); CHECK(p.tiles32_y == q.ty);
                                CHECK(p.list_stride == q.stride); CHECK(p.list_words == q.words); CHECK(p.scratch_words == q.scratch_words);
                            }
                        }
                        // (b)
                        CHECK((int)p.shade >= 0 && p.shade < LV_COUNT && (int)p.cull >= 0 && p.cull < LC_COUNT);
                        if ((int)p.shade < 0 || p.shade >= LV_COUNT || (int)p.cull < 0 || p.cull >= LC_COUNT) continue;
                        const Flags& f = kFlags[p.shade];
                        const CullFlags& c = kCullFlags[p.cull];
                        if (p.launch) { reached[p.shade]++; if (tiled) cull_reached[p.cull]++; }
                        CHECK(p.launch == !(in.packed && in.num_owned == 0));
                        CHECK((f.family == F_TILED) == tiled);
                        CHECK(f.packed == in.packed);
                        CHECK((f.family == F_SCALAR) == (!tiled && !in.width_mult4));
                        CHECK(f.nt == (!in.packed && f.family != F_SCALAR));          // the row-major quad kernels stream; the scalar one has no such form
                        if (!tiled) {
                            if (f.family == F_SCALAR) CHECK(f.extra && f.shadow == -1);        // a superset: every light type, the shadow at run time
                            else {
                                CHECK(f.shadow == (in.shadow ? 1 : 0));
                                CHECK(f.extra == (in.extra || in.shadow));
                                CHECK((f.family == F_HINTED) == in.hinted);
                            }
                            CHECK(!p.consume_ranges);
                        } else {
                            const bool ex = in.entry == LIGHT_TILED_EX;
                            CHECK(f.shadow == (in.shadow && ex ? 1 : 0));
                            CHECK(f.extra == (in.extra && ex));
                            CHECK(c.cone == (in.cone && ex));
                            IMPLIES(!ex, !f.extra && f.shadow == 0 && !c.cone);
                            CHECK(c.ranges == p.consume_ranges);
                            IMPLIES(p.consume_ranges, in.ranges_usable);
                            const int capped = in.num_lights < kPlanTileLightCap ? in.num_lights : kPlanTileLightCap;
                            CHECK(p.list_stride == capped + 1);
                            CHECK(p.list_words == (size_t)p.tiles32_x * p.tiles32_y * p.list_stride);
                            CHECK(p.tiles32_x * kPlanLightTile >= in.w && (p.tiles32_x - 1) * kPlanLightTile < in.w);
                            CHECK(p.tiles32_y * kPlanLightTile >= in.h && (p.tiles32_y - 1) * kPlanLightTile < in.h);
                            CHECK(p.macro_x * kPlanOwnerTile >= in.w && (p.macro_x - 1) * kPlanOwnerTile < in.w);
                            // k_light_cull's scratch: tile * (quarter * 4) + at most num_lights entries, for every macro tile
                            CHECK(p.scratch_words >= (size_t)p.macro_x * ((in.h + kPlanOwnerTile - 1) / kPlanOwnerTile) * (size_t)in.num_lights);
                            if (p.launch) CHECK(p.shade_grid == p.cull_grid * 16u || (!in.packed && p.shade_grid == (unsigned)(p.tiles32_x * p.tiles32_y)));
                            if (ex && !in.extra && !in.cone && !in.shadow) {
                                LightPlanIn plain = in; plain.entry = LIGHT_TILED;
                                CHECK(same_plan(p, light_plan(plain)));
                            }
                        }
                    }
    // (c)
    long sky_cases = 0, sky_refused = 0;
    for (int entry = LIGHT_STREAM; entry <= LIGHT_TILED_EX; entry++)
        for (unsigned bits = 0; bits < (1u << 7); bits++)
            for (int li = 0; li < 5; li++)
                for (int owned = 0; owned <= 1; owned++)
                    for (int si = 0; si < 3; si++) {
                        LightPlanIn in{};
                        unsigned b = bits;
                        auto next = [&b]() { const bool v = b & 1u; b >>= 1; return v; };
                        in.entry = (LightEntry)entry;
                        in.packed = next(); in.width_mult4 = next(); in.shadow = next(); in.extra = next(); in.cone = next();
                        in.hinted = next(); in.ranges_usable = next();
                        in.num_lights = kLights[li]; in.num_owned = owned;
                        const int* size = in.width_mult4 ? kSizes4[si] : kSizesOdd[si];
                        in.w = size[0]; in.h = size[1];
                        LightPlanIn safe = in;
                        CHECK(light_sky_ok(safe));
                        in.sky_not_zero = true;
                        CHECK(light_width_ok(in) == light_width_ok(safe));
                        if (!light_width_ok(in)) continue;
                        sky_cases++;
                        CHECK(light_sky_ok(in) == (in.entry == LIGHT_STREAM));
                        if (!light_sky_ok(in)) { sky_refused++; continue; }        // (the plan is asked for accepted calls only)
                        const LightPlan p = light_plan(in);
                        safe.hinted = false;
                        CHECK(same_plan(p, light_plan(safe)));
                        CHECK((int)p.shade >= 0 && p.shade < LV_COUNT);
                        if ((int)p.shade >= 0 && p.shade < LV_COUNT) CHECK(kFlags[p.shade].family == F_STREAM || kFlags[p.shade].family == F_SCALAR);
                    }
    std::printf("light_plan: outside sky_is_zero: %ld accepted widths (%ld refused: the tiled entry points)\n", sky_cases, sky_refused);
    for (int v = 0; v < LV_COUNT; v++)
        if (!reached[v]) { std::printf("FAIL shading variant %d is never chosen\n", v); failures++; }
    for (int c = 0; c < LC_COUNT; c++)
        if (!cull_reached[c]) { std::printf("FAIL culling variant %d is never chosen\n", c); failures++; }
    std::printf("light_plan: %ld cases (%ld refused widths, %ld the parent's entry point could not reach), %ld failures\n", cases, refused, unreachable, failures);
    return failures ? EXIT_FAILURE : EXIT_SUCCESS;
}
