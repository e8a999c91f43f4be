// Host check of vr_packed.h, the packed albedo footprint table of the fused tile pass, and of its dirty rule in vr_dirty.h.
//
//   1. decode: on random maps (1 x 1 up to 37 x 29, ragged ones included) every entry of the (w + 3) x (h + 3) table - the clamped rim
//      included - gives, through a 256-float table by the fields' byte offsets, the twelve floats of the four entries (ix, iy)
//      (ix + 1, iy) (ix, iy + 1) (ix + 1, iy + 1) of the float table (the decoded clamp-addressed texel (ix - 1, iy - 1), as
//      vr_fast_srgba8_entry writes it), compared as bits; every field is a multiple of four below 1024 and the top two bits are clear.
//   2. dirty rule: every rectangle of small maps is changed, the table rebuilt in full, and whatever changed lies inside
//      dirty_pack_srgba8_entries of the rectangle - which holds dirty_fast_srgba8_entries and is at most one entry per side wider than
//      what changed when every texel of the rectangle changes.
#include "vr_dirty.h"
#include "vr_packed.h"

#include <math.h>
#include <stdio.h>
#include <string.h>
#include <vector>

static uint32_t rng_state = 12345u;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

static float lut[256];
static int failures = 0;
static long cases = 0;
#define CHECK(cond, ...) do { cases++; if (!(cond)) { if (failures++ < 10) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

static std::vector<uint32_t> build(const std::vector<uint32_t>& map, int w, int h)
{
    std::vector<uint32_t> t((size_t)(w + 3) * (h + 3) * 4);
    for (int iy = 0; iy < h + 3; iy++) for (int ix = 0; ix < w + 3; ix++) vr_packed_entry(map.data(), w, h, ix, iy, &t[((size_t)iy * (w + 3) + ix) * 4]);
    return t;
}

static void check_decode(int w, int h)
{
    std::vector<uint32_t> map((size_t)w * h);
    for (auto& p : map) p = rnd() | (rnd() << 24);
    const std::vector<uint32_t> t = build(map, w, h);
    for (int iy = 0; iy < h + 3; iy++) for (int ix = 0; ix < w + 3; ix++) {
        const uint32_t* e = &t[((size_t)iy * (w + 3) + ix) * 4];
        for (int k = 0; k < 4; k++) {
            // the float table's entry (ix + (k & 1), iy + (k >> 1)): texel (that - 1), clamped
            const uint32_t p = map[(size_t)clampi(iy + (k >> 1) - 1, 0, h - 1) * w + clampi(ix + (k & 1) - 1, 0, w - 1)];
            CHECK((e[k] >> 30) == 0, "%dx%d (%d, %d) texel %d: top bits set", w, h, ix, iy, k);
            for (int c = 0; c < 3; c++) {
                const uint32_t off = vr_packed_lut_offset(e[k], c);
                CHECK((off & 3u) == 0 && off < 1024u, "%dx%d (%d, %d) texel %d channel %d: offset %u", w, h, ix, iy, k, c, off);
                float got, want = lut[(p >> (8 * c)) & 255u];
                memcpy(&got, reinterpret_cast<const char*>(lut) + off, 4);
                CHECK(memcmp(&got, &want, 4) == 0, "%dx%d (%d, %d) texel %d channel %d: %a, float table %a", w, h, ix, iy, k, c, got, want);
            }
        }
    }
}

static void check_dirty(int w, int h)
{
    std::vector<uint32_t> map((size_t)w * h);
    for (auto& p : map) p = rnd() & 0x7f7f7f7fu;
    const std::vector<uint32_t> before = build(map, w, h);
    for (int y0 = 0; y0 < h; y0++) for (int y1 = y0 + 1; y1 <= h; y1++) for (int x0 = 0; x0 < w; x0++) for (int x1 = x0 + 1; x1 <= w; x1++) {
        std::vector<uint32_t> m = map;
        for (int y = y0; y < y1; y++) for (int x = x0; x < x1; x++) m[(size_t)y * w + x] |= 0x80808080u;      // every texel of the rectangle changes
        const std::vector<uint32_t> after = build(m, w, h);
        DirtySpan sx, sy; sx.lo = x0; sx.hi = x1; sy.lo = y0; sy.hi = y1;
        const DirtySpan ex = dirty_pack_srgba8_entries(sx, w), ey = dirty_pack_srgba8_entries(sy, h);
        const DirtySpan fx = dirty_fast_srgba8_entries(sx, w), fy = dirty_fast_srgba8_entries(sy, h);
        CHECK(ex.lo <= fx.lo && fx.hi <= ex.hi && ey.lo <= fy.lo && fy.hi <= ey.hi, "%dx%d [%d,%d)x[%d,%d): the float table's span is not inside", w, h, x0, x1, y0, y1);
        int cx0 = w + 3, cx1 = -1, cy0 = h + 3, cy1 = -1;
        bool inside = true;
        for (int iy = 0; iy < h + 3; iy++) for (int ix = 0; ix < w + 3; ix++) {
            if (memcmp(&before[((size_t)iy * (w + 3) + ix) * 4], &after[((size_t)iy * (w + 3) + ix) * 4], 16) == 0) continue;
            inside = inside && ix >= ex.lo && ix < ex.hi && iy >= ey.lo && iy < ey.hi;
            cx0 = ix < cx0 ? ix : cx0; cx1 = ix > cx1 ? ix : cx1; cy0 = iy < cy0 ? iy : cy0; cy1 = iy > cy1 ? iy : cy1;
        }
        CHECK(inside, "%dx%d [%d,%d)x[%d,%d): a changed entry outside [%d,%d)x[%d,%d)", w, h, x0, x1, y0, y1, ex.lo, ex.hi, ey.lo, ey.hi);
        CHECK(cx0 - ex.lo <= 1 && ex.hi - 1 - cx1 <= 1 && cy0 - ey.lo <= 1 && ey.hi - 1 - cy1 <= 1, "%dx%d [%d,%d)x[%d,%d): the rule is wide: changed [%d,%d]x[%d,%d], predicted [%d,%d)x[%d,%d)",
              w, h, x0, x1, y0, y1, cx0, cx1, cy0, cy1, ex.lo, ex.hi, ey.lo, ey.hi);
    }
    // the whole map dirties the whole table
    const DirtySpan ax = dirty_pack_srgba8_entries(dirty_x(dirty_whole(w, h)), w), ay = dirty_pack_srgba8_entries(dirty_y(dirty_whole(w, h)), h);
    CHECK(ax.lo == 0 && ax.hi == w + 3 && ay.lo == 0 && ay.hi == h + 3, "%dx%d: the whole map is not the whole table", w, h);
}

int main()
{
    for (int i = 0; i < 256; i++) { const double c = i / 255.0; lut[i] = (float)(c <= 0.04045 ? c / 12.92 : pow((c + 0.055) / 1.055, 2.4)); }
    const int sizes[][2] = { { 1, 1 }, { 2, 1 }, { 1, 3 }, { 2, 2 }, { 5, 5 }, { 7, 2 }, { 16, 16 }, { 33, 17 }, { 37, 29 } };
    int maps = 0;
    for (const auto& s : sizes) { check_decode(s[0], s[1]); maps++; }
    int rect_maps = 0;
    for (int w = 1; w <= 6; w++) for (int h = 1; h <= 6; h++) { check_dirty(w, h); rect_maps++; }
    printf("%d maps decoded, %d maps of rectangles, %ld checks, %d failures\n", maps, rect_maps, cases, failures);
    return failures ? 1 : 0;
}
