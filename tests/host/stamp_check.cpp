// vr_stamp.h on the host, without HIP.
//   stamp_check                 seeded placements on small maps and stamps: no texel outside the prepared rectangle changes, every
//                               covered texel lies inside it, no prepared constant is an infinity or a NaN
//   stamp_check apply IN OUT    the cases of IN (tests/test_terrain_stamp_cpu.py writes them) through stamp_prepare and stamp_serial;
//                               OUT receives per case the eight prepared constants, the rectangle and the map's bytes
#include "vr_stamp.h"

#include <stdio.h>
#include <string.h>
#include <vector>

static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static double rnd()                       // [0, 1)
{
    g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17;
    return (double)(g_state >> 11) / 9007199254740992.0;
}

static long g_cases = 0, g_failures = 0;

template <int NC>
static void check_case(const StampDesc& d, float world, int w0, int h0, int sw, int sh, const char* what)
{
    g_cases++;
    std::vector<uint8_t> map((size_t)w0 * h0 * NC), stamp((size_t)sw * sh * NC);
    for (auto& b : map) b = (uint8_t)(rnd() * 256.0);
    for (auto& b : stamp) b = (uint8_t)(rnd() * 256.0);
    DirtyRect r;
    const StampConst k = stamp_prepare(d, world, w0, h0, sw, sh, &r);
    const float f[8] = { k.A00, k.A01, k.B0, k.A10, k.A11, k.B1, k.inv_u, k.inv_v };
    for (float v : f)
        if (!(v == v) || fabsf(v) > kTextureMaxFloat) { g_failures++; printf("FAIL %s: a prepared constant is not finite\n", what); return; }
    if (r.x0 < 0 || r.y0 < 0 || r.x1 > w0 || r.y1 > h0) { g_failures++; printf("FAIL %s: the rectangle leaves the map\n", what); return; }
    const auto fetch = [&](int x, int y) -> uint32_t {
        if (x < 0 || y < 0 || x >= sw || y >= sh) { g_failures++; printf("FAIL %s: a tap outside the stamp\n", what); return 0u; }
        const uint8_t* p = stamp.data() + ((size_t)y * sw + x) * NC;
        uint32_t t = 0;
        for (int c = 0; c < NC; c++) t |= (uint32_t)p[c] << (8 * c);
        return t;
    };
    // every covered texel of the whole map lies inside the rectangle
    for (int j = 0; j < h0; j++)
        for (int i = 0; i < w0; i++) {
            float val[NC];
            for (int c = 0; c < NC; c++) val[c] = (float)map[((size_t)j * w0 + i) * NC + c];
            const bool covered = stamp_texel<NC>(k, fetch, i, j, val);
            const bool in = i >= r.x0 && i < r.x1 && j >= r.y0 && j < r.y1;
            if (covered && !in) { g_failures++; printf("FAIL %s: texel (%d, %d) is covered outside the rectangle\n", what, i, j); return; }
            for (int c = 0; c < NC; c++)
                if (!(val[c] >= 0.0f && val[c] <= 255.0f)) { g_failures++; printf("FAIL %s: a value outside [0, 255]\n", what); return; }
        }
    // the serial evaluator over the WHOLE map changes nothing outside the rectangle
    std::vector<uint8_t> out = map;
    stamp_serial<NC>(out.data(), w0, h0, stamp.data(), k, dirty_whole(w0, h0));
    for (int j = 0; j < h0; j++)
        for (int i = 0; i < w0; i++) {
            const bool in = i >= r.x0 && i < r.x1 && j >= r.y0 && j < r.y1;
            if (!in && memcmp(&out[((size_t)j * w0 + i) * NC], &map[((size_t)j * w0 + i) * NC], NC)) {
                g_failures++; printf("FAIL %s: texel (%d, %d) changed outside the rectangle\n", what, i, j); return;
            }
        }
}

static int run_check()
{
    const int maps[4][2] = { { 1, 1 }, { 8, 8 }, { 17, 33 }, { 48, 40 } }, stamps[4][2] = { { 1, 1 }, { 5, 3 }, { 33, 17 }, { 64, 64 } };
    const float world = 64.0f;
    for (int i = 0; i < 200; i++) {
        StampDesc d;
        d.x = (float)((rnd() * 1.6 - 0.8) * world); d.z = (float)((rnd() * 1.6 - 0.8) * world);
        const double scale = i % 5 == 0 ? 0.01 : (i % 5 == 1 ? 3.0 : 0.6);
        d.size_x = (float)((0.02 + rnd()) * scale * world); d.size_z = (float)((0.02 + rnd()) * scale * world);
        d.rotation = i % 4 == 0 ? 0.0f : (float)((rnd() * 2.0 - 1.0) * 7.0);
        d.opacity = i % 6 == 0 ? 1.0f : (float)rnd();
        d.feather = i % 3 == 0 ? 0.0f : (float)rnd();
        d.gain = (float)((rnd() * 2.0 - 1.0) * 4.0); d.offset = (float)((rnd() * 2.0 - 1.0) * 255.0);
        d.op = i % 5; d.flags = 0; d.channel_mask = 1;
        if (i == 11) { d.size_x = 1.0e-30f; d.size_z = 3.0e38f; }
        if (i == 12) { d.x = 3.0e38f; d.z = -3.0e38f; }
        if (i == 13) { d.size_x = 3.0e38f; d.size_z = 1.0e-38f; d.feather = 1.0e-45f; }
        if (i == 14) { d.rotation = 3.0e38f; d.gain = 256.0f; d.offset = -255.0f; }
        for (const auto& m : maps)
            for (const auto& s : stamps) {
                char what[96];
                snprintf(what, sizeof(what), "set %d, map %dx%d, stamp %dx%d", i, m[0], m[1], s[0], s[1]);
                check_case<1>(d, world, m[0], m[1], s[0], s[1], what);
                StampDesc e = d;
                e.channel_mask = 1u + (uint32_t)(rnd() * 15.0); e.flags = i % 2 ? kStampUseAlpha : 0u;
                check_case<4>(e, world, m[0], m[1], s[0], s[1], what);
            }
    }
    printf("%ld cases, %ld failures\n", g_cases, g_failures);
    return g_failures ? 1 : 0;
}

template <int NC>
static bool apply_case(uint8_t* map, int w0, int h0, const uint8_t* stamp, const StampConst& k, const DirtyRect& r)
{
    stamp_serial<NC>(map, w0, h0, stamp, k, r);
    return true;
}

static int run_apply(const char* in_path, const char* out_path)
{
    FILE* fi = fopen(in_path, "rb");
    if (!fi) { printf("cannot read %s\n", in_path); return 2; }
    int32_t hd[4]; float world;
    if (fread(hd, 4, 4, fi) != 4 || fread(&world, 4, 1, fi) != 1) { fclose(fi); return 2; }
    const int w0 = hd[0], h0 = hd[1], nc = hd[2], cases = hd[3];
    if (w0 < 1 || h0 < 1 || w0 > 4096 || h0 > 4096 || (nc != 1 && nc != 4) || cases < 0 || cases > 65536) { fclose(fi); return 2; }
    std::vector<uint8_t> map((size_t)w0 * h0 * nc);
    if (fread(map.data(), 1, map.size(), fi) != map.size()) { fclose(fi); return 2; }
    FILE* fo = fopen(out_path, "wb");
    if (!fo) { fclose(fi); printf("cannot write %s\n", out_path); return 2; }
    bool ok = true;
    for (int s = 0; s < cases && ok; s++) {
        int32_t sz[2]; float f[9]; int32_t op; uint32_t cm, fl;
        if (fread(sz, 4, 2, fi) != 2 || fread(f, 4, 9, fi) != 9 || fread(&op, 4, 1, fi) != 1 || fread(&cm, 4, 1, fi) != 1 || fread(&fl, 4, 1, fi) != 1) { ok = false; break; }
        if (sz[0] < 1 || sz[1] < 1 || sz[0] > kStampMaxSide || sz[1] > kStampMaxSide) { ok = false; break; }
        std::vector<uint8_t> stamp((size_t)sz[0] * sz[1] * nc);
        if (fread(stamp.data(), 1, stamp.size(), fi) != stamp.size()) { ok = false; break; }
        StampDesc d;
        d.x = f[0]; d.z = f[1]; d.size_x = f[2]; d.size_z = f[3]; d.rotation = f[4]; d.opacity = f[5]; d.feather = f[6]; d.gain = f[7]; d.offset = f[8];
        d.op = op; d.channel_mask = cm; d.flags = fl;
        DirtyRect r;
        const StampConst k = stamp_prepare(d, world, w0, h0, sz[0], sz[1], &r);
        std::vector<uint8_t> out = map;
        if (!dirty_empty(r)) { if (nc == 1) apply_case<1>(out.data(), w0, h0, stamp.data(), k, r); else apply_case<4>(out.data(), w0, h0, stamp.data(), k, r); }
        const float c[8] = { k.A00, k.A01, k.B0, k.A10, k.A11, k.B1, k.inv_u, k.inv_v };
        const int32_t rect[4] = { r.x0, r.y0, r.x1, r.y1 };
        ok = fwrite(c, 4, 8, fo) == 8 && fwrite(rect, 4, 4, fo) == 4 && fwrite(out.data(), 1, out.size(), fo) == out.size();
    }
    fclose(fi);
    fclose(fo);
    return ok ? 0 : 2;
}

int main(int argc, char** argv)
{
    if (argc == 4 && !strcmp(argv[1], "apply")) return run_apply(argv[2], argv[3]);
    return run_check();
}
