// CPU check of vr_path.h, the definition of a path on a map (vr_terrain_path).  No HIP: g++ -std=c++17 -I vrenderer_amd/csrc.
//
//   path_check                  the span: 6000 seeded segments on seeded maps (square, 4:1 either way, 1 x n; zero-length segments;
//                               segments far outside the map and of enormous length; radii from a fraction of a texel to the whole
//                               map) - every texel of the map whose q against the segment is below 1 lies inside the segment's span,
//                               and its t in [0, 1].  Prints "N points, F failures".
//   path_check apply IN OUT     paths applied to a map with the header's functions (path_prepare, path_serial), for
//                               tests/test_path_model_cpu.py to compare with tests/path_model.py.
//                               IN:  int32 w, h, channels, sets; float world_size; w * h * channels bytes; per set: int32 op,
//                                    uint32 channel_mask, 3 floats (radius, hardness, opacity), 4 floats color, uint32 closed, uint32 n,
//                                    n x 3 floats (x, z, height)
//                               OUT: per set 7 floats (wx, wz, inv_r2, h2, k, opacity, cull_r), int32 segments, int32 x0, y0, x1, y1; per
//                                    segment 7 floats (ax, az, dx, dz, inv_len2, ha, dh) and 4 int32 (x0, x1, y0, y1); w * h * channels
//                                    bytes; w * h floats q, t, f; w * h int32 winner
#include "vr_path.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static double rnd()        // [0, 1)
{
    g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(g_rng >> 11) / 9007199254740992.0;
}

static long g_points = 0, g_failures = 0, g_covered = 0;

static void fail(const char* what, double a, double b, double c, double d)
{
    if (g_failures++ < 20) printf("FAIL %s: %.9g %.9g %.9g %.9g\n", what, a, b, c, d);
}

static void check_segment(int i, int w, int h, float world, const PathPoint& a, const PathPoint& b, float radius)
{
    const float color[4] = { 0, 0, 0, 0 };
    const PathConst k = path_const(radius, 0.5f, 1.0f, kPathLevel, color, 1u, world, w, h);
    const PathSeg s = path_segment(a, b, k, world, w, h);
    g_points++;
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            float q, t;
            path_texel(s, k, x, y, &q, &t);
            if (!(q < 1.0f)) continue;
            g_covered++;
            if (!(t >= 0.0f && t <= 1.0f)) fail("t outside [0, 1] on a covered texel", i, x, y, t);
            if (x < s.x0 || x >= s.x1 || y < s.y0 || y >= s.y1) fail("a covered texel outside the span", i, x, y, q);
        }
}

static int run_check()
{
    const int maps[6][2] = { { 64, 64 }, { 67, 45 }, { 256, 64 }, { 40, 160 }, { 1, 97 }, { 130, 1 } };
    for (int i = 0; i < 6000; i++) {
        const int w = maps[i % 6][0], h = maps[i % 6][1];
        const float world = i % 5 == 0 ? 1000.0f : 64.0f;
        const double S = world;
        const int kind = (i / 6) % 8;
        // ends: inside the map, or - kinds 5 .. 7 - out to 10, 1e4 and 1e9 world sizes away
        const double reach = kind < 5 ? 0.6 : (kind == 5 ? 10.0 : (kind == 6 ? 1.0e4 : 1.0e9));
        PathPoint a = { (float)((rnd() - 0.5) * 2.0 * reach * S), (float)((rnd() - 0.5) * 2.0 * reach * S), 10.0f };
        PathPoint b = { (float)((rnd() - 0.5) * 2.0 * reach * S), (float)((rnd() - 0.5) * 2.0 * reach * S), 200.0f };
        if (kind == 0) b = a;                                                           // zero length
        if (kind == 1) { b.x = a.x + (float)(rnd() * 1e-20); b.z = a.z; }                // so short that 1 / len^2 overflows, or zero
        if (kind == 7 && i % 2) { a.x = (float)((rnd() - 0.5) * S); a.z = (float)((rnd() - 0.5) * S); }     // one end inside, one far away
        const double tex = S / (w > h ? w : h);
        const float radius = (float)(i % 7 == 0 ? tex * (0.2 + rnd()) : (i % 7 == 1 ? S * (0.5 + rnd()) : tex * (1.0 + rnd() * 12.0)));
        check_segment(i, w, h, world, a, b, radius);
    }
    // a radius whose inverse square leaves fp32's range either way
    const PathPoint c = { 1.0f, 2.0f, 0.0f }, d = { 20.0f, -9.0f, 0.0f };
    check_segment(-1, 64, 64, 64.0f, c, d, 1.0e-25f);
    check_segment(-2, 64, 64, 64.0f, c, d, 1.0e25f);
    if (g_covered < 100000) fail("the sample covers too few texels to say anything", (double)g_covered, 0, 0, 0);
    printf("%ld covered texels\n", g_covered);
    printf("%ld points, %ld failures\n", g_points, g_failures);
    return g_failures ? 1 : 0;
}

static int run_apply(const char* in_path, const char* out_path)
{
    FILE* fi = fopen(in_path, "rb");
    if (!fi) { printf("cannot read %s\n", in_path); return 2; }
    int32_t hd[4]; float world;
    if (fread(hd, 4, 4, fi) != 4 || fread(&world, 4, 1, fi) != 1) { fclose(fi); return 2; }
    const int w = hd[0], h = hd[1], ch = hd[2], sets = hd[3];
    if (w < 1 || h < 1 || w > 4096 || h > 4096 || (ch != 1 && ch != 4) || sets < 0 || sets > 65536) { fclose(fi); return 2; }
    const size_t texels = (size_t)w * h;
    std::vector<uint8_t> map(texels * ch);
    if (fread(map.data(), 1, map.size(), fi) != map.size()) { fclose(fi); return 2; }
    FILE* fo = fopen(out_path, "wb");
    if (!fo) { fclose(fi); printf("cannot write %s\n", out_path); return 2; }
    bool ok = true;
    std::vector<float> q(texels), t(texels), f(texels);
    std::vector<int32_t> winner(texels);
    std::vector<PathSeg> segs;
    for (int s = 0; s < sets && ok; s++) {
        int32_t op; uint32_t cm, closed, n; float fl[7];
        if (fread(&op, 4, 1, fi) != 1 || fread(&cm, 4, 1, fi) != 1 || fread(fl, 4, 7, fi) != 7 || fread(&closed, 4, 1, fi) != 1 || fread(&n, 4, 1, fi) != 1) { ok = false; break; }
        if (n > (uint32_t)kPathMaxPoints) { ok = false; break; }
        std::vector<PathPoint> pts(n);
        for (uint32_t i = 0; i < n && ok; i++) { float v[3]; ok = fread(v, 4, 3, fi) == 3; pts[i] = PathPoint{ v[0], v[1], v[2] }; }
        if (!ok) break;
        const PathConst k = path_const(fl[0], fl[1], fl[2], op, fl + 3, cm, world, w, h);
        int32_t rect[4];
        path_prepare(pts.data(), n, closed != 0, k, world, w, h, segs, rect);
        const float consts[7] = { k.wx, k.wz, k.inv_r2, k.h2, k.k, k.opacity, k.cull_r };
        const int32_t ns = (int32_t)segs.size();
        ok = fwrite(consts, 4, 7, fo) == 7 && fwrite(&ns, 4, 1, fo) == 1 && fwrite(rect, 4, 4, fo) == 4;
        for (int32_t i = 0; i < ns && ok; i++) {
            const PathSeg& g = segs[i];
            const float sf[7] = { g.ax, g.az, g.dx, g.dz, g.inv_len2, g.ha, g.dh };
            const int32_t si[4] = { g.x0, g.x1, g.y0, g.y1 };
            ok = fwrite(sf, 4, 7, fo) == 7 && fwrite(si, 4, 4, fo) == 4;
        }
        std::vector<uint8_t> out = map;
        path_serial(out.data(), w, h, ch, segs.data(), (uint32_t)segs.size(), k, q.data(), t.data(), f.data(), winner.data());
        ok = ok && fwrite(out.data(), 1, out.size(), fo) == out.size() && fwrite(q.data(), 4, texels, fo) == texels && fwrite(t.data(), 4, texels, fo) == texels &&
             fwrite(f.data(), 4, texels, fo) == texels && fwrite(winner.data(), 4, texels, fo) == texels;
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
