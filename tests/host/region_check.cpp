// CPU check of vr_region.h, the definition of a region on a map (vr_terrain_region).  No HIP: g++ -std=c++17 -I vrenderer_amd/csrc.
//
//   region_check                the span: 3000 seeded polygons of 3 .. 7 vertices on six maps (square, 4:1 either way, odd sizes, 1 x n,
//                               n x 1) - vertices exactly on texel centres and on texel rows, horizontal and 45 degree edges through
//                               texel centres, zero-length edges, vertices out to 1e9 world sizes away: for every edge and every texel
//                               of its map, a texel outside the edge's span has neither `left` nor q < 1; a texel with q < 1 lies
//                               inside the distance box; and the whole map classified tile by tile with only the edges whose spans
//                               meet the tile has the parity and q* of no cull.  Prints "N polygons, F failures".
//   region_check apply IN OUT   regions applied to a map with the header's functions (region_prepare, region_serial), for
//                               tests/test_region_model_cpu.py to compare with tests/region_model.py.
//                               IN:  int32 w, h, channels, sets; float world_size; w * h * channels bytes; per set: int32 op,
//                                    uint32 channel_mask, 3 floats (target, feather, opacity), 4 floats color, uint32 flags,
//                                    uint32 num_contours, uint32 n, num_contours x uint32 counts, n x 2 floats (x, z)
//                               OUT: per set 6 floats (wx, wz, inv_r2, opacity, target, cull_r), uint32 flags, int32 edges, int32 x0, y0,
//                                    x1, y1; per edge 6 floats (ax, az, dx, dz, inv_len2, bz) and 5 int32 (x0, x1, y0, y1, dist_x1);
//                                    w * h * channels bytes; w * h bytes inside; w * h floats q, f
#include "vr_region.h"

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

static long g_polygons = 0, g_failures = 0, g_left = 0, g_near = 0;

static void fail(const char* what, double a, double b, double c, double d)
{
    if (g_failures++ < 20) printf("FAIL %s: %.9g %.9g %.9g %.9g\n", what, a, b, c, d);
}

static void check_polygon(int id, int w, int h, float world, const std::vector<RegionPoint>& pts, float feather)
{
    const float color[4] = { 0, 0, 0, 0 };
    const RegionConst k = region_const(feather, 1.0f, 100.0f, kRegionLevel, 0u, color, 1u, world, w, h);
    std::vector<RegionVertex> verts;
    std::vector<RegionEdge> edges;
    int32_t rect[4];
    region_prepare(pts.data(), (uint32_t)pts.size(), nullptr, 0, k, world, w, h, verts, edges, rect);
    g_polygons++;
    const bool soft = (k.flags & kRegionSoft) != 0;
    // every edge, the dropped ones too, against every texel: nothing outside the span
    for (size_t s = 0; s < pts.size(); s++) {
        const RegionEdge e = region_edge(verts[s], verts[(s + 1) % pts.size()], k, w, h);
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) {
                float px, pz, q = 2.0f, t = 0.0f;
                path_offset(e.ax, e.az, k.wx, k.wz, x, y, &px, &pz);
                const uint32_t left = region_left(e, px, pz, (float)y);
                if (soft) path_nearest(px, pz, e.dx, e.dz, e.inv_len2, k.inv_r2, &q, &t);
                const bool in_span = x >= e.x0 && x < e.x1 && y >= e.y0 && y < e.y1;
                g_left += left; g_near += q < 1.0f;
                if (left && !in_span) fail("an edge counts for a texel outside its span", id, (double)s, x, y);
                if (q < 1.0f && !(in_span && x < e.dist_x1)) fail("a texel with q < 1 outside the distance box", id, (double)s, x, y);
            }
    }
    // tile by tile with the culled list against no cull
    const uint32_t n = (uint32_t)edges.size();
    std::vector<uint8_t> map((size_t)w * h, 0), inside((size_t)w * h);
    std::vector<float> q((size_t)w * h);
    region_serial(map.data(), w, h, 1, edges.data(), n, k, inside.data(), q.data(), nullptr);
    bool any_inside = false;
    for (int ty = 0; ty < h; ty += 8)
        for (int tx = 0; tx < w; tx += 32) {
            const int tx1 = tx + 32 < w ? tx + 32 : w, ty1 = ty + 8 < h ? ty + 8 : h;
            for (int y = ty; y < ty1; y++)
                for (int x = tx; x < tx1; x++) {
                    uint32_t par = 0; float best = 1.0f;
                    for (uint32_t s = 0; s < n; s++) {
                        const RegionEdge& e = edges[s];
                        if (!(e.x0 < tx1 && e.x1 > tx && e.y0 < ty1 && e.y1 > ty)) continue;
                        float px, pz, qq, t;
                        path_offset(e.ax, e.az, k.wx, k.wz, x, y, &px, &pz);
                        par ^= region_left(e, px, pz, (float)y);
                        if (soft && e.dist_x1 > tx) { path_nearest(px, pz, e.dx, e.dz, e.inv_len2, k.inv_r2, &qq, &t); if (qq < best) best = qq; }
                    }
                    const size_t at = (size_t)y * w + x;
                    any_inside = any_inside || par;
                    if (par != inside[at] || memcmp(&best, &q[at], 4)) fail("the tile cull shows", id, x, y, best);
                    const bool in_rect = x >= rect[0] && x < rect[2] && y >= rect[1] && y < rect[3];
                    if ((par || best < 1.0f) && !in_rect) fail("a covered texel outside the call's rectangle", id, x, y, par);
                }
        }
    (void)any_inside;
}

static float snap(double world_coord, int n, double S, int kind)
{
    // kind 1: exactly on a texel centre; kind 2: exactly between two
    if (kind == 0) return (float)world_coord;
    const double tex = floor((world_coord + S / 2) / S * n) + (kind == 2 ? 0.5 : 0.0);
    return (float)((tex + 0.5) / n * S - S / 2);
}

static int run_check()
{
    const int maps[6][2] = { { 64, 64 }, { 67, 45 }, { 128, 32 }, { 40, 96 }, { 1, 70 }, { 90, 1 } };
    for (int i = 0; i < 3000; i++) {
        const int w = maps[i % 6][0], h = maps[i % 6][1];
        const float world = i % 5 == 0 ? 1000.0f : 64.0f;
        const double S = world;
        const int kind = (i / 6) % 8;
        const double reach = kind < 5 ? 0.6 : (kind == 5 ? 10.0 : (kind == 6 ? 1.0e4 : 1.0e9));
        const int nv = 3 + (int)(rnd() * 5.0);
        std::vector<RegionPoint> pts(nv);
        for (int v = 0; v < nv; v++) {
            const bool far_one = kind < 7 || v % 2 == 0;                                          // kind 7: every other vertex inside the map
            const double r = far_one ? reach : 0.5;
            const int sx = kind == 1 || kind == 2 ? kind : 0, sz = kind == 1 || kind == 3 ? 1 : (kind == 2 ? 2 : 0);
            pts[v].x = snap((rnd() - 0.5) * 2.0 * r * S, w, S, r < 1.0 ? sx : 0);
            pts[v].z = snap((rnd() - 0.5) * 2.0 * r * S, h, S, r < 1.0 ? sz : 0);
        }
        if (kind == 3 && nv > 3) pts[1].z = pts[0].z;                                              // a horizontal edge along a texel row
        if (kind == 1 && w == h) {                                                                // a 45 degree edge through texel centres
            const double step = S / w * (double)(1 + (int)(rnd() * 9.0));
            pts[1].x = (float)((double)pts[0].x + step); pts[1].z = (float)((double)pts[0].z + step);
        }
        if (kind == 4) pts[nv - 1] = pts[nv - 2];                                                  // a zero-length edge
        const double tex = S / (w > h ? w : h);
        const float feather = (float)(i % 4 == 0 ? 0.0 : (i % 4 == 1 ? tex * (0.2 + rnd()) : tex * (1.0 + rnd() * 10.0)));
        check_polygon(i, w, h, world, pts, feather);
    }
    if (g_left < 100000 || g_near < 100000) fail("the sample says too little", (double)g_left, (double)g_near, 0, 0);
    printf("%ld crossings, %ld near texels\n", g_left, g_near);
    printf("%ld polygons, %ld failures\n", g_polygons, g_failures);
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
    std::vector<float> q(texels), f(texels);
    std::vector<uint8_t> inside(texels);
    std::vector<RegionVertex> verts;
    std::vector<RegionEdge> edges;
    for (int s = 0; s < sets && ok; s++) {
        int32_t op; uint32_t cm, flags, nc, n; float fl[7];
        if (fread(&op, 4, 1, fi) != 1 || fread(&cm, 4, 1, fi) != 1 || fread(fl, 4, 7, fi) != 7 || fread(&flags, 4, 1, fi) != 1 || fread(&nc, 4, 1, fi) != 1 ||
            fread(&n, 4, 1, fi) != 1) { ok = false; break; }
        if (n > (uint32_t)kRegionMaxPoints || nc > n) { ok = false; break; }
        std::vector<uint32_t> counts(nc);
        if (nc && fread(counts.data(), 4, nc, fi) != nc) { ok = false; break; }
        std::vector<RegionPoint> pts(n);
        if (n && fread(pts.data(), 8, n, fi) != n) { ok = false; break; }
        if (!region_contours_ok(n, nc ? counts.data() : nullptr, nc)) { ok = false; break; }
        const RegionConst k = region_const(fl[1], fl[2], fl[0], op, flags, fl + 3, cm, world, w, h);
        int32_t rect[4];
        region_prepare(pts.data(), n, nc ? counts.data() : nullptr, nc, k, world, w, h, verts, edges, rect);
        const float consts[6] = { k.wx, k.wz, k.inv_r2, k.opacity, k.target, k.cull_r };
        const int32_t ne = (int32_t)edges.size();
        ok = fwrite(consts, 4, 6, fo) == 6 && fwrite(&k.flags, 4, 1, fo) == 1 && fwrite(&ne, 4, 1, fo) == 1 && fwrite(rect, 4, 4, fo) == 4;
        for (int32_t i = 0; i < ne && ok; i++) {
            const RegionEdge& g = edges[i];
            const float ef[6] = { g.ax, g.az, g.dx, g.dz, g.inv_len2, g.bz };
            const int32_t ei[5] = { g.x0, g.x1, g.y0, g.y1, g.dist_x1 };
            ok = fwrite(ef, 4, 6, fo) == 6 && fwrite(ei, 4, 5, fo) == 5;
        }
        std::vector<uint8_t> out = map;
        region_serial(out.data(), w, h, ch, edges.data(), (uint32_t)edges.size(), k, inside.data(), q.data(), f.data());
        ok = ok && fwrite(out.data(), 1, out.size(), fo) == out.size() && fwrite(inside.data(), 1, texels, fo) == texels && fwrite(q.data(), 4, texels, fo) == texels &&
             fwrite(f.data(), 4, texels, fo) == texels;
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
