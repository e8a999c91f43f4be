// CPU check of vr_brush.h, the definition of a brush stroke (vr_terrain_brush).  No HIP: g++ -std=c++17 -I vrenderer_amd/csrc.
//
//   brush_check                 containment: for maps of w, h in {1, 2, 3, 8, 17, 33} and 2000 seeded dabs per map - centres
//                               inside and outside the map, radii from 0.05 to 40 texels (log-uniform), any hardness, three world
//                               sizes - plus a handful at the ends of fp32's range, every texel of the WHOLE map that the header's
//                               own brush_weight puts inside the dab (q < 1) lies inside the span brush_prepare gave it.  The
//                               kernel visits a dab only inside its span, so a texel outside it would silently keep its value.
//                               Prints "N dabs, F failures".
//   brush_check apply IN OUT    a stroke applied to a map with the header's functions, the way k_brush applies it (per texel, the
//                               dabs in order), for tests/test_terrain_brush_cpu.py to compare with tests/brush_model.py.
//                               IN:  int32 op, w, h, n, channel_mask; float world_size, target, color[4]; n x 5 floats
//                                    (x, z, radius, hardness, strength); w * h * (PAINT ? 4 : 1) bytes
//                               OUT: int32 rect[4]; the stroked bytes
#include "vr_brush.h"

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

static long g_dabs = 0, g_failures = 0;

static void check_dab(const BrushDab& d, int w, int h, const char* what)
{
    g_dabs++;
    if (d.x0 < 0 || d.x1 > w || d.y0 < 0 || d.y1 > h) {
        g_failures++;
        printf("FAIL %s: %d x %d span [%d, %d) x [%d, %d) leaves the map\n", what, w, h, d.x0, d.x1, d.y0, d.y1);
        return;
    }
    for (int j = 0; j < h; j++)
        for (int i = 0; i < w; i++) {
            float f;
            if (!brush_weight(d, i, j, &f)) continue;
            if (i < d.x0 || i >= d.x1 || j < d.y0 || j >= d.y1 || !(f >= 0.0f && f <= 1.0f)) {
                g_failures++;
                printf("FAIL %s: %d x %d texel (%d, %d) weight %g outside span [%d, %d) x [%d, %d); c (%g, %g) s (%g, %g)\n", what, w, h, i, j, f,
                       d.x0, d.x1, d.y0, d.y1, d.cx, d.cz, d.sx, d.sz);
                return;
            }
        }
}

static int run_check()
{
    const int sizes[] = { 1, 2, 3, 8, 17, 33 };
    const float worlds[] = { 64.0f, 1.0f, 4096.0f };
    for (int w : sizes)
        for (int h : sizes) {
            for (int k = 0; k < 2000; k++) {
                const float S = worlds[k % 3];
                const double r_tex = 0.05 * pow(40.0 / 0.05, rnd());              // 0.05 .. 40 texels of the map's width
                // centres: mostly over the map, a share well outside, a share exactly on texel centres and map corners
                double x = (rnd() * 1.5 - 0.75) * S, z = (rnd() * 1.5 - 0.75) * S;
                if (k % 7 == 0) { x = ((int)(rnd() * (w + 1)) - 0.0) / w * S - S / 2; z = ((int)(rnd() * (h + 1)) - 0.0) / h * S - S / 2; }
                if (k % 11 == 0) { x = ((int)(rnd() * w) + 0.5) / w * S - S / 2; z = ((int)(rnd() * h) + 0.5) / h * S - S / 2; }
                check_dab(brush_prepare((float)x, (float)z, (float)(r_tex * S / w), (float)(rnd() * 0.999), 1.0f, S, w, h), w, h, "seeded");
            }
            // the ends of fp32's range: a centre that overflows, a scale that underflows or overflows
            const float big = 3.0e38f, tiny = 1.0e-44f;
            check_dab(brush_prepare(big, 0.0f, 1.0f, 0.5f, 1.0f, 1.0f, w, h), w, h, "huge centre");
            check_dab(brush_prepare(-big, big, big, 0.0f, 1.0f, 1.0f, w, h), w, h, "huge centre and radius");
            check_dab(brush_prepare(0.0f, 0.0f, big, 0.0f, 1.0f, 64.0f, w, h), w, h, "huge radius");
            check_dab(brush_prepare(0.0f, 0.0f, tiny, 0.9f, 1.0f, 64.0f, w, h), w, h, "tiny radius");
            check_dab(brush_prepare(big, -big, tiny, 0.0f, 1.0f, 1.0e-30f, w, h), w, h, "huge centre, tiny radius");
        }
    printf("%ld dabs, %ld failures\n", g_dabs, g_failures);
    return g_failures ? 1 : 0;
}

static int run_apply(const char* in_path, const char* out_path)
{
    FILE* fi = fopen(in_path, "rb");
    if (!fi) { printf("cannot read %s\n", in_path); return 2; }
    int32_t hd[5]; float fl[6];
    if (fread(hd, 4, 5, fi) != 5 || fread(fl, 4, 6, fi) != 6) { fclose(fi); return 2; }
    const int op = hd[0], w = hd[1], h = hd[2], n = hd[3], nc = op == kBrushPaint ? 4 : 1;
    const uint32_t mask = (uint32_t)hd[4];
    if (w < 1 || h < 1 || w > 4096 || h > 4096 || n < 0 || n > 65536) { fclose(fi); return 2; }
    std::vector<float> raw((size_t)n * 5);
    std::vector<uint8_t> map((size_t)w * h * nc);
    if (fread(raw.data(), 4, raw.size(), fi) != raw.size() || fread(map.data(), 1, map.size(), fi) != map.size()) { fclose(fi); return 2; }
    fclose(fi);
    std::vector<BrushDab> dabs;
    int32_t rect[4] = { 0, 0, 0, 0 };
    int x0 = 0, y0 = 0, x1 = 0, y1 = 0;
    for (int i = 0; i < n; i++) {
        const float* r = &raw[(size_t)i * 5];
        const BrushDab d = brush_prepare(r[0], r[1], r[2], r[3], r[4], fl[0], w, h);
        if (brush_dab_empty(d)) continue;
        if (dabs.empty()) { x0 = d.x0; y0 = d.y0; x1 = d.x1; y1 = d.y1; }
        else { x0 = d.x0 < x0 ? d.x0 : x0; y0 = d.y0 < y0 ? d.y0 : y0; x1 = d.x1 > x1 ? d.x1 : x1; y1 = d.y1 > y1 ? d.y1 : y1; }
        dabs.push_back(d);
    }
    if (!dabs.empty()) { rect[0] = x0; rect[1] = y0; rect[2] = x1 - x0; rect[3] = y1 - y0; }
    const std::vector<uint8_t> before = map;
    for (int j = 0; j < h; j++)
        for (int i = 0; i < w; i++) {
            float val[4], mean = 0.0f;
            for (int c = 0; c < nc; c++) val[c] = (float)before[((size_t)j * w + i) * nc + c];
            if (op == kBrushSmooth) {
                int sum = 0;
                for (int dy = -1; dy <= 1; dy++)
                    for (int dx = -1; dx <= 1; dx++) {
                        const int nx = i + dx < 0 ? 0 : (i + dx > w - 1 ? w - 1 : i + dx), ny = j + dy < 0 ? 0 : (j + dy > h - 1 ? h - 1 : j + dy);
                        sum += before[(size_t)ny * w + nx];
                    }
                mean = brush_mean9(sum);
            }
            bool touched = false;
            for (const BrushDab& d : dabs) {
                float f;
                if (i < d.x0 || i >= d.x1 || j < d.y0 || j >= d.y1 || !brush_weight(d, i, j, &f)) continue;
                touched = true;
                if (op == kBrushRaise) val[0] = brush_raise(val[0], f, d.strength);
                else if (op == kBrushFlatten) val[0] = brush_blend(val[0], f, d.strength, fl[1]);
                else if (op == kBrushSmooth) val[0] = brush_blend(val[0], f, d.strength, mean);
                else for (int c = 0; c < 4; c++) if (mask >> c & 1u) val[c] = brush_blend(val[c], f, d.strength, fl[2 + c]);
            }
            if (touched) for (int c = 0; c < nc; c++) map[((size_t)j * w + i) * nc + c] = brush_byte(val[c]);
        }
    FILE* fo = fopen(out_path, "wb");
    if (!fo) { printf("cannot write %s\n", out_path); return 2; }
    const bool ok = fwrite(rect, 4, 4, fo) == 4 && fwrite(map.data(), 1, map.size(), fo) == map.size();
    fclose(fo);
    return ok ? 0 : 2;
}

int main(int argc, char** argv)
{
    if (argc == 4 && !strcmp(argv[1], "apply")) return run_apply(argv[2], argv[3]);
    return run_check();
}
