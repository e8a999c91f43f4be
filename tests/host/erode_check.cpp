// CPU check of vr_erode.h, the definition of thermal erosion under a brush mask (vr_terrain_erode).  No HIP: g++ -std=c++17
// -ffp-contract=off -I vrenderer_amd/csrc.
//
//   erode_check                 the header's serial evaluator on seeded maps and dabs (maps of w, h in {1, 2, 3, 8, 17, 33}, 20 calls
//                               per map): dabs that all miss the map and a flat map change nothing, no texel outside the rectangle
//                               changes, and every byte stays inside the rectangle's [min, max] before the call.  Prints
//                               "N calls, F failures".
//   erode_check apply IN OUT    one call applied to a map by erode_serial, for tests/test_terrain_erode_cpu.py to compare with
//                               tests/erode_model.py.
//                               IN:  int32 w, h, n, iterations; float world_size, talus, rate; n x 5 floats
//                                    (x, z, radius, hardness, strength); w * h bytes
//                               OUT: int32 rect[4] = {x, y, w, h}; the eroded bytes
#include "vr_erode.h"

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

// prepares the dabs (n x 5 floats), drops the empty ones, runs the evaluator; rect = {x, y, w, h}
static void erode_call(std::vector<uint8_t>& map, int w, int h, const std::vector<float>& raw, float world, int iterations, float talus, float rate, int32_t rect[4])
{
    std::vector<BrushDab> dabs;
    int r[4] = { 0, 0, 0, 0 };
    for (size_t i = 0; i + 5 <= raw.size(); i += 5) {
        const BrushDab d = brush_prepare(raw[i], raw[i + 1], raw[i + 2], raw[i + 3], raw[i + 4], world, w, h);
        if (brush_dab_empty(d)) continue;
        if (dabs.empty()) { r[0] = d.x0; r[1] = d.y0; r[2] = d.x1; r[3] = d.y1; }
        else { r[0] = d.x0 < r[0] ? d.x0 : r[0]; r[1] = d.y0 < r[1] ? d.y0 : r[1]; r[2] = d.x1 > r[2] ? d.x1 : r[2]; r[3] = d.y1 > r[3] ? d.y1 : r[3]; }
        dabs.push_back(d);
    }
    rect[0] = rect[1] = rect[2] = rect[3] = 0;
    if (dabs.empty()) return;
    const size_t cells = (size_t)(r[2] - r[0]) * (size_t)(r[3] - r[1]);
    std::vector<float> mask(cells), a(cells), b(cells);
    erode_serial(map.data(), w, h, dabs.data(), dabs.size(), r, iterations, talus, rate, mask.data(), a.data(), b.data());
    rect[0] = r[0]; rect[1] = r[1]; rect[2] = r[2] - r[0]; rect[3] = r[3] - r[1];
}

static int run_check()
{
    const int sizes[] = { 1, 2, 3, 8, 17, 33 };
    long calls = 0, failures = 0;
    for (int w : sizes)
        for (int h : sizes)
            for (int k = 0; k < 20; k++) {
                const float world = 64.0f;
                std::vector<uint8_t> map((size_t)w * h);
                for (uint8_t& t : map) t = k % 5 == 0 ? 77 : (uint8_t)(rnd() * 256.0);             // every fifth map is flat
                std::vector<float> raw;
                const int n = 1 + (int)(rnd() * 4.0);
                for (int i = 0; i < n; i++) {
                    const bool miss = k % 7 == 0;                                                  // every seventh call misses the map
                    raw.push_back((float)((miss ? 3.0 + rnd() : rnd() * 1.4 - 0.7) * world));
                    raw.push_back((float)((rnd() * 1.4 - 0.7) * world));
                    raw.push_back((float)((miss ? 0.5 : 0.3 + rnd() * 20.0) * world / (w > h ? w : h)));
                    raw.push_back(i % 2 ? 0.7f : 0.0f);
                    raw.push_back((float)rnd());
                }
                const std::vector<uint8_t> before = map;
                int32_t rect[4];
                erode_call(map, w, h, raw, world, 1 + (int)(rnd() * 12.0), (float)(rnd() * 3.0), k % 2 ? 0.125f : 0.03f, rect);
                calls++;
                int lo = 255, hi = 0;
                for (int j = rect[1]; j < rect[1] + rect[3]; j++)
                    for (int i = rect[0]; i < rect[0] + rect[2]; i++) { const int v = before[(size_t)j * w + i]; lo = v < lo ? v : lo; hi = v > hi ? v : hi; }
                bool ok = true;
                for (int j = 0; j < h && ok; j++)
                    for (int i = 0; i < w && ok; i++) {
                        const bool in = i >= rect[0] && i < rect[0] + rect[2] && j >= rect[1] && j < rect[1] + rect[3];
                        const int v = map[(size_t)j * w + i], v0 = before[(size_t)j * w + i];
                        if (!in || k % 5 == 0 || k % 7 == 0) ok = v == v0;
                        else ok = v >= lo && v <= hi;
                        if (!ok) printf("FAIL %d x %d call %d: texel (%d, %d) %d -> %d, rect {%d, %d, %d, %d}, range [%d, %d]\n", w, h, k, i, j, v0, v, rect[0], rect[1], rect[2], rect[3], lo, hi);
                    }
                if (!ok) failures++;
            }
    printf("%ld calls, %ld failures\n", calls, failures);
    return failures ? 1 : 0;
}

static int run_apply(const char* in_path, const char* out_path)
{
    FILE* fi = fopen(in_path, "rb");
    if (!fi) { printf("cannot read %s\n", in_path); return 2; }
    int32_t hd[4]; float fl[3];
    if (fread(hd, 4, 4, fi) != 4 || fread(fl, 4, 3, fi) != 3) { fclose(fi); return 2; }
    const int w = hd[0], h = hd[1], n = hd[2], iterations = hd[3];
    if (w < 1 || h < 1 || w > 4096 || h > 4096 || n < 0 || n > 65536 || iterations < 1 || iterations > kErodeMaxIterations) { fclose(fi); return 2; }
    std::vector<float> raw((size_t)n * 5);
    std::vector<uint8_t> map((size_t)w * h);
    if (fread(raw.data(), 4, raw.size(), fi) != raw.size() || fread(map.data(), 1, map.size(), fi) != map.size()) { fclose(fi); return 2; }
    fclose(fi);
    int32_t rect[4];
    erode_call(map, w, h, raw, fl[0], iterations, fl[1], fl[2], rect);
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
