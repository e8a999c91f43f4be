// CPU check of vr_erode.h, the definition of thermal erosion under a brush mask (vr_terrain_erode).  No HIP: g++ -std=c++17
// -ffp-contract=off -I vrenderer_amd/csrc.
//
//   erode_check                 the header's serial evaluator on seeded maps and dabs (maps of w, h in {1, 2, 3, 8, 17, 33} and one of
//                               61 x 61, 20 calls per map): dabs that all miss the map and a flat map change nothing, no texel outside
//                               the rectangle changes, and every byte stays inside the rectangle's [min, max] before the call.  And
//                               against a tiled evaluation of the same header functions (erosion_check.h) that advances K sweeps per
//                               pass the way k_sweep_steps does, for tiles that do not divide the rectangle, K in {1, 2, 3, 5} and
//                               1 .. 14 iterations: the bytes must be equal.  Prints "N calls, F failures".
//   erode_check apply IN OUT    one call applied to a map by erode_serial, for tests/test_terrain_erode_cpu.py to compare with
//                               tests/erode_model.py.
//                               IN:  int32 w, h, n, iterations; float world_size, talus, rate; n x 5 floats
//                                    (x, z, radius, hardness, strength); w * h bytes
//                               OUT: int32 rect[4] = {x, y, w, h}; the eroded bytes
#include "vr_erode.h"
#include "erosion_check.h"

// the serial evaluator; rect = {x, y, w, h}
static void erode_call(std::vector<uint8_t>& map, int w, int h, const std::vector<float>& raw, float world, int iterations, float talus, float rate, int32_t rect[4])
{
    int r[4];
    const std::vector<BrushDab> dabs = prepare(raw, world, w, h, r);
    rect[0] = rect[1] = rect[2] = rect[3] = 0;
    if (dabs.empty()) return;
    const size_t cells = (size_t)(r[2] - r[0]) * (size_t)(r[3] - r[1]);
    std::vector<float> mask(cells), a(cells), b(cells);
    erode_serial(map.data(), w, h, dabs.data(), dabs.size(), r, iterations, talus, rate, mask.data(), a.data(), b.data());
    rect[0] = r[0]; rect[1] = r[1]; rect[2] = r[2] - r[0]; rect[3] = r[3] - r[1];
}

// the host-side model of the tiled evaluation (erosion_check.h): erode_edge x 8 in the header's order
struct ThermalModel {
    static constexpr int F = 1;
    float talus, talus_d, rate;
    void cell(const float* in, const float* im, size_t, int iw, size_t c, float* out) const
    {
        const size_t nb[8] = { c - iw - 1, c - iw, c - iw + 1, c - 1, c + 1, c + iw - 1, c + iw, c + iw + 1 };
        float acc = 0.0f;
        for (int e = 0; e < 8; e++) acc = erode_edge(acc, in[c], in[nb[e]], im[c], im[nb[e]], (e == 1 || e == 3 || e == 4 || e == 6) ? talus : talus_d, rate);
        out[c] = in[c] + acc;
    }
};

// The map the tiled K-sweeps-per-pass evaluation leaves, from the state zero sweeps leave (the mask, the bytes as floats).
static std::vector<uint8_t> tiled_call(const std::vector<uint8_t>& before, int w, int h, const std::vector<float>& raw, float world, int iterations, float talus, float rate,
                                       const int tile[2], int K)
{
    int r[4];
    const std::vector<BrushDab> dabs = prepare(raw, world, w, h, r);
    std::vector<uint8_t> tiled = before;
    if (dabs.empty()) return tiled;
    const int rw = r[2] - r[0], rh = r[3] - r[1];
    const size_t cells = (size_t)rw * (size_t)rh;
    std::vector<float> mask(cells), a(cells), b(cells);
    erode_serial(tiled.data(), w, h, dabs.data(), dabs.size(), r, 0, talus, rate, mask.data(), a.data(), b.data());
    const float* cur = tiled_run(ThermalModel{ talus, erode_diagonal_talus(talus), rate }, a.data(), b.data(), mask.data(), rw, rh, tile, K, iterations, [](const float*, int) {});
    for (int j = 0; j < rh; j++)
        for (int i = 0; i < rw; i++)
            if (mask[(size_t)j * rw + i] > 0.0f) tiled[(size_t)(r[1] + j) * w + (r[0] + i)] = erode_byte(cur[(size_t)j * rw + i]);
    return tiled;
}

static int run_check()
{
    const int sizes[] = { 1, 2, 3, 8, 17, 33 };
    std::vector<std::pair<int, int>> maps;
    for (int w : sizes)
        for (int h : sizes) maps.push_back({ w, h });
    maps.push_back({ 61, 61 });
    long calls = 0, failures = 0;
    int variant = 0;
    for (const std::pair<int, int>& wh : maps) {
            const int w = wh.first, h = wh.second;
            for (int k = 0; k < 20; k++, variant++) {
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
                const int iterations = 1 + (int)(rnd() * 14.0);
                const float talus = (float)(rnd() * 3.0), rate = k % 2 ? 0.125f : 0.03f;
                erode_call(map, w, h, raw, world, iterations, talus, rate, rect);
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
                const int* tile = kCheckTiles[variant % 4];
                const int K = kCheckKs[(variant / 4) % 4];
                const std::vector<uint8_t> tiled = tiled_call(before, w, h, raw, world, iterations, talus, rate, tile, K);
                if (tiled != map) {
                    ok = false;
                    long differ = 0;
                    for (size_t i = 0; i < map.size(); i++) differ += tiled[i] != map[i];
                    printf("FAIL %d x %d call %d: %ld bytes differ between the serial and the tiled evaluation (tile %d x %d, K %d, %d iterations)\n", w, h, k, differ,
                           tile[0], tile[1], K, iterations);
                }
                if (!ok) failures++;
            }
    }
    printf("%ld calls, %ld failures\n", calls, failures);
    return failures ? 1 : 0;
}

int main(int argc, char** argv)
{
    if (argc == 4 && !strcmp(argv[1], "apply"))
        return run_apply(argv[2], argv[3], 3, kErodeMaxIterations, [](std::vector<uint8_t>& map, int w, int h, const std::vector<float>& raw, int iterations, const float* fl, int32_t rect[4]) {
            erode_call(map, w, h, raw, fl[0], iterations, fl[1], fl[2], rect);
            return 0;
        });
    return run_check();
}
