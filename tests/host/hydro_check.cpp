// CPU check of vr_hydro.h, the definition of hydraulic erosion under a brush mask (vr_terrain_erode_hydraulic).  No HIP: g++
// -std=c++17 -ffp-contract=off -I vrenderer_amd/csrc.
//
//   hydro_check                 the header's serial evaluator on seeded maps and dabs (maps of w, h in {1, 2, 3, 8, 17, 33, 61}, 8 calls
//                               per map) against a tiled evaluation of the same header functions that advances K sweeps per pass
//                               the way k_sweep_steps does (erosion_check.h) - a tile plus a halo of K cells, zeros beyond the rectangle, the valid
//                               region one ring smaller per sweep - for tiles that do not divide the rectangle, K in {1, 2, 3, 5}
//                               and 1 .. 14 iterations: the bytes must be equal.  Also: no texel outside the rectangle or with
//                               mask 0 changes, dabs that all miss the map, rain = 0 and capacity = 0 change nothing, no d or s is
//                               ever negative, and on every edge of the states met the giver's q and ts are the taker's, bit for
//                               bit.  Prints "N calls, E edges, F failures".
//   hydro_check apply IN OUT    one call applied to a map by hydro_serial, for tests/test_terrain_hydro_cpu.py to compare with
//                               tests/hydro_model.py.
//                               IN:  int32 w, h, n, iterations; float world_size, rain, flow, capacity, dissolve, deposit,
//                                    evaporation; n x 5 floats (x, z, radius, hardness, strength); w * h bytes
//                               OUT: int32 rect[4] = {x, y, w, h}; the eroded bytes
#include "vr_hydro.h"
#include "erosion_check.h"

// the serial evaluator; rect = {x, y, w, h}; false if a d or an s went negative
static bool serial_call(std::vector<uint8_t>& map, int w, int h, const std::vector<float>& raw, float world, int iterations, const HydroConst& k, int32_t rect[4])
{
    int r[4];
    const std::vector<BrushDab> dabs = prepare(raw, world, w, h, r);
    rect[0] = rect[1] = rect[2] = rect[3] = 0;
    if (dabs.empty()) return true;
    const size_t cells = (size_t)(r[2] - r[0]) * (size_t)(r[3] - r[1]);
    std::vector<float> mask(cells), a(3 * cells), b(3 * cells);
    const bool ok = hydro_serial(map.data(), w, h, dabs.data(), dabs.size(), r, iterations, k, mask.data(), a.data(), b.data());
    rect[0] = r[0]; rect[1] = r[1]; rect[2] = r[2] - r[0]; rect[3] = r[3] - r[1];
    return ok;
}

// the host-side model of the tiled evaluation (erosion_check.h): hydro_edge x 4 in the header's order, then hydro_cell
struct HydroModel {
    static constexpr int F = 3;
    HydroConst k;
    void cell(const float* in, const float* im, size_t icells, int iw, size_t c, float* out) const
    {
        const size_t nb[4] = { c - iw, c - 1, c + 1, c + iw };
        HydroAcc acc = { 0.0f, 0.0f, 0.0f };
        for (int e = 0; e < 4; e++)
            hydro_edge(acc, in[c], in[icells + c], in[2 * icells + c], im[c], in[nb[e]], in[icells + nb[e]], in[2 * icells + nb[e]], im[nb[e]], k.flow);
        hydro_cell(in[c], in[icells + c], in[2 * icells + c], im[c], acc, k, &out[c], &out[icells + c], &out[2 * icells + c]);
    }
};

static bool same_bits(float a, float b) { return memcmp(&a, &b, 4) == 0; }

// every edge of the planes, from both ends: the giver's q and ts are the taker's; returns the number of edges that disagree
static long edge_failures(const float* st, const float* mask, int rw, int rh, float flow, long* edges)
{
    const size_t cells = (size_t)rw * (size_t)rh;
    long bad = 0;
    for (int j = 0; j < rh; j++)
        for (int i = 0; i < rw; i++)
            for (int dir = 0; dir < 2; dir++) {
                const int ni = i + (dir == 0), nj = j + (dir == 1);
                if (ni >= rw || nj >= rh) continue;
                const size_t c = (size_t)j * rw + i, n = (size_t)nj * rw + ni;
                HydroAcc ac = { 0.0f, 0.0f, 0.0f }, an = { 0.0f, 0.0f, 0.0f };
                HydroFlux xc, xn;
                hydro_edge(ac, st[c], st[cells + c], st[2 * cells + c], mask[c], st[n], st[cells + n], st[2 * cells + n], mask[n], flow, &xc);
                hydro_edge(an, st[n], st[cells + n], st[2 * cells + n], mask[n], st[c], st[cells + c], st[2 * cells + c], mask[c], flow, &xn);
                const float qc = xc.q, tc = xc.ts, qn = xn.q, tn = xn.ts;
                const bool gc = xc.gives, gn = xn.gives;
                (*edges)++;
                const bool tie = gc && gn;                                  // equal surfaces: both ends give, and what they give is zero
                const bool ok = tie ? (qc == 0.0f && qn == 0.0f && tc == 0.0f && tn == 0.0f) : (same_bits(qc, qn) && same_bits(tc, tn));
                // what one end loses the other gains: the sums move by the same q and ts
                const bool moved = tie || (gc ? (same_bits(ac.out, qc) && an.out == 0.0f) : (same_bits(an.out, qn) && ac.out == 0.0f));
                if (!ok || !moved) bad++;
            }
    return bad;
}

static int run_check()
{
    const int sizes[] = { 1, 2, 3, 8, 17, 33, 61 };
    long calls = 0, failures = 0, edges = 0;
    int variant = 0;
    for (int w : sizes)
        for (int h : sizes)
            for (int c = 0; c < 8; c++, variant++) {
                const float world = 64.0f;
                std::vector<uint8_t> map((size_t)w * h);
                for (uint8_t& t : map) t = (uint8_t)(rnd() * 256.0);
                std::vector<float> raw;
                const int n = 1 + (int)(rnd() * 4.0);
                const bool miss = c == 5;                                                          // one call per map misses it
                for (int i = 0; i < n; i++) {
                    raw.push_back((float)((miss ? 3.0 + rnd() : rnd() * 1.4 - 0.7) * world));
                    raw.push_back((float)((rnd() * 1.4 - 0.7) * world));
                    raw.push_back((float)((miss ? 0.5 : 0.3 + rnd() * 30.0) * world / (w > h ? w : h)));
                    raw.push_back(i % 2 ? 0.7f : 0.0f);
                    raw.push_back(i == 1 ? 0.0f : (float)rnd());                                   // the second dab covers texels with opacity 0
                }
                HydroConst k = { (float)(rnd() * 4.0), (float)(0.05 + rnd() * 0.95), (float)(rnd() * 16.0), (float)rnd(), (float)rnd(), hydro_keep((float)(rnd() * 0.3)) };
                if (c == 6) k.rain = 0.0f;                                                         // no water: nothing changes
                if (c == 7) k.capacity = 0.0f;                                                     // water moves, nothing dissolves
                const int iterations = 1 + (int)(rnd() * 14.0);
                const int* tile = kCheckTiles[variant % 4];
                const int K = kCheckKs[(variant / 4) % 4];
                const std::vector<uint8_t> before = map;
                int32_t rect[4];
                bool ok = serial_call(map, w, h, raw, world, iterations, k, rect);
                calls++;
                if (!ok) printf("FAIL %d x %d call %d: a negative d or s\n", w, h, c);
                // the tiled evaluation, from the state iterations = 0 leaves (the mask, the bytes as floats, rain * mask, 0)
                int r[4];
                const std::vector<BrushDab> dabs = prepare(raw, world, w, h, r);
                std::vector<uint8_t> tiled = before;
                const int rw = r[2] - r[0], rh = r[3] - r[1];
                if (!dabs.empty()) {
                    const size_t cells = (size_t)rw * (size_t)rh;
                    std::vector<float> mask(cells), a(3 * cells), b(3 * cells);
                    std::vector<uint8_t> untouched = before;
                    hydro_serial(untouched.data(), w, h, dabs.data(), dabs.size(), r, 0, k, mask.data(), a.data(), b.data());
                    if (untouched != before) { ok = false; printf("FAIL %d x %d call %d: zero sweeps changed the map\n", w, h, c); }
                    const float* cur = tiled_run(HydroModel{ k }, a.data(), b.data(), mask.data(), rw, rh, tile, K, iterations, [&](const float* st, int done) {
                        const long bad = edge_failures(st, mask.data(), rw, rh, k.flow, &edges);
                        if (bad) { ok = false; printf("FAIL %d x %d call %d: %ld edges whose ends disagree after %d sweeps\n", w, h, c, bad, done); }
                    });
                    for (size_t i = 0; i < 3 * cells; i++)
                        if (i >= cells && !(cur[i] >= 0.0f)) { ok = false; printf("FAIL %d x %d call %d: tiled d or s negative\n", w, h, c); break; }
                    for (int j = 0; j < rh; j++)
                        for (int i = 0; i < rw; i++) {
                            const size_t at = (size_t)j * rw + i;
                            if (mask[at] > 0.0f) tiled[(size_t)(r[1] + j) * w + (r[0] + i)] = hydro_byte(cur[at], cur[2 * cells + at]);
                            else if (map[(size_t)(r[1] + j) * w + (r[0] + i)] != before[(size_t)(r[1] + j) * w + (r[0] + i)]) {
                                ok = false; printf("FAIL %d x %d call %d: texel (%d, %d) of mask 0 changed\n", w, h, c, r[0] + i, r[1] + j);
                            }
                        }
                }
                if (tiled != map) {
                    ok = false;
                    long differ = 0;
                    for (size_t i = 0; i < map.size(); i++) differ += tiled[i] != map[i];
                    printf("FAIL %d x %d call %d: %ld bytes differ between the serial and the tiled evaluation (tile %d x %d, K %d, %d iterations)\n", w, h, c, differ,
                           tile[0], tile[1], K, iterations);
                }
                for (int j = 0; j < h && ok; j++)
                    for (int i = 0; i < w && ok; i++) {
                        const bool in = i >= rect[0] && i < rect[0] + rect[2] && j >= rect[1] && j < rect[1] + rect[3];
                        if ((!in || miss || c == 6 || c == 7) && map[(size_t)j * w + i] != before[(size_t)j * w + i]) {
                            ok = false;
                            printf("FAIL %d x %d call %d: texel (%d, %d) %d -> %d, rect {%d, %d, %d, %d}\n", w, h, c, i, j, before[(size_t)j * w + i], map[(size_t)j * w + i],
                                   rect[0], rect[1], rect[2], rect[3]);
                        }
                    }
                if (!ok) failures++;
            }
    printf("%ld calls, %ld edges, %ld failures\n", calls, edges, failures);
    return failures ? 1 : 0;
}

int main(int argc, char** argv)
{
    if (argc == 4 && !strcmp(argv[1], "apply"))
        return run_apply(argv[2], argv[3], 7, kHydroMaxIterations, [](std::vector<uint8_t>& map, int w, int h, const std::vector<float>& raw, int iterations, const float* fl, int32_t rect[4]) {
            const HydroConst k = { fl[1], fl[2], fl[3], fl[4], fl[5], hydro_keep(fl[6]) };
            if (serial_call(map, w, h, raw, fl[0], iterations, k, rect)) return 0;
            printf("a negative d or s\n");
            return 3;
        });
    return run_check();
}
