// CPU check of vr_hydro.h, the definition of hydraulic erosion under a brush mask (vr_terrain_erode_hydraulic).  No HIP: g++
// -std=c++17 -ffp-contract=off -I vrenderer_amd/csrc.
//
//   hydro_check                 the header's serial evaluator on seeded maps and dabs (maps of w, h in {1, 2, 3, 8, 17, 33, 61}, 8 calls
//                               per map) against a tiled evaluation of the same header functions that advances K sweeps per pass
//                               the way k_hydro_steps does - a tile plus a halo of K cells, zeros beyond the rectangle, the valid
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

// prepares the dabs (n x 5 floats) and drops the empty ones; r = {x0, y0, x1, y1}, all zero if none is left
static std::vector<BrushDab> prepare(const std::vector<float>& raw, float world, int w, int h, int r[4])
{
    std::vector<BrushDab> dabs;
    r[0] = r[1] = r[2] = r[3] = 0;
    for (size_t i = 0; i + 5 <= raw.size(); i += 5) {
        const BrushDab d = brush_prepare(raw[i], raw[i + 1], raw[i + 2], raw[i + 3], raw[i + 4], world, w, h);
        if (brush_dab_empty(d)) continue;
        if (dabs.empty()) { r[0] = d.x0; r[1] = d.y0; r[2] = d.x1; r[3] = d.y1; }
        else { r[0] = d.x0 < r[0] ? d.x0 : r[0]; r[1] = d.y0 < r[1] ? d.y0 : r[1]; r[2] = d.x1 > r[2] ? d.x1 : r[2]; r[3] = d.y1 > r[3] ? d.y1 : r[3]; }
        dabs.push_back(d);
    }
    return dabs;
}

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

// One pass over the planes of the rectangle (h, d, s: `cells` floats apart) the way the device's step kernel makes it: per tile an
// image of (tw + 2K) x (th + 2K) cells, zeros beyond the rectangle, `steps` <= K sweeps on two copies, the tile stored to dst.
static void tiled_pass(const float* src, float* dst, const float* mask, int rw, int rh, int tw, int th, int K, int steps, const HydroConst& k)
{
    const size_t cells = (size_t)rw * (size_t)rh;
    const int iw = tw + 2 * K, ih = th + 2 * K;
    const size_t icells = (size_t)iw * (size_t)ih;
    std::vector<float> im(icells), f[2] = { std::vector<float>(3 * icells), std::vector<float>(3 * icells) };
    for (int ty0 = 0; ty0 < rh; ty0 += th)
        for (int tx0 = 0; tx0 < rw; tx0 += tw) {
            const int ox = tx0 - K, oy = ty0 - K;
            for (int ly = 0; ly < ih; ly++)
                for (int lx = 0; lx < iw; lx++) {
                    const int x = ox + lx, y = oy + ly;
                    const bool in = x >= 0 && x < rw && y >= 0 && y < rh;
                    const size_t at = in ? (size_t)y * rw + x : 0, i = (size_t)ly * iw + lx;
                    im[i] = in ? mask[at] : 0.0f;
                    for (int p = 0; p < 3; p++) f[0][p * icells + i] = in ? src[p * cells + at] : 0.0f;
                }
            int cur = 0;
            for (int s = 1; s <= steps; s++, cur ^= 1) {
                const float* in = f[cur].data();
                float* out = f[cur ^ 1].data();
                for (int ly = s; ly < ih - s; ly++)
                    for (int lx = s; lx < iw - s; lx++) {
                        const size_t c = (size_t)ly * iw + lx;
                        const size_t nb[4] = { c - iw, c - 1, c + 1, c + iw };
                        HydroAcc acc = { 0.0f, 0.0f, 0.0f };
                        for (int e = 0; e < 4; e++)
                            hydro_edge(acc, in[c], in[icells + c], in[2 * icells + c], im[c], in[nb[e]], in[icells + nb[e]], in[2 * icells + nb[e]], im[nb[e]], k.flow);
                        hydro_cell(in[c], in[icells + c], in[2 * icells + c], im[c], acc, k, &out[c], &out[icells + c], &out[2 * icells + c]);
                    }
            }
            for (int y = ty0; y < ty0 + th && y < rh; y++)
                for (int x = tx0; x < tx0 + tw && x < rw; x++)
                    for (int p = 0; p < 3; p++) dst[p * cells + (size_t)y * rw + x] = f[cur][p * icells + (size_t)(y - oy) * iw + (x - ox)];
        }
}

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
    const int tiles[][2] = { { 5, 3 }, { 7, 11 }, { 16, 6 }, { 13, 13 } };
    const int Ks[] = { 1, 2, 3, 5 };
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
                const int* tile = tiles[variant % 4];
                const int K = Ks[(variant / 4) % 4];
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
                    float* cur = a.data(); float* nxt = b.data();
                    for (int done = 0; done < iterations; done += K) {
                        const long bad = edge_failures(cur, mask.data(), rw, rh, k.flow, &edges);
                        if (bad) { ok = false; printf("FAIL %d x %d call %d: %ld edges whose ends disagree after %d sweeps\n", w, h, c, bad, done); }
                        tiled_pass(cur, nxt, mask.data(), rw, rh, tile[0], tile[1], K, iterations - done < K ? iterations - done : K, k);
                        float* t = cur; cur = nxt; nxt = t;
                    }
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

static int run_apply(const char* in_path, const char* out_path)
{
    FILE* fi = fopen(in_path, "rb");
    if (!fi) { printf("cannot read %s\n", in_path); return 2; }
    int32_t hd[4]; float fl[7];
    if (fread(hd, 4, 4, fi) != 4 || fread(fl, 4, 7, fi) != 7) { fclose(fi); return 2; }
    const int w = hd[0], h = hd[1], n = hd[2], iterations = hd[3];
    if (w < 1 || h < 1 || w > 4096 || h > 4096 || n < 0 || n > 65536 || iterations < 1 || iterations > kHydroMaxIterations) { fclose(fi); return 2; }
    std::vector<float> raw((size_t)n * 5);
    std::vector<uint8_t> map((size_t)w * h);
    if (fread(raw.data(), 4, raw.size(), fi) != raw.size() || fread(map.data(), 1, map.size(), fi) != map.size()) { fclose(fi); return 2; }
    fclose(fi);
    int32_t rect[4];
    const HydroConst k = { fl[1], fl[2], fl[3], fl[4], fl[5], hydro_keep(fl[6]) };
    if (!serial_call(map, w, h, raw, fl[0], iterations, k, rect)) { printf("a negative d or s\n"); return 3; }
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
