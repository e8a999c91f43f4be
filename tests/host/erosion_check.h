// What tests/host/erode_check.cpp and tests/host/hydro_check.cpp share: the rng, the dab preparation with its hull, the tiled
// K-sweeps-per-pass evaluation the device's step kernel makes (k_sweep_steps, vr_erode.hip), over a host-side model, and the
// reading and writing of `apply`'s files.
//
// A host-side model: F, its number of state planes, and cell(in, im, icells, iw, c, out): cell c of an image `iw` cells wide whose F
// planes lie `icells` floats apart, from `in` (mask `im`) to `out`, by the definition header's functions in its order.
#pragma once
#include "vr_erode.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <utility>
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

// One pass over the F planes of the rectangle (`rw * rh` floats apart) the way the device's step kernel makes it: per tile an image
// of (tw + 2K) x (th + 2K) cells, zeros beyond the rectangle, `steps` <= K sweeps on two copies, the tile stored to dst.
template <class Model>
static void tiled_pass(const Model& model, const float* src, float* dst, const float* mask, int rw, int rh, int tw, int th, int K, int steps)
{
    constexpr int F = Model::F;
    const size_t cells = (size_t)rw * (size_t)rh;
    const int iw = tw + 2 * K, ih = th + 2 * K;
    const size_t icells = (size_t)iw * (size_t)ih;
    std::vector<float> im(icells), f[2] = { std::vector<float>(F * icells), std::vector<float>(F * icells) };
    for (int ty0 = 0; ty0 < rh; ty0 += th)
        for (int tx0 = 0; tx0 < rw; tx0 += tw) {
            const int ox = tx0 - K, oy = ty0 - K;
            for (int ly = 0; ly < ih; ly++)
                for (int lx = 0; lx < iw; lx++) {
                    const int x = ox + lx, y = oy + ly;
                    const bool in = x >= 0 && x < rw && y >= 0 && y < rh;
                    const size_t at = in ? (size_t)y * rw + x : 0, i = (size_t)ly * iw + lx;
                    im[i] = in ? mask[at] : 0.0f;
                    for (int p = 0; p < F; p++) f[0][p * icells + i] = in ? src[p * cells + at] : 0.0f;
                }
            int cur = 0;
            for (int s = 1; s <= steps; s++, cur ^= 1)
                for (int ly = s; ly < ih - s; ly++)
                    for (int lx = s; lx < iw - s; lx++) model.cell(f[cur].data(), im.data(), icells, iw, (size_t)ly * iw + lx, f[cur ^ 1].data());
            for (int y = ty0; y < ty0 + th && y < rh; y++)
                for (int x = tx0; x < tx0 + tw && x < rw; x++)
                    for (int p = 0; p < F; p++) dst[p * cells + (size_t)y * rw + x] = f[cur][p * icells + (size_t)(y - oy) * iw + (x - ox)];
        }
}

// `iterations` sweeps from the state in a, K per pass; before_pass(state, sweeps done) runs in front of every pass.  Returns the
// buffer (a or b) that holds the result.
template <class Model, class Before>
static float* tiled_run(const Model& model, float* a, float* b, const float* mask, int rw, int rh, const int tile[2], int K, int iterations, Before&& before_pass)
{
    float* cur = a; float* nxt = b;
    for (int done = 0; done < iterations; done += K) {
        before_pass((const float*)cur, done);
        tiled_pass(model, cur, nxt, mask, rw, rh, tile[0], tile[1], K, iterations - done < K ? iterations - done : K);
        float* t = cur; cur = nxt; nxt = t;
    }
    return cur;
}

// the tiles (none divides the rectangles met) and the sweeps per pass a check cycles through, by its running call number
static const int kCheckTiles[4][2] = { { 5, 3 }, { 7, 11 }, { 16, 6 }, { 13, 13 } };
static const int kCheckKs[4] = { 1, 2, 3, 5 };

// `apply`: IN is int32 w, h, n, iterations; `nfl` floats (world_size first); n x 5 floats (x, z, radius, hardness, strength);
// w * h bytes.  call(map, w, h, raw, iterations, fl, rect) applies the call and fills rect = {x, y, w, h}; non-zero ends the program
// with that code.  OUT is int32 rect[4]; the eroded bytes.
template <class Call>
static int run_apply(const char* in_path, const char* out_path, int nfl, int max_iterations, Call&& call)
{
    FILE* fi = fopen(in_path, "rb");
    if (!fi) { printf("cannot read %s\n", in_path); return 2; }
    int32_t hd[4];
    std::vector<float> fl((size_t)nfl);
    if (fread(hd, 4, 4, fi) != 4 || fread(fl.data(), 4, fl.size(), fi) != fl.size()) { fclose(fi); return 2; }
    const int w = hd[0], h = hd[1], n = hd[2], iterations = hd[3];
    if (w < 1 || h < 1 || w > 4096 || h > 4096 || n < 0 || n > 65536 || iterations < 1 || iterations > max_iterations) { fclose(fi); return 2; }
    std::vector<float> raw((size_t)n * 5);
    std::vector<uint8_t> map((size_t)w * h);
    if (fread(raw.data(), 4, raw.size(), fi) != raw.size() || fread(map.data(), 1, map.size(), fi) != map.size()) { fclose(fi); return 2; }
    fclose(fi);
    int32_t rect[4];
    { const int rc = call(map, w, h, raw, iterations, fl.data(), rect); if (rc) return rc; }
    FILE* fo = fopen(out_path, "wb");
    if (!fo) { printf("cannot write %s\n", out_path); return 2; }
    const bool ok = fwrite(rect, 4, 4, fo) == 4 && fwrite(map.data(), 1, map.size(), fo) == map.size();
    fclose(fo);
    return ok ? 0 : 2;
}
