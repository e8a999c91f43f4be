// CPU check of vr_noise.h, the definition of procedural noise on a map (vr_terrain_noise).  No HIP: g++ -std=c++17 -I vrenderer_amd/csrc.
//
//   noise_check                 the ranges the header states: per basis 400000 seeded points (cells of either sign up to 2^22, positions
//                               that include 0, 1 and values next to them, random seeds) - every n lies in [-1, 1], the fade in [0, 1],
//                               the gradient basis is 0 at a lattice point; 20000 seeded calls (1 .. 12 octaves, gain and lacunarity
//                               over their whole ranges, every fractal) - the weights are finite, non-negative and sum to 1 within
//                               12 roundings, no prepared constant is an infinity, and f lies in [-1, 1] at 16 texels each.  The 2^22
//                               refusal from both sides: per map the largest frequency noise_in_range admits is found by bisection
//                               over the fp32 values; there every corner coordinate the header's own fp32 arithmetic gives is below
//                               2^22 with a position in [0, 1], and the next frequency up is refused.
//                               Prints "N points, F failures".
//   noise_check apply IN OUT    parameter sets applied to a map with the header's functions (noise_serial), for
//                               tests/test_terrain_noise_cpu.py to compare with tests/noise_model.py.
//                               IN:  int32 w, h, channels, sets; float world_size; w * h * channels bytes; w * h floats (the mask);
//                                    per set: 7 floats (frequency, offset_x, offset_z, lacunarity, gain, amplitude, base), uint32 seed,
//                                    int32 octaves, basis, fractal, op, uint32 channel_mask
//                               OUT: per set 60 floats (sx, sz, ox, oz, a: 12 each), int32 in_range; then, if in range, w * h * channels
//                                    bytes, w * h floats f and 12 x w * h floats n_o
#include "vr_noise.h"

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

static long g_points = 0, g_failures = 0;

static bool finite32(float v) { return v == v && fabsf(v) <= kNoiseMaxFloat; }
static void fail(const char* what, double a, double b, double c)
{
    if (g_failures++ < 20) printf("FAIL %s: %.9g %.9g %.9g\n", what, a, b, c);
}

static float edge_position(int kind)
{
    switch (kind) {
    case 0: return 0.0f;
    case 1: return 1.0f;
    case 2: return nextafterf(1.0f, 0.0f);
    case 3: return nextafterf(0.0f, 1.0f);
    case 4: return 0.5f;
    default: return (float)rnd();
    }
}

static void check_bases()
{
    for (int basis = 0; basis < 2; basis++)
        for (int i = 0; i < 400000; i++) {
            g_points++;
            const double span = i % 3 == 0 ? 4.0 : (i % 3 == 1 ? 4096.0 : kNoiseCoordLimit);
            const uint32_t cx = (uint32_t)(int32_t)floor((rnd() * 2.0 - 1.0) * span), cz = (uint32_t)(int32_t)floor((rnd() * 2.0 - 1.0) * span);
            const float tx = edge_position(i % 16), tz = edge_position((i / 16) % 16);
            const uint32_t seed = (uint32_t)(rnd() * 4294967296.0);
            const float fx = noise_fade(tx);
            if (!(fx >= 0.0f && fx <= 1.0f)) fail("fade outside [0, 1]", tx, fx, 0);
            const float n = noise_basis(basis, cx, cz, tx, tz, seed);
            if (!(n >= -1.0f && n <= 1.0f)) fail("n outside [-1, 1]", basis, tx, n);
            if (basis == kNoiseGradient && noise_basis(basis, cx, cz, 0.0f, 0.0f, seed) != 0.0f) fail("gradient basis not 0 at a lattice point", cx, cz, seed);
        }
    // the fade over every fp32 value of the last binade below 1, where the unclamped product exceeds 1
    for (float t = 0.5f; t <= 1.0f; t = nextafterf(t, 2.0f)) {
        const float f = noise_fade(t);
        if (!(f >= 0.0f && f <= 1.0f)) fail("fade outside [0, 1]", t, f, 0);
    }
}

static void check_fractals()
{
    for (int i = 0; i < 20000; i++) {
        g_points++;
        NoiseDesc d;
        d.frequency = (float)pow(10.0, rnd() * 4.0 - 3.0);
        d.offset_x = (float)((rnd() - 0.5) * 200.0); d.offset_z = (float)((rnd() - 0.5) * 200.0);
        d.lacunarity = i % 7 == 0 ? 1.0f : (i % 7 == 1 ? 4.0f : (float)(1.0 + rnd() * 3.0));
        d.gain = i % 5 == 0 ? 0.0f : (i % 5 == 1 ? 1.0f : (float)rnd());
        d.amplitude = (float)((rnd() - 0.5) * 510.0); d.base = (float)(rnd() * 255.0);
        d.seed = (uint32_t)(rnd() * 4294967296.0);
        d.octaves = 1 + i % kNoiseMaxOctaves; d.basis = i % 2; d.fractal = i % 3; d.op = (i / 2) % 2; d.channel_mask = 1;
        const int w = 1 + (int)(rnd() * 100.0), h = 1 + (int)(rnd() * 100.0);
        const NoiseConst k = noise_prepare(d, 64.0f, w, h);
        double sum = 0.0;
        bool ok = true;
        for (int o = 0; o < kNoiseMaxOctaves; o++) {
            ok = ok && finite32(k.sx[o]) && finite32(k.sz[o]) && finite32(k.ox[o]) && finite32(k.oz[o]) && finite32(k.a[o]) && k.a[o] >= 0.0f;
            sum += (double)k.a[o];
        }
        if (!ok) { fail("a prepared constant is not finite, or a weight is negative", i, 0, 0); continue; }
        if (!(fabs(sum - 1.0) <= 12.0 * 5.9604645e-08)) fail("the weights do not sum to 1", i, sum, 0);
        if (!noise_in_range(k, w, h)) continue;
        for (int s = 0; s < 16; s++) {
            const float f = noise_fractal(k, (int)(rnd() * w), (int)(rnd() * h));
            if (!(f >= -1.0f && f <= 1.0f)) fail("f outside [-1, 1]", i, f, 0);
        }
    }
}

static NoiseConst boundary_const(float frequency, float offset, int octaves, int w, int h)
{
    NoiseDesc d;
    d.frequency = frequency; d.offset_x = offset; d.offset_z = -offset; d.lacunarity = 2.0f; d.gain = 0.5f; d.amplitude = 1.0f; d.base = 0.0f; d.seed = 1;
    d.octaves = octaves; d.basis = kNoiseGradient; d.fractal = kNoiseFbm; d.op = kNoiseAdd; d.channel_mask = 1;
    return noise_prepare(d, 64.0f, w, h);
}

static void check_boundary()
{
    const int maps[4][2] = { { 1, 1 }, { 64, 64 }, { 17, 33 }, { 2048, 512 } };
    for (int m = 0; m < 4; m++)
        for (int octaves = 1; octaves <= kNoiseMaxOctaves; octaves += 11)
            for (int side = 0; side < 2; side++) {
                g_points++;
                const int w = maps[m][0], h = maps[m][1];
                const float offset = side ? 100.0f : -3.0f;
                // bisection over the fp32 values: lo is admitted, hi refused
                float lo = 1.0e-6f, hi = 1.0e12f;
                if (!noise_in_range(boundary_const(lo, offset, octaves, w, h), w, h) || noise_in_range(boundary_const(hi, offset, octaves, w, h), w, h)) {
                    fail("the bisection's ends", w, h, octaves);
                    continue;
                }
                for (;;) {
                    uint32_t a, b;
                    memcpy(&a, &lo, 4); memcpy(&b, &hi, 4);
                    if (b - a <= 1u) break;
                    const uint32_t c = a + (b - a) / 2u;
                    float mid;
                    memcpy(&mid, &c, 4);
                    if (noise_in_range(boundary_const(mid, offset, octaves, w, h), w, h)) lo = mid; else hi = mid;
                }
                const NoiseConst k = boundary_const(lo, offset, octaves, w, h);
                double reach = 0.0;
                for (int o = 0; o < octaves; o++)
                    for (int c = 0; c < 4; c++) {
                        uint32_t cell; float t;
                        const int i = c & 1 ? (c & 2 ? h - 1 : w - 1) : 0;
                        if (c & 2) noise_axis(i, k.sz[o], k.oz[o], &cell, &t); else noise_axis(i, k.sx[o], k.ox[o], &cell, &t);
                        const double u = (double)(int32_t)cell + (double)t;
                        if (!(fabs(u) <= kNoiseCoordLimit && t >= 0.0f && t <= 1.0f)) fail("a corner coordinate of the last admitted frequency", u, t, lo);
                        if (fabs(u) > reach) reach = fabs(u);
                    }
                // the admitted side comes close to the bound, the refused side is the very next frequency
                if (!(reach > kNoiseCoordLimit * 0.999)) fail("the last admitted frequency stays far from 2^22", reach, lo, octaves);
                if (noise_in_range(boundary_const(nextafterf(lo, 1.0e30f), offset, octaves, w, h), w, h)) fail("the next frequency is admitted", lo, w, h);
            }
    // a frequency whose products overflow fp32: clamped in the preparation, refused by the range
    const NoiseConst big = boundary_const(3.0e38f, 0.0f, 12, 64, 64);
    for (int o = 0; o < kNoiseMaxOctaves; o++)
        if (!finite32(big.sx[o]) || !finite32(big.ox[o])) fail("an infinity in the preparation", o, big.sx[o], big.ox[o]);
    if (noise_in_range(big, 64, 64)) fail("an overflowing frequency is admitted", 0, 0, 0);
}

static int run_check()
{
    check_bases();
    check_fractals();
    check_boundary();
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
    std::vector<float> mask(texels);
    if (fread(map.data(), 1, map.size(), fi) != map.size() || fread(mask.data(), 4, texels, fi) != texels) { fclose(fi); return 2; }
    FILE* fo = fopen(out_path, "wb");
    if (!fo) { fclose(fi); printf("cannot write %s\n", out_path); return 2; }
    bool ok = true;
    std::vector<float> f(texels), n(texels * kNoiseMaxOctaves);
    for (int s = 0; s < sets && ok; s++) {
        float fl[7]; uint32_t seed, cm; int32_t iv[4];
        if (fread(fl, 4, 7, fi) != 7 || fread(&seed, 4, 1, fi) != 1 || fread(iv, 4, 4, fi) != 4 || fread(&cm, 4, 1, fi) != 1) { ok = false; break; }
        if (iv[0] < 1 || iv[0] > kNoiseMaxOctaves) { ok = false; break; }
        NoiseDesc d;
        d.frequency = fl[0]; d.offset_x = fl[1]; d.offset_z = fl[2]; d.lacunarity = fl[3]; d.gain = fl[4]; d.amplitude = fl[5]; d.base = fl[6];
        d.seed = seed; d.octaves = iv[0]; d.basis = iv[1]; d.fractal = iv[2]; d.op = iv[3]; d.channel_mask = cm;
        const NoiseConst k = noise_prepare(d, world, w, h);
        const int32_t in_range = noise_in_range(k, w, h) ? 1 : 0;
        ok = fwrite(k.sx, 4, 12, fo) == 12 && fwrite(k.sz, 4, 12, fo) == 12 && fwrite(k.ox, 4, 12, fo) == 12 && fwrite(k.oz, 4, 12, fo) == 12 &&
             fwrite(k.a, 4, 12, fo) == 12 && fwrite(&in_range, 4, 1, fo) == 1;
        if (!ok || !in_range) continue;
        std::vector<uint8_t> out = map;
        noise_serial(out.data(), w, h, ch, k, mask.data());
        for (int j = 0; j < h; j++)
            for (int i = 0; i < w; i++) {
                float no[kNoiseMaxOctaves];
                f[(size_t)j * w + i] = noise_fractal(k, i, j, no);
                for (int o = 0; o < kNoiseMaxOctaves; o++) n[(size_t)o * texels + (size_t)j * w + i] = no[o];
            }
        ok = fwrite(out.data(), 1, out.size(), fo) == out.size() && fwrite(f.data(), 4, texels, fo) == texels && fwrite(n.data(), 4, n.size(), fo) == n.size();
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
