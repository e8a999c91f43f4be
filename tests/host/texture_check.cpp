// CPU check of vr_texture.h, the definition of rule-based texturing (vr_terrain_texture).  No HIP: g++ -std=c++17 -I vrenderer_amd/csrc.
//
//   texture_check                 the preparation and the weight: 20000 seeded layers (fades of 0, fades that clamp away, zero-width
//                                 bands, values at the ends of fp32's range, three max_heights) - every prepared edge and reciprocal
//                                 is finite, no reciprocal is negative or subnormal, and over a sweep of heights and squared tangents
//                                 every layer weight lies in [0, opacity]; a texel whose layers all weigh 0 keeps its four bytes.
//                                 Prints "N layers, F failures".
//   texture_check apply IN OUT    layer sets applied to an albedo under a heightmap with the header's functions and a mask of 1
//                                 (texture_serial), for tests/test_terrain_texture_cpu.py to compare with tests/texture_model.py.
//                                 IN:  int32 w0, h0, wa, ha, sets; float world_size, max_height; w0 * h0 bytes; wa * ha * 4 bytes;
//                                      per set: int32 n, then n x (11 floats: color[4], opacity, alt_lo, alt_hi, alt_fade, slope_lo,
//                                      slope_hi, slope_fade; uint32 channel_mask)
//                                 OUT: per set wa * ha * 4 bytes - the albedo of IN under that set
#include "vr_texture.h"

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

static long g_layers = 0, g_failures = 0;

static bool finite32(float v) { return v == v && fabsf(v) <= kTextureMaxFloat; }

static void check_layer(const TextureLayerDesc& d, float max_height, const char* what)
{
    g_layers++;
    const TextureLayer l = texture_prepare_layer(d, max_height);
    for (int r = 0; r < 4; r++)
        if (!finite32(l.edge[r]) || !finite32(l.inv[r]) || l.inv[r] < 0.0f || (l.inv[r] != 0.0f && l.inv[r] < 1.17549435e-38f)) {
            g_failures++;
            printf("FAIL %s: ramp %d edge %g inv %g (alt %g %g %g slope %g %g %g, max_height %g)\n", what, r, l.edge[r], l.inv[r], d.alt_lo, d.alt_hi,
                   d.alt_fade, d.slope_lo, d.slope_hi, d.slope_fade, max_height);
            return;
        }
    TextureConst k;
    memset(&k, 0, sizeof(k));
    k.num_layers = 1; k.layer[0] = l;
    for (int a = 0; a <= 255; a += 5)
        for (int s = 0; s < 40; s++) {
            const float h = (float)a + (float)(s % 4) * 0.25f, s2 = s == 0 ? 0.0f : (float)pow(10.0, -4.0 + 0.25 * s);
            const float w = texture_layer_weight(l, h, s2);
            if (!(w >= 0.0f && w <= d.opacity)) {
                g_failures++;
                printf("FAIL %s: weight %g at h %g s2 %g, opacity %g\n", what, w, h, s2, d.opacity);
                return;
            }
            if (w == 0.0f) {
                float val[4] = { 0.0f, 1.0f, 128.0f, 255.0f };
                texture_composite(k, h, s2, 1.0f, val);
                if (brush_byte(val[0]) != 0 || brush_byte(val[1]) != 1 || brush_byte(val[2]) != 128 || brush_byte(val[3]) != 255) {
                    g_failures++;
                    printf("FAIL %s: a layer of weight 0 moved a byte\n", what);
                    return;
                }
            }
        }
}

static int run_check()
{
    const float heights[] = { 400.0f, 1.0e-3f, 3.0e30f };
    const float big = 3.0e38f;
    for (int i = 0; i < 20000; i++) {
        const float mh = heights[i % 3];
        TextureLayerDesc d;
        for (int c = 0; c < 4; c++) d.color[c] = (float)(rnd() * 255.0);
        d.opacity = i % 5 == 0 ? 1.0f : (float)rnd();
        double lo = (rnd() * 1.5 - 0.25) * mh, hi = lo + rnd() * 0.5 * mh;
        if (i % 7 == 0) hi = lo;
        d.alt_lo = (float)lo; d.alt_hi = (float)hi; if (d.alt_hi < d.alt_lo) d.alt_hi = d.alt_lo;
        d.alt_fade = i % 4 == 0 ? 0.0f : (float)(rnd() * 0.2 * mh);
        double slo = rnd() * 89.0, shi = slo + rnd() * (89.0 - slo);
        if (i % 6 == 0) slo = 0.0;
        if (i % 9 == 0) shi = 89.0;
        if (i % 11 == 0) shi = slo;
        d.slope_lo = (float)slo; d.slope_hi = (float)shi; if (d.slope_hi < d.slope_lo) d.slope_hi = d.slope_lo;
        if (d.slope_hi > 89.0f) d.slope_hi = 89.0f;
        if (d.slope_lo > d.slope_hi) d.slope_lo = d.slope_hi;
        d.slope_fade = i % 3 == 0 ? 0.0f : (float)(rnd() * 30.0);
        d.channel_mask = 1u + (uint32_t)(rnd() * 15.0);
        if (i % 1000 == 1) { d.alt_lo = -big; d.alt_hi = big; d.alt_fade = big; }
        if (i % 1000 == 2) { d.alt_lo = d.alt_hi = big; d.alt_fade = 1.0e-45f; }
        if (i % 1000 == 3) { d.alt_fade = 1.0e-45f; d.slope_fade = 1.0e-45f; }
        if (i % 1000 == 4) { d.slope_fade = big; }
        check_layer(d, mh, "seeded");
    }
    printf("%ld layers, %ld failures\n", g_layers, g_failures);
    return g_failures ? 1 : 0;
}

static int run_apply(const char* in_path, const char* out_path)
{
    FILE* fi = fopen(in_path, "rb");
    if (!fi) { printf("cannot read %s\n", in_path); return 2; }
    int32_t hd[5]; float fl[2];
    if (fread(hd, 4, 5, fi) != 5 || fread(fl, 4, 2, fi) != 2) { fclose(fi); return 2; }
    const int w0 = hd[0], h0 = hd[1], wa = hd[2], ha = hd[3], sets = hd[4];
    if (w0 < 1 || h0 < 1 || wa < 1 || ha < 1 || w0 > 4096 || h0 > 4096 || wa > 4096 || ha > 4096 || sets < 0 || sets > 65536) { fclose(fi); return 2; }
    std::vector<uint8_t> height((size_t)w0 * h0), albedo((size_t)wa * ha * 4);
    if (fread(height.data(), 1, height.size(), fi) != height.size() || fread(albedo.data(), 1, albedo.size(), fi) != albedo.size()) { fclose(fi); return 2; }
    FILE* fo = fopen(out_path, "wb");
    if (!fo) { fclose(fi); printf("cannot write %s\n", out_path); return 2; }
    const std::vector<float> mask((size_t)wa * ha, 1.0f);
    bool ok = true;
    for (int s = 0; s < sets && ok; s++) {
        int32_t n;
        if (fread(&n, 4, 1, fi) != 1 || n < 1 || n > kTextureMaxLayers) { ok = false; break; }
        TextureLayerDesc desc[kTextureMaxLayers];
        for (int i = 0; i < n && ok; i++) {
            float f[11]; uint32_t cm;
            if (fread(f, 4, 11, fi) != 11 || fread(&cm, 4, 1, fi) != 1) { ok = false; break; }
            TextureLayerDesc& d = desc[i];
            for (int c = 0; c < 4; c++) d.color[c] = f[c];
            d.opacity = f[4]; d.alt_lo = f[5]; d.alt_hi = f[6]; d.alt_fade = f[7]; d.slope_lo = f[8]; d.slope_hi = f[9]; d.slope_fade = f[10];
            d.channel_mask = cm;
        }
        if (!ok) break;
        const TextureConst k = texture_prepare(desc, n, fl[1], fl[0], w0, h0, wa, ha);
        std::vector<uint8_t> out = albedo;
        texture_serial(height.data(), w0, h0, out.data(), wa, ha, k, mask.data());
        ok = fwrite(out.data(), 1, out.size(), fo) == out.size();
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
