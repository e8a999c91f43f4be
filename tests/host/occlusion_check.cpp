// CPU check of vr_occlusion.h, the definition of baked sky visibility (vr_terrain_occlusion).  No HIP: g++ -std=c++17 -I vrenderer_amd/csrc.
//
//   occlusion_check               the staged footprint: 300 seeded pairs of map sizes, radii and direction counts, whole map.  Every
//                                 32 x 8 tile of the albedo builds its footprint as the kernel does - origin at the first texel's
//                                 centre less the reach, occlusion_footprint's size, every load clamped into the map - and evaluates
//                                 its texels through OcclusionFoot; the bytes must be those of OcclusionDirect, and no clamp of the
//                                 fetch may bind: a centre outside the footprint or an address outside its fw * fh bytes is counted.
//                                 A radius one step too long must be refused by occlusion_prepare, and the longest one it accepts
//                                 reaches at most 64.  Prints "N maps, B binds, F failures".
//   occlusion_check apply IN OUT  calls applied to an albedo under a heightmap with the header's functions (occlusion_serial, direct
//                                 fetch), for tests/test_occlusion_model_cpu.py to compare with tests/occlusion_model.py.
//                                 IN:  int32 w0, h0, wa, ha, sets; float world_size, max_height; w0 * h0 bytes; wa * ha * 4 bytes;
//                                      per set: 8 floats (radius, gain, bias, opacity, color[4]); uint32 channel_mask; int32
//                                      directions; uint32 mode; int32 has_mask; with has_mask wa * ha floats, else the mask is 1
//                                 OUT: per set int32 accepted, the OcclusionConst as it is in memory, wa * ha * 4 bytes - the albedo of
//                                      IN after that call (unchanged where the call was refused)
#include "vr_occlusion.h"

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

static long g_maps = 0, g_binds = 0, g_failures = 0;

// OcclusionFoot, counting what its clamps would hide
struct CountingFoot {
    OcclusionFoot f;
    int at(int x, int y) const
    {
        if (x - f.ox < 0 || x - f.ox >= f.fw || y - f.oy < 0 || y - f.oy >= f.fh) g_binds++;
        return f.at(x, y);
    }
    int step(int dx, int dz) const { return f.step(dx, dz); }
    int load(int a) const
    {
        if (a < 0 || a >= f.fw * f.fh) g_binds++;
        return f.load(a);
    }
};

static void fail(const char* what, int w0, int h0, int wa, int ha, double radius)
{
    g_failures++;
    printf("FAIL %s: heightmap %d x %d, albedo %d x %d, radius %g\n", what, w0, h0, wa, ha, radius);
}

static void check_map(int w0, int h0, int wa, int ha, float world, float radius, int directions, uint32_t mode)
{
    g_maps++;
    std::vector<uint8_t> height((size_t)w0 * h0), albedo((size_t)wa * ha * 4);
    for (auto& b : height) b = (uint8_t)(rnd() * 256.0);
    // (half the maps smooth, so that far horizons win)
    if (g_maps % 2)
        for (int y = 0; y < h0; y++)
            for (int x = 0; x < w0; x++) height[(size_t)y * w0 + x] = (uint8_t)(128.0 + 100.0 * sin(0.11 * x + 0.3) * cos(0.07 * y) + 20.0 * rnd());
    for (auto& b : albedo) b = (uint8_t)(rnd() * 256.0);
    OcclusionDesc d;
    d.radius = radius; d.max_height = 12.5f; d.gain = 1.5f; d.bias = g_maps % 3 ? 0.0f : 0.125f; d.opacity = 0.75f;
    d.color[0] = 10.0f; d.color[1] = 0.0f; d.color[2] = 77.5f; d.color[3] = 255.0f;
    d.channel_mask = 1u + (uint32_t)(rnd() * 15.0); d.directions = directions; d.mode = mode;
    OcclusionConst k;
    if (!occlusion_prepare(d, world, w0, h0, &k)) { fail("a radius inside the limit was refused", w0, h0, wa, ha, radius); return; }
    if (k.reach_x > kOcclusionMaxReach || k.reach_z > kOcclusionMaxReach) { fail("reach above 64", w0, h0, wa, ha, radius); return; }
    const std::vector<float> mask((size_t)wa * ha, 1.0f);
    std::vector<uint8_t> direct = albedo, tiled = albedo;
    const OcclusionDirect whole = { height.data(), w0 };
    occlusion_serial(w0, h0, direct.data(), wa, ha, k, mask.data(), [&](int, int) { return whole; });
    int64_t fw64, fh64;
    occlusion_footprint(k, w0, h0, wa, ha, 32, 8, &fw64, &fh64);
    const int fw = (int)fw64, fh = (int)fh64;
    // one footprint per tile, built as k_occlusion builds it; the texels of the map read through the footprint of their own tile
    const int tiles_x = (wa + 31) / 32, tiles_y = (ha + 7) / 8;
    std::vector<std::vector<uint8_t>> feet((size_t)tiles_x * tiles_y, std::vector<uint8_t>((size_t)fw * fh));
    for (int ty = 0; ty < tiles_y; ty++)
        for (int tx = 0; tx < tiles_x; tx++) {
            const int ox = occlusion_centre(tx * 32, w0, wa) - k.reach_x, oy = occlusion_centre(ty * 8, h0, ha) - k.reach_z;
            std::vector<uint8_t>& foot = feet[(size_t)ty * tiles_x + tx];
            for (int ly = 0; ly < fh; ly++)
                for (int lx = 0; lx < fw; lx++)
                    foot[(size_t)ly * fw + lx] = height[(size_t)occlusion_clampi(oy + ly, 0, h0 - 1) * w0 + occlusion_clampi(ox + lx, 0, w0 - 1)];
        }
    occlusion_serial(w0, h0, tiled.data(), wa, ha, k, mask.data(), [&](int i, int j) {
        const int tx = i / 32, ty = j / 8;
        CountingFoot c;
        c.f.foot = feet[(size_t)ty * tiles_x + tx].data();
        c.f.ox = occlusion_centre(tx * 32, w0, wa) - k.reach_x; c.f.oy = occlusion_centre(ty * 8, h0, ha) - k.reach_z;
        c.f.fw = fw; c.f.fh = fh;
        return c;
    });
    if (tiled != direct) fail("the staged footprint's bytes differ from the direct loads'", w0, h0, wa, ha, radius);
    // one step further along the x axis than 64 is refused
    OcclusionDesc over = d;
    over.radius = (float)(65.5 * (double)world / (double)w0);
    OcclusionConst unused;
    if (occlusion_prepare(over, world, w0, h0, &unused)) fail("a reach of 65 texels was accepted", w0, h0, wa, ha, over.radius);
}

static int run_check()
{
    for (int i = 0; i < 300; i++) {
        int w0 = 1 + (int)(rnd() * 150.0), h0 = 1 + (int)(rnd() * 150.0), wa = 1 + (int)(rnd() * 100.0), ha = 1 + (int)(rnd() * 100.0);
        if (i % 10 == 0) { wa = w0; ha = h0; }
        if (i % 10 == 1) { w0 = 4 * wa; h0 = 8 * ha; }
        if (i % 10 == 2) { w0 = 1 + w0 % 40; h0 = 1 + h0 % 30; wa = 2 * w0 + 1; ha = 3 * h0; }
        const float world = i % 2 ? 64.0f : 150.0f;
        // a radius of up to 64 texels of the finer axis: every direction then stays inside the limit
        const double texel = (double)world / (double)(w0 > h0 ? w0 : h0);
        const double steps = i % 7 == 0 ? 64.0 : rnd() * 64.5;
        const float radius = (float)((steps > 64.0 ? 64.0 : steps) * texel * 0.999 + 1.0e-3 * texel);
        check_map(w0, h0, wa, ha, world, radius, 4 << (i % 3), (uint32_t)(i % 2));
    }
    printf("%ld maps, %ld binds, %ld failures\n", g_maps, g_binds, g_failures);
    return g_failures || g_binds ? 1 : 0;
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
    bool ok = true;
    for (int s = 0; s < sets && ok; s++) {
        float f[8]; uint32_t cm, mode; int32_t directions, has_mask;
        if (fread(f, 4, 8, fi) != 8 || fread(&cm, 4, 1, fi) != 1 || fread(&directions, 4, 1, fi) != 1 || fread(&mode, 4, 1, fi) != 1 || fread(&has_mask, 4, 1, fi) != 1) { ok = false; break; }
        if (directions != 4 && directions != 8 && directions != 16) { ok = false; break; }
        std::vector<float> mask((size_t)wa * ha, 1.0f);
        if (has_mask && fread(mask.data(), 4, mask.size(), fi) != mask.size()) { ok = false; break; }
        OcclusionDesc d;
        d.radius = f[0]; d.max_height = fl[1]; d.gain = f[1]; d.bias = f[2]; d.opacity = f[3];
        for (int c = 0; c < 4; c++) d.color[c] = f[4 + c];
        d.channel_mask = cm; d.directions = directions; d.mode = mode;
        OcclusionConst k;
        memset(&k, 0, sizeof(k));
        const int32_t accepted = occlusion_prepare(d, fl[0], w0, h0, &k) ? 1 : 0;
        std::vector<uint8_t> out = albedo;
        const OcclusionDirect whole = { height.data(), w0 };
        if (accepted) occlusion_serial(w0, h0, out.data(), wa, ha, k, mask.data(), [&](int, int) { return whole; });
        ok = fwrite(&accepted, 4, 1, fo) == 1 && fwrite(&k, sizeof(k), 1, fo) == 1 && fwrite(out.data(), 1, out.size(), fo) == out.size();
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
