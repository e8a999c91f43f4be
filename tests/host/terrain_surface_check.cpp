// Check of the terrain's surface constants (vrenderer_amd/csrc/vr_terrain_surface.h) and of the three facts the TERRAIN flavour
// of the shading (vr_deferred_dev.h) folds with:
//   1. the constants equal decode_surface's generic expressions evaluated in float on the bits main_ps writes;
//   2. fmaxf((float)i * sn16, -1.0f) == (float)i * sn16 for every snorm16 code the encoder can emit, i in [-32767, 32767];
//   3. x * 0.0f + 1.0f == 1.0f (separately rounded and as one fma) for x in [0, 1] - NdotH comes out of a saturate.
// Plain C++17, no GPU: g++ -std=c++17 -Wall -Werror -ffp-contract=off -I vrenderer_amd/csrc tests/host/terrain_surface_check.cpp
#include "vr_terrain_surface.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

static long cases = 0, failures = 0;
#define CHECK(cond) do { cases++; if (!(cond)) { failures++; std::printf("FAIL line %d: %s\n", __LINE__, #cond); } } while (0)

static uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

int main()
{
    // ---- 1. the generic decode (vr_deferred_dev.h: decode_surface), on the word pixel_shader_fast packs -----------------------
    {
        volatile uint32_t n23 = (0x1234u & 0xffffu) | (kTerrainRoughBits << 16);      // (volatile: evaluated at run time, in float)
        volatile float sn16 = 1.0f / 32767.0f;
        const float rough = fmaxf((float)(int16_t)(n23 >> 16) * sn16, -1.0f);
        const float alpha = fmaxf(0.01f, rough * rough);
        const float a2 = alpha * alpha;
        const float kk = ((rough + 1.0f) * (rough + 1.0f)) * 0.125f;
        CHECK(bits(sn16) == bits(kSnorm16Scale));
        CHECK(bits(rough) == bits(kTerrainRough) && rough == 1.0f);
        CHECK(bits(alpha) == bits(kTerrainAlpha) && alpha == 1.0f);
        CHECK(bits(a2) == bits(kTerrainA2) && bits(a2 - 1.0f) == 0u);                 // +0, not -0
        CHECK(bits(kk) == bits(kTerrainKk) && kk == 0.5f);
        CHECK(bits(a2 * a2) == bits(1.0f));                                            // the factor num drops
        CHECK(bits(1.0f - kk) == bits(0.5f));
    }
    // ---- 2. the normal decode's clamp is an identity on the encoder's range --------------------------------------------------
    {
        long bad = 0;
        for (int i = -32767; i <= 32767; i++) {
            volatile float v = (float)i * kSnorm16Scale;
            if (bits(fmaxf(v, -1.0f)) != bits(v)) bad++;
        }
        CHECK(bad == 0);
        volatile float lowest = -32767.0f * kSnorm16Scale;
        CHECK(bits(lowest) == bits(-1.0f));
        // (the one code the encoder never emits is the one the clamp exists for)
        volatile float below = -32768.0f * kSnorm16Scale;
        CHECK(below < -1.0f);
    }
    // ---- 3. dd = NdotH^2 * (a2 - 1) + 1 with a2 - 1 == +0 -------------------------------------------------------------------
    {
        const float zero = kTerrainA2 - 1.0f;
        long bad = 0, n = 0;
        auto one = [&](float x) {
            volatile float xx = x * x;
            volatile float p = xx * zero;
            volatile float d = p + 1.0f;
            n++;
            if (bits(d) != bits(1.0f) || bits(fmaf(xx, zero, 1.0f)) != bits(1.0f)) bad++;
            volatile float q = x * zero;
            volatile float e = q + 1.0f;
            if (bits(e) != bits(1.0f) || bits(fmaf(x, zero, 1.0f)) != bits(1.0f)) bad++;
        };
        const int steps = 1 << 20;
        for (int i = 0; i <= steps; i++) one((float)i / (float)steps);                 // dense, both endpoints
        for (uint32_t u = 0; u < 0x00800000u; u += 0x3fffu) { float x; std::memcpy(&x, &u, 4); one(x); }     // denormals
        for (uint32_t u = 0x3f800000u; u > 0x3f800000u - 4096u; u--) { float x; std::memcpy(&x, &u, 4); one(x); }       // the last floats below 1
        CHECK(bad == 0 && n > steps);
    }
    std::printf("terrain_surface: %ld cases, %ld failures\n", cases, failures);
    return failures ? EXIT_FAILURE : EXIT_SUCCESS;
}
