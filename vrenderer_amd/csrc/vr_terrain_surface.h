// What every terrain pixel's G-buffer texel holds beyond its albedo and normal, and what the lighting model derives from it:
// main_ps writes roughness 1 (terrain_ps.hlsl:79), one specular word for the whole launch (:76) and no emissive (:80).  ONE
// place for the producer (pixel_shader / pixel_shader_fast, vr_raster.hip) and for the consumer that knows its texel came from
// that producer (the TERRAIN flavour of decode_surface / add_light, vr_deferred_dev.h: the fused resolve of k_raster), so that
// the two cannot drift apart.  Plain C++17, host and device; tests/host/terrain_surface_check.cpp.
#pragma once
#include <stdint.h>

constexpr uint32_t kTerrainRoughBits = 32767u;                 // snorm16 of roughness 1: the upper half of the normal plane's second word
constexpr float kSnorm16Scale = 1.0f / 32767.0f;               // decode_surface's sn16
// (a > b ? a : b is fmaxf for operands that are not NaN; usable in a constant expression by every compiler)
constexpr float terrain_max(float a, float b) { return a > b ? a : b; }
// decode_surface's expressions, evaluated on those bits (none of them has a mul feeding an add: contraction changes nothing)
constexpr float kTerrainRough = terrain_max((float)(int16_t)kTerrainRoughBits * kSnorm16Scale, -1.0f);
constexpr float kTerrainAlpha = terrain_max(0.01f, kTerrainRough * kTerrainRough);
constexpr float kTerrainA2 = kTerrainAlpha * kTerrainAlpha;
constexpr float kTerrainKk = ((kTerrainRough + 1.0f) * (kTerrainRough + 1.0f)) * 0.125f;

// The facts the TERRAIN flavour's folds rest on:
static_assert(kTerrainRough == 1.0f, "32767 * (1 / 32767f) is exactly 1: alpha = 1, kk = 0.5");
static_assert(kTerrainA2 - 1.0f == 0.0f, "dd = NdotH^2 * (a2 - 1) + 1 is exactly 1 for every finite NdotH; a2 * a2 is 1");
static_assert(-32767.0f * kSnorm16Scale == -1.0f, "no snorm16 code the encoder emits ([-32767, 32767]) decodes below -1: the decode's fmax is an identity");
static_assert(kTerrainAlpha == 1.0f && kTerrainKk == 0.5f, "the values the comments of the TERRAIN flavour quote");
