// Check of light_domain() (vrenderer_amd/csrc/vr_light_domain.h) against an fp32 restatement of the cleared-texel path of
// shade_pixel (vrenderer_amd/csrc/vr_deferred_dev.h: decode_surface, add_light, finish_pixel), in the header's operation order
// with the intrinsics as their IEEE counterparts (v_rcp_f32 -> 1 / x, v_rsq_f32 -> 1 / sqrt(x), v_med3_f32(x, 0, 1) ->
// fmin(fmax(x, 0), 1), v_max / v_min -> fmaxf / fminf; no contraction).
//  (a) sky_is_zero implies +0 (the bit pattern) in all three channels at every pixel of 8x4, 64x48 and 127x5 frames: over seeded
//      scenes that draw every parameter from ranges far wider than the predicate admits, and at each boundary of the predicate
//      approached from both sides (the admitted side must shade to +0; the other side must be rejected);
//  (b) every NaN and infinity in a field the light's type reads, the matrix, the camera position or an ambient channel is refused
//      and named; a non-finite value in a field the type does not read is not;
//  (c) every seeded ORDINARY scene - the cameras of tests/common.py at 5 to 150 degrees of field of view with the light ranges of
//      test_deferred_fuzz_random_gbuffer_and_lights - is accepted: a predicate that rejected those would turn the fast paths off.
// Plain C++17, no GPU: g++ -std=c++17 -Wall -Werror -I vrenderer_amd/csrc tests/host/light_domain_check.cpp
#include "vr_light_domain.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

struct Light {                     // vr_light's members (include/vrterrain.h)
    float direction[3]; int32_t type; float position[3]; float radius; float color[3]; float intensity;
    float angular_size_or_inv_range; float inner_angle, outer_angle; float out_of_bounds_shadow;
};
struct Scene { float c2w[16], cam[3], amb_top[3], amb_bot[3]; std::vector<Light> lights; };

// ---- the cleared-texel path of shade_pixel, fp32 -------------------------------------------------------------------------------
static float rcp(float x) { return 1.0f / x; }
static float rsq(float x) { return 1.0f / sqrtf(x); }
static float sat(float x) { return fminf(fmaxf(x, 0.0f), 1.0f); }
static float dot3(const float a[3], const float b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

struct Surface { float albedo[3], F0[3], E[3], N[3], wp[3], vi[3], R[3], occlusion, alpha, a2, kk, gv; };
static Surface decode_cleared(const Scene& s, int w, int h, int px, int py)
{
    Surface f{};                                                      // albedo = F0 = lut[0] = 0, occlusion 0, N = 0, E = 0
    const float rough = 0.0f, depth = 1.0f;
    const float sx = 2.0f / (float)w, sy = -2.0f / (float)h;
    const float cx = ((float)px + 0.5f) * sx + -1.0f, cy = ((float)py + 0.5f) * sy + 1.0f;
    float e4[4];
    for (int j = 0; j < 4; j++) e4[j] = ((cx * s.c2w[j] + cy * s.c2w[4 + j]) + depth * s.c2w[8 + j]) + s.c2w[12 + j];
    const float rw = rcp(e4[3]);                                      // (vr_rcp_exact and v_rcp_f32 alike: the sun-only path's contracted sums are not restated)
    for (int c = 0; c < 3; c++) f.wp[c] = e4[c] * rw;
    const float d[3] = { f.wp[0] - s.cam[0], f.wp[1] - s.cam[1], f.wp[2] - s.cam[2] };
    const float dl = rsq(dot3(d, d));
    for (int c = 0; c < 3; c++) f.vi[c] = d[c] * dl;
    const float NdotVi = dot3(f.vi, f.N), two = 2.0f * NdotVi;
    for (int c = 0; c < 3; c++) f.R[c] = f.vi[c] - f.N[c] * two;
    const float NdotV = sat(-NdotVi);
    f.alpha = fmaxf(0.01f, rough * rough); f.a2 = f.alpha * f.alpha; f.kk = ((rough + 1.0f) * (rough + 1.0f)) * 0.125f;
    f.gv = NdotV * (1.0f - f.kk) + f.kk;
    return f;
}
static void add_light(const Surface& s, const Light& l, float intensity, float diffuseTerm[3], float specularTerm[3])
{
    const float INV_PI = 0.318309886183790671538f;
    float cosH, sinH, tanH, L[3], irr;
    dom_half_angle(l.type == kDomDirectional ? l.angular_size_or_inv_range : 0.0f, &cosH, &sinH, &tanH);
    if (l.type == kDomDirectional) { for (int c = 0; c < 3; c++) L[c] = -l.direction[c]; irr = intensity; }
    else {
        const float inv_range = l.angular_size_or_inv_range;
        const float stl[3] = { l.position[0] - s.wp[0], l.position[1] - s.wp[1], l.position[2] - s.wp[2] };
        const float d2 = dot3(stl, stl), rd = rsq(d2);
        for (int c = 0; c < 3; c++) L[c] = stl[c] * rd;
        float att = 1.0f;
        if (inv_range > 0.0f) {
            const float q2 = d2 * (inv_range * inv_range), sa = sat(1.0f - q2 * q2);
            att = sa * sa;
            if (att == 0.0f) return;
        }
        irr = intensity * (rd * rd);
        if (l.type == kDomSpot) {
            const float LdotD = fminf(fmaxf(-dot3(L, l.direction), -1.0f), 1.0f);
            const float ts = sat((acosf(LdotD) - l.inner_angle) * rcp(l.outer_angle - l.inner_angle));
            const float spotlight = 1.0f - ts * ts * (3.0f - 2.0f * ts);
            if (spotlight == 0.0f) return;
            att *= spotlight;
        }
        if (l.radius > 0.0f) {
            const float x = fminf(l.radius * rd, 1.0f), halfAng = atanf(x);
            irr = (intensity * rcp(l.radius * l.radius)) * (halfAng * halfAng);
            tanH = x; cosH = rsq(1.0f + x * x); sinH = x * cosH;
        }
        irr *= att;
    }
    const float NdotLd = fmaxf(dot3(s.N, L), 0.0f);
    const float kd = (NdotLd * INV_PI) * irr;
    const float cosT = fminf(fmaxf(dot3(s.R, L), -1.0f), 1.0f);
    float k1 = 0.0f, k2 = 1.0f;
    if (cosT < cosH) { k2 = sinH * rsq(fmaxf(1.0f - cosT * cosT, 1e-12f)); k1 = cosH - cosT * k2; }
    float CL[3], Hv[3];
    for (int c = 0; c < 3; c++) { CL[c] = L[c] * k1 + s.R[c] * k2; Hv[c] = CL[c] - s.vi[c]; }
    const float hl2 = dot3(Hv, Hv), hs = hl2 > 0.0f ? rsq(hl2) : 0.0f;
    const float NdotH = sat(dot3(s.N, Hv) * hs), NdotL = sat(dot3(s.N, CL)), VdotH = sat(-dot3(s.vi, Hv) * hs);
    const float corrAlpha = sat(s.alpha + 0.5f * tanH);
    const float dd = (NdotH * NdotH) * (s.a2 - 1.0f) + 1.0f;
    const float gl = NdotL * (1.0f - s.kk) + s.kk;
    const float num = (s.a2 * s.a2) * (NdotL * irr) * (0.25f * INV_PI);
    const float den = ((corrAlpha * dd) * (corrAlpha * dd)) * (gl * s.gv);
    const float ks = num * rcp(den);
    const float om = 1.0f - VdotH, om2 = om * om, fw = (om2 * om2) * om;
    for (int c = 0; c < 3; c++) {
        const float F = s.F0[c] + (1.0f - s.F0[c]) * fw;
        diffuseTerm[c] += (s.albedo[c] * kd) * l.color[c];
        specularTerm[c] += (F * ks) * l.color[c];
    }
}
// sf: the shadow term of light 0 where that is directional (shade_pixel<_, SHADOW>: skipped at 0, intensity * sf otherwise)
static void shade_cleared(const Scene& s, int w, int h, int px, int py, float sf, float out[3])
{
    const Surface f = decode_cleared(s, w, h, px, py);
    float dT[3] = { 0.0f, 0.0f, 0.0f }, sT[3] = { 0.0f, 0.0f, 0.0f };
    for (size_t i = 0; i < s.lights.size(); i++) {
        const Light& l = s.lights[i];
        if (i == 0 && l.type == kDomDirectional && sf != 1.0f) { if (sf != 0.0f) add_light(f, l, l.intensity * sf, dT, sT); continue; }
        add_light(f, l, l.intensity, dT, sT);
    }
    const float tt = f.N[1] * 0.5f + 0.5f;
    for (int c = 0; c < 3; c++) {
        const float amb = (s.amb_bot[c] + (s.amb_top[c] - s.amb_bot[c]) * tt) * f.occlusion;
        out[c] = (dT[c] + amb * f.albedo[c]) + (sT[c] + amb * f.F0[c]) + f.E[c];
    }
}

// ---- scenes --------------------------------------------------------------------------------------------------------------------
static bool invert4(const double m[16], double inv[16])
{
    double a[4][8];
    for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) { a[i][j] = m[i * 4 + j]; a[i][4 + j] = i == j ? 1.0 : 0.0; }
    for (int c = 0; c < 4; c++) {
        int p = c;
        for (int r = c + 1; r < 4; r++) if (fabs(a[r][c]) > fabs(a[p][c])) p = r;
        if (a[p][c] == 0.0) return false;
        for (int j = 0; j < 8; j++) { const double t = a[c][j]; a[c][j] = a[p][j]; a[p][j] = t; }
        const double d = a[c][c];
        for (int j = 0; j < 8; j++) a[c][j] /= d;
        for (int r = 0; r < 4; r++) if (r != c) { const double f = a[r][c]; for (int j = 0; j < 8; j++) a[r][j] -= f * a[c][j]; }
    }
    for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) inv[i * 4 + j] = a[i][4 + j];
    return true;
}
// look-at + D3D-style perspective, row vectors (clip = world * view * proj); z_far <= 0: an infinite far plane
static void camera(Scene& s, const double eye[3], const double tgt[3], double vfov_deg, double aspect, double zn, double zf)
{
    double f[3] = { tgt[0] - eye[0], tgt[1] - eye[1], tgt[2] - eye[2] };
    const double fl = sqrt(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]);
    for (double& v : f) v /= fl;
    double up[3] = { 0.0, 1.0, 0.0 };
    if (fabs(f[1]) > 0.999) { up[1] = 0.0; up[2] = 1.0; }
    double r[3] = { up[1] * f[2] - up[2] * f[1], up[2] * f[0] - up[0] * f[2], up[0] * f[1] - up[1] * f[0] };
    const double rl = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
    for (double& v : r) v /= rl;
    const double u[3] = { f[1] * r[2] - f[2] * r[1], f[2] * r[0] - f[0] * r[2], f[0] * r[1] - f[1] * r[0] };
    const double view[16] = { r[0], u[0], f[0], 0, r[1], u[1], f[1], 0, r[2], u[2], f[2], 0,
                              -(r[0] * eye[0] + r[1] * eye[1] + r[2] * eye[2]), -(u[0] * eye[0] + u[1] * eye[1] + u[2] * eye[2]),
                              -(f[0] * eye[0] + f[1] * eye[1] + f[2] * eye[2]), 1 };
    const double ys = 1.0 / tan(0.5 * vfov_deg * 3.14159265358979323846 / 180.0), xs = ys / aspect, zs = zf > 0.0 ? zf / (zf - zn) : 1.0;
    const double proj[16] = { xs, 0, 0, 0, 0, ys, 0, 0, 0, 0, zs, 1, 0, 0, -zn * zs, 0 };
    double w2c[16], inv[16];
    for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) { double t = 0.0; for (int k = 0; k < 4; k++) t += view[i * 4 + k] * proj[k * 4 + j]; w2c[i * 4 + j] = t; }
    if (!invert4(w2c, inv)) { std::printf("FAIL singular camera\n"); std::exit(EXIT_FAILURE); }
    for (int i = 0; i < 16; i++) s.c2w[i] = (float)inv[i];
    for (int c = 0; c < 3; c++) s.cam[c] = (float)eye[c];
}
static Light directional(float dx, float dy, float dz, float irradiance, float angular_deg)
{
    Light l{};
    const float n = sqrtf(dx * dx + dy * dy + dz * dz);
    l.type = kDomDirectional; l.direction[0] = dx / n; l.direction[1] = dy / n; l.direction[2] = dz / n;
    l.color[0] = l.color[1] = l.color[2] = 1.0f; l.intensity = irradiance; l.angular_size_or_inv_range = angular_deg * 0.017453292f;
    return l;
}
static Light point(float x, float y, float z, float intensity, float range, float radius = 0.0f)
{
    Light l{};
    l.type = kDomPoint; l.position[0] = x; l.position[1] = y; l.position[2] = z; l.color[0] = l.color[1] = l.color[2] = 1.0f;
    l.intensity = intensity; l.angular_size_or_inv_range = range > 0.0f ? 1.0f / range : 0.0f; l.radius = radius;
    return l;
}
static Light spot(float x, float y, float z, float dx, float dy, float dz, float intensity, float range, float inner_deg, float outer_deg, float radius = 0.0f)
{
    Light l = point(x, y, z, intensity, range, radius);
    const float n = sqrtf(dx * dx + dy * dy + dz * dz);
    l.type = kDomSpot; l.direction[0] = dx / n; l.direction[1] = dy / n; l.direction[2] = dz / n;
    l.inner_angle = inner_deg * 0.017453292f; l.outer_angle = outer_deg * 0.017453292f;
    return l;
}

// ---- the checks ----------------------------------------------------------------------------------------------------------------
static long failures = 0, pixels = 0;
static void fail(const char* what, const char* name) { if (failures++ < 30) std::printf("FAIL %s: %s\n", what, name); }
static LightDomain domain(const Scene& s) { return light_domain(s.c2w, s.cam, 64, 48, s.amb_top, s.amb_bot, s.lights.data(), (int)s.lights.size()); }

static const int kFrames[3][2] = { { 8, 4 }, { 64, 48 }, { 127, 5 } };
// every pixel of the three frames is +0 in every channel, without a shadow term and with one on light 0: inside the map (0.37, 0)
// and outside it, where shadow_factor returns the light's out_of_bounds_shadow
static bool all_plus_zero(const Scene& s, const char* name, bool report)
{
    const float kShadow[4] = { 1.0f, 0.37f, 0.0f, s.lights.empty() ? 1.0f : s.lights[0].out_of_bounds_shadow };
    for (const auto& fr : kFrames)
        for (int py = 0; py < fr[1]; py++)
            for (int px = 0; px < fr[0]; px++)
                for (float sf : kShadow) {
                    float out[3];
                    shade_cleared(s, fr[0], fr[1], px, py, sf, out);
                    pixels++;
                    uint32_t bits[3];
                    std::memcpy(bits, out, sizeof(bits));
                    if (bits[0] | bits[1] | bits[2]) {
                        if (report && failures < 30) std::printf("  %s: %dx%d pixel (%d, %d) shadow %g -> %g %g %g\n", name, fr[0], fr[1], px, py, sf, out[0], out[1], out[2]);
                        return false;
                    }
                    if (s.lights.empty() || s.lights[0].type != kDomDirectional) break;
                }
    return true;
}
// (a): an accepted scene shades to +0; returns whether it was accepted
static bool hold(const Scene& s, const char* name)
{
    const LightDomain d = domain(s);
    if (d.refuse) { fail("refused", name); return false; }
    if (d.sky_is_zero && !all_plus_zero(s, name, true)) fail("sky_is_zero but a pixel is not +0", name);
    return d.sky_is_zero;
}
static long boundary_cases = 0;
static void boundary(const Scene& inside, const Scene& outside, const char* name)
{
    boundary_cases++;
    if (!hold(inside, name)) fail("the admitted side of a boundary is rejected", name);
    if (hold(outside, name)) fail("the far side of a boundary is admitted", name);
}

static Scene ordinary_base()
{
    Scene s{};
    const double eye[3] = { -300.0, 120.0, 80.0 }, tgt[3] = { 200.0, 60.0, -40.0 };
    camera(s, eye, tgt, 60.0, 16.0 / 9.0, 0.1, 10000.0);
    s.amb_top[0] = 0.3f; s.amb_top[1] = 0.4f; s.amb_top[2] = 0.5f; s.amb_bot[0] = 0.1f; s.amb_bot[1] = 0.09f; s.amb_bot[2] = 0.08f;
    return s;
}
static float up(float x) { return nextafterf(x, INFINITY); }

int main()
{
    // ---- (c) ordinary scenes: tests/common.py's CAMERAS, raw and as scaled_camera scales them for a 256-unit world
    const double kCams[8][2][3] = { { { 0, 300, -600 }, { 0, 0, 0 } }, { { 600, 250, 0 }, { 0, 0, 0 } }, { { 0, 250, -600 }, { 0, 0, 0 } }, { { -424.26, 250, 424.26 }, { 0, 0, 0 } },
                                    { { 10, 900, 10 }, { 0, 0, 1 } }, { { -300, 120, 80 }, { 200, 60, -40 } }, { { 50, 40, -20 }, { 300, 80, 200 } }, { { 900, 500, 900 }, { 0, 0, 0 } } };
    std::mt19937 rng(4711);
    auto uni = [&rng](double lo, double hi) { return (float)(lo + (hi - lo) * (double)(rng() >> 8) * (1.0 / 16777216.0)); };
    long ordinary = 0, ordinary_accepted = 0;
    for (int it = 0; it < 400; it++) {
        Scene s{};
        const int ci = it % 8;
        const double k = (it / 8) % 2 ? 0.125 : 1.0;
        const double eye[3] = { kCams[ci][0][0] * k, kCams[ci][0][1] * k, kCams[ci][0][2] * k }, tgt[3] = { kCams[ci][1][0] * k, kCams[ci][1][1] * k, kCams[ci][1][2] * k };
        const double fov = it < 16 ? 60.0 : uni(5.0, 150.0);
        const int* fr = kFrames[it % 3];
        camera(s, eye, tgt, fov, it % 5 == 0 ? 320.0 / 180.0 : (double)fr[0] / fr[1], 0.1, 10000.0);
        for (int c = 0; c < 3; c++) { s.amb_top[c] = uni(0.0, 1.0); s.amb_bot[c] = uni(0.0, 1.0); }
        const int n = 1 + (int)(rng() % 8);
        for (int i = 0; i < n; i++) {                                  // the fuzz test's ranges
            Light l;
            const int kind = (int)(rng() % 4);
            const float x = uni(-60, 60), y = uni(20, 120), z = uni(-60, 60);
            const float ranges[3] = { 0.0f, 80.0f, 200.0f };
            if (kind == 0) l = directional(uni(-1, 1), uni(-1, 1) - 0.01f, uni(-1, 1), uni(0.2, 2.0), uni(0.1, 5.0));
            else if (kind == 1) l = point(x, y, z, uni(500, 5000), ranges[rng() % 3]);
            else if (kind == 2) l = point(x, y, z, uni(500, 5000), 150.0f, uni(0.5, 8.0));
            else { const float inner = uni(3, 30);
                   l = spot(x, y, z, uni(-1, 1), uni(-1, 1) - 1.5f, uni(-1, 1), uni(1000, 9000), rng() % 2 ? 250.0f : 0.0f, inner, inner + uni(2, 30), rng() % 2 ? 2.0f : 0.0f); }
            for (int c = 0; c < 3; c++) l.color[c] = uni(0.1, 1.0);
            l.out_of_bounds_shadow = 1.0f;
            s.lights.push_back(l);
        }
        ordinary++;
        if (hold(s, "ordinary scene")) ordinary_accepted++;
        else if (failures < 30) { const LightDomain d = domain(s); std::printf("  ordinary scene %d (camera %d x %g, fov %g) rejected: %s (light %d)\n", it, ci, k, fov, d.why ? d.why : "?", d.light); }
    }
    if (ordinary_accepted != ordinary) fail("the predicate rejects ordinary scenes", "(c)");

    // ---- (a) boundaries, from both sides.  `base` is accepted; each case moves one quantity to its limit and one step beyond.
    const Scene base = ordinary_base();
    if (!hold(base, "base")) fail("the base scene is rejected", "base");
    {
        Scene a = base, b = base;
        a.lights = { directional(-0.9f, -0.25f, 0.35f, kDomParamMax, 0.53f) }; b.lights = { directional(-0.9f, -0.25f, 0.35f, up(kDomParamMax), 0.53f) };
        boundary(a, b, "directional intensity at 2^40");
        a.lights = { directional(-0.9f, -0.25f, 0.35f, -kDomParamMax, 0.53f) }; b.lights = { directional(-0.9f, -0.25f, 0.35f, -up(kDomParamMax), 0.53f) };
        boundary(a, b, "directional intensity at -2^40");
        a.lights = { directional(-0.9f, -0.25f, 0.35f, kDomParamMax, 0.53f) }; b.lights = a.lights;
        for (int c = 0; c < 3; c++) { a.lights[0].color[c] = kDomParamMax; b.lights[0].color[c] = kDomParamMax; }
        b.lights[0].color[1] = up(kDomParamMax);
        boundary(a, b, "directional intensity and color at 2^40");
        a.lights = { directional(-0.9f, -0.25f, 0.35f, kDomParamMax, 0.53f) }; b.lights = a.lights;
        a.lights[0].out_of_bounds_shadow = kDomParamMax; b.lights[0].out_of_bounds_shadow = up(kDomParamMax);
        boundary(a, b, "out_of_bounds_shadow and intensity at 2^40");
        a.lights[0].out_of_bounds_shadow = -kDomParamMax; b.lights[0].out_of_bounds_shadow = -up(kDomParamMax);
        boundary(a, b, "out_of_bounds_shadow at -2^40");
        {   // the bound is needed: intensity * out_of_bounds_shadow overflows, irr = Inf, 0 * Inf = NaN
            Scene o = base; o.lights = { directional(-0.9f, -0.25f, 0.35f, 1e9f, 0.53f) }; o.lights[0].out_of_bounds_shadow = 1e30f;
            boundary_cases++;
            if (domain(o).sky_is_zero) fail("intensity 1e9 with out_of_bounds_shadow 1e30 is admitted", "out_of_bounds_shadow");
            if (all_plus_zero(o, "out_of_bounds_shadow", false)) fail("the restatement does not see the shadow term's overflow", "out_of_bounds_shadow");
        }
        a.lights = { directional(1, 1, 1, 1.0f, 0.53f) }; b.lights = a.lights;
        for (int c = 0; c < 3; c++) { a.lights[0].direction[c] = c == 1 ? -kDomParamMax : kDomParamMax; b.lights[0].direction[c] = a.lights[0].direction[c]; }
        b.lights[0].direction[2] = up(kDomParamMax);
        boundary(a, b, "directional direction at 2^40");
        // half angle: the largest angular size whose half angle has cos > 0 and tan >= 0 in fp32, and the next float
        float ang = 3.0f;
        for (;;) { float ch, sh, th; dom_half_angle(up(ang), &ch, &sh, &th); if (!(ch > 0.0f && sh >= 0.0f && th >= 0.0f)) break; ang = up(ang); }
        a.lights = { directional(-0.9f, -0.25f, 0.35f, 2.0f, 0.0f) }; b.lights = a.lights;
        a.lights[0].angular_size_or_inv_range = ang; b.lights[0].angular_size_or_inv_range = up(ang);
        boundary(a, b, "directional half angle below pi/2");
        a.lights[0].angular_size_or_inv_range = 0.0f; b.lights[0].angular_size_or_inv_range = -1e-3f;
        boundary(a, b, "directional angular size at 0");
        for (int type = kDomSpot; type <= kDomPoint; type++) {
            const Light l0 = type == kDomPoint ? point(10, 50, -20, 1.0f, 0.0f) : spot(10, 50, -20, 0.3f, -1, 0.2f, 1.0f, 0.0f, 20, 35);
            a.lights = { l0 }; b.lights = { l0 };
            a.lights[0].intensity = kDomParamMax; b.lights[0].intensity = up(kDomParamMax);
            for (int c = 0; c < 3; c++) a.lights[0].color[c] = b.lights[0].color[c] = kDomParamMax;
            boundary(a, b, type == kDomPoint ? "unranged point intensity at 2^40" : "unranged spot intensity at 2^40");
            a.lights = { l0 }; b.lights = { l0 };
            a.lights[0].angular_size_or_inv_range = kDomParamMax; b.lights[0].angular_size_or_inv_range = up(kDomParamMax);
            boundary(a, b, "1/range at 2^40");
            a.lights[0] = l0; b.lights[0] = l0;
            a.lights[0].radius = kDomRadiusMin; b.lights[0].radius = nextafterf(kDomRadiusMin, 0.0f);
            boundary(a, b, "source radius at 2^-20");
            a.lights[0].radius = kDomParamMax; b.lights[0].radius = up(kDomParamMax);
            boundary(a, b, "source radius at 2^40");
            a.lights[0] = l0; b.lights[0] = l0;
            a.lights[0].position[1] = (float)kDomPosMax; b.lights[0].position[1] = up((float)kDomPosMax);
            boundary(a, b, "light position at 2^60");
        }
        {
            const Light l0 = spot(10, 50, -20, 0.3f, -1, 0.2f, 3000.0f, 250.0f, 20, 35);
            a.lights = { l0 }; b.lights = { l0 };
            a.lights[0].inner_angle = 0.5f; a.lights[0].outer_angle = 0.5f + kDomConeMin; b.lights[0].inner_angle = 0.5f; b.lights[0].outer_angle = nextafterf(0.5f + kDomConeMin, 0.0f);
            boundary(a, b, "spot cone outer - inner at 2^-20");
            a.lights[0] = l0; b.lights[0] = l0;
            for (int c = 0; c < 3; c++) { a.lights[0].direction[c] = kDomParamMax; b.lights[0].direction[c] = kDomParamMax; }
            b.lights[0].direction[0] = -up(kDomParamMax);
            boundary(a, b, "spot axis at 2^40");
        }
        a = base; b = base;
        a.lights = { directional(-0.9f, -0.25f, 0.35f, 1.0f, 0.53f) }; b.lights = a.lights;
        for (int c = 0; c < 3; c++) { a.amb_top[c] = kDomParamMax; a.amb_bot[c] = -kDomParamMax; b.amb_top[c] = kDomParamMax; b.amb_bot[c] = -kDomParamMax; }
        b.amb_bot[2] = -up(kDomParamMax);
        boundary(a, b, "ambient colours at +-2^40");
        // w: the matrix is homogeneous - scaled as a whole it reconstructs the same positions - so w_lo and w_max reach their
        // limits by bisection on the scale
        for (int side = 0; side < 2; side++) {
            double lo = side ? 1.0 : 0x1p-80, hi = side ? 0x1p80 : 1.0;      // side 0: accepted at hi; side 1: accepted at lo
            for (int i = 0; i < 200; i++) {
                const double mid = sqrt(lo * hi);
                Scene t = base; t.lights = { point(10, 50, -20, 800.0f, 0.0f) };
                for (float& v : t.c2w) v = (float)((double)v * mid);
                const bool ok = domain(t).sky_is_zero;
                if (ok == (side == 1)) lo = mid; else hi = mid;
            }
            a = base; b = base; a.lights = b.lights = { point(10, 50, -20, 800.0f, 0.0f), directional(-0.9f, -0.25f, 0.35f, 1.0f, 0.53f) };
            for (int i = 0; i < 16; i++) { a.c2w[i] = (float)((double)base.c2w[i] * (side ? lo : hi)); b.c2w[i] = (float)((double)base.c2w[i] * (side ? hi : lo)); }
            boundary(a, b, side ? "w at depth 1 at 2^60" : "w at depth 1 at 2^-60");
        }
        // distance: a positional light that walks from the camera along the view direction through the far plane (bisection on
        // the predicate between the camera side and the plane), of every kind
        for (int kind = 0; kind < 4; kind++) {
            const double eye[3] = { -300.0, 120.0, 80.0 }, tgt[3] = { 200.0, 60.0, -40.0 };
            double f[3] = { tgt[0] - eye[0], tgt[1] - eye[1], tgt[2] - eye[2] };
            const double fl = sqrt(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]);
            auto at = [&](double t) { Light l = kind == 0 ? point(0, 0, 0, 800.0f, 0.0f) : kind == 1 ? point(0, 0, 0, 800.0f, 150.0f) : kind == 2 ? point(0, 0, 0, 800.0f, 0.0f, 4.0f)
                                                         : spot(0, 0, 0, (float)f[0], (float)f[1], (float)f[2], 800.0f, 0.0f, 20, 35);
                                      for (int c = 0; c < 3; c++) l.position[c] = (float)(eye[c] + f[c] / fl * t);
                                      return l; };
            double lo = 100.0, hi = 10000.0;                               // the far plane is 10000 along the axis
            for (int i = 0; i < 100; i++) { const double mid = 0.5 * (lo + hi); Scene t = base; t.lights = { at(mid) }; if (domain(t).sky_is_zero) lo = mid; else hi = mid; }
            a = base; b = base; a.lights = { at(lo) }; b.lights = { at(hi) };
            boundary(a, b, "positional light approaching the far plane");
            // and ON the far plane's computed position of a pixel: rejected, and the model really leaves +0 there
            Scene on = base;
            const Surface sf = decode_cleared(base, 64, 48, 31, 23);
            on.lights = { at(0.0) };
            for (int c = 0; c < 3; c++) on.lights[0].position[c] = sf.wp[c];
            boundary_cases++;
            if (domain(on).sky_is_zero) fail("a light on a far-plane pixel is admitted", "on the far plane");
            if (kind == 0 && all_plus_zero(on, "on the far plane", false)) fail("the restatement shades a light at distance 0 to +0: it cannot tell the sides apart", "on the far plane");
        }
        // the ranged light whose range ends on the far plane, camera side
        a = base; a.lights = { point(-300.0f + 0.9701f * 9000.0f, 120.0f - 0.1164f * 9000.0f, 80.0f - 0.2328f * 9000.0f, 5000.0f, 1000.0f) };
        if (!hold(a, "ranged light ending on the far plane")) fail("rejected", "ranged light ending on the far plane");
        // the camera: far plane at the camera's distance limit (an orthographic-like degenerate: the eye ON the far plane)
        {
            Scene t = base;
            const Surface sf = decode_cleared(base, 64, 48, 10, 10);
            for (int c = 0; c < 3; c++) t.cam[c] = sf.wp[c];
            boundary_cases++;
            if (domain(t).sky_is_zero) fail("camera_pos on the far plane is admitted", "camera");
        }
        // the two accepted-but-outside classes the device tests use
        Scene inf = base;
        { const double eye[3] = { -300.0, 120.0, 80.0 }, tgt[3] = { 200.0, 60.0, -40.0 }; camera(inf, eye, tgt, 60.0, 16.0 / 9.0, 0.1, -1.0); }
        inf.lights = { directional(-0.9f, -0.25f, 0.35f, 1.0f, 0.53f) };
        boundary_cases++;
        { const LightDomain d = domain(inf); if (d.refuse || d.sky_is_zero) fail("an infinite far plane must be accepted and outside sky_is_zero", "infinite far plane"); }
        Scene sun = base; sun.lights = { directional(-0.9f, -0.25f, 0.35f, 3e38f, 0.53f) };
        for (int c = 0; c < 3; c++) sun.lights[0].color[c] = 10.0f;
        boundary_cases++;
        { const LightDomain d = domain(sun); if (d.refuse || d.sky_is_zero) fail("the 3e38 x 10 sun must be accepted and outside sky_is_zero", "3e38 sun"); }
    }

    // ---- (a) seeded wide scenes: magnitudes log-uniform over far more than the predicate admits
    long wide = 0, wide_accepted = 0;
    auto mag = [&](double lo_exp, double hi_exp) { const float m = (float)exp2(uni(lo_exp, hi_exp)); return rng() & 1 ? m : -m; };
    for (int it = 0; it < 1500; it++) {
        Scene s{};
        const double k = exp2(uni(-8, 24));
        const double eye[3] = { uni(-1, 1) * k, uni(-1, 1) * k, uni(-1, 1) * k }, tgt[3] = { eye[0] + uni(-1, 1), eye[1] + uni(-0.9, 0.9), eye[2] + uni(0.1, 1) };
        const double zn = exp2(uni(-10, 4)), zf = it % 11 == 0 ? -1.0 : zn * exp2(uni(1, 30));
        camera(s, eye, tgt, uni(5, 150), exp2(uni(-2, 2)), zn, zf);
        const double scale = it % 3 == 0 ? exp2(uni(-70, 70)) : 1.0;
        for (float& v : s.c2w) v = (float)((double)v * scale);
        for (int c = 0; c < 3; c++) { s.amb_top[c] = mag(-20, 43); s.amb_bot[c] = mag(-20, 43); }
        const int n = (int)(rng() % 4);
        for (int i = 0; i < n; i++) {
            Light l;
            const int kind = (int)(rng() % 4);
            const float far_d = zf > 0.0 ? (float)zf : 1.0f;
            // positions: anywhere, or near the far plane along the view axis
            double p[3] = { eye[0] + mag(-10, 30), eye[1] + mag(-10, 30), eye[2] + mag(-10, 30) };
            if (rng() % 3 == 0) { const double fl = sqrt((tgt[0] - eye[0]) * (tgt[0] - eye[0]) + (tgt[1] - eye[1]) * (tgt[1] - eye[1]) + (tgt[2] - eye[2]) * (tgt[2] - eye[2]));
                                  const double t = far_d * (1.0 + uni(-1, 1) * exp2(uni(-20, 0)));
                                  for (int c = 0; c < 3; c++) p[c] = eye[c] + (tgt[c] - eye[c]) / fl * t; }
            if (kind == 0) { l = directional(uni(-1, 1), uni(-1, 1), uni(0.01, 1), 1.0f, 0.0f); l.angular_size_or_inv_range = rng() % 4 ? uni(0, 3.2) : mag(-20, 10);
                             if (rng() % 4 == 0) for (float& d : l.direction) d *= (float)exp2(uni(0, 60));
                             l.out_of_bounds_shadow = rng() % 4 ? 1.0f : mag(-10, 60); }
            else if (kind == 3) { l = spot((float)p[0], (float)p[1], (float)p[2], uni(-1, 1), uni(-1, 1), uni(0.01, 1), 1.0f, 0.0f, 10, 20);
                                  l.inner_angle = uni(-1, 2); l.outer_angle = l.inner_angle + (rng() % 3 ? uni(0.01, 1.0) : (float)exp2(uni(-30, -10))); }
            else l = point((float)p[0], (float)p[1], (float)p[2], 1.0f, 0.0f);
            if (kind != 0) { l.angular_size_or_inv_range = rng() % 2 ? 0.0f : (float)exp2(uni(-40, 50)); l.radius = rng() % 2 ? 0.0f : (float)exp2(uni(-30, 50)); }
            l.intensity = mag(-10, 60);
            for (float& c : l.color) c = mag(-10, 60);
            s.lights.push_back(l);
        }
        wide++;
        if (hold(s, "wide scene")) wide_accepted++;
    }
    if (wide_accepted < wide / 20 || wide_accepted > wide - wide / 20) fail("the wide scenes do not exercise both answers", "(a)");

    // ---- (b) non-finite values
    long refusals = 0;
    const float kBad[3] = { NAN, INFINITY, -INFINITY };
    auto refused = [&](const Scene& s, const char* name, bool want) {
        const LightDomain d = domain(s);
        refusals++;
        if (d.refuse != want) fail(want ? "a non-finite value is not refused" : "a value the type does not read is refused", name);
        if (want && (!d.field || d.sky_is_zero)) fail("a refusal names no field, or claims sky_is_zero", name);
    };
    for (float v : kBad) {
        Scene s = base; s.lights = { directional(-0.9f, -0.25f, 0.35f, 1.0f, 0.53f) };
        for (int i = 0; i < 16; i++) { Scene t = s; t.c2w[i] = v; refused(t, "clip_to_world", true); }
        for (int c = 0; c < 3; c++) {
            Scene t = s; t.cam[c] = v; refused(t, "camera_pos", true);
            t = s; t.amb_top[c] = v; refused(t, "ambient_top", true);
            t = s; t.amb_bot[c] = v; refused(t, "ambient_bottom", true);
        }
        const Light kinds[3] = { directional(-0.9f, -0.25f, 0.35f, 1.0f, 0.53f), spot(10, 50, -20, 0.3f, -1, 0.2f, 3000.0f, 250.0f, 20, 35), point(10, 50, -20, 800.0f, 150.0f, 2.0f) };
        for (const Light& l0 : kinds) {
            const bool dir = l0.type == kDomDirectional, sp = l0.type == kDomSpot;
            for (int at = 0; at < 2; at++) {                           // the light alone, and behind an ordinary one
                auto with = [&](const Light& l) { Scene t = s; t.lights.clear(); if (at) t.lights.push_back(kinds[0]); t.lights.push_back(l); return t; };
                for (int c = 0; c < 3; c++) {
                    Light l = l0; l.direction[c] = v; refused(with(l), "direction", dir || sp);
                    l = l0; l.position[c] = v; refused(with(l), "position", !dir);
                    l = l0; l.color[c] = v; refused(with(l), "color", true);
                }
                Light l = l0; l.intensity = v; refused(with(l), "intensity", true);
                l = l0; l.angular_size_or_inv_range = v; refused(with(l), "angular_size_or_inv_range", true);
                l = l0; l.radius = v; refused(with(l), "radius", !dir);
                l = l0; l.inner_angle = v; refused(with(l), "inner_angle", sp);
                l = l0; l.outer_angle = v; refused(with(l), "outer_angle", sp);
                l = l0; l.out_of_bounds_shadow = v; refused(with(l), "out_of_bounds_shadow", dir);
            }
        }
    }
    std::printf("light_domain: %ld ordinary scenes (%ld accepted), %ld boundary cases, %ld wide scenes (%ld accepted), %ld non-finite cases, %ld pixels shaded, %ld failures\n",
                ordinary, ordinary_accepted, boundary_cases, wide, wide_accepted, refusals, pixels, failures);
    return failures ? EXIT_FAILURE : EXIT_SUCCESS;
}
