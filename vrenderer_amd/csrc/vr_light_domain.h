// The lighting model's domain as one pure function of what a lighting call is given: the view's clip_to_world and camera
// position, the frame size, both ambient colours and the light list.  Plain C++17: no HIP, no library types (the light is a
// template parameter with vr_light's member names) - a CPU program holds it to an fp32 restatement of the cleared-texel path of
// shade_pixel (tests/host/light_domain_check.cpp).  vr_light_check (vr_deferred.hip) and vr_terrain_render_lit (vr_raster.hip) ask
// it in front of every effect; the answer's second half goes into LightPlanIn (vr_light_plan.h) and the tile pass's LitRequest.
//
// Two answers.
//
// refuse: some value the call reads is a NaN or an infinity - the matrix, the camera position, an ambient channel, a float field
// of a light that its type reads (directional: direction, color, intensity, angular size, out_of_bounds_shadow; point: position,
// color, intensity, 1/range, radius; spot: a point light's and direction, inner_angle, outer_angle) or a half-angle term
// fill_light derives from the angular size.  `field` names it, `light` is its index (-1: not a light's).  VR_ERR_INVALID_ARGUMENT.
//
// sky_is_zero: a cleared texel (depth 1.0, every other plane 0) is GUARANTEED to shade to +0 in all three channels at every
// pixel of the frame.  Three places store +0 for such a texel without shading it: k_deferred (a wave of cleared texels),
// k_deferred_tiled (its background pixels receive no light) and the fused resolve of k_raster (an uncovered pixel).  They agree
// with the kernels that always shade - k_deferred_stream, k_deferred_scalar - exactly where this holds.  Conservative: false where
// the bounds below cannot show it, never true where a pixel of the frame could come out as anything but +0.
//
// Derivation, along decode_surface, add_light, finish_pixel and shadow_factor (vr_deferred_dev.h) as they are written, u = 2^-24.
// A cleared texel decodes to albedo = F0 = lut[0] = 0, occlusion = 0, N = 0, roughness 0 (alpha = 0.01, kk = 1/8), E = 0.
// Every term of the result is then a product with one of those zeros, and 0 * x is 0 for every FINITE x: what has to be shown is
// that no factor is an infinity or a NaN.  (Signs take care of themselves: the sums start from +0 and +0 + -0 = +0.)
//  (1) w at depth 1.  e_j = ((cx M0j + cy M1j) + depth M2j) + M3j with |cx|, |cy| <= 1 is affine in (cx, cy), so its extremes
//      over the frame are at the four corners (+-1, +-1): the corners' w must have one sign.  The fp32 sum is within 8u T_j of
//      the exact one, T_j = |M0j| + |M1j| + |M2j| + |M3j| (the bound of k_light_cull's pad; the contracted order of
//      the sun-only path rounds less often).  Required: w_lo = min |w| - 8u T_3 >= 2^-60 and max |w| + 8u T_3 <= 2^60, which is
//      vr_rcp_exact's stated range and keeps v_rcp_f32 away from denormals.  An infinite far plane has w = 0 there: false.
//  (2) The reconstructed position.  With E, W the exact sums and Q = E / W the exact far-plane point of a pixel, the computed
//      position is (E_c + de_c) / (W + dw) with |de_c| <= 8u T_c, |dw| <= 8u T_3: the point s Q with s = W / (W + dw) in
//      [s0, s1] = [1 / (1 + rho), 1 / (1 - rho)], rho = 8u T_3 / min |w| (< 1 by (1)) - Q moved along its ray through the origin,
//      which is where the cancellation in w goes: 10 % of the distance for a far plane 10^5 near planes away - plus a small
//      error |small_c| <= 8u T_c / w_lo + 4u s1 A_c (the reciprocal and the product; A_c = the largest |Q_c| of the corners).
//      The exact points Q of the frame lie in the convex hull of the four exact corner points Q_k = e(corner) / w(corner) (a
//      projective map of a square with w of one sign), a planar quad, so |wp_c| <= s1 A_c + small_c, required <= 2^60 like
//      |camera_pos_c| and every positional light's |position_c|.  Then d = wp - x has |d_c| <= 2^61 and d . d <= 3 * 2^122.
//  (3) Away from the camera and the lights.  rsq(d . d) is finite only for d . d > 0 (and v_rsq_f32 takes no denormal).  With
//      the quad's plane n . Q = h, a computed position s Q + small has n . (s Q - x) = s h - n . x: where that keeps its sign
//      over [s0, s1] the point x is at least min |s h - n . x| away.  It is also no nearer than its distance to the segment
//      [s0 C, s1 C] less s1 R (C the corners' mean, R the largest |Q_k - C|).  The subtraction adds u (|wp_c| + |x_c|).
//      Required for the camera and for EVERY positional light, ranged or not (with d . d = 0 a ranged light's direction is
//      NaN before its attenuation is looked at):
//          max(plane bound, segment bound) - |small| - 2u (|wp| + |x|) >= 2^-20.
//      Then rd <= 2^20, vi and L are finite vectors of about unit length, N . vi = N . L = 0, R = vi, NdotV = 0, gv = 1/8.
//  (4) Parameters: |intensity|, |color_c|, |direction_c|, |ambient_c| <= 2^40.  irr = intensity * rd^2 <= 2^80 and every later
//      product ((NdotL * irr) * const, x * color_c) has a zero factor and a finite one.  The issue of overflow is therefore not
//      the zero products themselves but their finite factors; 2^40 leaves 2^48 of headroom everywhere.
//      A range: 0 < 1/range <= 2^40 (q2 = d2 / range^2 may overflow to +Inf: saturate(1 - Inf) = 0, the light returns).
//  (5) A directional light's half angle in [0, pi/2): cosH > 0, sinH >= 0, tanH >= 0, so that corrAlpha = saturate(0.01 +
//      tanH / 2) >= 0.01 and den = corrAlpha^2 / 64 > 0 (rcp(0) would be Inf, times num = 0: NaN); k2 <= sinH * 10^6, CL and
//      Hv stay below 2^62, Hv . Hv below 2^126.
//  (6) A spherical source: radius <= 0 (punctual) or 2^-20 <= radius <= 2^40: radius^2 and rcp(radius^2) are normal, intensity *
//      rcp(radius^2) <= 2^80, x = min(radius * rd, 1) in (0, 1].
//  (7) A spot light: |inner_angle|, |outer_angle| <= 2^40 and outer - inner (in fp32, as the kernel subtracts) >= 2^-20: the
//      reciprocal is finite and (acos - inner) * rcp is no 0 * Inf.
//  (8) The shadow term: shade_pixel<_, SHADOW> hands add_light intensity * sf, and shadow_factor returns the light's
//      out_of_bounds_shadow unless u, v, z pass comparisons that a NaN fails (a far-plane pixel is usually outside the map), a sum
//      of weights in [0, 1] over 9 otherwise.  |out_of_bounds_shadow| <= 2^40 keeps that product at or below 2^80 like every
//      other irradiance of (4).  (Required of every directional light: any of them may carry the binding.)
//  One thing is taken as given and not derived: Hv . Hv, where it is not exactly 0, is a normal number (it is the squared length
//  of the difference of two vectors of about unit length; a positive value below 2^-126 would need them to agree to 2^-64 in
//  every component without being equal).
#pragma once
#include <math.h>
#include <stddef.h>

constexpr int kDomDirectional = 1, kDomSpot = 2, kDomPoint = 3;      // VR_LIGHT_* (vr_deferred.hip asserts)
constexpr double kDomWMin = 0x1p-60, kDomWMax = 0x1p60;               // (1)
constexpr double kDomPosMax = 0x1p60;                                 // (2)
constexpr double kDomMinDist = 0x1p-20;                               // (3)
constexpr float kDomParamMax = 0x1p40f;                               // (4), (6), (7), (8)
constexpr float kDomRadiusMin = 0x1p-20f, kDomConeMin = 0x1p-20f;     // (6), (7)

struct LightDomain {
    bool refuse;           // a NaN or an infinity: `field` names it, `light` is the light's index or -1
    const char* field;
    int light;
    bool sky_is_zero;      // (false whenever refuse)
    const char* why;       // the first bound that could not be shown (sky_is_zero false), for messages and the host check
};

inline bool dom_finite(float x) { return x == x && fabsf(x) <= 3.402823466e38f; }
inline bool dom_finite3(const float v[3]) { return dom_finite(v[0]) && dom_finite(v[1]) && dom_finite(v[2]); }
inline bool dom_small3(const float v[3], float m) { return fabsf(v[0]) <= m && fabsf(v[1]) <= m && fabsf(v[2]) <= m; }

// what fill_light derives from a directional light's angular size
inline void dom_half_angle(float angular_size, float* cosH, float* sinH, float* tanH)
{
    const double half = 0.5 * (double)angular_size;
    *cosH = (float)cos(half); *sinH = (float)sin(half); *tanH = (float)tan(half);
}

// the far plane of the frame as (2) and (3) need it
struct DomFarQuad { double C[3], R, n[3], h, s0, s1, err, Wn; bool plane; };
// a lower bound of the distance between x and any pixel's computed far-plane position, less the subtraction's rounding
inline double dom_far_distance(const DomFarQuad& q, const float x[3])
{
    double xn = 0.0, x1 = 0.0, cc = 0.0, xc = 0.0, xx = 0.0;
    for (int c = 0; c < 3; c++) { xn += q.n[c] * (double)x[c]; x1 += fabs((double)x[c]); cc += q.C[c] * q.C[c]; xc += q.C[c] * (double)x[c]; xx += (double)x[c] * (double)x[c]; }
    double plane = 0.0;
    if (q.plane) {
        const double a0 = q.s0 * q.h - xn, a1 = q.s1 * q.h - xn;
        if ((a0 > 0.0 && a1 > 0.0) || (a0 < 0.0 && a1 < 0.0)) plane = fabs(a0) < fabs(a1) ? fabs(a0) : fabs(a1);
    }
    // x to the segment [s0 C, s1 C]: the nearest s is x . C / C . C, clamped
    double sn = cc > 0.0 ? xc / cc : q.s0;
    sn = sn < q.s0 ? q.s0 : sn > q.s1 ? q.s1 : sn;
    const double seg2 = xx - 2.0 * sn * xc + sn * sn * cc;
    const double sphere = sqrt(seg2 > 0.0 ? seg2 : 0.0) - q.s1 * q.R;
    const double scale = q.s1 * (q.R + sqrt(cc)) + x1;
    return (sphere > plane ? sphere : plane) - q.err - 0x1p-23 * (q.Wn + x1) - 1e-9 * scale;      // (1e-9: this arithmetic is double, not exact)
}

template <class Light>
inline LightDomain light_domain(const float c2w[16], const float cam[3], int w, int h, const float amb_top[3], const float amb_bottom[3],
                                const Light* lights, int num_lights)
{
    (void)w; (void)h;      // (the corners of clip space bound every frame size: pixel centres lie inside them)
    LightDomain r{};
    r.light = -1;
    // ---- refuse
    const auto bad = [&r](const char* field, int light) { r.refuse = true; r.field = field; r.light = light; r.why = field; return r; };
    for (int i = 0; i < 16; i++) if (!dom_finite(c2w[i])) return bad("view.clip_to_world", -1);
    if (!dom_finite3(cam)) return bad("view.camera_pos", -1);
    if (!dom_finite3(amb_top)) return bad("ambient_top", -1);
    if (!dom_finite3(amb_bottom)) return bad("ambient_bottom", -1);
    for (int i = 0; i < num_lights; i++) {
        const Light& l = lights[i];
        if (l.type != kDomDirectional && l.type != kDomSpot && l.type != kDomPoint) continue;      // (fill_light refuses it)
        if (!dom_finite3(l.color)) return bad("light.color", i);
        if (!dom_finite(l.intensity)) return bad("light.intensity", i);
        if (!dom_finite(l.angular_size_or_inv_range)) return bad("light.angular_size_or_inv_range", i);
        if (l.type == kDomDirectional) {
            if (!dom_finite3(l.direction)) return bad("light.direction", i);
            if (!dom_finite(l.out_of_bounds_shadow)) return bad("light.out_of_bounds_shadow", i);
            float ch, sh, th;
            dom_half_angle(l.angular_size_or_inv_range, &ch, &sh, &th);
            if (!dom_finite(ch) || !dom_finite(sh) || !dom_finite(th)) return bad("light.angular_size_or_inv_range (half-angle terms)", i);
        } else {
            if (!dom_finite3(l.position)) return bad("light.position", i);
            if (!dom_finite(l.radius)) return bad("light.radius", i);
            if (l.type == kDomSpot) {
                if (!dom_finite3(l.direction)) return bad("light.direction", i);
                if (!dom_finite(l.inner_angle)) return bad("light.inner_angle", i);
                if (!dom_finite(l.outer_angle)) return bad("light.outer_angle", i);
            }
        }
    }
    // ---- sky_is_zero
    const auto no = [&r](const char* why, int light) { r.sky_is_zero = false; r.why = why; r.light = light; return r; };
    const double u8 = 8.0 * 0x1p-24 * 1.001;
    double T[4], Q[4][3], wmin = INFINITY, wmax = 0.0;
    int pos = 0, neg = 0;
    for (int j = 0; j < 4; j++) T[j] = fabs((double)c2w[j]) + fabs((double)c2w[4 + j]) + fabs((double)c2w[8 + j]) + fabs((double)c2w[12 + j]);
    for (int k = 0; k < 4; k++) {
        const double cx = k & 1 ? 1.0 : -1.0, cy = k & 2 ? 1.0 : -1.0;
        double e[4];
        for (int j = 0; j < 4; j++) e[j] = cx * (double)c2w[j] + cy * (double)c2w[4 + j] + (double)c2w[8 + j] + (double)c2w[12 + j];
        if (e[3] > 0.0) pos++; else if (e[3] < 0.0) neg++;
        const double aw = fabs(e[3]);
        if (aw < wmin) wmin = aw;
        if (aw > wmax) wmax = aw;
        for (int c = 0; c < 3; c++) Q[k][c] = aw > 0.0 ? e[c] / e[3] : 0.0;
    }
    if (pos != 4 && neg != 4) return no("w at depth 1 changes sign or is zero inside the frame (an infinite far plane?)", -1);
    const double wlo = wmin - u8 * T[3];
    if (!(wlo >= kDomWMin) || !(wmax + u8 * T[3] <= kDomWMax)) return no("w at depth 1 is outside [2^-60, 2^60] or cancels to rounding noise", -1);
    DomFarQuad q{};
    const double rho = u8 * T[3] / wmin;                              // (< 1: w_lo > 0)
    q.s0 = 1.0 / (1.0 + rho); q.s1 = 1.0 / (1.0 - rho);
    double err2 = 0.0;
    for (int c = 0; c < 3; c++) {
        double A = 0.0;
        for (int k = 0; k < 4; k++) if (fabs(Q[k][c]) > A) A = fabs(Q[k][c]);
        const double small = u8 * T[c] / wlo + 0x1p-22 * q.s1 * A, P = q.s1 * A + small;
        if (!(P <= kDomPosMax) || !(fabs((double)cam[c]) <= kDomPosMax)) return no("far-plane positions or camera_pos beyond 2^60", -1);
        err2 += small * small; q.Wn += P;
        q.C[c] = 0.25 * (Q[0][c] + Q[1][c] + Q[2][c] + Q[3][c]);
    }
    q.err = sqrt(err2);
    for (int k = 0; k < 4; k++) {
        double d2 = 0.0;
        for (int c = 0; c < 3; c++) d2 += (Q[k][c] - q.C[c]) * (Q[k][c] - q.C[c]);
        if (sqrt(d2) > q.R) q.R = sqrt(d2);
    }
    {
        const double a[3] = { Q[1][0] - Q[0][0], Q[1][1] - Q[0][1], Q[1][2] - Q[0][2] }, b[3] = { Q[2][0] - Q[0][0], Q[2][1] - Q[0][1], Q[2][2] - Q[0][2] };
        const double n[3] = { a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0] };
        const double len = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
        q.plane = len > 0.0 && len < INFINITY;
        if (q.plane) for (int c = 0; c < 3; c++) { q.n[c] = n[c] / len; q.h += q.n[c] * q.C[c]; }
    }
    if (!(dom_far_distance(q, cam) >= kDomMinDist)) return no("the far plane cannot be shown to stay away from camera_pos", -1);
    if (!dom_small3(amb_top, kDomParamMax) || !dom_small3(amb_bottom, kDomParamMax)) return no("an ambient colour beyond 2^40", -1);
    for (int i = 0; i < num_lights; i++) {
        const Light& l = lights[i];
        if (l.type != kDomDirectional && l.type != kDomSpot && l.type != kDomPoint) continue;
        if (!(fabsf(l.intensity) <= kDomParamMax) || !dom_small3(l.color, kDomParamMax)) return no("a light's intensity or color beyond 2^40", i);
        if (l.type == kDomDirectional) {
            if (!dom_small3(l.direction, kDomParamMax)) return no("a directional light's direction beyond 2^40", i);
            float ch, sh, th;
            dom_half_angle(l.angular_size_or_inv_range, &ch, &sh, &th);
            if (!(fabsf(l.out_of_bounds_shadow) <= kDomParamMax)) return no("a directional light's out_of_bounds_shadow beyond 2^40", i);
            if (!(l.angular_size_or_inv_range >= 0.0f && ch > 0.0f && sh >= 0.0f && th >= 0.0f)) return no("a directional light's half angle outside [0, pi/2)", i);
            continue;
        }
        if (!(fabs((double)l.position[0]) <= kDomPosMax && fabs((double)l.position[1]) <= kDomPosMax && fabs((double)l.position[2]) <= kDomPosMax))
            return no("a light's position beyond 2^60", i);
        if (!(dom_far_distance(q, l.position) >= kDomMinDist)) return no("the far plane cannot be shown to stay away from a positional light", i);
        if (!(l.angular_size_or_inv_range <= kDomParamMax)) return no("a light's 1/range beyond 2^40", i);
        if (l.radius > 0.0f && !(l.radius >= kDomRadiusMin && l.radius <= kDomParamMax)) return no("a source radius outside [2^-20, 2^40]", i);
        if (l.type == kDomSpot) {
            if (!dom_small3(l.direction, kDomParamMax)) return no("a spot light's axis beyond 2^40", i);
            if (!(fabsf(l.inner_angle) <= kDomParamMax && fabsf(l.outer_angle) <= kDomParamMax && l.outer_angle - l.inner_angle >= kDomConeMin))
                return no("a spot light's cone: angles beyond 2^40 or outer - inner below 2^-20", i);
        }
    }
    r.sky_is_zero = true;
    r.light = -1;
    return r;
}
