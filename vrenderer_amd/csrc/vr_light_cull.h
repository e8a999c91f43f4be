// The two geometric tests of the tiled lighting pass's culling stage (k_light_cull, vr_deferred.hip), for the device and for the
// host: the host compiles this header alone (tests/host/light_cull_check.cpp) and checks the cone test against a double-precision
// sampling of the box.  Both tests use +, -, *, / and sqrt only, with no contraction - the operations IEEE 754 rounds the
// same way everywhere - so the function the host checks is, bit for bit, the function the device runs.
// A culled light must have a term of exactly +0 at every pixel of the cell; the margins are derived there.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define VR_CULL_FN __host__ __device__ __forceinline__
#else
#define VR_CULL_FN inline
#endif

// squared distance from a point to a box, compared with the light's range (attenuation is exactly 0 from the range outwards).
// The caller passes r2 = range^2 * 1.0001: the test's own fp32 rounding (three squares and two sums, the reciprocal and
// the square of the range: < 8 u relative) cannot turn a touching sphere into a miss.
VR_CULL_FN bool sphere_touches(const float* __restrict__ box, const float pos[3], float r2)
{
    float d2 = 0.0f;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int c = 0; c < 3; c++) { const float d = __builtin_fmaxf(__builtin_fmaxf(box[c] - pos[c], pos[c] - box[3 + c]), 0.0f); d2 += d * d; }
    return d2 <= r2;
}

// ---- spot cones -----------------------------------------------------------------------------------------------------------
// kConeAngleMargin (radians) is added to outer_angle: it covers acosf's error, the rounding of (angle - inner) and the 1-ulp
// reciprocal of (outer - inner) in add_light (vr_deferred_dev.h), where the cone term is exactly 0 only if ts reaches 1.
// kConeCosMargin is taken from the cosine: it covers the rounding of L . axis in add_light, an axis whose length differs from 1
// by up to kConeAxisTolerance / 2, and this test's own rounding (all relative to |v|: the position roundings go into rb).
constexpr float kConeAngleMargin = 1.0e-5f;
constexpr float kConeCosMargin = 2.0e-5f;
constexpr float kConeAxisTolerance = 1.0e-6f;     // | |axis|^2 - 1 | beyond which a cone is not culled
constexpr float kConeMaxSin = 0.7f;               // a box whose bounding sphere subtends more than asin(0.7) at the apex is kept

// Host side, once per light: cos and sin of (outer_angle + kConeAngleMargin), or (0, 0) = "this cone is not culled" (outer_angle
// of pi/2 or more, a non-positive one, or an axis that is not of unit length).
inline void cone_cull_terms(const float axis[3], float outer_angle, float* cos_m, float* sin_m)
{
    *cos_m = *sin_m = 0.0f;
    const double a2 = (double)axis[0] * axis[0] + (double)axis[1] * axis[1] + (double)axis[2] * axis[2];
    const double phi = (double)outer_angle + (double)kConeAngleMargin;
    if (!(fabs(a2 - 1.0) <= (double)kConeAxisTolerance) || !(outer_angle > 0.0f) || !(phi < 1.5707)) return;
    *cos_m = (float)cos(phi); *sin_m = (float)sin(phi);
}

// true: no point of the box [box[0..2], box[3..5]] lies inside the cone (apex pos, unit axis, half angle outer_angle) - by the
// box's bounding sphere (centre c, radius rb; v = c - pos): with theta = angle(v, axis) and alpha = asin(rb / |v|) the smallest
// angle any point of the sphere makes with the axis is theta - alpha, and
//     theta - alpha >= phi   <=>   v . axis <= |v| cos(phi + alpha) = cos(phi) sqrt(|v|^2 - rb^2) - sin(phi) rb
// (phi + alpha < pi: phi < pi/2 and rb <= 0.7 |v|).  false whenever nothing can be said: the apex inside the sphere or near it,
// an unbounded or empty box (the culling boxes' pad may be "everything"), a cone that is not culled (cos_m == 0).
VR_CULL_FN bool cone_misses_box(const float* __restrict__ box, const float pos[3], const float axis[3], float cos_m, float sin_m)
{
    if (!(cos_m > 0.0f)) return false;
    const float cx = 0.5f * (box[0] + box[3]), cy = 0.5f * (box[1] + box[4]), cz = 0.5f * (box[2] + box[5]);
    const float hx = 0.5f * (box[3] - box[0]), hy = 0.5f * (box[4] - box[1]), hz = 0.5f * (box[5] - box[2]);
    const float vx = cx - pos[0], vy = cy - pos[1], vz = cz - pos[2];
    // c, the half extents and v are each rounded once: the exact box lies in the sphere about the COMPUTED v whose radius is the
    // half diagonal plus 2^-24 (|c|_1 + |v|_1 + |h|_1), and the square root and the sums below add a few 2^-24 relative
    const float m = ((fabsf(cx) + fabsf(cy)) + fabsf(cz)) + ((fabsf(vx) + fabsf(vy)) + fabsf(vz));
    const float rb = sqrtf((hx * hx + hy * hy) + hz * hz) * 1.000001f + m * 2.5e-7f;
    if (!(rb < 1.0e18f)) return false;                    // unbounded, empty (lo > hi: |h| is huge) or not finite
    const float d2 = (vx * vx + vy * vy) + vz * vz;
    const float d = sqrtf(d2);
    if (!(rb <= kConeMaxSin * d)) return false;           // (also: the apex inside the sphere)
    const float t = (vx * axis[0] + vy * axis[1]) + vz * axis[2];
    const float lim = (cos_m * sqrtf(d2 - rb * rb) - sin_m * rb) - kConeCosMargin * d;
    return t <= lim;
}
