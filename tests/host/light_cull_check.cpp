// Host check of the tiled lighting pass's cone test (vrenderer_amd/csrc/vr_light_cull.h: cone_misses_box, with the terms
// cone_cull_terms gives the device).  The header compiles without HIP; the test uses +, -, *, / and sqrt only, so what runs here
// is what the culling kernel runs.
//
// Over a fixed-seed set of (cone, box) pairs the box is sampled - its 8 corners, 12 edge midpoints, 6 face midpoints and a 9^3
// lattice - and each sample's angle to the cone's axis is evaluated in double precision:
//   1. the fp32 test never drops a cone for which some sample has an angle below outer_angle (one failure per such pair);
//   2. it is not vacuous: of the pairs whose every sample is more than 5 degrees outside the cone it drops at least half.
// The pairs: boxes anywhere around the apex, boxes that contain the apex, boxes on the axis, boxes whose nearest corner or whose
// bounding sphere touches the cone's surface from either side, far and near boxes at coordinates up to 2048, and the culling
// stage's two special boxes (unbounded, empty).  outer_angle runs from 0.5 to 89 degrees.
//
// Prints "<pairs> pairs, <clear> clear of the cone by 5 degrees, <dropped> of them dropped, <n> failures".
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "vr_light_cull.h"

namespace {

const double kPi = 3.14159265358979323846;

struct Rng {
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed) {}
    uint64_t next() { s += 0x9e3779b97f4a7c15ull; uint64_t z = s; z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull; return z ^ (z >> 31); }
    double uni() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }               // [0, 1)
    double range(double lo, double hi) { return lo + (hi - lo) * uni(); }
    void unit(double v[3])
    {
        for (;;) {
            v[0] = range(-1, 1); v[1] = range(-1, 1); v[2] = range(-1, 1);
            const double n = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
            if (n > 0.05 && n <= 1.0) { v[0] /= n; v[1] /= n; v[2] /= n; return; }
        }
    }
};

struct Pair { float box[6]; float pos[3]; float axis[3]; float outer; };

// angle between (q - pos) and the axis, in double; a sample at the apex is inside every cone
double angle_to_axis(const double q[3], const Pair& p)
{
    const double v[3] = { q[0] - (double)p.pos[0], q[1] - (double)p.pos[1], q[2] - (double)p.pos[2] };
    const double a[3] = { p.axis[0], p.axis[1], p.axis[2] };
    const double c[3] = { v[1] * a[2] - v[2] * a[1], v[2] * a[0] - v[0] * a[2], v[0] * a[1] - v[1] * a[0] };
    const double cross = sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]), dot = v[0] * a[0] + v[1] * a[1] + v[2] * a[2];
    if (cross == 0.0 && dot == 0.0) return 0.0;
    return atan2(cross, dot);
}

// the smallest angle over the samples: every (i, j, k) of the 9^3 lattice, which holds the corners (0 / 8), the edge and face
// midpoints (4) and the centre
double min_sample_angle(const Pair& p)
{
    double best = 10.0;
    for (int i = 0; i <= 8; i++)
        for (int j = 0; j <= 8; j++)
            for (int k = 0; k <= 8; k++) {
                const double q[3] = { (double)p.box[0] + ((double)p.box[3] - (double)p.box[0]) * (i / 8.0),
                                      (double)p.box[1] + ((double)p.box[4] - (double)p.box[1]) * (j / 8.0),
                                      (double)p.box[2] + ((double)p.box[5] - (double)p.box[2]) * (k / 8.0) };
                const double ang = angle_to_axis(q, p);
                if (ang < best) best = ang;
            }
    return best;
}

void set_axis(Pair& p, const double d[3])
{
    // as a host hands it over: normalised in fp32 (vr_light::direction)
    const float x = (float)d[0], y = (float)d[1], z = (float)d[2];
    const float n = sqrtf((x * x + y * y) + z * z);
    p.axis[0] = x / n; p.axis[1] = y / n; p.axis[2] = z / n;
}

void set_box(Pair& p, const double c[3], const double h[3])
{
    for (int k = 0; k < 3; k++) { p.box[k] = (float)(c[k] - h[k]); p.box[3 + k] = (float)(c[k] + h[k]); }
}

// a direction at `angle` from the axis, at a random azimuth
void off_axis(Rng& r, const Pair& p, double angle, double out[3])
{
    double t[3];
    const double a[3] = { p.axis[0], p.axis[1], p.axis[2] };
    for (;;) {
        r.unit(t);
        const double d = t[0] * a[0] + t[1] * a[1] + t[2] * a[2];
        for (int k = 0; k < 3; k++) t[k] -= d * a[k];
        const double n = sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
        if (n > 0.1) { for (int k = 0; k < 3; k++) t[k] /= n; break; }
    }
    for (int k = 0; k < 3; k++) out[k] = cos(angle) * a[k] + sin(angle) * t[k];
}

Pair make_pair(Rng& r, int kind)
{
    Pair p;
    const double span = (kind & 8) ? 2048.0 : 300.0;                  // coordinates up to 2048
    double apex[3], ax[3];
    for (int k = 0; k < 3; k++) apex[k] = r.range(-span, span);
    if (r.uni() < 0.05) for (int k = 0; k < 3; k++) apex[k] = r.uni() < 0.5 ? span : -span;
    for (int k = 0; k < 3; k++) p.pos[k] = (float)apex[k];
    r.unit(ax);
    if (r.uni() < 0.1) { ax[0] = 0.0; ax[1] = -1.0; ax[2] = 0.0; }    // straight down
    set_axis(p, ax);
    const double u = r.uni();
    const double outer_deg = u < 0.1 ? 0.5 : u < 0.2 ? 89.0 : r.range(0.5, 89.0);
    p.outer = (float)(outer_deg * kPi / 180.0);
    const double outer = (double)p.outer;
    double c[3], h[3], dir[3];
    for (int k = 0; k < 3; k++) h[k] = r.uni() < 0.3 ? r.range(0.01, 2.0) : r.range(0.1, 40.0);
    const double hd = sqrt(h[0] * h[0] + h[1] * h[1] + h[2] * h[2]);
    switch (kind & 7) {
    case 0: case 1: {                                                // anywhere around the apex
        r.unit(dir);
        const double d = r.uni() < 0.5 ? r.range(0.5, 60.0) : r.range(10.0, 1500.0);
        for (int k = 0; k < 3; k++) c[k] = apex[k] + dir[k] * d;
        break; }
    case 2:                                                          // the box contains the apex
        for (int k = 0; k < 3; k++) c[k] = apex[k] + r.range(-1.0, 1.0) * h[k];
        break;
    case 3: {                                                        // on the axis, in front of and behind the apex
        const double d = r.range(-400.0, 400.0);
        for (int k = 0; k < 3; k++) c[k] = apex[k] + (double)p.axis[k] * d;
        break; }
    case 4: {                                                        // the nearest corner touches the cone's surface
        const double d = r.range(2.0, 800.0), eps = r.range(-1.0e-4, 1.0e-4);
        double q[3];
        off_axis(r, p, outer + eps, dir);
        for (int k = 0; k < 3; k++) q[k] = apex[k] + dir[k] * d;      // a point on the surface (within eps): a corner of the box
        for (int k = 0; k < 3; k++) c[k] = q[k] + (r.uni() < 0.5 ? h[k] : -h[k]);
        break; }
    case 5: {                                                        // the bounding sphere touches the surface from outside
        const double d = hd * r.range(1.5, 60.0), alpha = asin(hd / d);
        const double ang = outer + alpha * r.range(0.98, 1.02) + r.range(-1.0e-5, 1.0e-5);
        off_axis(r, p, ang < kPi ? ang : kPi, dir);
        for (int k = 0; k < 3; k++) c[k] = apex[k] + dir[k] * d;
        break; }
    case 6: {                                                        // well outside the cone, small against its distance
        const double d = hd * r.range(2.0, 80.0);
        const double ang = outer + r.range(6.0, 90.0) * kPi / 180.0 + asin(hd / d);
        off_axis(r, p, ang < kPi ? ang : kPi, dir);
        for (int k = 0; k < 3; k++) c[k] = apex[k] + dir[k] * d;
        break; }
    default: {                                                       // a frustum cell's shape: long and thin, far away
        h[0] = r.range(0.05, 3.0); h[1] = r.range(0.05, 3.0); h[2] = r.range(0.05, 30.0);
        r.unit(dir);
        const double d = r.range(20.0, 2500.0);
        for (int k = 0; k < 3; k++) c[k] = apex[k] + dir[k] * d;
        break; }
    }
    set_box(p, c, h);
    return p;
}

bool dropped(const Pair& p)
{
    float cm, sm;
    cone_cull_terms(p.axis, p.outer, &cm, &sm);
    return cone_misses_box(p.box, p.pos, p.axis, cm, sm);
}

}  // namespace

int main()
{
    Rng r(0x5eed2026ull);
    const int kPairs = 120000;
    long failures = 0, clear = 0, clear_dropped = 0, drops = 0, apex_inside = 0, on_surface = 0;
    const double five = 5.0 * kPi / 180.0;
    for (int n = 0; n < kPairs; n++) {
        const Pair p = make_pair(r, n & 15);
        const bool drop = dropped(p);
        const double a = min_sample_angle(p);
        drops += drop;
        if ((n & 7) == 2) apex_inside++;
        if (fabs(a - (double)p.outer) < 1.0e-3) on_surface++;
        if (drop && a < (double)p.outer) {
            if (failures++ < 10)
                printf("FAIL pair %d: dropped, but a sample is at %.9g rad from the axis, outer_angle %.9g (box %g %g %g .. %g %g %g, apex %g %g %g)\n", n, a,
                       (double)p.outer, p.box[0], p.box[1], p.box[2], p.box[3], p.box[4], p.box[5], p.pos[0], p.pos[1], p.pos[2]);
        }
        if (a > (double)p.outer + five) { clear++; clear_dropped += drop; }
    }
    // the culling stage's special boxes, and cones that are not culled at all
    {
        Pair p = make_pair(r, 6);
        const float big = 3.0e38f;
        const float all[6] = { -big, -big, -big, big, big, big }, none[6] = { big, big, big, -big, -big, -big };
        float cm, sm;
        cone_cull_terms(p.axis, p.outer, &cm, &sm);
        if (cone_misses_box(all, p.pos, p.axis, cm, sm)) { failures++; printf("FAIL: the unbounded box was dropped\n"); }
        if (cone_misses_box(none, p.pos, p.axis, cm, sm)) { failures++; printf("FAIL: the empty box gave a verdict\n"); }
        if (!dropped(p)) { failures++; printf("FAIL: a box far outside the cone was kept\n"); }
        cone_cull_terms(p.axis, 1.5707964f, &cm, &sm);
        if (cm != 0.0f || cone_misses_box(p.box, p.pos, p.axis, cm, sm)) { failures++; printf("FAIL: a cone of pi/2 was culled\n"); }
        const float twice[3] = { 2.0f * p.axis[0], 2.0f * p.axis[1], 2.0f * p.axis[2] };
        cone_cull_terms(twice, p.outer, &cm, &sm);
        if (cm != 0.0f) { failures++; printf("FAIL: an axis of length 2 was accepted\n"); }
        const float nan_box[6] = { NAN, 0, 0, 1, 1, 1 };
        cone_cull_terms(p.axis, p.outer, &cm, &sm);
        if (cone_misses_box(nan_box, p.pos, p.axis, cm, sm)) { failures++; printf("FAIL: a NaN box was dropped\n"); }
    }
    if (clear < kPairs / 10) { failures++; printf("FAIL: only %ld pairs are clear of the cone by 5 degrees\n", clear); }
    if (2 * clear_dropped < clear) { failures++; printf("FAIL: vacuous: %ld of %ld clear pairs dropped\n", clear_dropped, clear); }
    if (on_surface < 1000 || apex_inside < 1000) { failures++; printf("FAIL: the set misses its edge cases (%ld on the surface, %ld with the apex inside)\n", on_surface, apex_inside); }
    printf("%d pairs (%ld dropped, %ld within 1e-3 rad of the surface), %ld clear of the cone by 5 degrees, %ld of them dropped, %ld failures\n",
           kPairs, drops, on_surface, clear, clear_dropped, failures);
    return failures ? 1 : 0;
}
