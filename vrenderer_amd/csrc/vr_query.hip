// Terrain queries: batched height samples and ray casts against the surface the vertex stage draws
// (grown from QuadTree::GetHeightValue, QuadTree.h:84, QuadTree.cpp:153-162 - one nearest-texel lookup on the CPU).
//
//   H(x, z) = SampleLevel(heightmap, linear-clamp, uv, 0.1).r * max_height,  uv = ((x, z) + world_size / 2) / world_size
//
// k_query_heights   : one point per lane; H with exactly k_vertex's statements (vr_raster.hip, sampleHeight) through the
//                     shared quad_tap / quad_filter of vr_tex_dev.h, so a height is bit for bit the drawn vertex's.
// the bound pyramid : a min / max pyramid over H / max_height, built by vr_derive.hip (vr_derive_pyramid).  Level 0 has one cell
//                     per level-0 bilinear footprint (texel-centre interval, plus the clamp border: (w + 1) x (h + 1) cells,
//                     indexed like the quad table); a cell keeps a uint8 pair (lo, hi) with lo / 255 <= H / max_height <= hi / 255
//                     on the cell; each higher level is the min / max of 2 x 2 children, ragged edges included.
// k_query_rays      : one ray per lane.  Slab clip to the box, then a hierarchical DDA over the pyramid from the coarsest
//                     level: a cell whose bound lies below the ray's segment is stepped over, any other is entered one level
//                     down; crossing a cell boundary that is also the parent's goes one level up again, so no stack is
//                     needed and the state (two level-0 cell indices, the level, the parameter) stays in registers.  At
//                     level 0 H along the ray is a quadratic on each of the at most three pieces the level-1 footprint
//                     boundaries cut the segment into (the ray crosses at most one per axis inside a cell); its smallest
//                     root is refined against the sampler itself, and the reported point's height is the sampler's value.
#include "vr_internal.h"
#include "vr_tex_dev.h"
#include "vr_dirty.h"
#include "vr_experiments.h"

#include <math.h>
#include <string.h>

constexpr float kInf = __builtin_huge_valf();
// The walk starts at the pyramid's top; the experiment build of tools/exp_queries.py pins it to level 0 (a plain DDA over
// the finest cells) to show what the pyramid buys.
constexpr bool kWalkPinnedToLevel0 = kExpQueryLevel0;

struct QueryArgs {
    float world_size, max_height;
    int step_cap;                           // hard cap of the walk's iterations, computed on the host
    int pad;
};

// ---------------------------------------------------------------------------------------
// the surface
// ---------------------------------------------------------------------------------------
struct HeightSample {
    float hv;                               // H / max_height, k_vertex's value
    float du, dv;                           // d(hv) / du, d(hv) / dv (analytic, of the two bilinear interpolants)
};

__device__ __forceinline__ void quad_gradient(uint32_t e, const QuadTap& q, const float* __restrict__ r8, float& gx, float& gy)
{
    const float t00 = r8[e & 255u], t10 = r8[(e >> 8) & 255u], t01 = r8[(e >> 16) & 255u], t11 = r8[e >> 24];
    const float dx0 = t10 - t00, dx1 = t11 - t01, dy0 = t01 - t00, dy1 = t11 - t10;
    gx = __builtin_fmaf(dx1 - dx0, q.fy, dx0);
    gy = __builtin_fmaf(dy1 - dy0, q.fx, dy0);
}

template <bool kGradient>
__device__ __forceinline__ HeightSample sample_height(const DevTex& hm, const uint32_t* __restrict__ s_qoff, const float* __restrict__ r8,
                                                      float world_size, float x, float z)
{
    HeightSample o; o.du = 0.0f; o.dv = 0.0f;
    // sampleHeight (terrain_vs.hlsl:27-33) as k_vertex evaluates it
    const float halfSize = world_size * 0.5f;
    const float u = (x + halfSize) / world_size, w_ = (z + halfSize) / world_size;
    const LodSplit ls = vr_lod_split(hm.levels, 0.1f);
    const int l1 = min(ls.l0 + 1, hm.levels - 1);
    const int w0 = max(1, hm.w0 >> ls.l0), h0 = max(1, hm.h0 >> ls.l0), w1 = max(1, hm.w0 >> l1), h1 = max(1, hm.h0 >> l1);
    const QuadTap t0 = quad_tap(w0, h0, u, w_), t1 = quad_tap(w1, h1, u, w_);
    const uint32_t e0 = hm.quad[s_qoff[ls.l0] + t0.idx], e1 = hm.quad[s_qoff[l1] + t1.idx];
    const float s0 = quad_filter(e0, t0, r8), s1 = quad_filter(e1, t1, r8);
    o.hv = ls.f > 0.0f ? __builtin_fmaf(s1 - s0, ls.f, s0) : s0;
    if (kGradient) {
        float g0x, g0y, g1x, g1y;
        quad_gradient(e0, t0, r8, g0x, g0y);
        quad_gradient(e1, t1, r8, g1x, g1y);
        g0x *= (float)w0; g0y *= (float)h0; g1x *= (float)w1; g1y *= (float)h1;     // per texel -> per unit of uv
        o.du = __builtin_fmaf(g1x - g0x, ls.f, g0x);
        o.dv = __builtin_fmaf(g1y - g0y, ls.f, g0y);
    }
    return o;
}

// normalize(-dH/dx, 1, -dH/dz)
__device__ __forceinline__ void surface_normal(const HeightSample& s, float max_height, float world_size, float& nx, float& ny, float& nz)
{
    const float k = max_height / world_size;
    const float gx = s.du * k, gz = s.dv * k;
    const float inv = 1.0f / sqrtf((gx * gx + 1.0f) + gz * gz);
    nx = -gx * inv; ny = inv; nz = -gz * inv;
}

__global__ __launch_bounds__(256) void k_query_heights(DevTex hm, QueryArgs a, const float2* __restrict__ xz, uint32_t n,
                                                        float* __restrict__ out_height, float* __restrict__ out_normal)
{
    __shared__ float r8[256];
    __shared__ uint32_t s_qoff[kMaxLevels];
    r8[threadIdx.x] = (float)threadIdx.x / 255.0f;     // UNORM8 -> float, correctly rounded
    if (threadIdx.x < kMaxLevels) s_qoff[threadIdx.x] = hm.qoff[threadIdx.x];
    __syncthreads();
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const float2 p = xz[i];
        if (out_normal) {
            const HeightSample s = sample_height<true>(hm, s_qoff, r8, a.world_size, p.x, p.y);
            out_height[i] = s.hv * a.max_height;
            float nx, ny, nz;
            surface_normal(s, a.max_height, a.world_size, nx, ny, nz);
            float* o = out_normal + (size_t)i * 3;
            o[0] = nx; o[1] = ny; o[2] = nz;
        } else {
            const HeightSample s = sample_height<false>(hm, s_qoff, r8, a.world_size, p.x, p.y);
            out_height[i] = s.hv * a.max_height;
        }
    }
}

// ---------------------------------------------------------------------------------------
// ray casts
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ bool vr_finite(float x) { return fabsf(x) <= 3.402823466e38f; }     // false for NaN and infinities

struct Bilinear { float a, bx, bz, c; };     // a + bx fx + bz fz + c fx fz
__device__ __forceinline__ Bilinear bilinear_of(uint32_t e, const float* __restrict__ r8)
{
    const float t00 = r8[e & 255u], t10 = r8[(e >> 8) & 255u], t01 = r8[(e >> 16) & 255u], t11 = r8[e >> 24];
    Bilinear b; b.a = t00; b.bx = t10 - t00; b.bz = t01 - t00; b.c = (t11 - t01) - (t10 - t00);
    return b;
}

// smallest root in [0, len] of qa s^2 + qb s + qc with qc > 0; kInf when there is none
__device__ __forceinline__ float first_root(float qa, float qb, float qc, float len)
{
    float r = kInf;
    if (qa == 0.0f) {
        if (qb < 0.0f) r = -qc / qb;
    } else {
        const float disc = __builtin_fmaf(qb, qb, -4.0f * qa * qc);
        if (disc >= 0.0f) {
            const float sq = sqrtf(disc);
            const float q = -0.5f * (qb + (qb >= 0.0f ? sq : -sq));
            const float r1 = q / qa, r2 = q != 0.0f ? qc / q : kInf;
            if (r1 >= 0.0f && r1 < r) r = r1;
            if (r2 >= 0.0f && r2 < r) r = r2;
        }
    }
    return r <= len ? r : kInf;
}

__global__ __launch_bounds__(256) void k_query_rays(DevTex hm, QueryArgs a, PyrDesc pd, const uchar2* __restrict__ pyr,
                                                     const float4* __restrict__ rays, uint32_t n, float4* __restrict__ hits)
{
    __shared__ float r8[256];
    __shared__ uint32_t s_qoff[kMaxLevels];
    r8[threadIdx.x] = (float)threadIdx.x / 255.0f;
    if (threadIdx.x < kMaxLevels) s_qoff[threadIdx.x] = hm.qoff[threadIdx.x];
    __syncthreads();
    const int w0 = hm.w0, h0 = hm.h0;
    const int l1 = min(1, hm.levels - 1);
    const int w1 = max(1, w0 >> l1), h1 = max(1, h0 >> l1);
    const uint32_t q0 = s_qoff[0], q1 = s_qoff[l1];
    const float mh = a.max_height, ws = a.world_size, half = ws * 0.5f;
    const float kx = (float)w0 / ws, kz = (float)h0 / ws;                 // level-0 cells per world unit
    const float rx = (float)w1 / (float)w0, rz = (float)h1 / (float)h0;   // level-1 cells per level-0 cell
    const float ylo = vr_min(0.0f, mh), yhi = vr_max(0.0f, mh);
    const float lodf = vr_lod_split(hm.levels, 0.1f).f;                   // the sampler's weight of level 1
    const int top = kWalkPinnedToLevel0 ? 0 : pd.levels - 1;
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const float4 ra = rays[2 * (size_t)i], rb = rays[2 * (size_t)i + 1];
        const float ox = ra.x, oy = ra.y, oz = ra.z, tmax = ra.w, dx = rb.x, dy = rb.y, dz = rb.z;
        uint32_t status = VR_RAY_MISS;
        float t_hit = 0.0f;
        bool polish = false;
        const float dm = vr_max(fabsf(dx), vr_max(fabsf(dy), fabsf(dz)));
        if (!(vr_finite(ox) && vr_finite(oy) && vr_finite(oz) && vr_finite(dx) && vr_finite(dy) && vr_finite(dz) && dm > 0.0f && tmax >= 0.0f)) {
            status = VR_RAY_INVALID;
        } else {
            // the walk runs on the direction scaled to a largest component of 1 (T = t * dm): no product of it can overflow
            const float nx = dx / dm, ny = dy / dm, nz = dz / dm;
            float T0 = 0.0f, T1 = tmax * dm;
            bool inside = true, floor_exit = false;
            // 1. slab clip; a zero component is "inside the slab or not" and is never divided by
            if (nx != 0.0f) { const float inv = 1.0f / nx, p = (-half - ox) * inv, q = (half - ox) * inv; T0 = vr_max(T0, vr_min(p, q)); T1 = vr_min(T1, vr_max(p, q)); }
            else if (ox < -half || ox > half) inside = false;
            if (nz != 0.0f) { const float inv = 1.0f / nz, p = (-half - oz) * inv, q = (half - oz) * inv; T0 = vr_max(T0, vr_min(p, q)); T1 = vr_min(T1, vr_max(p, q)); }
            else if (oz < -half || oz > half) inside = false;
            if (ny != 0.0f) {
                const float inv = 1.0f / ny, p = (ylo - oy) * inv, q = (yhi - oy) * inv;
                T0 = vr_max(T0, vr_min(p, q));
                // a ray that leaves the box through its floor has crossed the surface (H >= the floor everywhere)
                if (ny < 0.0f && p <= T1) floor_exit = true;
                T1 = vr_min(T1, vr_max(p, q));
            } else if (oy < ylo || oy > yhi) inside = false;
            if (inside && T0 <= T1) {
                // re-based at the entry point: positions in level-0 cell coordinates (cell ix covers [ix, ix + 1), the quad
                // table's indexing: texel-centre coordinate + 1), parameter s = T - T0 in [0, S1]
                const float S1 = T1 - T0;
                const float bx = __builtin_fmaf(T0, nx, ox), by = __builtin_fmaf(T0, ny, oy), bz = __builtin_fmaf(T0, nz, oz);
                const float cxb = __builtin_fmaf(bx + half, kx, 0.5f), czb = __builtin_fmaf(bz + half, kz, 0.5f);
                const float dcx = nx * kx, dcz = nz * kz;
                float invx = dcx != 0.0f ? 1.0f / dcx : 0.0f, invz = dcz != 0.0f ? 1.0f / dcz : 0.0f;
                const bool hasx = dcx != 0.0f && vr_finite(invx), hasz = dcz != 0.0f && vr_finite(invz);
                int ix = vr_clampi((int)floorf(vr_clampf(cxb, 0.0f, (float)w0)), 0, w0), iz = vr_clampi((int)floorf(vr_clampf(czb, 0.0f, (float)h0)), 0, h0);
                if (!(cxb == cxb)) ix = 0;
                if (!(czb == czb)) iz = 0;
                const float slack_mh = fabsf(mh) * (1.0f / 16384.0f);
                int L = top;
                float s = 0.0f;
                bool done = false;
                int it = 0;
                for (; it < a.step_cap && !done; it++) {
                    const int cellx = ix >> L, cellz = iz >> L;
                    float sbx = kInf, sbz = kInf;
                    if (hasx) { sbx = ((float)((dcx > 0.0f ? cellx + 1 : cellx) << L) - cxb) * invx; if (!(sbx >= s)) sbx = s; }
                    if (hasz) { sbz = ((float)((dcz > 0.0f ? cellz + 1 : cellz) << L) - czb) * invz; if (!(sbz >= s)) sbz = s; }
                    const float se = vr_min(vr_min(sbx, sbz), S1);
                    const int wl = (pd.cw + (1 << L) - 1) >> L;
                    const uchar2 mm = pyr[pd.off[L] + (uint32_t)cellz * (uint32_t)wl + (uint32_t)cellx];
                    const float ya = __builtin_fmaf(s, ny, by), yb = __builtin_fmaf(se, ny, by);
                    const float smax = vr_max(r8[mm.x] * mh, r8[mm.y] * mh);
                    const float slack = slack_mh + 1.0e-6f * (fabsf(ya) + fabsf(yb));
                    bool advance = vr_min(ya, yb) > smax + slack;          // 2. the segment lies wholly above the cell's bound: step over
                    if (!advance && L > 0) { L--; continue; }              //    otherwise descend
                    if (!advance) {
                        // level 0: H along the ray is a quadratic on each piece between the level-1 footprint boundaries
                        const Bilinear b0 = bilinear_of(hm.quad[q0 + (uint32_t)iz * (uint32_t)(w0 + 2) + (uint32_t)ix], r8);
                        const float c1xs = __builtin_fmaf(__builtin_fmaf(s, dcx, cxb) - 0.5f, rx, 0.5f), c1zs = __builtin_fmaf(__builtin_fmaf(s, dcz, czb) - 0.5f, rz, 0.5f);
                        const float d1x = dcx * rx, d1z = dcz * rz;
                        const float c1xe = __builtin_fmaf(se - s, d1x, c1xs), c1ze = __builtin_fmaf(se - s, d1z, c1zs);
                        float cut0 = se, cut1 = se;
                        { const float fa = floorf(c1xs), fe = floorf(c1xe);
                          if (fa != fe && d1x != 0.0f) { const float c = s + (vr_max(fa, fe) - c1xs) / d1x; cut0 = vr_clampf(c == c ? c : se, s, se); } }
                        { const float fa = floorf(c1zs), fe = floorf(c1ze);
                          if (fa != fe && d1z != 0.0f) { const float c = s + (vr_max(fa, fe) - c1zs) / d1z; cut1 = vr_clampf(c == c ? c : se, s, se); } }
                        if (cut1 < cut0) { const float tmp = cut0; cut0 = cut1; cut1 = tmp; }
                        float pa = s;
                        advance = true;
#pragma unroll 1
                        for (int piece = 0; piece < 3; piece++) {
                            const float pb = piece == 0 ? cut0 : (piece == 1 ? cut1 : se);
                            if (piece > 0 && !(pb > pa)) continue;                  // an empty piece (the first is evaluated even when it is a point)
                            const float mid = 0.5f * (pa + pb);
                            const int jx = vr_clampi((int)floorf(vr_clampf(__builtin_fmaf(mid - s, d1x, c1xs), 0.0f, (float)w1)), 0, w1);
                            const int jz = vr_clampi((int)floorf(vr_clampf(__builtin_fmaf(mid - s, d1z, c1zs), 0.0f, (float)h1)), 0, h1);
                            const Bilinear b1 = bilinear_of(hm.quad[q1 + (uint32_t)jz * (uint32_t)(w1 + 2) + (uint32_t)jx], r8);
                            const float fx = __builtin_fmaf(pa, dcx, cxb) - (float)ix, fz = __builtin_fmaf(pa, dcz, czb) - (float)iz;
                            const float gx = __builtin_fmaf(pa - s, d1x, c1xs) - (float)jx, gz = __builtin_fmaf(pa - s, d1z, c1zs) - (float)jz;
                            const float v0 = b0.a + b0.bx * fx + b0.bz * fz + b0.c * fx * fz, v1 = b1.a + b1.bx * gx + b1.bz * gz + b1.c * gx * gz;
                            const float m0 = b0.bx * dcx + b0.bz * dcz + b0.c * (fx * dcz + fz * dcx), m1 = b1.bx * d1x + b1.bz * d1z + b1.c * (gx * d1z + gz * d1x);
                            const float k0 = b0.c * dcx * dcz, k1 = b1.c * d1x * d1z;
                            const float hv = __builtin_fmaf(v1 - v0, lodf, v0), hm1 = __builtin_fmaf(m1 - m0, lodf, m0), hk = __builtin_fmaf(k1 - k0, lodf, k0);
                            const float qc = __builtin_fmaf(pa, ny, by) - mh * hv, qb = ny - mh * hm1, qa = -mh * hk;
                            if (qc <= 0.0f || !(qc == qc)) { status = VR_RAY_HIT; t_hit = T0 + pa; done = true; advance = false; break; }   // at or below the surface already
                            const float r = first_root(qa, qb, qc, pb - pa);
                            if (r < kInf) { status = VR_RAY_HIT; t_hit = T0 + (pa + r); polish = true; done = true; advance = false; break; }
                            pa = pb;
                        }
                    }
                    if (advance) {
                        if (!(se < S1)) { done = true; break; }            // the end of the clipped segment
                        s = se;
                        bool up;
                        if (sbx <= sbz) {
                            const int nc = dcx > 0.0f ? cellx + 1 : cellx - 1;
                            up = dcx > 0.0f ? !(nc & 1) : (nc & 1);
                            ix = dcx > 0.0f ? (nc << L) : (cellx << L) - 1;
                            if (ix < 0 || ix > w0) { done = true; break; }
                            if (L > 0) {
                                const float cz = vr_clampf(__builtin_fmaf(s, dcz, czb), 0.0f, (float)h0);
                                iz = vr_clampi(cz == cz ? (int)floorf(cz) : iz, cellz << L, min(((cellz + 1) << L) - 1, h0));
                            }
                        } else {
                            const int nc = dcz > 0.0f ? cellz + 1 : cellz - 1;
                            up = dcz > 0.0f ? !(nc & 1) : (nc & 1);
                            iz = dcz > 0.0f ? (nc << L) : (cellz << L) - 1;
                            if (iz < 0 || iz > h0) { done = true; break; }
                            if (L > 0) {
                                const float cx = vr_clampf(__builtin_fmaf(s, dcx, cxb), 0.0f, (float)w0);
                                ix = vr_clampi(cx == cx ? (int)floorf(cx) : ix, cellx << L, min(((cellx + 1) << L) - 1, w0));
                            }
                        }
                        if (up && L < top) L++;                            //    level-up on crossing the parent's boundary
                    }
                }
                if (!done) status = VR_RAY_STEP_LIMIT;                     // 3. the cap: no ray, whatever its bits, may spin
                else if (status == VR_RAY_MISS && floor_exit) { status = VR_RAY_HIT; t_hit = T1; }
            }
        }
        float4 o0 = make_float4(tmax, 0.0f, 0.0f, 0.0f), o1 = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(status));
        if (status == VR_RAY_HIT) {
            float t = vr_min(vr_max(t_hit / dm, 0.0f), tmax);
            HeightSample hs = sample_height<true>(hm, s_qoff, r8, ws, __builtin_fmaf(t, dx, ox), __builtin_fmaf(t, dz, oz));
            if (polish) {
                // Newton on g(t) = origin.y + t dir.y - H(origin.xz + t dir.xz) with the sampler's own values: two steps at most, the best kept
                float g = __builtin_fmaf(t, dy, oy) - hs.hv * mh;
#pragma unroll 1
                for (int k = 0; k < 2; k++) {
                    const float gp = dy - (mh / ws) * (hs.du * dx + hs.dv * dz);
                    if (g == 0.0f || !(fabsf(gp) > 0.0f)) break;
                    const float tn = vr_min(vr_max(t - g / gp, 0.0f), tmax);
                    if (!(tn == tn) || tn == t) break;
                    const HeightSample hn = sample_height<true>(hm, s_qoff, r8, ws, __builtin_fmaf(tn, dx, ox), __builtin_fmaf(tn, dz, oz));
                    const float gn = __builtin_fmaf(tn, dy, oy) - hn.hv * mh;
                    if (!(fabsf(gn) < fabsf(g))) break;
                    t = tn; g = gn; hs = hn;
                }
            }
            float nx, ny, nz;
            surface_normal(hs, mh, ws, nx, ny, nz);
            o0 = make_float4(t, __builtin_fmaf(t, dx, ox), hs.hv * mh, __builtin_fmaf(t, dz, oz));
            o1 = make_float4(nx, ny, nz, __uint_as_float(status));
        }
        hits[2 * (size_t)i] = o0;                                         // 4. written for every ray
        hits[2 * (size_t)i + 1] = o1;
    }
}

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------

static int grid_for(uint32_t n)
{
    const uint32_t blocks = (n + 255u) / 256u;
    return (int)(blocks < 16384u ? (blocks ? blocks : 1u) : 16384u);          // grid-stride beyond 4M elements
}

// staging of the host-pointer mode: kept with the terrain, grown by doubling
int vr_query_reserve_stage(vr_terrain* t, size_t bytes)
{
    // (its users leave it idle when they return: only what the caller has queued since can still be running)
    return vr_reserve(&t->d_query_stage, &t->query_stage_bytes, bytes, [t]() -> int { VR_HIP(hipStreamSynchronize(t->ctx->stream)); return VR_OK; });
}

void vr_query_release(vr_terrain* t)
{
    (void)hipFree(t->d_query_stage); t->d_query_stage = nullptr; t->query_stage_bytes = 0;
    (void)hipFree(t->d_pyramid); t->d_pyramid = nullptr; t->pyramid_bytes = 0;
    if (t->ord_pyramid.ev) (void)hipEventDestroy(t->ord_pyramid.ev);
    t->ord_pyramid = VrOrderSide();
}

PyrDesc vr_pyramid_desc(const vr_terrain* t, size_t* cells)
{
    PyrDesc pd; memset(&pd, 0, sizeof(pd));
    pd.cw = t->height.w0 + 1; pd.ch = t->height.h0 + 1;
    size_t off = 0;
    int w = pd.cw, h = pd.ch, l = 0;
    for (;; l++) {
        pd.off[l] = (uint32_t)off;
        off += (size_t)w * h;
        if ((w == 1 && h == 1) || l == kPyrMaxLevels - 1) break;
        w = (w + 1) / 2; h = (h + 1) / 2;
    }
    pd.levels = l + 1;
    if (cells) *cells = off;
    return pd;
}

// built lazily by the first ray cast of a terrain, on the context's stream; kept until vr_terrain_destroy
static int ensure_pyramid(vr_terrain* t, PyrDesc* out)
{
    size_t cells = 0;
    *out = vr_pyramid_desc(t, &cells);
    hipStream_t s = t->ctx->stream;
    if (t->d_pyramid) return order_side_begin(t->ord_pyramid, VrOrderOps(), s);
    VR_REQUIRE(((t->height.w0 + 1) >> (kPyrMaxLevels - 1)) <= 1 && ((t->height.h0 + 1) >> (kPyrMaxLevels - 1)) <= 1, "heightmap too large for the query pyramid");
    uchar2* p = nullptr;
    hipEvent_t ev = nullptr;
    {
        const hipError_t e = hipMalloc((void**)&p, cells * sizeof(uchar2));
        if (e != hipSuccess) { (void)hipGetLastError(); vr_set_error("terrain query: %zu bytes for the bound pyramid: %s", cells * sizeof(uchar2), hipGetErrorString(e)); return VR_ERR_OUT_OF_MEMORY; }
        if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) { (void)hipFree(p); vr_set_error("terrain query: hipEventCreate failed"); return VR_ERR_HIP; }
    }
    {
        VrKernelScope ks(t->ctx, VR_K_QUERY_PYRAMID, t->ctx->stream);
        const int w0 = t->height.w0, h0 = t->height.h0, lv1 = t->height.levels > 1 ? 1 : 0;
        vr_derive_pyramid(t->height, *out, p, dirty_whole(w0, h0), dirty_whole(dirty_level_size(w0, lv1), dirty_level_size(h0, lv1)), s);
    }
    const hipError_t le = hipGetLastError();
    VrOrderSide built; built.ev = ev;
    if (le != hipSuccess || order_side_end(built, VrOrderOps(), s) != VR_OK) {
        (void)hipStreamSynchronize(s); (void)hipFree(p); (void)hipEventDestroy(ev);
        vr_set_error("terrain query: building the bound pyramid: %s", hipGetErrorString(le));
        return VR_ERR_HIP;
    }
    t->d_pyramid = p; t->pyramid_bytes = cells * sizeof(uchar2); t->ord_pyramid = built;
    return VR_OK;
}

extern "C" VR_API int vr_terrain_query_heights(vr_terrain* t, const float* xz, uint32_t n, float max_height,
                                                float* out_height, float* out_normal, int device_pointers)
{
    // the argument checks come before any use of the device (and of the terrain)
    VR_REQUIRE(t != nullptr, "terrain is NULL");
    VR_REQUIRE(host_finite(max_height), "max_height is NaN or infinite");
    if (n == 0) return VR_OK;
    VR_REQUIRE(xz && out_height, "NULL array with n > 0");
    // the kernel loads a point as one float2 from the caller's device memory
    VR_REQUIRE(!device_pointers || (((uintptr_t)xz & 7u) == 0 && ((uintptr_t)out_height & 3u) == 0 && ((uintptr_t)out_normal & 3u) == 0),
               "device pointers: xz must be 8-byte aligned, the outputs 4-byte aligned");
    VR_HIP(hipSetDevice(t->ctx->device));
    hipStream_t s = t->ctx->stream;
    QueryArgs a; a.world_size = t->p.world_size; a.max_height = max_height; a.step_cap = 0; a.pad = 0;
    const float2* d_xz = (const float2*)xz; float* d_h = out_height; float* d_n = out_normal;
    const size_t b_xz = (size_t)n * 8, b_h = ((size_t)n * 4 + 15) / 16 * 16, b_n = (size_t)n * 12;
    if (!device_pointers) {
        const int rc = vr_query_reserve_stage(t, b_xz + b_h + (out_normal ? b_n : 0));
        if (rc) return rc;
        char* base = (char*)t->d_query_stage;
        d_xz = (const float2*)base; d_h = (float*)(base + b_xz); d_n = out_normal ? (float*)(base + b_xz + b_h) : nullptr;
        VR_HIP(hipMemcpyAsync(base, xz, b_xz, hipMemcpyHostToDevice, s));
    }
    {
        VrKernelScope ks(t->ctx, VR_K_QUERY_HEIGHTS, t->ctx->stream);
        hipLaunchKernelGGL(k_query_heights, dim3(grid_for(n)), dim3(256), 0, s, t->height, a, d_xz, n, d_h, d_n);
    }
    VR_HIP(hipGetLastError());
    if (!device_pointers) {
        VR_HIP(hipMemcpyAsync(out_height, d_h, (size_t)n * 4, hipMemcpyDeviceToHost, s));
        if (out_normal) VR_HIP(hipMemcpyAsync(out_normal, d_n, b_n, hipMemcpyDeviceToHost, s));
        VR_HIP(hipStreamSynchronize(s));
    }
    return VR_OK;
}

extern "C" VR_API int vr_terrain_cast_rays(vr_terrain* t, const vr_ray* rays, uint32_t n, float max_height,
                                            vr_ray_hit* hits, int device_pointers)
{
    static_assert(sizeof(vr_ray) == 32 && sizeof(vr_ray_hit) == 32, "vr_ray / vr_ray_hit layout");
    VR_REQUIRE(t != nullptr, "terrain is NULL");
    VR_REQUIRE(host_finite(max_height), "max_height is NaN or infinite");
    if (n == 0) return VR_OK;
    VR_REQUIRE(rays && hits, "NULL array with n > 0");
    // the kernel moves a ray and a hit as two float4 each
    VR_REQUIRE(!device_pointers || ((((uintptr_t)rays | (uintptr_t)hits) & 15u) == 0), "device pointers: rays and hits must be 16-byte aligned");
    VR_HIP(hipSetDevice(t->ctx->device));
    hipStream_t s = t->ctx->stream;
    const float4* d_rays = (const float4*)rays; float4* d_hits = (float4*)hits;
    const size_t b = (size_t)n * 32;
    if (!device_pointers) {
        const int rc = vr_query_reserve_stage(t, 2 * b);
        if (rc) return rc;
        d_rays = (const float4*)t->d_query_stage; d_hits = (float4*)((char*)t->d_query_stage + b);
    }
    PyrDesc pd;
    { const int rc = ensure_pyramid(t, &pd); if (rc) return rc; }
    QueryArgs a; a.world_size = t->p.world_size; a.max_height = max_height; a.pad = 0;
    a.step_cap = 4 * (t->height.w0 + t->height.h0) + 64 * pd.levels;
    if (!device_pointers) VR_HIP(hipMemcpyAsync((void*)d_rays, rays, b, hipMemcpyHostToDevice, s));
    {
        VrKernelScope ks(t->ctx, VR_K_QUERY_RAYS, t->ctx->stream);
        hipLaunchKernelGGL(k_query_rays, dim3(grid_for(n)), dim3(256), 0, s, t->height, a, pd, (const uchar2*)t->d_pyramid, d_rays, n, d_hits);
    }
    VR_HIP(hipGetLastError());
    if (!device_pointers) {
        VR_HIP(hipMemcpyAsync(hits, d_hits, b, hipMemcpyDeviceToHost, s));
        VR_HIP(hipStreamSynchronize(s));
    }
    return VR_OK;
}

// The pyramid as it is on the device: every level in order, cw * ch pairs (lo, hi) each, as PyrDesc lays them out.  The copy runs on
// the context's stream behind the pyramid's last writer, as a ray cast's kernel does (the refresh of an edit may have run on another
// stream), and the entry returns when it has completed, as a query's download does.  No kernel, and nothing is built: a terrain on
// which no ray was cast has no pyramid to show.
extern "C" VR_API int vr_debug_terrain_query_pyramid(vr_terrain* t, int32_t* out_levels, int32_t out_dims[2 * 16], uint8_t* out, size_t capacity_bytes)
{
    static_assert(kPyrMaxLevels == 16, "out_dims of the header");
    VR_REQUIRE(t != nullptr, "terrain is NULL");
    VR_REQUIRE(out_levels != nullptr && out_dims != nullptr, "out_levels or out_dims is NULL");
    size_t cells = 0;
    PyrDesc pd; memset(&pd, 0, sizeof(pd));
    if (t->d_pyramid) pd = vr_pyramid_desc(t, &cells);
    if (!(out == nullptr && capacity_bytes == 0)) {
        VR_REQUIRE(out != nullptr, "out is NULL with a capacity");
        VR_REQUIRE(capacity_bytes >= cells * sizeof(uchar2), "capacity below 2 bytes per cell of every level");
    }
    *out_levels = pd.levels;
    for (int l = 0, w = pd.cw, h = pd.ch; l < kPyrMaxLevels; l++, w = (w + 1) / 2, h = (h + 1) / 2) {
        out_dims[2 * l] = l < pd.levels ? w : 0; out_dims[2 * l + 1] = l < pd.levels ? h : 0;
    }
    if (out == nullptr || pd.levels == 0) return VR_OK;
    VR_HIP(hipSetDevice(t->ctx->device));
    hipStream_t s = t->ctx->stream;
    { const int rc = order_side_begin(t->ord_pyramid, VrOrderOps(), s); if (rc) return rc; }
    VR_HIP(hipMemcpyAsync(out, t->d_pyramid, cells * sizeof(uchar2), hipMemcpyDeviceToHost, s));
    VR_HIP(hipStreamSynchronize(s));
    return VR_OK;
}

// ---- vr_view_pixel_ray (host only) ---------------------------------------------------------------------
// The world point that world_to_clip sends to NDC (x, y, z): clip_j - ndc_j clip_w = 0 for j = x, y, z is a 3 x 3 linear system
// in the point.  It is solved in double against world_to_clip - the matrix a renderer projects with - because the fp32
// clip_to_world is ill-conditioned at the far plane (its w row cancels to 1 / z_far) and sends a far-plane pixel 2e-4 NDC aside.
static double det3(const double m[3][3])
{
    return m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0]) + m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]);
}
static bool unproject(const float* W, const double ndc[3], double out[3])
{
    double A[3][3], rhs[3];
    for (int j = 0; j < 3; j++) {
        for (int c = 0; c < 3; c++) A[j][c] = (double)W[c * 4 + j] - ndc[j] * W[c * 4 + 3];
        rhs[j] = ndc[j] * W[3 * 4 + 3] - (double)W[3 * 4 + j];
    }
    const double det = det3(A);
    if (!(fabs(det) > 0.0)) return false;                              // singular or NaN
    for (int c = 0; c < 3; c++) {
        double M[3][3];
        for (int r = 0; r < 3; r++) for (int cc = 0; cc < 3; cc++) M[r][cc] = cc == c ? rhs[r] : A[r][cc];
        out[c] = det3(M) / det;
        if (!(out[c] == out[c]) || fabs(out[c]) > 3.0e38) return false;
    }
    return true;
}
// squared NDC distance of the fp32 point q from (x, y); infinite behind the eye
static double ndc_error(const float* W, const float q[3], double x, double y)
{
    double cl[4];
    for (int j = 0; j < 4; j++) cl[j] = (((double)q[0] * W[0 * 4 + j] + (double)q[1] * W[1 * 4 + j]) + (double)q[2] * W[2 * 4 + j]) + W[3 * 4 + j];
    if (!(cl[3] > 0.0)) return INFINITY;
    const double ex = cl[0] / cl[3] - x, ey = cl[1] / cl[3] - y;
    return ex * ex + ey * ey;
}

extern "C" VR_API int vr_view_pixel_ray(const vr_view* view, float px, float py, vr_ray* out)
{
    VR_REQUIRE(view && out, "NULL argument");
    VR_REQUIRE(view->viewport_w > 0 && view->viewport_h > 0, "the view has an empty viewport");
    VR_REQUIRE(host_finite(px) && host_finite(py), "pixel coordinates are NaN or infinite");
    const double x = (((double)px + 0.5) - view->viewport_x) / view->viewport_w * 2.0 - 1.0;
    const double y = 1.0 - (((double)py + 0.5) - view->viewport_y) / view->viewport_h * 2.0;
    const float* W = view->world_to_clip;
    const double ndc_near[3] = { x, y, 0.0 }, ndc_far[3] = { x, y, 1.0 };
    double pn[3], pf[3], dn[3], len = 0.0;
    VR_REQUIRE(unproject(W, ndc_near, pn) && unproject(W, ndc_far, pf), "world_to_clip does not un-project this pixel");
    for (int j = 0; j < 3; j++) { dn[j] = pf[j] - pn[j]; len += dn[j] * dn[j]; }
    len = sqrt(len);
    VR_REQUIRE(len > 0.0, "near and far plane coincide");
    // The origin has to be an fp32 point, and the near plane is so close to the eye that rounding alone moves the projection:
    // one ulp of a coordinate near 1000 is 1e-3 NDC at z_near = 0.1.  So the origin is not the near point rounded once: the ray
    // is followed from the near plane in quarter-ulp steps, for at most 64 ulp of the largest coordinate, and the first of the
    // eight fp32 neighbours of a step that projects within 5e-5 NDC of the pixel's centre is taken (else the closest seen).
    double ulp = 0.0;
    for (int j = 0; j < 3; j++) { const float f = fabsf((float)pn[j]); ulp = fmax(ulp, (double)nextafterf(f, INFINITY) - (double)f); }
    float origin[3] = { (float)pn[0], (float)pn[1], (float)pn[2] };
    double best = ndc_error(W, origin, x, y);
    for (int k = 0; k < 256 && best > 2.5e-9; k++) {
        float lo[3], hi[3];
        for (int j = 0; j < 3; j++) {
            const double q = pn[j] + dn[j] / len * (0.25 * k * ulp);
            const float f = (float)q;
            lo[j] = (double)f <= q ? f : nextafterf(f, -INFINITY);
            hi[j] = (double)lo[j] == q ? lo[j] : nextafterf(lo[j], INFINITY);
        }
        for (int c = 0; c < 8; c++) {
            const float cand[3] = { c & 1 ? hi[0] : lo[0], c & 2 ? hi[1] : lo[1], c & 4 ? hi[2] : lo[2] };
            const double e = ndc_error(W, cand, x, y);
            if (e < best) { best = e; origin[0] = cand[0]; origin[1] = cand[1]; origin[2] = cand[2]; }
        }
    }
    memset(out, 0, sizeof(*out));
    for (int j = 0; j < 3; j++) { out->origin[j] = origin[j]; out->dir[j] = (float)(pf[j] - (double)origin[j]); }
    out->t_max = 1.0f;
    return VR_OK;
}
