"""An exact-arithmetic evaluation of the terrain draw, written from the HLSL / D3D semantics - NOT from oracle/vr_oracle.c.

Test infrastructure: tests/test_oracle_cpu.py and tests/test_raster_clip_cpu.py bound the C oracle's raster / sampler model
(revision 3: plane equations, fused sampler arithmetic, a pinned cubic for log2) against this file, and
tests/test_raster_clip_f64.py the HIP tile pass.  What is taken as given, because the text of the reference or of D3D pins it:
  - the vertex stage's fp32 outputs, the node list (ot.select) and the mip chains: they are not this model's subject but
    no longer rest on the oracle alone - tests/f64_frontend.py states main_vs (terrain_vs.hlsl:10-62), NodeSelect, SetHeight
    and the box-filtered chains from the text and bounds the oracle (tests/test_frontend_cpu.py) and the HIP kernels
    (tests/test_frontend_f64.py) by it;
  - what the rasteriser is handed per vertex of a triangle that needs no clipping: the fp32 viewport transform and
    perspective divide and the snap to 8 sub-pixel bits (D3D11 3.4.1 / 3.4.3): X, Y as 24.8 integers, z = z_clip * (1 / w), 1 / w;
  - D3D's coverage rules: pixel centres at +0.5, top-left rule, in-order LessOrEqual depth test.
Everything after that is evaluated here the way the specification states it, in float64 with exact integer edge
functions - none of the oracle's implementation choices:
  - barycentrics l_i = E_i / (2 area) as exact rationals (E_i and the area are integers below 2^53), depth and 1 / w
    interpolated linearly, attributes perspective-correctly: attr = sum(l_i a_i / w_i) / sum(l_i / w_i);
  - Texture2D::Sample's implicit level of detail from the analytic screen-space derivatives of that interpolant,
    lod = log2(max(|d uv / dx| * dims, |d uv / dy| * dims)) with the true log2;
  - bilinear / trilinear filtering (terrain_ps.hlsl:10-24: uv = (pos + half) / size; clamp addressing) on texels decoded
    in float64 (UNORM8 / 255; sRGB EOTF), main_ps's central differences and normalize (terrain_ps.hlsl:59-63), and the
    render targets' conversions (SRGBA8: round to nearest of the OETF; RGBA16_SNORM: round half away from zero).

Triangles that need the near-plane / guard-band clipper ("parents") are not rasterised through any clipper's vertices.  A
clipped polygon lies in its parent's plane, so a pixel of it is evaluated from the parent's three fp32 clip-space vertices
alone, by homogeneous interpolation: lambda solves sum lambda_i (x_i, y_i, w_i) = (ndc_x, ndc_y, 1) (the 3 x 3 inverse in
exact rationals), depth = sum lambda_i z_i, 1 / w = sum lambda_i, attribute / w = sum lambda_i a_i - each an affine function
F of the pixel position - and the LOD's derivatives are those functions' constant gradients.  Where the polygon lies is
the parent clipped in float64 (Sutherland-Hodgman, as D3D's clipper) and projected in float64.  An implementation's
clipper makes new fp32 vertices, snaps them and rasterises SOME fan of sub-triangles; how far that may be from the parent
is derived per parent, first order in u = 2^-24 (terms in u^2 are below 2^-20 of the bound and dropped):

  new vertex v = a + (b - a) t, t = da / (da - db), a inside, b outside, every operation rounded once:
    v_k = (a_k + (b_k - a_k) t^ (1 + e1)(1 + e2))(1 + e3), |e| <= u, with ONE t^ for all components.  The common factor of
    t^ moves v along the parent's edge a-b, inside the parent's plane with all its attributes; what leaves the plane is
      eps_k <= u (2 |v_k - a_k| + |v_k|) <= u (3 |v_k| + 2 |a_k|)                  per component k of (x, y, z, w, wx, wz),
    plus the larger of the ends' own eps where an end is itself a new vertex.
    t^ = t (1 + 2u) for exact distances (near plane: d = z); a guard-band distance d = fl(fl(100 w) +- x) carries
      err(d) <= u (|100 w| + |d|) + 100 eps_w + eps_xy,   err(t) <= (|db| err(da) + |da| err(db)) / (da - db)^2 + 2 u t.
  on the screen (half = viewport size / 2, n = ndc):
    across the plane     perp_x = half_x (eps_x + |n_x| eps_w) / w
    along the edge       along  = |d screen / d t| err(t), d screen_x / d t = half_x ((x_b - x_a) w - x (w_b - w_a)) / w^2,
                         plus the larger of the ends' own
    viewport transform   round_x = u (size_x (|n_x| + 2 |n_x / 2 + 1/2|) + 2 |s_x| + 2^-9)   (1 / w, the product, the sum, the
                         product with the size, the sum with the origin, the sum with 1/2 before the floor)
    snap                 2^-9 per axis
    d_val = |(perp + round + snap)_xy|, d_cov = d_val + along; delta = max d_cov over the polygon's vertices.
  vertex residuals against the parent's plane F at the vertex's snapped position (Zv = z / w):
    depth      r_Z = (eps_z + |Zv| eps_w) / w + 2 u |Zv| + |grad Z| d_val            (fl(z fl(1 / w)): two roundings)
    1 / w      r_Q = eps_w / w^2 + u / w + |grad Q| d_val
    attr / w   r_N = (eps_a + |a| (eps_w / w + u)) / w + |grad N| d_val              (the product a * (1 / w) is exact in double)
  Inside a sub-triangle an affine quantity is a convex combination of its vertex values, so its distance from F is at
  most R_F = max r_F over the polygon's vertices - whatever fan was chosen.  To that the plane-equation evaluation
  fmaf(py, dy, fmaf(px, dx, p0)) adds u (|p0| + |px dx| + |py dy|) for the three rounded coefficients, u |inner| and
  u |result| for the two fused operations, together <= 3 u E_F, E_F = max |F| + |F_x| width + |F_y| height over the
  polygon's viewport-clamped bounding box (any sub-triangle's anchor and offsets lie in it), and the double-precision
  set-up 72 * 2^-53 L max|f| (three dot products of three terms, barycentrics up to L in magnitude: L is the largest ratio
  of a triangle (p, v_j, v_k) to a triangle (v_i, v_j, v_k) over the box's corners p and the polygon's vertex triples).
    tolerance of Z, Q, N at a pixel   tol_F = R_F + 3 u E_F + set-up
    world xz of a clipped parent, N and Q jointly (they share t^ and the snap): for a pixel with exact a0 = N / Q the function
    e = (G_N - F_N) - a0 (G_Q - F_Q) of a sub-triangle's planes G is affine and is what the quotient is off by, times 1 / Q.
    At a vertex with attribute a_v, 1 / w = Q_v and screen displacement d,
      e_v = (a_v - a0)(err(Q_v) - grad Q . d) + Q_v (eps_a - grad A(v) . d),  grad A(v) = (grad F_N - a_v grad F_Q) / Q_v,
      |e_v| <= |a_v - a0| r_Q(v) + Q_v (eps_a + |grad A(v)| d_val),
    so tol = (max_v |e_v| + 3 u (E_N + |a0| E_Q) + set-up) / |Q| + 2 u |a0| over the polygon's vertices (1 / q and the product).
    LOD: the actual sub-triangle is one of the polygon's vertex triples T that hold the pixel (within delta); on it
    |grad e| <= 2 max_(v in T) |e_v| / h_T and |grad (G_Q - F_Q)| <= 2 max r_Q / h_T, h_T its smallest altitude less
    2 delta, and the derivative D = (N_x - a0 Q_x) / Q moves by at most
      (2 e_T / h_T + tol (|Q_x| + 2 r_Q / h_T) + 2 u (|N_x| + |a0 Q_x|)) / |Q| + |D| (tol_Q / |Q| + 2 u);
    rho moves by the length of the moved pair and the LOD by -log2(1 - err(rho) / rho), the largest over the triples that
    hold the pixel (a triple thinner than 2 delta makes it infinite for the pixels IT holds only), on top of the LOD
    function's own error (lod_fn_tol: half the pinned cubic's error, which lod_cubic_error() measures, and 16 u (1 + |lod|)).
    A triangle that needs no clipping: world xz tol = (tol_N + |N / Q| tol_Q) / |Q| + 2 u |N / Q| and the derivative's
      (g_N + |N / Q| g_Q + |Q_x| tol_xz + u (|N_x| + |N / Q| |Q_x|)) / |Q| + |D| (tol_Q / |Q| + 2 u), g = u |F_x| + set-up.
  A triangle that needs no clipping has R = 0 and delta = 0 and keeps the same evaluation terms, per pixel about its own
  anchor (the first pixel of its viewport-clamped box): 3 u (|F(anchor)| + |F_x| dx + |F_y| dy) + set-up.  The "within 1 ulp"
  of depth in tests/test_oracle_cpu.py is a property of its four cameras, not of this model.

Coverage is stated in three classes.  A pixel centre inside a front-facing parent's exact polygon by more than delta,
with depth inside (0, 1) by more than tol_Z, is a certain fragment; one outside every polygon by more than delta is none;
between, a fragment may or may not exist.  (The union of any fan of the displaced polygon contains the first set and lies
in the complement of the second: winding number.  A polygon no wider than 2 delta may face either way after the snap: all
of it is "may".)  A shift of a guard-band vertex along the guard-band line, 99 half-viewports outside the viewport, moves
no edge inside the viewport by more than its other end moves.  Triangles that need no clipping keep the exact top-left
rule.  Per pixel the nearest fragment P and the next A are kept with their tolerances: MUST be covered = P certain, or P
"may" and A certain; EMPTY = no fragment; BAND otherwise.  Where A could have won (closer than the sum of the
tolerances, or P only "may"), `either` is set and a value may match P's or A's; where a third could, `multi` is set and
the pixel's values are not compared (it counts towards the band share the tests limit).
"""
import itertools
from fractions import Fraction

import numpy as np

GUARD_BAND = 100.0
G = 32
S = G + 1
U = 2.0 ** -24
SNAP = 2.0 ** -9
OWNER_TILE = 128                                    # vr_partition: owner tiles, dealt round-robin along the diagonals
EMPTY, BAND, MUST = 0, 1, 2
# slot layout: depth, its tolerance, certain, from the clipper, q, wx, wz, four derivatives, tol wx, tol wz, LOD term
K = 14


def _tri_indices():
    ci, cj = np.meshgrid(np.arange(G), np.arange(G), indexing="ij")
    bl = (ci * S + cj).ravel()
    tl = bl + S
    tr = tl + 1
    br = bl + 1
    # index buffer (TerrainPass.cpp:68-87): per cell (BL, TL, TR), (BL, TR, BR); row = z, column = x
    return np.stack([np.stack([bl, tl, tr], 1), np.stack([bl, tr, br], 1)], 1).reshape(-1, 3)


_TRIS = _tri_indices()


def lod_cubic_error():
    """max |p(t) - log2(1 + t)| of the cubic the LOD is taken from (a pinned constant of the model revision), in float64."""
    t = np.linspace(0.0, 1.0, 200001)
    return float(np.abs(t * (1.4208646 + t * (-0.57725066 + t * 0.1563861)) - np.log2(1.0 + t)).max())


def lod_fn_tol(lod):
    return 0.5 * lod_cubic_error() + 16.0 * U * (1.0 + np.abs(lod))


def _to_screen_f32(clip, vp):
    """What the rasteriser is handed: fp32 perspective divide + viewport transform, snapped to 24.8 (round to nearest)."""
    f = np.float32
    c = clip.astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        iw = f(1.0) / c[..., 3]
        nx, ny = c[..., 0] * iw, c[..., 1] * iw
        sx = (nx * f(0.5) + f(0.5)) * f(vp[2]) + f(vp[0])
        sy = (ny * f(-0.5) + f(0.5)) * f(vp[3]) + f(vp[1])
        X = np.floor(sx * f(256.0) + f(0.5))
        Y = np.floor(sy * f(256.0) + f(0.5))
        z = c[..., 2] * iw
    ok = np.isfinite(X) & np.isfinite(Y) & (np.abs(X) < 2.0 ** 40) & (np.abs(Y) < 2.0 ** 40)
    X = np.where(ok, X, 0.0).astype(np.int64)
    Y = np.where(ok, Y, 0.0).astype(np.int64)
    return X, Y, z.astype(np.float64), iw.astype(np.float64)


def _clip_poly64(poly, plane, half):
    """Sutherland-Hodgman against one plane in float64; poly = list of (v[6] = clip xyzw, world x, world z; eps[6]; along):
    the exact vertex, what an fp32 clipper's vertex may be off the parent's plane per component, and how far along it in
    pixels (module docstring).  half = half the viewport's size."""
    def dist(c):
        if plane == 0:
            return c[2]
        if plane == 1:
            return GUARD_BAND * c[3] + c[0]
        if plane == 2:
            return GUARD_BAND * c[3] - c[0]
        if plane == 3:
            return GUARD_BAND * c[3] + c[1]
        return GUARD_BAND * c[3] - c[1]

    def dist_err(p, dd):
        c, e = p[0], p[1]
        if plane == 0:
            return e[2]
        return U * (abs(GUARD_BAND * c[3]) + abs(dd)) + GUARD_BAND * e[3] + e[0 if plane in (1, 2) else 1]
    out = []
    n = len(poly)
    d = [dist(p[0]) for p in poly]
    for i in range(n):
        j = (i + 1) % n
        ini, inj = d[i] >= 0.0, d[j] >= 0.0
        if ini:
            out.append(poly[i])
        if ini != inj:
            a, b = (poly[i], poly[j]) if ini else (poly[j], poly[i])
            da, db = (d[i], d[j]) if ini else (d[j], d[i])
            t = da / (da - db)
            v = a[0] + (b[0] - a[0]) * t
            eps = U * (3.0 * np.abs(v) + 2.0 * np.abs(a[0])) + np.maximum(a[1], b[1])
            terr = (abs(db) * dist_err(a, da) + abs(da) * dist_err(b, db)) / (da - db) ** 2 + 2.0 * U * t
            dv = b[0] - a[0]
            sdx = half[0] * (dv[0] * v[3] - v[0] * dv[3]) / v[3] ** 2
            sdy = half[1] * (dv[1] * v[3] - v[1] * dv[3]) / v[3] ** 2
            out.append((v, eps, float(np.hypot(sdx, sdy)) * terr + max(a[2], b[2])))
    return out


def _parent_planes(c, wx, wz, vp):
    """Z, Q = 1 / w, NX = world x / w, NZ = world z / w of the plane of a triangle with clip-space vertices c (3, 4) as
    (F0, Fx, Fy): F at pixel (i, j)'s centre = F0 + Fx i + Fy j.  The inverse in exact rationals; None if singular."""
    fr = Fraction
    m = [[fr(float(c[k, r])) for k in range(3)] for r in (0, 1, 3)]            # rows x, y, w; columns the vertices
    cof = [[m[(r + 1) % 3][(k + 1) % 3] * m[(r + 2) % 3][(k + 2) % 3] - m[(r + 1) % 3][(k + 2) % 3] * m[(r + 2) % 3][(k + 1) % 3]
            for k in range(3)] for r in range(3)]
    det = sum(m[0][k] * cof[0][k] for k in range(3))
    if det == 0:
        return None
    inv = [[cof[r][k] / det for r in range(3)] for k in range(3)]              # inv[k][r]: lambda_k = sum_r inv[k][r] rhs_r
    vx, vy, vw, vh = (fr(float(x)) for x in vp)
    # ndc_x = 2 (i + 1/2 - vx) / vw - 1, ndc_y = 1 - 2 (j + 1/2 - vy) / vh
    ax, bx = 2 / vw, 2 * (fr(1, 2) - vx) / vw - 1
    ay, by = -2 / vh, 1 - 2 * (fr(1, 2) - vy) / vh
    out = []
    for a in ([fr(float(c[k, 2])) for k in range(3)], [fr(1)] * 3, [fr(float(x)) for x in wx], [fr(float(x)) for x in wz]):
        g = [sum(a[k] * inv[k][r] for k in range(3)) for r in range(3)]
        out.append((float(g[0] * bx + g[1] * by + g[2]), float(g[0] * ax), float(g[1] * ay)))
    return out


class Frame:
    pass


def render(ot, view, w, h, max_height, world_size, hm_levels, al_levels, lod_for_sampling=None, part=None):
    """The frame TerrainPass::Render draws for `view` into a cleared w x h target, evaluated exactly.
    ot: the oracle terrain (used for NodeSelect and the vertex stage only); hm_levels / al_levels: the mip chains as
    uint8 arrays.  lod_for_sampling: an (h, w) array of levels of detail to sample with instead of this model's own
    (the test passes the oracle's, so that the filter arithmetic is compared at equal LOD and the LOD itself separately).
    part: (rank, world size) of a vr_partition; pixels of other ranks' tiles stay empty."""
    n, ids, inst = ot.select(view, max_height)
    vp = (float(view.viewport_x), float(view.viewport_y), float(view.viewport_w), float(view.viewport_h))
    half = (vp[2] * 0.5, vp[3] * 0.5)
    vx0, vy0 = max(view.viewport_x, 0), max(view.viewport_y, 0)
    vx1, vy1 = min(view.viewport_x + view.viewport_w - 1, w - 1), min(view.viewport_y + view.viewport_h - 1, h - 1)
    mirrored = bool(view.mirrored)
    W0, H0 = hm_levels[0].shape[1], hm_levels[0].shape[0]
    own = np.ones((h, w), bool)
    if part is not None and part[1] > 1:
        yy, xx = np.mgrid[0:h, 0:w]
        own = (xx // OWNER_TILE + yy // OWNER_TILE) % part[1] == part[0]

    slots = np.zeros((h, w, 2, K))                  # the nearest fragment P and the next A
    slots[..., 0] = np.inf
    third = np.full((h, w), np.inf)                 # the least depth - tolerance of every further fragment
    ambiguous = np.zeros((h, w), bool)              # the depth test was decided by less than a few fp32 ulps
    tri_count = dict(total=0, rasterised=0, clipped=0, near=0, guard=0, near_and_guard=0, poly_verts=0, poly_subtris=0, degenerate=0, behind=0, behind_pixels=0)
    delta_max = [0.0]

    def insert(y0, y1, x0, x1, cand, C):
        sub = slots[y0:y1 + 1, x0:x1 + 1]
        tl = third[y0:y1 + 1, x0:x1 + 1]
        Pz, Az, Cz = sub[..., 0, 0], sub[..., 1, 0], C[..., 0]
        ulp = np.spacing(np.maximum(np.abs(Cz), 2.0 ** -126).astype(np.float32)).astype(np.float64)
        ambiguous[y0:y1 + 1, x0:x1 + 1] |= cand & np.isfinite(Pz) & (np.abs(Cz - Pz) <= 4.0 * ulp)
        front = cand & (Cz <= Pz)                                       # LessOrEqual, in draw order
        mid = cand & ~front & (Cz <= Az)
        back = cand & ~front & ~mid
        push = front | mid
        tl[push] = np.minimum(tl[push], (Az - sub[..., 1, 1])[push])
        tl[back] = np.minimum(tl[back], (Cz - C[..., 1])[back])
        sub[..., 1, :][front] = sub[..., 0, :][front]
        sub[..., 1, :][mid] = C[mid]
        sub[..., 0, :][front] = C[front]

    def only_behind(y0, y1, x0, x1, cand, zz, tz):
        """True if every fragment lies behind both kept ones: then only `third` learns of them."""
        if (zz <= slots[y0:y1 + 1, x0:x1 + 1, 1, 0])[cand].any():
            return False
        tl = third[y0:y1 + 1, x0:x1 + 1]
        tl[cand] = np.minimum(tl[cand], (zz - tz)[cand])
        return True

    def fragments(zz, tz, inside, certain, clipped, q, nx, nz, gr, tq, tnx, tnz, gq, gnx, gnz, over=None):
        """Pack the fragments of one triangle or parent.  zz, q, nx, nz: the planes over the box; tz, tq, tnx, tnz their
        tolerances; gr = (qx, qy, nxx, nxy, nzx, nzy) the gradients per pixel, gq / gnx / gnz = (x, y) their tolerances;
        over: a parent's own (tol wx, tol wz, LOD term) in place of the ones made from those."""
        cand = inside & (zz >= -tz) & (zz <= 1.0 + tz)                  # depth clip
        if not cand.any():
            return cand, None
        cert = certain & (zz > tz) & (zz < 1.0 - tz)
        qx, qy, nxx, nxy, nzx, nzy = gr
        C = np.zeros(zz.shape + (K,))
        with np.errstate(divide="ignore", invalid="ignore"):
            aq = np.abs(q)
            pwx, pwz = nx / q, nz / q
            twx = (tnx + np.abs(pwx) * tq) / aq + 2.0 * U * np.abs(pwx)
            twz = (tnz + np.abs(pwz) * tq) / aq + 2.0 * U * np.abs(pwz)
            D, dD = [], []
            for pw, tw, gn, nd, qd, k in ((pwx, twx, gnx, nxx, qx, 0), (pwx, twx, gnx, nxy, qy, 1), (pwz, twz, gnz, nzx, qx, 0), (pwz, twz, gnz, nzy, qy, 1)):
                d = (nd - pw * qd) / q
                D.append(d)
                dD.append((gn[k] + np.abs(pw) * gq[k] + abs(qd) * tw + U * (abs(nd) + np.abs(pw) * abs(qd))) / aq + np.abs(d) * (tq / aq + 2.0 * U))
            # D = dwx/dx, dwx/dy, dwz/dx, dwz/dy
            rx, ry = np.hypot(D[0] * W0, D[2] * H0), np.hypot(D[1] * W0, D[3] * H0)
            drho = np.maximum(np.hypot(dD[0] * W0, dD[2] * H0), np.hypot(dD[1] * W0, dD[3] * H0)) + U * np.maximum(rx, ry)
            rel = drho / np.maximum(rx, ry)
            lterm = np.where(rel <= 0.5, -np.log2(1.0 - np.minimum(rel, 0.5)), np.inf)
        C[..., 0], C[..., 1], C[..., 2], C[..., 3] = zz, tz, cert, clipped
        C[..., 4], C[..., 5], C[..., 6] = q, pwx, pwz
        C[..., 7], C[..., 8], C[..., 9], C[..., 10] = D[0], D[2], D[1], D[3]      # dwx/dx, dwz/dx, dwx/dy, dwz/dy
        if over is not None:
            twx, twz, lterm = over
        C[..., 11], C[..., 12], C[..., 13] = twx, twz, np.nan_to_num(lterm, nan=np.inf)
        return cand, C

    def raster(X, Y, z, iw, wx, wz):
        """One triangle that needs no clipping, vertices in submission order (three of each)."""
        area2 = (X[1] - X[0]) * (Y[2] - Y[0]) - (X[2] - X[0]) * (Y[1] - Y[0])
        if area2 == 0:
            return
        cw = area2 > 0
        if (not cw) if not mirrored else cw:        # back faces: front = clockwise unless mirrored
            return
        o = [0, 1, 2] if cw else [0, 2, 1]
        X, Y, z, iw, wx, wz = X[o], Y[o], z[o], iw[o], wx[o], wz[o]
        area2 = abs(int(area2))
        x0 = max((int(X.min()) - 128 + 255) >> 8, vx0); x1 = min((int(X.max()) - 128) >> 8, vx1)
        y0 = max((int(Y.min()) - 128 + 255) >> 8, vy0); y1 = min((int(Y.max()) - 128) >> 8, vy1)
        if x0 > x1 or y0 > y1:
            return
        PX = (np.arange(x0, x1 + 1, dtype=np.int64) * 256 + 128)[None, :]
        PY = (np.arange(y0, y1 + 1, dtype=np.int64) * 256 + 128)[:, None]

        def edge(a, b):
            return (X[b] - X[a]) * (PY - Y[a]) - (Y[b] - Y[a]) * (PX - X[a])

        def top_left(a, b):
            dx, dy = X[b] - X[a], Y[b] - Y[a]
            return dy < 0 or (dy == 0 and dx > 0)
        E0, E1, E2 = edge(1, 2), edge(2, 0), edge(0, 1)
        inside = (E0 - (0 if top_left(1, 2) else 1) >= 0) & (E1 - (0 if top_left(2, 0) else 1) >= 0) & (E2 - (0 if top_left(0, 1) else 1) >= 0)
        if not inside.any():
            return
        tri_count["rasterised"] += 1
        inside &= own[y0:y1 + 1, x0:x1 + 1]
        a2 = float(area2)
        l0, l1, l2 = E0 / a2, E1 / a2, E2 / a2                          # exact rationals, correctly rounded to float64
        # d l_i / dx = d E_i / d px * 256 / area2 (one pixel = 256 sub-pixel units)
        dldx = np.array([-(Y[2] - Y[1]), -(Y[0] - Y[2]), -(Y[1] - Y[0])], np.float64) * 256.0 / a2
        dldy = np.array([(X[2] - X[1]), (X[0] - X[2]), (X[1] - X[0])], np.float64) * 256.0 / a2
        dxs = np.arange(0, x1 - x0 + 1, dtype=np.float64)[None, :]
        dys = np.arange(0, y1 - y0 + 1, dtype=np.float64)[:, None]
        lmax = max(np.abs(l0).max(), np.abs(l1).max(), np.abs(l2).max())

        def plane(a):
            f = l0 * a[0] + l1 * a[1] + l2 * a[2]
            fx, fy = float(dldx @ a), float(dldy @ a)
            setup = 72.0 * 2.0 ** -53 * lmax * np.abs(a).max()
            return f, fx, fy, 3.0 * U * (abs(f[0, 0]) + abs(fx) * dxs + abs(fy) * dys) + setup, (U * abs(fx) + setup, U * abs(fy) + setup)
        zz, _, _, tz, _ = plane(z)
        cand = inside & (zz >= -tz) & (zz <= 1.0 + tz)
        if not cand.any() or only_behind(y0, y1, x0, x1, cand, zz, tz):
            return
        q, qx, qy, tq, gq = plane(iw)
        nx, nxx, nxy, tnx, gnx = plane(wx * iw)
        nz, nzx, nzy, tnz, gnz = plane(wz * iw)
        cand, C = fragments(zz, tz, inside, inside, False, q, nx, nz, (qx, qy, nxx, nxy, nzx, nzy), tq, tnx, tnz, gq, gnx, gnz)
        if C is not None:
            insert(y0, y1, x0, x1, cand, C)

    def parent(c, pwx, pwz):
        """One triangle that needs the clipper: fragments from its plane, coverage classes from its exact polygon."""
        if (c[0] == c[1]).all() or (c[1] == c[2]).all() or (c[2] == c[0]).all():
            return                                  # two vertices morphed into one: no area in any arithmetic
        planes = _parent_planes(c, pwx, pwz, vp)
        if planes is None:
            tri_count["degenerate"] += 1
            return
        poly = [(np.array([c[k, 0], c[k, 1], c[k, 2], c[k, 3], pwx[k], pwz[k]], np.float64), np.zeros(6), 0.0) for k in range(3)]
        behind = bool((c[:, 3] <= 0).any())
        near = any(p[0][2] < 0 for p in poly)
        if near:
            poly = _clip_poly64(poly, 0, half)
        guard = len(poly) >= 3 and any(abs(p[0][0]) > GUARD_BAND * p[0][3] or abs(p[0][1]) > GUARD_BAND * p[0][3] for p in poly)
        tri_count["near"] += near
        tri_count["guard"] += guard
        tri_count["near_and_guard"] += near and guard
        if guard:
            for pl in range(1, 5):
                poly = _clip_poly64(poly, pl, half)
                if len(poly) < 3:
                    break
        if len(poly) < 3:
            return
        tri_count["poly_verts"] += len(poly)
        tri_count["poly_subtris"] += len(poly) - 2
        V, E, AL = np.array([p[0] for p in poly]), np.array([p[1] for p in poly]), np.array([p[2] for p in poly])
        pw = V[:, 3]
        ndx, ndy = V[:, 0] / pw, V[:, 1] / pw
        sx, sy = (ndx * 0.5 + 0.5) * vp[2] + vp[0], (ndy * -0.5 + 0.5) * vp[3] + vp[1]
        perp_x, perp_y = half[0] * (E[:, 0] + np.abs(ndx) * E[:, 3]) / pw, half[1] * (E[:, 1] + np.abs(ndy) * E[:, 3]) / pw
        rnd_x = U * (vp[2] * (np.abs(ndx) + 2.0 * np.abs(ndx * 0.5 + 0.5)) + 2.0 * np.abs(sx) + SNAP)
        rnd_y = U * (vp[3] * (np.abs(ndy) + 2.0 * np.abs(ndy * -0.5 + 0.5)) + 2.0 * np.abs(sy) + SNAP)
        d_val = np.hypot(perp_x + rnd_x + SNAP, perp_y + rnd_y + SNAP)
        delta = float((d_val + AL).max())
        (Z0, Zx, Zy), (Q0, Qx, Qy), (NX0, NXx, NXy), (NZ0, NZx, NZy) = planes
        Zv = V[:, 2] / pw
        R_Z = float(((E[:, 2] + np.abs(Zv) * E[:, 3]) / pw + 2.0 * U * np.abs(Zv) + np.hypot(Zx, Zy) * d_val).max())
        R_Q = float((E[:, 3] / pw ** 2 + U / pw + np.hypot(Qx, Qy) * d_val).max())
        R_NX = float(((E[:, 4] + np.abs(V[:, 4]) * (E[:, 3] / pw + U)) / pw + np.hypot(NXx, NXy) * d_val).max())
        R_NZ = float(((E[:, 5] + np.abs(V[:, 5]) * (E[:, 3] / pw + U)) / pw + np.hypot(NZx, NZy) * d_val).max())
        # the polygon on the screen, pixel (i, j)'s centre at (i + 1/2, j + 1/2); repeated vertices dropped
        pts, keep = [], []
        for k, p in enumerate(zip(sx - 0.5, sy - 0.5)):
            if not pts or p != pts[-1]:
                pts.append(p)
                keep.append(k)
        if len(pts) > 1 and pts[0] == pts[-1]:
            pts.pop()
            keep.pop()
        if len(pts) < 3:
            return
        P = np.array(pts)
        Pn = np.roll(P, -1, 0)
        area2 = float((P[:, 0] * Pn[:, 1] - Pn[:, 0] * P[:, 1]).sum())     # > 0: clockwise on the (y-down) target
        if area2 == 0.0:
            return
        sgn = 1.0 if area2 > 0 else -1.0
        elen = np.hypot(Pn[:, 0] - P[:, 0], Pn[:, 1] - P[:, 1])
        # signed distance of point (x, y) from edge k, positive inside
        def edge_dist(k, x, y):
            return sgn * ((Pn[k, 0] - P[k, 0]) * (y - P[k, 1]) - (Pn[k, 1] - P[k, 1]) * (x - P[k, 0])) / elen[k]
        width = min(max(edge_dist(k, P[:, 0], P[:, 1])) for k in range(len(P)))
        sliver = width <= 2.0 * delta
        front = (area2 > 0) != mirrored
        if not front and not sliver:
            return
        x0 = max(int(np.ceil(np.clip(P[:, 0].min() - delta, -1e9, 1e9))), vx0); x1 = min(int(np.floor(np.clip(P[:, 0].max() + delta, -1e9, 1e9))), vx1)
        y0 = max(int(np.ceil(np.clip(P[:, 1].min() - delta, -1e9, 1e9))), vy0); y1 = min(int(np.floor(np.clip(P[:, 1].max() + delta, -1e9, 1e9))), vy1)
        if x0 > x1 or y0 > y1:
            return
        xs = np.arange(x0, x1 + 1, dtype=np.float64)[None, :]
        ys = np.arange(y0, y1 + 1, dtype=np.float64)[:, None]
        dmin = np.full((y1 - y0 + 1, x1 - x0 + 1), np.inf)
        for k in range(len(P)):
            dmin = np.minimum(dmin, edge_dist(k, xs, ys))
        inside = (dmin >= -delta) & own[y0:y1 + 1, x0:x1 + 1]
        if not inside.any():
            return
        certain = inside & (dmin > delta) & (not sliver)
        delta_max[0] = max(delta_max[0], delta)
        # every vertex triple: the smallest altitude, and the largest barycentric of a corner of the box or a vertex
        corners = np.array([(x0 - 1.0, y0 - 1.0), (x1 + 1.0, y0 - 1.0), (x0 - 1.0, y1 + 1.0), (x1 + 1.0, y1 + 1.0)])
        probe = np.concatenate([corners, P])
        hmin, lmax = np.inf, 1.0

        def tri_area(a, b, cc):
            return 0.5 * np.abs((b[..., 0] - a[..., 0]) * (cc[..., 1] - a[..., 1]) - (cc[..., 0] - a[..., 0]) * (b[..., 1] - a[..., 1]))
        for i, j, k in itertools.combinations(range(len(P)), 3):
            ar = float(tri_area(P[i], P[j], P[k]))
            side = max(np.hypot(*(P[i] - P[j])), np.hypot(*(P[j] - P[k])), np.hypot(*(P[k] - P[i])))
            hmin = min(hmin, 2.0 * ar / side)
            ar_min = max(ar - delta * 1.5 * side, 2.0 ** -17)           # the snapped triangle's area: at least one 24.8 unit
            big = max(tri_area(probe, P[a], P[b]).max() for a, b in ((i, j), (j, k), (k, i))) + delta * 1.5 * side
            lmax = max(lmax, big / ar_min)
        hmin = hmin - 2.0 * delta
        inv_h = 2.0 / hmin if hmin > 0 else np.inf
        bx = np.array([x0 - 1.0, x1 + 1.0, x0 - 1.0, x1 + 1.0])
        by = np.array([y0 - 1.0, y0 - 1.0, y1 + 1.0, y1 + 1.0])

        def tol(F0, Fx, Fy, R, vmax):
            setup = 72.0 * 2.0 ** -53 * lmax * (vmax + R)
            Ef = np.abs(F0 + Fx * bx + Fy * by).max() + abs(Fx) * (x1 - x0 + 2) + abs(Fy) * (y1 - y0 + 2)
            return R + 3.0 * U * Ef + setup, (R * inv_h + U * abs(Fx) + setup, R * inv_h + U * abs(Fy) + setup)
        tz, _ = tol(Z0, Zx, Zy, R_Z, np.abs(Zv).max())
        tq, gq = tol(Q0, Qx, Qy, R_Q, (1.0 / pw).max())
        tnx, gnx = tol(NX0, NXx, NXy, R_NX, np.abs(V[:, 4] / pw).max())
        tnz, gnz = tol(NZ0, NZx, NZy, R_NZ, np.abs(V[:, 5] / pw).max())
        zz = Z0 + Zx * xs + Zy * ys
        q = Q0 + Qx * xs + Qy * ys
        nx = NX0 + NXx * xs + NXy * ys
        nz = NZ0 + NZx * xs + NZy * ys
        # world xz and the LOD jointly (module docstring): per vertex the residual of N - wx0 Q against the parent's
        Vk, Ek, dk = V[keep], E[keep], d_val[keep]
        Qv = 1.0 / Vk[:, 3]
        rQv = Ek[:, 3] * Qv ** 2 + U * Qv + np.hypot(Qx, Qy) * dk
        setup_q = 72.0 * 2.0 ** -53 * lmax * (Qv.max() + R_Q)
        E_Q = np.abs(Q0 + Qx * bx + Qy * by).max() + abs(Qx) * (x1 - x0 + 2) + abs(Qy) * (y1 - y0 + 2)
        with np.errstate(divide="ignore", invalid="ignore"):
            aq = np.abs(q)
            joint = []
            for comp, (F0, Fx, Fy), f in ((4, planes[2], nx), (5, planes[3], nz)):
                av = Vk[:, comp]
                cv = Qv * (Ek[:, comp] + np.hypot(Fx - av * Qx, Fy - av * Qy) / Qv * dk)
                a0 = f / q
                ev = [np.abs(av[k] - a0) * rQv[k] + cv[k] for k in range(len(P))]
                E_N = np.abs(F0 + Fx * bx + Fy * by).max() + abs(Fx) * (x1 - x0 + 2) + abs(Fy) * (y1 - y0 + 2)
                setup_n = 72.0 * 2.0 ** -53 * lmax * (np.abs(av * Qv).max() + R_NX + R_NZ)
                ta = (np.maximum.reduce(ev) + 3.0 * U * (E_N + np.abs(a0) * E_Q) + setup_n + np.abs(a0) * setup_q) / aq + 2.0 * U * np.abs(a0)
                joint.append((a0, ta, ev, (Fx, Fy)))
            lterm = np.zeros(zz.shape)
            seen = np.zeros(zz.shape, bool)
            for i, j, k in itertools.combinations(range(len(P)), 3):
                cross = (P[j, 0] - P[i, 0]) * (P[k, 1] - P[i, 1]) - (P[k, 0] - P[i, 0]) * (P[j, 1] - P[i, 1])
                if cross == 0.0:
                    continue
                o = (i, j, k) if cross > 0 else (i, k, j)
                side = max(np.hypot(*(P[i] - P[j])), np.hypot(*(P[j] - P[k])), np.hypot(*(P[k] - P[i])))
                dist = np.full(zz.shape, np.inf)
                for a, b in ((o[0], o[1]), (o[1], o[2]), (o[2], o[0])):
                    ln = np.hypot(*(P[b] - P[a]))
                    dist = np.minimum(dist, ((P[b, 0] - P[a, 0]) * (ys - P[a, 1]) - (P[b, 1] - P[a, 1]) * (xs - P[a, 0])) / ln)
                has = dist >= -delta
                if not has.any():
                    continue
                seen |= has
                hT = abs(cross) / side - 2.0 * delta
                if hT <= 0.0:
                    lterm = np.where(has, np.inf, lterm)
                    continue
                gQ = 2.0 * max(rQv[i], rQv[j], rQv[k]) / hT
                dD, D0 = [], []
                for a0, ta, ev, (Fx, Fy) in joint:
                    eT = np.maximum(np.maximum(ev[i], ev[j]), ev[k])
                    for nd, qd in ((Fx, Qx), (Fy, Qy)):
                        d0 = (nd - a0 * qd) / q
                        D0.append(d0)
                        dD.append((2.0 * eT / hT + ta * (abs(qd) + gQ) + 2.0 * U * (abs(nd) + np.abs(a0) * abs(qd))) / aq + np.abs(d0) * (tq / aq + 2.0 * U))
                rx, ry = np.hypot(D0[0] * W0, D0[2] * H0), np.hypot(D0[1] * W0, D0[3] * H0)
                drho = np.maximum(np.hypot(dD[0] * W0, dD[2] * H0), np.hypot(dD[1] * W0, dD[3] * H0)) + U * np.maximum(rx, ry)
                rel = drho / np.maximum(rx, ry)
                lT = np.where(rel <= 0.5, -np.log2(1.0 - np.minimum(rel, 0.5)), np.inf)
                lterm = np.where(has, np.maximum(lterm, np.nan_to_num(lT, nan=np.inf)), lterm)
            lterm = np.where(seen, lterm, np.inf)
        cand, C = fragments(zz, np.full(zz.shape, tz), inside, certain, True, q, nx, nz, (Qx, Qy, NXx, NXy, NZx, NZy),
                            tq, tnx, tnz, gq, gnx, gnz, over=(joint[0][1], joint[1][1], lterm))
        if C is None:
            return
        if behind:                                   # a parent that reaches behind the eye contributes only in front of it
            tri_count["behind"] += 1
            tri_count["behind_pixels"] += int(cand.sum())
            assert (q[cand] > 0.0).all(), "a clipped parent with a vertex at w <= 0 contributes a pixel with 1 / w <= 0"
        insert(y0, y1, x0, x1, cand, C)

    for i in range(n):
        clip = np.empty((S * S, 4), np.float32)
        world = np.empty((S * S, 3), np.float32)
        for vz in range(S):
            for vx in range(S):
                c, wv = ot.vertex(view, max_height, inst[i], vx, vz)
                clip[vz * S + vx] = c
                world[vz * S + vx] = wv
        X, Y, z, iw = _to_screen_f32(clip, vp)
        wx, wz = world[:, 0].astype(np.float64), world[:, 2].astype(np.float64)
        c3 = clip[_TRIS]                                            # (2048, 3, 4)
        cx, cy, cz, cw_ = c3[..., 0], c3[..., 1], c3[..., 2], c3[..., 3]
        rejected = ((cx < -cw_).all(1) | (cx > cw_).all(1) | (cy < -cw_).all(1) | (cy > cw_).all(1) | (cz < 0).all(1) | (cz > cw_).all(1))
        g = GUARD_BAND * cw_
        hard = ~rejected & ((cz < 0).any(1) | ((cx < -g) | (cx > g) | (cy < -g) | (cy > g)).any(1))
        tri_count["total"] += int((~rejected).sum())
        for t in np.nonzero(~rejected)[0]:
            idx = _TRIS[t]
            if not hard[t]:
                raster(X[idx], Y[idx], z[idx], iw[idx], wx[idx], wz[idx])
                continue
            tri_count["clipped"] += 1
            parent(clip[idx].astype(np.float64), wx[idx], wz[idx])

    fr = Frame()
    P_, A_ = slots[..., 0, :], slots[..., 1, :]
    hasP, hasA = np.isfinite(P_[..., 0]), np.isfinite(A_[..., 0])
    Pc, Ac = hasP & (P_[..., 2] > 0), hasA & (A_[..., 2] > 0)
    reach = P_[..., 0] + P_[..., 1]
    close_a = hasA & (A_[..., 0] - A_[..., 1] <= reach)
    close_t = third <= reach
    fr.cls = np.where(Pc | (hasP & ~Pc & Ac), MUST, np.where(hasP, BAND, EMPTY))
    maybe = hasP & ~Pc
    fr.multi = (Pc & close_t) | (maybe & hasA & (~Ac | (third <= A_[..., 0] + A_[..., 1])))
    fr.either = ~fr.multi & ((Pc & close_a) | (maybe & Ac))
    fr.covered = fr.cls == MUST
    fr.band = fr.cls == BAND
    fr.ambiguous = ambiguous
    fr.from_clipper = hasP & (P_[..., 3] > 0)
    fr.depth = np.where(hasP, P_[..., 0], 1.0)
    fr.depth_tol = np.where(hasP, P_[..., 1], 0.0)
    fr.tri_count = tri_count
    fr.nodes = n
    fr.delta = delta_max[0]
    half_w = world_size * 0.5

    def shade(slot, valid):
        """wx, wz, their tolerances, the LOD and its input term, and the sampled codes of one slot."""
        o = Frame()
        o.valid = valid
        o.depth, o.depth_tol = np.where(valid, slot[..., 0], 1.0), np.where(valid, slot[..., 1], 0.0)
        o.from_clipper = valid & (slot[..., 3] > 0)
        o.wx, o.wz = slot[..., 5], slot[..., 6]
        o.wx_tol, o.wz_tol, o.lod_term = slot[..., 11], slot[..., 12], slot[..., 13]
        u, v = (o.wx + half_w) / world_size, (o.wz + half_w) / world_size
        dudx, dvdx, dudy, dvdy = (slot[..., k] / world_size for k in (7, 8, 9, 10))
        with np.errstate(divide="ignore", invalid="ignore"):
            rho = np.maximum(np.hypot(dudx * W0, dvdx * H0), np.hypot(dudy * W0, dvdy * H0))
            o.lod = np.where(valid, np.log2(rho), 0.0)                   # D3D11 7.18.11, isotropic, exact log2; before the sampler's clamp
        lod_s = o.lod if lod_for_sampling is None else np.asarray(lod_for_sampling, np.float64)
        uu, vv = np.where(valid, u, 0.5), np.where(valid, v, 0.5)
        off = 0.1                                                            # terrain_ps.hlsl:59
        hDx = trilinear(hml, lod_s, uu + off, vv) - trilinear(hml, lod_s, uu - off, vv)      # :60
        hDy = trilinear(hml, lod_s, uu, vv + off) - trilinear(hml, lod_s, uu, vv - off)      # :61
        nrm = np.stack([-hDx, np.full_like(hDx, 2.0 * off), -hDy], -1)                        # :63
        nrm = nrm / np.linalg.norm(nrm, axis=-1, keepdims=True)
        s16 = np.clip(nrm, -1.0, 1.0) * 32767.0
        o.normal_codes = np.where(s16 >= 0, np.floor(s16 + 0.5), np.ceil(s16 - 0.5)).astype(np.int64)      # RGBA16_SNORM, round half away
        o.normal = nrm
        col = trilinear(all_, lod_s, uu, vv)                                                  # :68
        enc = np.where(col <= 0.0031308, col * 12.92, 1.055 * np.maximum(col, 0.0) ** (1.0 / 2.4) - 0.055)
        o.albedo_codes = np.floor(np.clip(enc, 0.0, 1.0) * 255.0 + 0.5).astype(np.int64)     # SRGBA8, round to nearest
        o.albedo = col
        return o

    def decode_height(level):
        return level.astype(np.float64) / 255.0

    def decode_albedo(level):
        c = level[..., :3].astype(np.float64) / 255.0
        return np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)

    def bilinear(tex, uu, vv):
        th, tw = tex.shape[0], tex.shape[1]
        x, y = uu * tw - 0.5, vv * th - 0.5
        x0, y0 = np.floor(x), np.floor(y)
        fx, fy = x - x0, y - y0
        xi0 = np.clip(x0, 0, tw - 1).astype(np.int64); xi1 = np.clip(x0 + 1, 0, tw - 1).astype(np.int64)
        yi0 = np.clip(y0, 0, th - 1).astype(np.int64); yi1 = np.clip(y0 + 1, 0, th - 1).astype(np.int64)
        if tex.ndim == 3:
            fx, fy = fx[..., None], fy[..., None]
        top = tex[yi0, xi0] * (1 - fx) + tex[yi0, xi1] * fx
        bot = tex[yi1, xi0] * (1 - fx) + tex[yi1, xi1] * fx
        return top * (1 - fy) + bot * fy

    def trilinear(levels, lod, uu, vv):
        lod = np.clip(np.nan_to_num(lod, nan=0.0, posinf=64.0, neginf=0.0), 0.0, len(levels) - 1)
        l0 = np.floor(lod).astype(np.int64)
        f = lod - l0
        out = None
        for lv in range(len(levels)):
            m0, m1 = l0 == lv, (l0 + 1 == lv) & (f > 0)
            if not (m0.any() or m1.any()):
                continue
            s = bilinear(levels[lv], uu, vv)
            if out is None:
                out = np.zeros(s.shape)
            wgt = np.where(m0, 1 - f, 0.0) + np.where(m1, f, 0.0)
            out = out + s * (wgt[..., None] if s.ndim == 3 else wgt)
        return out

    hml = [decode_height(l) for l in hm_levels]
    all_ = [decode_albedo(l) for l in al_levels]
    first = shade(P_, hasP)
    for k in ("wx", "wz", "wx_tol", "wz_tol", "lod", "lod_term", "normal_codes", "normal", "albedo_codes", "albedo"):
        setattr(fr, k, getattr(first, k))
    fr.first = first
    fr.second = shade(A_, hasA & fr.either) if fr.either.any() else None
    return fr
