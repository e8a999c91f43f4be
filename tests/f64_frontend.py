"""An exact / float64 model of the geometry front end - mip chains, QuadTree::SetHeight, QuadTree::NodeSelect and main_vs -
written from the reference's text (QuadTree.cpp, QuadTree.h, TerrainPass.cpp, shaders/terrain/terrain_vs.hlsl) and the
D3D / Donut rules DESIGN.md section 2 cites, NOT from oracle/vr_oracle.c or the kernels.

Test infrastructure.  tests/test_frontend_cpu.py holds the C oracle to this file, tests/test_frontend_f64.py the HIP
kernels (k_derive_mip_*, k_node_heights_*, k_derive_minmax_*, k_select, k_vertex).  What is taken as given:
  - the level-0 textures, the terrain parameters and the view as the caller hands them over in fp32: the two matrices, the
    six planes (outward normal, distance) and the camera position;
  - the numbering of nodes (include/vrterrain.h: id = (4^d - 1) / 3 + iz 2^d + ix, surfaces one tree after the other) and
    the 112-byte InstanceData layout (TerrainPass.cpp:245-249 with Donut's affineToColumnMajor: rows (ex 0 0 px),
    (0 ey 0 py), (0 0 ez pz));
  - the height surface of tests/f64_queries.py (Surface64: SampleLevel at 0.1 = 0.9 level 0 + 0.1 level 1, linear clamp).
Every bound below is a forward error bound of the fp32 expression the text implies, with u = 2^-24 and
gamma_n = n u / (1 - n u); none carries an empirical margin.  The worlds the tests use have dyadic node extents (surface
sizes that are powers of two, or 200 = 25 * 8 whose halvings stay exact in fp32 down to the leaves), so node boxes,
gridExtents = 2 sqrt(ex^2) and int(log2(gridExtents)) are exact and not themselves in question.
"""
from fractions import Fraction

import numpy as np

from tests.f64_queries import Surface64, ulp32  # noqa: F401  (Surface64 is re-exported for the tests)

U = 2.0 ** -24
MAX_LODS = 12                                      # QuadTree.h:67
GRID = 32                                          # GRID_SIZE (TerrainPass.cpp:52-66): 33 x 33 vertices at (w / 16, 0, h / 16)


def gamma(n):
    return n * U / (1.0 - n * U)


# ---- mip chains --------------------------------------------------------------------------------------------------------
def _quad(level):
    """The four texels of every 2 x 2 box of `level` ((h, w) or (h, w, c)); the last row / column is clamped at odd sizes
    and a side of one texel stays one texel (Donut's mip generation, 2 x 2 box blits)."""
    h, w = level.shape[:2]
    dh, dw = max(h >> 1, 1), max(w >> 1, 1)
    y0, x0 = 2 * np.arange(dh), 2 * np.arange(dw)
    y1, x1 = np.minimum(y0 + 1, h - 1), np.minimum(x0 + 1, w - 1)
    return level[y0][:, x0], level[y0][:, x1], level[y1][:, x0], level[y1][:, x1]


def mip_r8(level):
    """Next level of an R8 (or alpha) plane: round-half-up of the mean of four, in integers - exact."""
    a, b, c, d = (q.astype(np.int64) for q in _quad(level))
    return ((a + b + c + d + 2) >> 2).astype(np.uint8)


def eotf(c):
    return np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)


def oetf(x):
    return np.where(x <= 0.0031308, x * 12.92, 1.055 * np.maximum(x, 0.0) ** (1.0 / 2.4) - 0.055)


MIP_EPS = gamma(4)


def mip_srgb(level):
    """Next level of the colour channels of an sRGBA8 texture: (lo, hi) uint8 codes per texel; lo == hi where the code is
    decided, else the texel is flagged and may hold either.

    The level is the mean of the four EOTF values, encoded by the round-to-nearest OETF.  The fp32 evaluation decodes each
    texel through a table entry rounded once (1 + d), adds four of them with three additions - an entry passes through at
    most three of them in any order - and scales by 0.25, which is exact: mean32 = mean (1 + t), |t| <= gamma_4 (n = 1 + 3).
    The code is a monotone function of the mean, so it is decided when 255 OETF(mean (1 - gamma_4)) and
    255 OETF(mean (1 + gamma_4)) round to the same integer; float64's own error (2^-53 per operation) is 2^-28 of that."""
    a, b, c, d = (eotf(q[..., :3].astype(np.float64) / 255.0) for q in _quad(level))
    mean = ((a + b) + (c + d)) * 0.25
    lo = np.floor(255.0 * oetf(mean * (1.0 - MIP_EPS)) + 0.5)
    hi = np.floor(255.0 * oetf(mean * (1.0 + MIP_EPS)) + 0.5)
    return np.clip(lo, 0, 255).astype(np.uint8), np.clip(hi, 0, 255).astype(np.uint8)


def check_mip(prev, got, srgb):
    """Compares one level `got` with the model applied to `prev` (the level below, as the same implementation holds it).
    Returns dict(bad = texel components that are wrong, flagged = share of colour components the model leaves open)."""
    if not srgb:
        want = mip_r8(prev)
        assert got.shape == want.shape, (got.shape, want.shape)
        return dict(bad=int((got != want).sum()), flagged=0.0)
    lo, hi = mip_srgb(prev)
    alpha = mip_r8(prev[..., 3])
    assert got.shape[:2] == alpha.shape, (got.shape, alpha.shape)
    g = got[..., :3]
    bad = int(((g != lo) & (g != hi)).sum()) + int((got[..., 3] != alpha).sum())
    return dict(bad=bad, flagged=float((lo != hi).mean()))


def num_mip_levels(w, h):
    return int(np.floor(np.log2(max(w, h)))) + 1


# ---- the tree ----------------------------------------------------------------------------------------------------------
def level_base(d):
    return ((1 << (2 * d)) - 1) // 3


class Tree:
    """Geometry of the quadtrees TerrainPass::Init builds (TerrainPass.cpp:97-110) and QuadTree::Split refines
    (QuadTree.cpp:210-232): a node at depth d, column ix, row iz of surface s has half-extent S / 2^(d+1) and centre
    loc_s - S/2 + (2 i + 1) S / 2^(d+1) per axis; TL / TR are the +z children, TR / BR the +x ones (:213-216)."""

    def __init__(self, surface_size, world_size, location=(0.0, 0.0, 0.0)):
        self.S, self.W = float(surface_size), float(world_size)
        self.num_lods = min(MAX_LODS - 1, int(np.floor(np.log2(self.S))))          # QuadTree.cpp:22
        self.per_side = int(self.W) // int(self.S)
        self.nodes_per_tree = level_base(self.num_lods + 1)
        self.num_nodes = self.nodes_per_tree * self.per_side ** 2
        self.loc = []
        for i in range(self.per_side ** 2):
            col, row = i % self.per_side, i // self.per_side
            x, y = -0.5 * (self.per_side - 1) + col, -0.5 * (self.per_side - 1) + row    # TerrainPass.cpp:105-108
            self.loc.append((location[0] + x * self.S, location[1], location[2] + y * self.S))
        e = self.S / 2.0 ** (self.num_lods + 1)
        assert e * 2.0 ** 20 == np.floor(e * 2.0 ** 20) and self.S < 2.0 ** 12, "node extents must be exact in fp32"

    def ext(self, d):
        return self.S / 2.0 ** (d + 1)

    def centres(self, s, d):
        """(cx[ix], cz[iz]) of depth d of surface s."""
        k = (2.0 * np.arange(1 << d) + 1.0) * self.ext(d)
        return self.loc[s][0] - 0.5 * self.S + k, self.loc[s][2] - 0.5 * self.S + k


def lod_ranges(min_lod_distance=4.0):
    return [min_lod_distance * 2.0 ** i for i in range(MAX_LODS)]                    # QuadTree.cpp:234-241


# ---- SetHeight ---------------------------------------------------------------------------------------------------------
def _limits(lo_w, width, texel):
    """QuadTree.cpp:166-173 on one axis for a row of nodes: the exact values of minV = (centre - width/2 + W/2) texel and
    maxV = minV + width texel, the footprint [floor(minV), ceil(maxV)) and the alternatives within the fp32 rounding.

    lo_w = centre - width/2 + W/2 and width are exact in fp32 (dyadic); texel is the fp32 member m_TexelSize (:29), taken as
    stored.  Both products have at most 24 + 13 bits, so float64 holds minV, width texel and their sum exactly.  In fp32
    minV is one product: off by at most u |minV|, and by nothing when the exact value is an fp32 number.  maxV adds a second
    product (u |width texel|, or nothing) and one addition (u |maxV|, or nothing when both parts were exact and the sum is
    an fp32 number).  floor / ceil is in question when an integer lies within that distance."""
    f32 = lambda v: v.astype(np.float32).astype(np.float64)
    mn = lo_w * texel
    wt = width * texel
    mx = mn + wt
    e_mn = np.where(f32(mn) == mn, 0.0, U * np.abs(mn))
    e_wt = U * abs(wt) if float(np.float32(wt)) != wt else 0.0
    e_mx = e_mn + e_wt
    e_mx = np.where((e_mx == 0.0) & (f32(mx) == mx), 0.0, (e_mx + U * np.abs(mx)) * (1.0 + 4 * U))
    a0, a1 = np.floor(mn - e_mn).astype(np.int64), np.floor(mn + e_mn).astype(np.int64)
    b0, b1 = np.ceil(mx - e_mx).astype(np.int64), np.ceil(mx + e_mx).astype(np.int64)
    return (np.floor(mn).astype(np.int64), np.ceil(mx).astype(np.int64)), (a0, a1, b0, b1)


def _range_minmax(E, ox, oy, x0, x1, y0, y1):
    """min and max byte of E over [x0[i], x1[i]) x [y0[j], y1[j]) for every (j, i); E's origin is texel (ox, oy).  An empty
    range gives (256, -1) as the reference's (+inf, -inf)."""
    def seg(a, lo, hi, axis, fn, empty):
        idx = np.stack([lo, np.maximum(hi, lo)], 1).ravel()
        r = np.take(fn.reduceat(a, idx, axis=axis), np.arange(0, idx.size, 2), axis=axis)
        shape = [1, 1]; shape[axis] = -1
        return np.where((hi <= lo).reshape(shape), empty, r)
    mn = seg(seg(E, x0 - ox, x1 - ox, 1, np.minimum, 256), y0 - oy, y1 - oy, 0, np.minimum, 256)
    mx = seg(seg(E, x0 - ox, x1 - ox, 1, np.maximum, -1), y0 - oy, y1 - oy, 0, np.maximum, -1)
    return mn, mx


def _finish(mn, mx):
    """QuadTree.cpp:186 and :193-198 from the integer bytes: (pos.y, ext.y) as the exact rationals (mn + mx) / 510 and
    (mx - mn) / 510 (one float64 division each, 2^-53), and their fp32 bounds.

    The text divides each byte by 255 (correctly rounded: u mn', u mx' with mn' = mn / 255), sets min to 0 when max - min is
    0, subtracts (u |mx' - mn'|), halves (exact) and adds min (u |pos|):
        |d ext| <= u (mn' + mx') / 2 + u ext,      |d pos| <= u mn' + |d ext| + u pos.
    With all values in [0, 1] that is at most 1.5 u = 1.5 ulp32 at 1/2 for ext and 3.5 u for pos; the per-node formula is
    what is asserted."""
    mn = np.where(mn == mx, 0, mn).astype(np.float64)
    mx = mx.astype(np.float64)
    ext, pos = (mx - mn) / 510.0, (mx + mn) / 510.0
    t_ext = U * (mn + mx) / 510.0 + U * np.abs(ext) + 2.0 ** -52
    t_pos = U * mn / 255.0 + t_ext + U * np.abs(pos) + 2.0 ** -52
    return pos, ext, t_pos, t_ext


class NodeHeights:
    pass


def set_height(tree, tex, world_size=None):
    """QuadTree::SetHeight over every node of every surface (QuadTree.cpp:153-208).  Returns a NodeHeights with, per node id:
    pos, ext (float64 of the exact rationals), t_pos, t_ext (fp32 bounds), mn, mx (bytes; the reference's +-inf of an empty
    footprint appear as 256 / -1 and their pos / ext as nan), flagged, and alt: for a flagged node the list of (pos, ext,
    t_pos, t_ext) of every footprint within the rounding.

    GetHeightValue's flat index x + y w (:157) is kept, clamped to the array: a column outside [0, w) reads the neighbouring
    row.  The index is formed in fp32, exact while w h <= 2^24 - asserted."""
    H, Wt = tex.shape
    assert H * Wt <= 1 << 24
    ws = tree.W if world_size is None else float(world_size)
    tx, tz = float(np.float32(Wt) / np.float32(ws)), float(np.float32(H) / np.float32(ws))          # QuadTree.cpp:29
    flat = tex.ravel()
    out = NodeHeights()
    n = tree.num_nodes
    out.pos, out.ext, out.t_pos, out.t_ext = (np.zeros(n) for _ in range(4))
    out.mn, out.mx = np.zeros(n, np.int64), np.zeros(n, np.int64)
    out.flagged = np.zeros(n, bool)
    out.alt = {}
    for s in range(tree.per_side ** 2):
        for d in range(tree.num_lods + 1):
            cx, cz = tree.centres(s, d)
            width = 2.0 * tree.ext(d)
            (x0, x1), ax = _limits(cx - width / 2 + ws / 2, width, tx)
            (y0, y1), ay = _limits(cz - width / 2 + ws / 2, width, tz)
            ox, oy = int(min(ax[0].min(), ax[1].min())), int(min(ay[0].min(), ay[1].min()))
            ex, ey = int(max(ax[2].max(), ax[3].max())) + 1, int(max(ay[2].max(), ay[3].max())) + 1
            if ox >= 0 and oy >= 0 and ex <= Wt + 1 and ey <= H + 1 and int(max(ax[2].max(), ax[3].max())) <= Wt \
                    and int(max(ay[2].max(), ay[3].max())) <= H:
                E = np.pad(tex[oy:ey, ox:ex].astype(np.int16), ((0, ey - min(ey, H)), (0, ex - min(ex, Wt))))    # padding is never read
            else:
                idx = np.arange(ox, ex)[None, :] + np.arange(oy, ey)[:, None] * Wt
                E = flat[np.clip(idx, 0, flat.size - 1)].astype(np.int16)
            mn, mx = _range_minmax(E, ox, oy, x0, x1, y0, y1)
            base = s * tree.nodes_per_tree + level_base(d)
            sl = slice(base, base + (1 << (2 * d)))
            out.mn[sl], out.mx[sl] = mn.ravel(), mx.ravel()
            with np.errstate(invalid="ignore"):
                vals = _finish(mn, mx)
            empty = (mx < 0).ravel()
            for arr, v in zip((out.pos, out.ext, out.t_pos, out.t_ext), vals):
                arr[sl] = np.where(empty, np.nan, v.ravel())
            fx = (ax[0] != ax[1]) | (ax[2] != ax[3])
            fy = (ay[0] != ay[1]) | (ay[2] != ay[3])
            fl = fy[:, None] | fx[None, :]
            if fl.any():
                out.flagged[sl] = fl.ravel()
                alts = []
                for xa in (ax[0], ax[1]):
                    for xb in (ax[2], ax[3]):
                        for ya in (ay[0], ay[1]):
                            for yb in (ay[2], ay[3]):
                                m0, m1 = _range_minmax(E, ox, oy, xa, xb, ya, yb)
                                alts.append([v.ravel() for v in _finish(m0, m1)])
                for k in np.nonzero(fl.ravel())[0]:
                    out.alt[base + int(k)] = [tuple(float(v[k]) for v in a) for a in alts]
    return out


def check_node_heights(model, got):
    """got: (n, 2) fp32 (pos.y, ext.y).  Returns dict(bad, worst = largest |error| / bound over unflagged nodes, flagged)."""
    got = np.asarray(got, np.float64)
    with np.errstate(invalid="ignore"):
        rp = np.abs(got[:, 0] - model.pos) / model.t_pos
        re = np.abs(got[:, 1] - model.ext) / model.t_ext
    ok = (rp <= 1.0) & (re <= 1.0)
    ok |= np.isnan(model.pos) & ~np.isfinite(got).all(1)              # an empty footprint keeps the reference's infinities
    for k, alts in model.alt.items():
        ok[k] = any(abs(got[k, 0] - p) <= tp and abs(got[k, 1] - e) <= te for p, e, tp, te in alts)
    free = ~model.flagged & ~np.isnan(model.pos)
    return dict(bad=int((~ok).sum()), first=np.nonzero(~ok)[0][:4].tolist(), flagged=float(model.flagged.mean()),
                worst=float(max(rp[free].max(initial=0.0), re[free].max(initial=0.0))))


# ---- NodeSelect --------------------------------------------------------------------------------------------------------
class Selection:
    pass


def node_select(tree, view, max_height, heights=None, ranges=None, strict=False, capacity=None):
    """TerrainPass.cpp:176-187 + QuadTree::NodeSelect (QuadTree.cpp:80-131) + Node::Intersects (QuadTree.h:31-45) +
    dm::frustum::intersectsWith(box3) (per plane the box corner nearest the inside - min where the outward
    normal is positive, else max - and out when n . corner - d > 0), in exact rational arithmetic on the fp32 inputs.

    heights: a NodeHeights for m_HeightLoaded = true (:87-91: y = (pos.y -+ ext.y) maxHeight), None for false (:92-96: y in
    [0, camera.y]).  strict: True or the uses ("range_first", "range_finer") whose squared distance is compared with `<` -
    not the reference; the CPU tests use it to show that the tie views tell the two apart.

    Every decision records its margin against tau, the forward error of the fp32 expression:
      range: dot(d, d) <= r^2 with d = position - edge per axis (one subtraction), three products of which one is 0 0, two
        additions: every term carries 2 (subtraction, squared) + 1 (product) + 2 (additions) roundings: tau = gamma_5 (dx^2 +
        dz^2).  r^2 = (4 2^i)^2 is exact.
      plane: n . p - d: three products, two additions, one subtraction: tau = gamma_4 (sum |n_i p_i| + |d|), n = 1 + 3.  With
        heights loaded p.y = (pos.y -+ ext.y) maxHeight carries SetHeight's bounds, one addition and one product:
        tau += |n_y| (maxHeight (t_pos + t_ext) + 2 u |p.y|).
    A margin of exactly zero is decided (`<=` holds, `> 0` does not); a non-zero margin below tau makes the view ambiguous
    (`why` lists those decisions).  Returns a Selection: count, ids, fields (ex, ey, ez, px, py, pz per instance), tol_y, ambiguous,
    ties (zero-margin decisions by kind) and decisions."""
    ranges = ranges or lod_ranges()
    F = Fraction
    cam = [F(float(view.camera_pos[k])) for k in range(3)]
    planes = [[float(view.planes[i][k]) for k in range(4)] for i in range(6)]
    mh = F(float(np.float32(max_height)))
    out = Selection()
    out.ambiguous, out.ties, out.decisions, out.why = 0, dict(range_first=0, range_finer=0, plane=0), 0, []
    sel = []

    def in_range(box, lod, use):
        (x0, x1), (z0, z1) = box
        dx = cam[0] - x0 if cam[0] < x0 else (cam[0] - x1 if cam[0] > x1 else F(0))
        dz = cam[2] - z0 if cam[2] < z0 else (cam[2] - z1 if cam[2] > z1 else F(0))
        s, r2 = dx * dx + dz * dz, F(ranges[lod]) ** 2
        margin = abs(s - r2)
        out.decisions += 1
        if margin == 0:
            out.ties[use] += 1
        elif margin < gamma(5) * s:
            out.ambiguous += 1
            out.why.append(("range", use, float(s), float(r2)))
        return s < r2 if (strict is True or (strict and use in strict)) else s <= r2

    def in_frustum(box, y0, y1, ty0, ty1):
        (x0, x1), (z0, z1) = box
        for pl in planes:
            py, ty = (y0, ty0) if pl[1] > 0.0 else (y1, ty1)
            p = (x0 if pl[0] > 0.0 else x1, py, z0 if pl[2] > 0.0 else z1)
            terms = [F(pl[k]) * p[k] for k in range(3)]
            dist = sum(terms) - F(pl[3])
            tau = gamma(4) * float(sum(abs(t) for t in terms) + abs(F(pl[3]))) + abs(pl[1]) * ty
            out.decisions += 1
            if dist == 0:
                out.ties["plane"] += 1
            elif abs(dist) < tau:
                out.ambiguous += 1
                out.why.append(("plane", pl, tuple(float(c) for c in p), float(dist), tau))
            if dist > 0:
                return False
        return True

    def visit(s, d, ix, iz):
        lod = tree.num_lods - d
        e = F(tree.ext(d))
        cx = F(tree.loc[s][0]) - F(tree.S) / 2 + (2 * ix + 1) * e
        cz = F(tree.loc[s][2]) - F(tree.S) / 2 + (2 * iz + 1) * e
        box = ((cx - e, cx + e), (cz - e, cz + e))
        nid = s * tree.nodes_per_tree + level_base(d) + iz * (1 << d) + ix
        if not in_range(box, lod, "range_first"):                                   # :82
            return False, nid
        if heights is not None:                                                     # :87-91
            lo = 0 if heights.mn[nid] == heights.mx[nid] else int(heights.mn[nid])
            y0, y1 = F(lo, 255) * mh, F(int(heights.mx[nid]), 255) * mh
            t = float(mh) * (heights.t_pos[nid] + heights.t_ext[nid])
            ty0, ty1 = t + 2 * U * abs(float(y0)), t + 2 * U * abs(float(y1))
        else:                                                                       # :92-96
            y0, y1, ty0, ty1 = F(0), cam[1], 0.0, 0.0
        if not in_frustum(box, y0, y1, ty0, ty1):                                   # :99-103
            return True, nid
        if lod == 0 or not in_range(box, lod - 1, "range_finer"):                   # :105-117
            sel.append((nid, s, d, ix, iz))
            return True, nid
        for cix, ciz in ((2 * ix, 2 * iz + 1), (2 * ix + 1, 2 * iz + 1), (2 * ix, 2 * iz), (2 * ix + 1, 2 * iz)):   # TL TR BL BR
            hit, cid = visit(s, d + 1, cix, ciz)
            if not hit:                                                             # :122-126: out of range, no frustum test
                sel.append((cid, s, d + 1, cix, ciz))
        return True, nid

    for s in range(tree.per_side ** 2):                                             # TerrainPass.cpp:176-186
        visit(s, 0, 0, 0)
    out.count = len(sel)
    cap = len(sel) if capacity is None else min(capacity, len(sel))
    out.ids = np.array([r[0] for r in sel[:cap]], np.uint32)
    # UpdateTransforms (TerrainPass.cpp:234-256): scaling(extents) * translation(position); the rest of InstanceData is 0, 0, 1, 0
    out.fields = np.zeros((cap, 6))                                                 # ex, ey, ez, px, py, pz
    out.tol_y = np.zeros((cap, 2))                                                  # bounds of ey, py
    for k, (nid, s, d, ix, iz) in enumerate(sel[:cap]):
        e = tree.ext(d)
        px = tree.loc[s][0] - tree.S / 2 + (2 * ix + 1) * e
        pz = tree.loc[s][2] - tree.S / 2 + (2 * iz + 1) * e
        if heights is not None:
            ey, py, out.tol_y[k] = heights.ext[nid], heights.pos[nid], (heights.t_ext[nid], heights.t_pos[nid])
        else:
            ey, py = 0.0, tree.loc[s][1]
        out.fields[k] = (e, ey, e, px, py, pz)
    return out


def instance_fields(inst_bytes):
    """(ex, ey, ez, px, py, pz) and the untouched rest of (n, 112) InstanceData bytes."""
    f = np.ascontiguousarray(inst_bytes).view(np.float32).reshape(-1, 28)
    u = np.ascontiguousarray(inst_bytes).view(np.uint32).reshape(-1, 28)
    t = f[:, 4:16].astype(np.float64)
    fields = t[:, [0, 5, 10, 3, 7, 11]]
    rest_zero = (np.delete(t, [0, 5, 10, 3, 7, 11], axis=1) == 0).all() and (u[:, [0, 1, 2]] == 0).all() and (u[:, 3] == 1).all() \
        and (u[:, 16:] == 0).all()
    return fields, bool(rest_zero)


def check_selection(model, n, ids, inst_bytes):
    """None when (n, ids, instances) is the model's selection, else what differs."""
    if n != model.count:
        return f"count {n} != {model.count}"
    if not np.array_equal(ids, model.ids):
        k = int(np.argmax(ids != model.ids))
        return f"ids differ first at {k}: {ids[k]} != {model.ids[k]}"
    fields, rest = instance_fields(inst_bytes)
    if not rest:
        return "InstanceData fields other than the transform's scale and translation are not 0, 0, 1, 0"
    if not np.array_equal(fields[:, [0, 2, 3, 5]], model.fields[:, [0, 2, 3, 5]]):
        return "instance xz scale / translation differ"
    dy = np.abs(fields[:, [1, 4]] - model.fields[:, [1, 4]])
    if not (dy <= model.tol_y).all():
        return f"instance y scale / translation off by {float((dy / np.maximum(model.tol_y, 1e-300)).max()):.2f} x bound"
    return None


# ---- main_vs -----------------------------------------------------------------------------------------------------------
def main_vs(fields, view, surf, ranges=None, morph_start=np.float32(0.85)):
    """terrain_vs.hlsl:10-62 for all 1,089 grid vertices of one instance in float64, with a bound per output.

    fields: (ex, ey, ez, px, py, pz) of the instance; surf: the Surface64 (its world size and max height are the constants of
    :29-32).  Returns dict(xz (1089, 2), h, clip (1089, 4), morph, uv, t_xz, t_h, t_clip (1089, 4)); vertex index = vz 33 + vx.

      :44 world = M (pos, 1): one product and one addition per axis (the product with pos.y = 0 is exact): t0 = gamma_2 (|e p| +
        |c|) - zero in fact on dyadic worlds, kept for the general case.
      :46 distance = length(world.xz - camera.xz): two subtractions (u), two squares (u), one addition (u), one square root
        (halves what came before, adds u): |d dist| <= (2.5 u) dist + sqrt(2) t0 <= 3 u dist + sqrt(2) t0.
      :47 gridExtents = 2 sqrt(ex^2) = 2 ex exactly; :18 lod = int(log2(gridExtents)) exactly (dyadic extents).
      :20-23 start = range 0.85f (u start); delta = end - start is exact by Sterbenz (start in [end / 2, end]) but inherits
        start's error; morph = (distance - start) / delta: subtraction u |num|, division u |morph|:
            |d morph| <= (|d dist| + u start + u |num|) / delta + |morph| (u start / delta) + u |morph|  =: t_k,
        the cancellation in distance - start divided by end - start.  saturate is continuous, so t_k bounds morphK too; where
        morph -+ t_k lies wholly outside [0, 1] morphK is exactly 0 or 1.
      :12-13 fracPart = frac(gridPos 16) 2 / 32 is 0 or 1/32 exactly, fracPart gridExtents = one grid step, exactly; times
        morphK (u) and subtracted (u): t_xz = t0 + step (t_k + u morphK) + u |xz|.
      :27-33 height: Surface64.height_tol at the model's xz plus the slope bound times |t_xz|.
      :60-61 two row-vector products, four products and three additions per component: gamma_4 sum |terms| (n = 1 + 3) plus the
        matrix's absolute values applied to the bound of the vector that goes in."""
    ranges = ranges or lod_ranges()
    ex, ey, ez, px, py, pz = (float(v) for v in fields)
    g = (np.arange(GRID + 1) - GRID // 2) / (GRID / 2.0)                             # TerrainPass.cpp:58-66
    gx, gz = np.meshgrid(g, g)                                                      # index = vz 33 + vx
    gx, gz = gx.ravel(), gz.ravel()
    wx0, wz0 = ex * gx + px, ez * gz + pz
    t0x, t0z = gamma(2) * (np.abs(ex * gx) + abs(px)), gamma(2) * (np.abs(ez * gz) + abs(pz))
    t0x = np.where(wx0.astype(np.float32) == wx0, 0.0, t0x); t0z = np.where(wz0.astype(np.float32) == wz0, 0.0, t0z)
    cx, cz = float(view.camera_pos[0]), float(view.camera_pos[2])                   # matViewToWorld[3].xz
    dist = np.hypot(wx0 - cx, wz0 - cz)
    t_dist = 3.0 * U * dist + np.hypot(t0x, t0z)
    ge = 2.0 * ex
    lod = int(np.clip(int(np.floor(np.log2(ge))), 0, 11))
    end = float(ranges[lod])
    start = end * float(morph_start)
    delta = end - start
    num = dist - start
    morph = num / delta
    t_k = (t_dist + U * start + U * np.abs(num)) / (delta - U * start) + np.abs(morph) * (U * start / (delta - U * start)) + U * np.abs(morph)
    k = np.clip(morph, 0.0, 1.0)
    t_k = np.where((morph - t_k > 1.0) | (morph + t_k < 0.0), 0.0, t_k)
    gpx, gpz = (gx + 1.0) * 0.5, (gz + 1.0) * 0.5                                   # :49
    fx = (gpx * GRID * 0.5) % 1.0 * 2.0 / GRID                                      # :12
    fz = (gpz * GRID * 0.5) % 1.0 * 2.0 / GRID
    x, z = wx0 - fx * ge * k, wz0 - fz * ge * k                                     # :13
    t_x = t0x + fx * ge * (t_k + U * k) + U * np.abs(x)
    t_z = t0z + fz * ge * (t_k + U * k) + U * np.abs(z)
    h = surf.H(x, z)                                                                # :27-33
    t_h = surf.height_tol(x, z) + surf.slope_bound(x, z) * np.hypot(t_x, t_z)
    W2V = np.array(view.world_to_view[:], np.float64).reshape(4, 4)
    V2C = np.array(view.view_to_clip[:], np.float64).reshape(4, 4)
    world = np.stack([x, h, z, np.ones_like(x)], 1)
    t_world = np.stack([t_x, t_h, t_z, np.zeros_like(x)], 1)
    vpos = world @ W2V                                                              # :60
    t_v = gamma(4) * (np.abs(world) @ np.abs(W2V)) + t_world @ np.abs(W2V)
    clip = vpos @ V2C                                                               # :61
    t_c = gamma(4) * (np.abs(vpos) @ np.abs(V2C)) + t_v @ np.abs(V2C)
    half = 0.5 * surf.ws
    return dict(xz=np.stack([x, z], 1), h=h, clip=clip, morph=k, uv=np.stack([(x + half) / surf.ws, (z + half) / surf.ws], 1),
                t_xz=np.stack([t_x, t_z], 1), t_h=t_h, t_clip=t_c, odd=(fx > 0) | (fz > 0))


def _ratio(err, tol):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(err == 0.0, 0.0, err / tol)


def check_vertices(m, clip, xz, height=None):
    """Worst |error| / bound of an implementation's outputs for one instance: dict(xz, clip, h)."""
    r = dict(xz=float(_ratio(np.abs(np.asarray(xz, np.float64) - m["xz"]), m["t_xz"]).max()),
             clip=float(_ratio(np.abs(np.asarray(clip, np.float64) - m["clip"]), m["t_clip"]).max()))
    if height is not None:
        r["h"] = float(_ratio(np.abs(np.asarray(height, np.float64) - m["h"]), m["t_h"]).max())
    return r
