"""Model of the query pyramid (vrenderer_amd/csrc/vr_terrain_dev.h: vr_pyramid_leaf_cell, vr_pyramid_up_cell), in numpy, written from
the contract comments of those two functions - integer arithmetic rounded outwards, so "equal to the model" means every byte.

Level 0 has (w0 + 1) x (h0 + 1) cells, indexed like the quad table: cell (ix, iz) covers the texel-centre coordinates
X0 in [ix - 1, ix], Z0 in [iz - 1, iz] and keeps (lo, hi) with lo / 255 <= H / max_height <= hi / 255 there.

    level-0 part   the four clamp-addressed texels (ix - 1, iz - 1) (ix, iz - 1) (ix - 1, iz) (ix, iz): mn0, mx0
    level-1 part   every level-1 texel a bilinear tap at a point of the cell can touch: X1 = (X0 + 1/2) w1 / w0 - 1/2 over the cell,
                   floor(X1) .. floor(X1) + 1, widened by 1/64 texel, clamped - in fp32, each operation rounded: mn1, mx1
    lo, hi         (9 mn0 + mn1) // 10, min((9 mx0 + mx1 + 9) // 10, 255)

Every further level is the min / max of 2 x 2 children, min(2 p + 1, c - 1) at ragged edges, down to 1 x 1.

`fault` plants one of the mistakes the tests must be able to see (tests/test_queries_cpu.py holds each against the true model); it is
never set by a test that looks at the device."""
import numpy as np

SLACK = 2.0 ** -14                      # slack_mh / |max_height| of k_query_rays: what the walk adds to a cell's bound
FAULTS = ("leaf swaps lo and hi", "leaf hi without + 9", "up cell without the clamp")
OFFSETS = (0.0, 0.25, 0.5, 0.75, 1.0)


def _window(n0, n1):
    """(j0, j1) per cell index 0 .. n0 of one axis: the level-1 texels the cell's taps can touch, in the kernel's fp32."""
    f = np.float32
    i = np.arange(n0 + 1).astype(f)
    r = f(n1) / f(n0)                                                   # correctly rounded, as the device's division
    m, half = f(1.0 / 64.0), f(0.5)
    j0 = np.floor(((i - half) * r - half) - m).astype(np.int64)
    j1 = np.floor(((i + half) * r - half) + m).astype(np.int64) + 1
    assert ((i - half) * r).dtype == np.float32                          # numpy keeps float32 op by op
    return np.clip(j0, 0, n1 - 1), np.clip(j1, 0, n1 - 1)


def _range_reduce(a, j0, j1, axis, fn):
    """fn over a[j0[k] .. j1[k]] along `axis` for every k (windows are a few texels wide)."""
    out = None
    for d in range(int((j1 - j0).max()) + 1):
        v = np.take(a, np.minimum(j0 + d, j1), axis=axis)
        out = v if out is None else fn(out, v)
    return out


def leaf(l0, l1, fault=None):
    """Level 0 of the pyramid of the (h, w) uint8 levels 0 and 1 (a one-level chain passes level 0 twice): (h0 + 1, w0 + 1, 2) uint8."""
    assert fault is None or fault in FAULTS
    l0, l1 = np.asarray(l0, np.uint8), np.asarray(l1, np.uint8)
    (h0, w0), (h1, w1) = l0.shape, l1.shape
    xa, xb = np.clip(np.arange(w0 + 1) - 1, 0, w0 - 1), np.clip(np.arange(w0 + 1), 0, w0 - 1)
    za, zb = np.clip(np.arange(h0 + 1) - 1, 0, h0 - 1), np.clip(np.arange(h0 + 1), 0, h0 - 1)
    t = l0.astype(np.int64)
    four = np.stack([t[za][:, xa], t[za][:, xb], t[zb][:, xa], t[zb][:, xb]])
    mn0, mx0 = four.min(0), four.max(0)
    jx0, jx1 = _window(w0, w1)
    jz0, jz1 = _window(h0, h1)
    s = l1.astype(np.int64)
    mn1 = _range_reduce(_range_reduce(s, jz0, jz1, 0, np.minimum), jx0, jx1, 1, np.minimum)
    mx1 = _range_reduce(_range_reduce(s, jz0, jz1, 0, np.maximum), jx0, jx1, 1, np.maximum)
    lo = (9 * mn0 + mn1) // 10
    hi = np.minimum((9 * mx0 + mx1 + (0 if fault == "leaf hi without + 9" else 9)) // 10, 255)
    if fault == "leaf swaps lo and hi":
        lo, hi = hi, lo
    return np.stack([lo, hi], -1).astype(np.uint8)


def up(child, fault=None):
    """The next level of a (ch, cw, 2) level: ((ch + 1) // 2, (cw + 1) // 2, 2)."""
    ch, cw = child.shape[:2]
    ph, pw = (ch + 1) // 2, (cw + 1) // 2
    z0, x0 = 2 * np.arange(ph), 2 * np.arange(pw)
    if fault == "up cell without the clamp":
        # 2 p + 1 as an address: one cell past a row's end is the next row's first cell, past the level's end the level's last (kept in bounds)
        flat = child.reshape(-1, 2)
        at = lambda z, x: flat[np.minimum(z[:, None] * cw + x[None, :], ch * cw - 1)]
        four = np.stack([at(z0, x0), at(z0, x0 + 1), at(z0 + 1, x0), at(z0 + 1, x0 + 1)])
    else:
        z1, x1 = np.minimum(z0 + 1, ch - 1), np.minimum(x0 + 1, cw - 1)
        four = np.stack([child[z0][:, x0], child[z0][:, x1], child[z1][:, x0], child[z1][:, x1]])
    return np.stack([four[..., 0].min(0), four[..., 1].max(0)], -1).astype(np.uint8)


def levels(l0, l1, fault=None):
    """Every level of the pyramid, level 0 first: a list of (ch, cw, 2) uint8 arrays ending with the 1 x 1 level."""
    out = [leaf(l0, l1, fault)]
    while out[-1].shape[:2] != (1, 1):
        out.append(up(out[-1], fault))
    return out


def chain_pair(hm):
    """(level 0, level 1) of a heightmap under the project's box-filter model (tests/f64_frontend.py); a one-texel map has one level."""
    from tests import f64_frontend as fe
    hm = np.asarray(hm, np.uint8)
    return hm, (fe.mip_r8(hm) if max(hm.shape) > 1 else hm)


# ---- the points of a leaf cell at which the surface is held to the cell's bound ----------------------------------------------------
def axis_points(n0, n1):
    """(n0 + 1, 7) texel-centre coordinates per cell index of one axis: the cell's lower end + OFFSETS, and the cell's level-1
    footprint cuts X0 = (j + 1/2) n0 / n1 - 1/2 (the first and the last inside the cell; the lower end again where there is none)."""
    i = np.arange(n0 + 1, dtype=np.float64)
    pts = [i - 1.0 + o for o in OFFSETS]
    cuts = (np.arange(n1, dtype=np.float64) + 0.5) * n0 / n1 - 0.5
    inside = (cuts[None, :] >= i[:, None] - 1.0) & (cuts[None, :] <= i[:, None])
    first = np.where(inside.any(1), cuts[np.argmax(inside, 1)], i - 1.0)
    last = np.where(inside.any(1), cuts[n1 - 1 - np.argmax(inside[:, ::-1], 1)], i - 1.0)
    return np.stack(pts + [first, last], 1)


def cell_points(w0, h0, w1, h1, world_size):
    """World (x, z) of every leaf cell's points: two float64 arrays of shape (h0 + 1, w0 + 1, 7, 7)."""
    px, pz = axis_points(w0, w1), axis_points(h0, h1)
    x = (px + 0.5) / w0 * world_size - 0.5 * world_size
    z = (pz + 0.5) / h0 * world_size - 0.5 * world_size
    return np.broadcast_to(x[None, :, None, :], (h0 + 1, w0 + 1, 7, 7)), np.broadcast_to(z[:, None, :, None], (h0 + 1, w0 + 1, 7, 7))


def excess(leaf_level, hv):
    """How far hv (heights / max_height at cell_points, shape (h0 + 1, w0 + 1, 7, 7)) leaves its cell's [lo / 255, hi / 255]: the
    largest of lo / 255 - hv and hv - hi / 255 over all points (negative: inside everywhere)."""
    lo = leaf_level[..., 0].astype(np.float64)[:, :, None, None] / 255.0
    hi = leaf_level[..., 1].astype(np.float64)[:, :, None, None] / 255.0
    hv = np.asarray(hv, np.float64)
    return float(max((lo - hv).max(), (hv - hi).max()))


# ---- the in-place refresh cases, shared by the model's self-check and the device test -------------------------------------------------
CLIP = (20, 230)                        # heights are clipped to this first, so that 0 and 255 are new extremes of the whole map


def refresh_edits(w, h):
    """(name, x, y, ew, eh) of the level-0 rectangles of a w x h map (w >= 65, h >= 19, or 64 x 64) that are filled with 255, then
    with 0, then restored: single texels at the places a refresh goes wrong, then a column, a row and an interior rectangle."""
    singles = [("(0, 0)", 0, 0), ("(w - 1, h - 1)", w - 1, h - 1), ("(w - 1, 0)", w - 1, 0),
               ("the last column alone", w - 1, 20),             # odd w: no level-1 texel reads it, the level-1 rectangle is empty
               ("the last row alone", 30, h - 1),                # odd h: likewise
               ("(31, 17)", 31, 17), ("(32, 18)", 32, 18),       # either side of a level-1 footprint boundary
               ("(63, 3)", 63, 3), (f"({min(64, w - 1)}, 4)", min(64, w - 1), 4)]      # cells on both sides of column 64 / row 4 of the 64 x 4 tiling
    return [(n, x, y, 1, 1) for n, x, y in singles] + [("a 1 x h column", w // 2 - 1, 0, 1, h), ("a w x 1 row", 0, 13, w, 1), ("7 x 9 at (3, 5)", 3, 5, 7, 9)]


def clipped(hm):
    return np.clip(np.asarray(hm, np.uint8), CLIP[0], CLIP[1]).astype(np.uint8)
