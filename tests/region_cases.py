"""The scenes, polygons and preconditions the vr_terrain_region tests share (tests/test_region_model_cpu.py checks the preconditions
on the oracle's synthetic maps, without a device; tests/test_terrain_region_gpu.py asserts them again on the maps it runs and holds
the device to the model).

Scenes are those of tests/path_cases.py: 64^2 + 64^2, 67x45 height + 33x50 albedo, the 2x2-surface world of 128 on 128^2 maps, and
"wide", a 512x32 heightmap over a 32^2 albedo.  They are the smallest at which a tile edge, a partial last tile, a non-square texel, a
tile reached by an edge far to its left and a chunked list all occur."""
import numpy as np

from tests import path_cases as pc
from tests import region_model as rm

F = np.float32
SCENES = pc.SCENES
WORLD = pc.WORLD
HEIGHT_OPS = (rm.LEVEL, rm.CUT, rm.FILL, rm.RAISE)
MODES = ("skirt", "inside", "hard")               # the default feather, VR_REGION_FEATHER_INSIDE, feather == 0
scene_maps = pc.scene_maps


def vertex(shape, world, tx, ty):
    """A vertex at texel coordinate (tx, ty) of a map of `shape`."""
    return pc.point(shape, world, tx, ty)[:2]


def scene_op(name):
    """The one heightmap op a scene other than fast64 runs."""
    return {"fast64": rm.LEVEL, "odd": rm.FILL, "multi": rm.RAISE, "wide": rm.CUT}[name]


def reflex_vertices(pts):
    """How many vertices of a simple polygon turn against its orientation."""
    p = np.asarray(pts, np.float64)
    a, b, c = np.roll(p, 1, 0), p, np.roll(p, -1, 0)
    turn = (b[:, 0] - a[:, 0]) * (c[:, 1] - b[:, 1]) - (b[:, 1] - a[:, 1]) * (c[:, 0] - b[:, 0])
    area = 0.5 * np.sum(p[:, 0] * np.roll(p[:, 1], -1) - np.roll(p[:, 0], -1) * p[:, 1])
    return int((np.sign(turn) != np.sign(area)).sum())


def concave(shape, world, x_lo=0.15, x_hi=0.85):
    """Six vertices, two of them reflex: a bow with notches in its top and bottom sides, over [x_lo, x_hi] of the map's width."""
    h, w = shape[:2]
    fr = ((0.0, 0.2), (0.5, 0.45), (1.0, 0.15), (0.93, 0.85), (0.5, 0.6), (0.07, 0.8))
    pts = np.float32([vertex(shape, world, (x_lo + fx * (x_hi - x_lo)) * w, fy * h) for fx, fy in fr])
    assert reflex_vertices(pts) == 2
    return pts


def scene_polygon(name, shape):
    """(points, feather) of a scene's main polygon on a map of `shape`; on the 512x32 map it spans every tile column."""
    world = WORLD[name]
    if name == "wide" and shape[1] >= 8 * shape[0]:
        return concave(shape, world, -0.02, 1.02), 5.0
    return concave(shape, world), 0.06 * world


def mode_params(mode, feather):
    return dict(feather=0.0 if mode == "hard" else feather, feather_inside=mode == "inside")


def height_target(hm, op):
    """A level that some of the map lies above and some below; RAISE's signed delta."""
    return -37.5 if op == rm.RAISE else float(np.median(hm)) + 0.25


def height_case(name, hm, op, mode="skirt"):
    pts, feather = scene_polygon(name, hm.shape)
    return pts, None, rm.params(op=op, target=height_target(hm, op), opacity=0.85, channel_mask=1, **mode_params(mode, feather))


def albedo_case(name, al, mode="skirt"):
    """PAINT on channels 0 and 2 (mask 5)."""
    pts, feather = scene_polygon(name, al.shape)
    return pts, None, rm.params(op=rm.PAINT, color=(250.0, 33.0, 12.5, 99.0), channel_mask=5, opacity=0.85, **mode_params(mode, feather))


def sawtooth(shape, world):
    """300 vertices - 300 edges, two chunks of the walk: 298 along a sawtooth whose teeth all cross the rows 8 .. 15 of a 64^2 map,
    closed underneath."""
    k = np.arange(298)
    top = [vertex(shape, world, 4.37 + 55.26 * i / 297.0, 5.3 if i % 2 else 18.6) for i in k]
    return np.float32(top + [vertex(shape, world, 59.63, 30.2), vertex(shape, world, 4.37, 30.2)])


def sawtooth_params():
    return rm.params(op=rm.LEVEL, target=200.0, feather=1.5, opacity=0.9)


def sawtooth_precondition(detail, shape):
    """In the tile [32, 64) x [8, 16): how many inside texels have crossings to their left from edges both below and at or above
    index 256; every edge's span meets that tile."""
    h, w = shape[:2]
    edges, k = detail["edges"], detail["prepared"]
    assert len(edges) == 300 and all(e["x0"] < 64 and e["x1"] > 32 and e["y0"] < 16 and e["y1"] > 8 for e in edges[:298])
    xs, ys = np.arange(32, 64), np.arange(8, 16)
    lo, hi = np.zeros((8, 32), bool), np.zeros((8, 32), bool)
    for i, e in enumerate(edges):
        left = rm.edge_chain(e, k, w, h, xs, ys)[0]
        if i < 256:
            lo |= left
        else:
            hi |= left
    return int((detail["inside"][8:16, 32:64] & lo & hi).sum())


def shadow_case(shape, world):
    """On the 512x32 map: a rectangle from column 100 to 400 with a feather of a few columns - its middle tiles are inside and see the
    left edge, some hundred texels away, through its span alone."""
    pts = np.float32([vertex(shape, world, 100.3, 3.4), vertex(shape, world, 400.7, 3.4), vertex(shape, world, 400.7, 28.6), vertex(shape, world, 100.3, 28.6)])
    return pts, None, rm.params(op=rm.LEVEL, target=30.0, feather=1.0, opacity=1.0)


def shadow_precondition(detail):
    """The tiles that hold inside texels at least 96 texels right of the left edge and no texel with q* < 1."""
    inside, q = detail["inside"], detail["q"]
    h, w = inside.shape
    out = []
    for ty in range(0, h, rm.TILE_H):
        for tx in range(200, w, rm.TILE_W):
            if inside[ty:ty + rm.TILE_H, tx:tx + rm.TILE_W].any() and (q[ty:ty + rm.TILE_H, tx:tx + rm.TILE_W] >= 1).all():
                out.append((tx, ty))
    return out


def shape_cases(shape, world):
    """name -> (points, contours, params): an island, a hole within a hole, a bow-tie, a polygon partly off the map on all four sides,
    a polygon that contains the whole map, a square - turned, so that its edges pass through no other - with its vertices exactly on texel centres."""
    h, w = shape[:2]
    V = lambda fx, fy: vertex(shape, world, fx * w, fy * h)
    box = lambda a, b: [V(a, a), V(b, a + 0.013), V(b - 0.011, b), V(a + 0.017, b)]
    f = 0.03 * world
    return {
        "island": (np.float32(box(0.1, 0.9) + box(0.35, 0.65)), (4, 4), rm.params(op=rm.CUT, target=20.0, feather=f, opacity=0.9)),
        "hole in hole": (np.float32(box(0.05, 0.95) + box(0.26, 0.74)[::-1] + box(0.4, 0.6)), (4, 4, 4), rm.params(op=rm.FILL, target=230.0, feather=f, opacity=1.0)),
        "bow-tie": (np.float32([V(0.11, 0.15), V(0.9, 0.86), V(0.91, 0.2), V(0.1, 0.81)]), None, rm.params(op=rm.LEVEL, target=128.0, feather=f, opacity=0.8, feather_inside=True)),
        "off all sides": (np.float32([V(0.5, -0.3), V(1.25, 0.45), V(0.55, 1.3), V(-0.2, 0.5)]), None, rm.params(op=rm.RAISE, target=60.0, feather=f, opacity=0.7)),
        "contains the map": (np.float32([V(-0.6, -0.5), V(1.7, -0.4), V(1.5, 1.6), V(-0.5, 1.8)]), None, rm.params(op=rm.RAISE, target=-45.0, feather=f, opacity=1.0)),
        "on texel centres": (np.float32([vertex(shape, world, x, y) for x, y in ((12, 9), (47, 12), (44, 47), (9, 44))]), None,
                             rm.params(op=rm.LEVEL, target=222.0, feather=0.0, opacity=1.0)),
    }


def aligned_square(shape, world):
    """An axis-aligned square with its vertices on texel centres: every texel of its outline is a tie, decided by the half-open rule.
    (All of them lie within the rounding allowance of an edge, so the exact classifier's cap leaves this case out; the CPU test writes
    its bits out instead.)"""
    return np.float32([vertex(shape, world, x, y) for x, y in ((12, 9), (50, 9), (50, 40), (12, 40))]), None, rm.params(op=rm.LEVEL, target=222.0, feather=0.0, opacity=1.0)


def run_model(texels, pts, contours, p, world, cull=False):
    """(texels, rect, detail) of the model."""
    detail = {}
    out, rect = rm.region(texels, pts, p, world, contours=contours, detail=detail, cull=cull)
    return out, rect, detail


def check_preconditions(before, out, p, detail, what):
    """Asserted on the model's output alone: the call can tell a wrong kernel from a right one.  At least 200 texels change; at least
    50 inside texels have f == 1; with a feather at least 50 covered texels have 0 < f < 1 - outside the polygon by default, inside it
    with FEATHER_INSIDE - and without one every covered texel has f == 1 and is inside; at least 10 uncovered texels lie inside the
    rectangle; no uncovered texel and no unselected channel changes; for CUT and for FILL at least 30 covered texels keep their byte
    because of the min or max, and at least 30 change.  Returns the counts."""
    cov, f, ins = detail["covered"], detail["f"], detail["inside"]
    b3, o3 = before.reshape(cov.shape + (-1,)), out.reshape(cov.shape + (-1,))
    changed = (b3 != o3).any(-1)
    assert not changed[~cov].any(), what
    for c in range(b3.shape[2]):
        if not p["channel_mask"] >> c & 1:
            assert np.array_equal(b3[..., c], o3[..., c]), (what, c)
    x, y, w, h = detail["rect"]
    soft = cov & (f > 0) & (f < 1)
    counts = dict(covered=int(cov.sum()), inside=int(ins.sum()), changed=int(changed.sum()), full=int((ins & (f == 1)).sum()), soft=int(soft.sum()),
                  soft_inside=int((soft & ins).sum()), uncovered_in_rect=int((~cov[y:y + h, x:x + w]).sum()), edges=len(detail["edges"]))
    assert counts["changed"] >= 200 and counts["full"] >= 50 and counts["uncovered_in_rect"] >= 10, (what, counts)
    if p["feather"] == 0.0:
        assert counts["soft"] == 0 and np.array_equal(cov, ins), (what, counts)
    elif p["feather_inside"]:
        assert counts["soft_inside"] >= 50 and counts["soft"] == counts["soft_inside"] and np.array_equal(cov, ins), (what, counts)
    else:
        assert counts["soft"] >= 50 and counts["soft_inside"] == 0, (what, counts)
    if p["op"] in (rm.CUT, rm.FILL):
        v = before.astype(F)
        held = cov & ((v <= F(p["target"])) if p["op"] == rm.CUT else (v >= F(p["target"])))
        counts["held"] = int(held.sum())
        assert not changed[held].any(), what
        assert counts["held"] >= 30 and int((cov & changed).sum()) >= 30, (what, counts)
    return counts


def all_cases(synth_heightmap, synth_albedo):
    """(what, which, texels, world, points, contours, params, kind) of every call the GPU tests make against the model; kind 'main'
    cases meet check_preconditions, the others their own."""
    out = []
    for name in SCENES:
        hm, al = scene_maps(name, synth_heightmap, synth_albedo)
        S = WORLD[name]
        if name == "fast64":
            for op in HEIGHT_OPS:
                for mode in MODES:
                    out.append((f"{name} {rm.OP_IDS[op]} {mode}", "height", hm, S, *height_case(name, hm, op, mode), "main"))
        else:
            out.append((f"{name} {rm.OP_IDS[scene_op(name)]}", "height", hm, S, *height_case(name, hm, scene_op(name)), "main"))
        out.append((f"{name} paint", "albedo", al, S, *albedo_case(name, al), "main"))
    hm, _ = scene_maps("fast64", synth_heightmap, synth_albedo)
    out.append(("sawtooth", "height", hm, 64.0, sawtooth(hm.shape, 64.0), None, sawtooth_params(), "sawtooth"))
    wide, _ = scene_maps("wide", synth_heightmap, synth_albedo)
    out.append(("shadow", "height", wide, WORLD["wide"], *shadow_case(wide.shape, WORLD["wide"]), "shadow"))
    for what, (pts, contours, p) in shape_cases(hm.shape, 64.0).items():
        out.append((what, "height", hm, 64.0, pts, contours, p, "shape"))
    out.append(("aligned on texel centres", "height", hm, 64.0, *aligned_square(hm.shape, 64.0), "aligned"))
    return out
