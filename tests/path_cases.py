"""The scenes, paths and preconditions the vr_terrain_path tests share (tests/test_path_model_cpu.py checks the preconditions on the
oracle's synthetic maps, without a device; tests/test_terrain_path_gpu.py asserts them again on the maps it runs and holds the device
to the model).

Scenes are those of tests/noise_cases.py: 64^2 + 64^2, 67x45 height + 33x50 albedo, the 2x2-surface world of 128 on 128^2 maps, and
"wide", a 512x32 heightmap (a texel an eighth of a world unit wide and two tall) over a 32^2 albedo.  They are the smallest at which a
tile edge, a partial last tile, a non-square texel and a chunked list all occur."""
import numpy as np

from tests import path_model as pm
from tests import texture_cases as tc

F = np.float32
SCENES = ("fast64", "odd", "multi", "wide")
WORLD = {n: tc.WORLD[n] for n in SCENES}
HEIGHT_OPS = (pm.LEVEL, pm.CUT, pm.FILL)
OP_IDS = {pm.LEVEL: "level", pm.CUT: "cut", pm.FILL: "fill", pm.PAINT: "paint"}
scene_maps = tc.scene_maps


def point(shape, world, tx, ty, height=0.0):
    """A control point at texel coordinate (tx, ty) of a map of `shape`."""
    h, w = shape[:2]
    return [(tx + 0.5) / w * world - world / 2, (ty + 0.5) / h * world - world / 2, height]


def scene_op(name):
    """The one heightmap op a scene other than fast64 runs."""
    return {"fast64": pm.LEVEL, "odd": pm.FILL, "multi": pm.CUT, "wide": pm.LEVEL}[name]


def bent_path(shape, world):
    """Five points, a different height at each; the bend at the third is sharper than 90 degrees (the directions in and out have a
    negative dot product), so its inside is nearer to two segments than the radius and its outside is a round cap."""
    h, w = shape[:2]
    fr = ((0.1, 0.2, 35.0), (0.5, 0.15, 110.0), (0.8, 0.5, 50.0), (0.45, 0.6, 80.0), (0.2, 0.9, 12.0))
    pts = np.float32([point(shape, world, fx * w, fy * h, hh) for fx, fy, hh in fr])
    d0, d1 = pts[2, :2] - pts[1, :2], pts[3, :2] - pts[2, :2]
    assert float(d0 @ d1) < 0.0
    return pts


def long_path(shape, world):
    """From beyond the left edge to beyond the right one, wandering over the rows: it crosses every tile column of the map."""
    h, w = shape[:2]
    xs = np.linspace(-6.0, w + 5.0, 12)
    ys = 0.5 * h + 0.3 * h * np.sin(np.arange(12) * 1.3)
    return np.float32([point(shape, world, x, y, 30.0 + 17.0 * i) for i, (x, y) in enumerate(zip(xs, ys))])


def scene_path(name, shape):
    """(points, params without op) of a scene's main path on a map of `shape`."""
    world = WORLD[name]
    if name == "wide" and shape[1] >= 8 * shape[0]:
        return long_path(shape, world), dict(radius=6.0, hardness=0.5, opacity=0.85)
    return bent_path(shape, world), dict(radius=0.08 * world, hardness=0.5, opacity=0.85)


def height_case(name, hm, op):
    pts, kw = scene_path(name, hm.shape)
    return pts, pm.params(op=op, channel_mask=1, **kw)


def albedo_case(name, al):
    """PAINT on channels 0 and 2 (mask 5)."""
    pts, kw = scene_path(name, al.shape)
    return pts, pm.params(op=pm.PAINT, color=(250.0, 33.0, 12.5, 99.0), channel_mask=5, **kw)


def zigzag(shape, world):
    """301 points - 300 segments, two chunks of the walk - zigzagging inside the tile [0, 32) x [8, 16) of a 64^2 map."""
    i = np.arange(301)
    return np.float32([point(shape, world, 6.0 + 20.0 * k / 300.0, 10.0 + 4.5 * (k % 2), 60.0 + (k * 37) % 120) for k in i])


def zigzag_params():
    return pm.params(1.5, hardness=0.3, opacity=0.9, op=pm.LEVEL)


def degenerate_cases(shape, world):
    """name -> (points, params): a closed loop, a single point, a repeated point, a path that leaves the map and comes back."""
    h, w = shape[:2]
    P = lambda tx, ty, hh: point(shape, world, tx, ty, hh)
    r = 0.06 * world
    return {
        "closed": (np.float32([P(0.2 * w, 0.2 * h, 40.0), P(0.8 * w, 0.3 * h, 120.0), P(0.6 * w, 0.8 * h, 220.0), P(0.25 * w, 0.7 * h, 90.0)]),
                   pm.params(r, 0.4, 0.9, pm.LEVEL, closed=True)),
        "single": (np.float32([P(0.4 * w, 0.55 * h, 180.0)]), pm.params(3.0 * r, 0.6, 1.0, pm.LEVEL)),
        "repeated": (np.float32([P(0.1 * w, 0.5 * h, 10.0), P(0.5 * w, 0.4 * h, 240.0), P(0.5 * w, 0.4 * h, 240.0), P(0.9 * w, 0.6 * h, 60.0)]),
                     pm.params(r, 0.2, 0.8, pm.FILL)),
        "leaves": (np.float32([P(0.3 * w, 0.7 * h, 200.0), P(0.6 * w, -0.4 * h, 100.0), P(1.5 * w, -0.5 * h, 50.0), P(1.3 * w, 0.5 * h, 30.0), P(0.7 * w, 0.6 * h, 150.0)]),
                   pm.params(r, 0.5, 1.0, pm.LEVEL)),
    }


def run_model(texels, pts, p, world):
    """(texels, rect, detail) of the model."""
    detail = {}
    out, rect = pm.path(texels, pts, p, world, detail=detail)
    return out, rect, detail


def check_preconditions(before, out, p, detail, what, every_segment=True):
    """Asserted on the model's output alone: the call can tell a wrong kernel from a right one.  At least 200 texels change; at least
    50 covered texels have f == 1 and at least 50 have 0 < f < 1; at least 10 uncovered texels lie inside the rectangle; no uncovered
    texel and no unselected channel changes; every segment index wins somewhere; t takes the value 0, the value 1 and values between;
    for CUT and for FILL at least 30 covered texels keep their byte because of the min or max, and at least 30 change.  Returns the
    counts."""
    cov, f, t, win = detail["covered"], detail["f"], detail["t"], detail["winner"]
    b3, o3 = before.reshape(cov.shape + (-1,)), out.reshape(cov.shape + (-1,))
    changed = (b3 != o3).any(-1)
    assert not changed[~cov].any(), what
    for c in range(b3.shape[2]):
        if not p["channel_mask"] >> c & 1:
            assert np.array_equal(b3[..., c], o3[..., c]), (what, c)
    x, y, w, h = detail["rect"]
    tc_ = t[cov]
    counts = dict(covered=int(cov.sum()), changed=int(changed.sum()), full=int((cov & (f == 1)).sum()), soft=int((cov & (f > 0) & (f < 1)).sum()),
                  uncovered_in_rect=int((~cov[y:y + h, x:x + w]).sum()), segments=len(detail["segments"]), winners=len(set(win[cov].tolist())),
                  t0=int((tc_ == 0).sum()), t1=int((tc_ == 1).sum()), t_between=int(((tc_ > 0) & (tc_ < 1)).sum()))
    assert counts["changed"] >= 200, (what, counts)
    assert counts["full"] >= 50 and counts["soft"] >= 50, (what, counts)
    assert counts["uncovered_in_rect"] >= 10, (what, counts)
    if every_segment:
        assert counts["winners"] == counts["segments"], (what, counts)
    assert counts["t0"] >= 1 and counts["t1"] >= 1 and counts["t_between"] >= 1, (what, counts)
    if p["op"] in (pm.CUT, pm.FILL):
        v = before.astype(F)
        held = cov & ((v <= detail["target"]) if p["op"] == pm.CUT else (v >= detail["target"]))
        counts["held"] = int(held.sum())
        assert not changed[held].any(), what
        assert counts["held"] >= 30 and int((cov & changed).sum()) >= 30, (what, counts)
    return counts
