"""The scenes, calls and preconditions the vr_terrain_occlusion tests share (tests/test_occlusion_model_cpu.py checks the preconditions
on the oracle's synthetic maps, without a device; tests/test_terrain_occlusion_gpu.py asserts them again on the maps it runs and holds
the device to the model).

Scenes are tests/texture_cases.py's five.  The radius is 8 world units unless a case says otherwise: 8 height texels on fast64 and
multi, 8 by 5 on odd, 32 on fine and 64 by 4 on wide.  Which path the kernel takes is worked out here by the host's own arithmetic
(staged): the tile's footprint - (ceil(32 w0 / wa) + 1 + 2 reach_x) x (ceil(8 h0 / ha) + 1 + 2 reach_z) bytes - is staged in LDS where it
is at most 32 KiB; fine's is not, at either radius, so fine is the scene of the direct loads.

A call is the tuple (heightmap, dabs or None, parameters, whole_map, max_height) - what tests/level0_common.Level0Op passes around."""
import numpy as np

from tests import occlusion_model as om
from tests import texture_cases as tc

F = np.float32
SCENES = tc.SCENES
WORLD = tc.WORLD
FOOT_BYTES = 32768
TILE_W, TILE_H = 32, 8
STAGED = {"fast64": True, "odd": True, "multi": True, "fine": False, "wide": True}          # at radius 8
LONG = (("multi", 64.0, True), ("fine", 16.0, False), ("fast64", 64.0, True))                # (scene, radius, staged): reach 64 texels each


def scene_maps(name, synth_heightmap, synth_albedo):
    return tc.scene_maps(name, synth_heightmap, synth_albedo)


def max_height(name):
    return tc.max_height(name)


def footprint(hm_shape, al_shape, reach):
    (h0, w0), (ha, wa) = hm_shape, al_shape[:2]
    return (-(-TILE_W * w0 // wa) + 1 + 2 * reach[0], -(-TILE_H * h0 // ha) + 1 + 2 * reach[1])


def staged(hm_shape, al_shape, p, mh, world):
    """True where the kernel stages the tile's footprint in LDS - the host's arithmetic (occlusion_launch)."""
    k = om.prepare(p, mh, world, hm_shape[1], hm_shape[0])
    fw, fh = footprint(hm_shape, al_shape, k["reach"])
    return fw * fh <= FOOT_BYTES


def call(hm, mh, dabs=None, whole_map=False, **kw):
    return (hm, None if dabs is None else np.ascontiguousarray(dabs, F), om.params(**kw), bool(whole_map), float(mh))


def run_model(al, c, world):
    hm, dabs, p, whole, mh = c
    return om.occlusion(hm, al, p, mh, world, dabs=dabs, whole_map=whole)


def five_dabs_call(name, hm, al):
    """1. TINT, 16 directions, channels 0 and 2, under texture_cases.five_dabs."""
    return call(hm, max_height(name), dabs=tc.five_dabs(al.shape, WORLD[name], tc.DAB_SCALE[name]), color=(20.0, 0.0, 45.5, 255.0), channel_mask=5)


def store_call(name, hm):
    """2. The whole map, the visibility stored into channel 3 alone."""
    return call(hm, max_height(name), whole_map=True, mode=om.STORE, channel_mask=8)


def variant_calls(name, hm):
    """3. what -> call: 4 and 8 directions on fast64; a bias of 0.25 and a gain of 4 on odd."""
    mh = max_height(name)
    if name == "fast64":
        return {f"{d} directions": call(hm, mh, whole_map=True, directions=d, color=(10.0, 5.0, 30.0, 255.0)) for d in (4, 8)}
    assert name == "odd"
    return {"bias 0.25": call(hm, mh, whole_map=True, bias=0.25, opacity=0.9), "gain 4": call(hm, mh, whole_map=True, gain=4.0)}


def long_call(name, hm, radius):
    """4. A march of 64 height texels along the axes, over the whole map."""
    return call(hm, max_height(name), whole_map=True, radius=radius, gain=2.0)


def all_cases(synth_heightmap, synth_albedo):
    """(what, scene, heightmap, albedo, world, call, kind, staged) of every single-call case of the GPU tests."""
    maps = {n: scene_maps(n, synth_heightmap, synth_albedo) for n in SCENES}
    out = []
    for n in SCENES:
        hm, al = maps[n]
        out.append((f"{n}, five dabs", n, hm, al, WORLD[n], five_dabs_call(n, hm, al), "dabs", STAGED[n]))
        out.append((f"{n}, stored", n, hm, al, WORLD[n], store_call(n, hm), "whole", STAGED[n]))
    for n in ("fast64", "odd"):
        hm, al = maps[n]
        for what, c in variant_calls(n, hm).items():
            out.append((f"{n}, {what}", n, hm, al, WORLD[n], c, "gain" if "gain" in what else "whole", STAGED[n]))
    for n, radius, st in LONG:
        hm, al = maps[n]
        out.append((f"{n}, radius {radius:g}", n, hm, al, WORLD[n], long_call(n, hm, radius), "long", st))
    return out


def sides(detail):
    """How many masked texels have a sample skipped beyond the map's left, right, top and bottom edge."""
    h0, w0 = detail["hm_shape"]
    x0, y0, m = detail["x0"][None, :], detail["y0"][:, None], detail["mask"] > 0
    left, right, top, bottom = (np.zeros(m.shape, bool) for _ in range(4))
    for dx, dz, n, _ in detail["prepared"]["dirs"]:
        left |= x0 + n * dx < 0
        right |= x0 + n * dx > w0 - 1
        top |= y0 + n * dz < 0
        bottom |= y0 + n * dz > h0 - 1
    return [int((s & m).sum()) for s in (left, right, top, bottom)]


def winners_in_other_tiles(detail, rect):
    """How many masked texels have, in some direction, a winning sample - num > 0 - inside the centre span of another 32 x 8 tile of
    the call's rectangle than their own."""
    x0, y0, m = detail["x0"], detail["y0"], detail["mask"] > 0
    rx, ry, rw, rh = rect
    ha, wa = m.shape
    ii, jj = np.meshgrid(np.arange(wa), np.arange(ha))
    tcol, trow = (ii - rx) // TILE_W, (jj - ry) // TILE_H
    in_rect = (ii >= rx) & (ii < rx + rw) & (jj >= ry) & (jj < ry + rh)

    def tile_of(v, c0, first, size, count):
        """the tile (along one axis) whose centre span holds height coordinate v, -1 where none does"""
        starts = np.arange(first, first + count, size)
        lo, hi = c0[starts], c0[np.minimum(starts + size, first + count) - 1]
        t = np.searchsorted(lo, v, "right") - 1
        ok = (t >= 0) & (v <= hi[np.clip(t, 0, len(hi) - 1)])
        return np.where(ok, t, -1)

    found = np.zeros(m.shape, bool)
    for d, (dx, dz, n, _) in enumerate(detail["prepared"]["dirs"]):
        num, den = detail["num"][d], detail["den"][d]
        sx, sz = x0[None, :] + den * dx, y0[:, None] + den * dz
        c, r = tile_of(sx, x0, rx, TILE_W, rw), tile_of(sz, y0, ry, TILE_H, rh)
        found |= (num > 0) & (c >= 0) & (r >= 0) & ((c != tcol) | (r != trow))
    return int((found & m & in_rect).sum())


def check_preconditions(al, out, c, rect, detail, what, kind):
    """Asserted on the model's output alone: the call can tell a wrong kernel from a right one.  At least 200 texels change; at least 50
    masked texels have a horizon set by a step beyond the first; masked texels skip samples beyond the map's edge - on each of the four
    sides for a call over the whole map, on the left and the top at least under the five dabs, which do not reach every edge of every
    scene; at least 30 masked texels have a winning sample in another tile's centre span.  `long`: at least 30 texel-directions whose
    winner lies more than 32 height texels out on an axis.  `gain`: at least 10 texels with o = 1 and at least 10 with 0 < o < 1.
    Returns the counts."""
    m = detail["mask"] > 0
    changed = (al != out).any(-1)
    far = ((detail["den"] > 1) & (detail["num"] > 0)).any(0) & m
    counts = dict(changed=int(changed.sum()), far=int(far.sum()), sides=sides(detail), other_tiles=winners_in_other_tiles(detail, rect))
    assert counts["changed"] >= 200 and counts["far"] >= 50, (what, counts)
    assert min(counts["sides"] if kind != "dabs" else counts["sides"][0:1] + counts["sides"][2:3]) > 0, (what, counts)
    assert counts["other_tiles"] >= 30, (what, counts)
    if kind == "long":
        steps = np.array([max(abs(dx), abs(dz)) for dx, dz, _, _ in detail["prepared"]["dirs"]])[:, None, None]
        counts["long"] = int(((detail["den"] * steps > 32) & (detail["num"] > 0) & m[None]).sum())
        assert counts["long"] >= 30, (what, counts)
    if kind == "gain":
        o = detail["o"]
        counts["saturated"], counts["between"] = int(((o == 1) & m).sum()), int(((o > 0) & (o < 1) & m).sum())
        assert counts["saturated"] >= 10 and counts["between"] >= 10, (what, counts)
    return counts
