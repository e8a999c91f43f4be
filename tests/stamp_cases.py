"""The stamps, placements and preconditions the vr_terrain_stamp tests share (tests/test_stamp_model_cpu.py checks the preconditions
on the oracle's synthetic maps, without a device, and tests/test_terrain_stamp_cpu.py holds vr_stamp.h under g++ to the model on
every case; tests/test_terrain_stamp_gpu.py asserts the preconditions again on the maps it runs and holds the device to the model).

Scenes are those of tests/test_terrain_edit_gpu.py - 64^2 + 64^2, 67x45 height + 33x50 albedo, the 2x2-surface world of 128 on 128^2
maps.  A case is one call: a scene, the map it writes, a stamp and a placement.  Placements are stated in texels of the map -
centre, extent along the stamp's own axes, angle in degrees - and turned into the world units the entry point takes."""
import math

import numpy as np

from tests import stamp_model as sm
from tests.texture_cases import WORLD, scene_maps  # noqa: F401  (the scenes' maps and world sizes are shared)

F = np.float32
SCENES = ("fast64", "odd", "multi")
OPS = (("blend", sm.BLEND), ("add", sm.ADD), ("sub", sm.SUB), ("max", sm.MAX), ("min", sm.MIN))


def stamp_texels(w, h, channels=1, seed=0):
    """A stamp of uint8 (h, w) or (h, w, 4): a bump with a seeded roughness, stretched to the whole range, with every other 2 x 2 block
    black - so that 0 and 255 both occur next to each other all over it; the alpha channel of an SRGBA8 stamp is a ramp from 0 to 255
    across it."""
    rng = np.random.default_rng(1000 * w + 10 * h + channels + seed)
    y, x = np.mgrid[0:h, 0:w]
    r2 = ((x + 0.5) / w - 0.5) ** 2 + ((y + 0.5) / h - 0.5) ** 2
    out = []
    for c in range(channels):
        v = np.exp(-6.0 * r2) * (1.0 + 0.3 * c) + 0.35 * rng.random((h, w))
        v = (v - v.min()) / max(v.max() - v.min(), 1e-9) if w * h > 1 else np.full((h, w), 0.8)
        out.append(np.round(255.0 * np.where((x // 2 + y // 2) & 1, 0.0, v)))
    if channels == 4:
        out[3] = np.round(255.0 * (x + y) / max(w + h - 2, 1))
    a = np.stack(out, -1).astype(np.uint8)
    return a[..., 0] if channels == 1 else a


def place(map_shape, world, cx, cy, ex, ey, deg=0.0, **kw):
    """Placement centred at texel coordinate (cx, cy) of a map of `map_shape`, ex x ey of its texels large along the stamp's own axes
    (a texel is world / w0 wide; on a map that is not square the z extent is measured in rows), turned by `deg` degrees."""
    h0, w0 = map_shape[:2]
    return sm.params((cx + 0.5) / w0 * world - world / 2, (cy + 0.5) / h0 * world - world / 2, ex * world / w0, ey * world / h0,
                     math.radians(deg), **kw)


# ---- 1. the five ops on the heightmap --------------------------------------------------------------------------------------
# (stamp, extent in texels): 5 x 3 magnified about three times, 33 x 17 slightly minified
STAMPS = (((5, 3), (15.3, 9.4)), ((33, 17), (29.5, 15.2)))
ANGLES = (0.0, 30.0, 180.0)
FEATHERS = (0.0, 0.5)
CENTRES = ("inside", "left", "right", "top", "bottom", "corner")


def centre(name, map_shape):
    """Texel coordinates of a call's centre: well inside the map, or so near an edge (or the corner) that the stamp lies across it."""
    h0, w0 = map_shape[:2]
    return {"inside": (0.43 * w0 + 0.3, 0.55 * h0 + 0.2), "left": (1.3, 0.4 * h0 + 0.4), "right": (w0 - 2.3, 0.6 * h0 + 0.1), "top": (0.55 * w0 + 0.7, 1.8),
            "bottom": (0.35 * w0 + 0.15, h0 - 2.6), "corner": (w0 - 3.4, h0 - 3.2)}[name]


def op_sequence(scene, op_index, map_shape):
    """The six calls of one op on a scene's heightmap, one per centre, applied one after the other: across the five ops every pairing
    of stamp, angle and feather occurs, and within every op both stamps, all three angles and both feathers do."""
    world = WORLD[scene]
    op = OPS[op_index][1]
    calls = []
    for ci, cname in enumerate(CENTRES):
        n = op_index + ci
        (sw, sh), (ex, ey) = STAMPS[n % 2]
        deg, feather = ANGLES[n % 3], FEATHERS[(n // 2 + op_index) % 2]
        cx, cy = centre(cname, map_shape)
        if op in (sm.ADD, sm.SUB):                                   # s' from -255 to 637 (SUB: from 255 to -637): the clamps bind at both ends
            kw = dict(gain=3.5, offset=-255.0, opacity=0.9) if op == sm.ADD else dict(gain=-3.5, offset=255.0, opacity=0.9)
        elif op == sm.BLEND:
            kw = dict(gain=0.75, offset=20.0, opacity=0.85)
        else:
            kw = dict(gain=1.0, offset=80.0, opacity=1.0 if ci % 2 else 0.7) if op == sm.MAX else dict(gain=0.6, offset=-30.0, opacity=1.0 if ci % 2 else 0.7)
        calls.append(dict(name=f"{OPS[op_index][0]}/{cname}", stamp=stamp_texels(sw, sh, 1, seed=n), rotated=deg != 0.0,
                          params=place(map_shape, world, cx, cy, ex, ey, deg, feather=feather, op=op, channel_mask=1, **kw)))
    return calls


# ---- 2. the albedo ---------------------------------------------------------------------------------------------------------
def albedo_calls(scene, map_shape):
    world, (h0, w0) = WORLD[scene], map_shape[:2]
    st = stamp_texels(33, 17, 4)
    calls = []
    for k, (mask, alpha) in enumerate(((0x7, False), (0xF, False), (0x7, True), (0xF, True))):
        calls.append(dict(name=f"albedo/mask {mask:#x}{'/alpha' if alpha else ''}", stamp=st, rotated=True,
                          params=place(map_shape, world, (0.3 + 0.15 * k) * w0, (0.35 + 0.1 * k) * h0, 0.62 * w0, 0.3 * h0, 30.0 + 25.0 * k, feather=0.5 * (k % 2),
                                       opacity=0.9, gain=1.0, offset=0.0, op=sm.BLEND, channel_mask=mask, flags=sm.USE_ALPHA if alpha else 0)))
    return calls


# ---- 3. the variants -------------------------------------------------------------------------------------------------------
def variant_calls(scene, map_shape):
    """A 256^2 stamp squeezed onto 24 texels of the map and turned (ten stamp texels per map texel), the same stamp over the whole
    map (four per texel), a 1 x 1 stamp, a stamp larger than the map that covers every texel.  (The kernel has one variant: it reads
    the stamp from memory at every ratio - DESIGN.md 4y - so there is no threshold between two kernels to place cases about.)"""
    world, (h0, w0) = WORLD[scene], map_shape[:2]
    big = stamp_texels(256, 256, 1)
    return [dict(name="mini256", stamp=big, rotated=True, params=place(map_shape, world, 0.5 * w0 + 0.3, 0.45 * h0, 24.0, 24.0, 30.0, feather=0.5, op=sm.BLEND, opacity=0.9)),
            dict(name="whole256", stamp=big, rotated=False, params=place(map_shape, world, 0.5 * w0 - 0.5, 0.5 * h0 - 0.5, float(w0), float(h0), 0.0, op=sm.MAX)),
            dict(name="one texel", stamp=np.full((1, 1), 200, np.uint8), rotated=True,
                 params=place(map_shape, world, 0.4 * w0, 0.6 * h0, 9.0, 7.0, 30.0, feather=0.5, op=sm.BLEND)),
            dict(name="covers all", stamp=stamp_texels(33, 17, 1), rotated=False, covers_all=True,
                 params=place(map_shape, world, 0.5 * w0, 0.5 * h0, 3.0 * w0, 3.0 * h0, 30.0, feather=1.0, op=sm.BLEND, gain=0.5, offset=60.0))]


def miss_params(scene, map_shape):
    """A stamp that lies wholly outside the map."""
    h0, w0 = map_shape[:2]
    return place(map_shape, WORLD[scene], -40.0, 0.5 * h0, 20.0, 12.0, 30.0, op=sm.BLEND)


# ---- preconditions, asserted on the model's output alone -------------------------------------------------------------------
def check_preconditions(before, after, call, detail, what):
    """The call can tell a wrong kernel from a right one: at least 30 texels change; at least 10 covered texels have fractional tu
    and tv (a one-texel axis has no fraction: its taps clamp); with a feather at least 10 covered texels weigh strictly between 0 and 1; ADD and SUB clamp at 0 and at 255 (3 texels
    each at least); a rotated call leaves texels of its rectangle uncovered.  Returns the counts."""
    p = call["params"]
    changed = (before != after) if before.ndim == 2 else (before != after).any(-1)
    cov = detail["covered"]
    assert not (changed & ~cov).any(), what
    frac = int((cov & (detail["tu"] > 0) & (detail["tv"] > 0)).sum())
    counts = dict(changed=int(changed.sum()), covered=int(cov.sum()), fractional=frac)
    assert counts["changed"] >= 30 and (frac >= 10 or min(call["stamp"].shape[:2]) == 1), (what, counts)
    if p["feather"] > 0:
        counts["on_feather"] = int((cov & (detail["wf"] > 0) & (detail["wf"] < 1)).sum())
        assert counts["on_feather"] >= 10, (what, counts)
    if p["op"] in (sm.ADD, sm.SUB):
        val = (before[..., None] if before.ndim == 2 else before).astype(F)
        lo = hi = 0
        for c in range(val.shape[2]):
            if p["channel_mask"] >> c & 1:
                sp = (detail["s"][..., c] * F(p["gain"]) + F(p["offset"])).astype(F)
                t = val[..., c] + detail["a"] * sp if p["op"] == sm.ADD else val[..., c] - detail["a"] * sp
                lo += int((cov & (t < 0)).sum())
                hi += int((cov & (t > 255)).sum())
        counts.update(clamped_at_0=lo, clamped_at_255=hi)
        assert lo >= 3 and hi >= 3, (what, counts)
    if call.get("rotated"):
        x0, y0, x1, y1 = detail["rect"]
        counts["uncovered_in_rect"] = int((~cov[y0:y1, x0:x1]).sum())
        assert counts["uncovered_in_rect"] >= 1, (what, counts)
    if call.get("covers_all"):
        assert cov.all(), (what, counts)
    return counts


def model(level0, call, world):
    """(new level 0, rect, detail) of the model for one call."""
    detail = {}
    out, rect = sm.stamp(level0, call["stamp"], call["params"], world, detail=detail)
    return out, rect, detail
