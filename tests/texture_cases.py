"""The scenes, layers, dabs and preconditions the vr_terrain_texture tests share (tests/test_terrain_texture_cpu.py checks the
preconditions on the oracle's synthetic maps, without a device; tests/test_terrain_texture_gpu.py asserts them again on the maps it
runs and holds the device to the model).

Scenes are those of tests/test_terrain_edit_gpu.py - 64^2 + 64^2, 67x45 height + 33x50 albedo, the 2x2-surface world of 128 on 128^2
maps - and two whose tile footprint exceeds the 4 KiB of LDS the kernel stages, so that their lanes read memory directly: "fine", a
256^2 heightmap under a 32^2 albedo ((256 + 4) x (64 + 4) bytes), and "wide", a 512x32 heightmap under a 32^2 albedo ((512 + 4) x
(8 + 4) bytes).  With eight height texels per albedo texel no sample point of "fine" comes nearer than 3.5 texels to the heightmap's
edge - its texels cannot sit on a clamped edge, whatever the layers - so "wide", whose rows map one to one, is the scene that reaches
the clamps through the direct loads."""
import numpy as np

from tests import texture_model as tm
from tests.queries_common import scaled_max_height

F = np.float32
SCENES = ("fast64", "odd", "multi", "fine", "wide")
REACHES_EDGE = {"fast64": True, "odd": True, "multi": True, "fine": False, "wide": True}
DAB_SCALE = {"fast64": 1.0, "odd": 1.0, "multi": 1.0, "fine": 1.0, "wide": 1.4}       # five_dabs' radii, so that "wide"'s reach its edge rows
WORLD = {"fast64": 64.0, "odd": 64.0, "multi": 128.0, "fine": 64.0, "wide": 64.0}


def scene_maps(name, synth_heightmap, synth_albedo):
    """(heightmap, albedo) of a scene; synth_heightmap(size), synth_albedo(size, heightmap): the synthetic maps."""
    if name == "fast64":
        hm = synth_heightmap(64)
        return hm, synth_albedo(64, hm)
    if name == "odd":
        hm = np.ascontiguousarray(synth_heightmap(67)[:45, :67])
        return hm, np.ascontiguousarray(synth_albedo(50, synth_heightmap(50))[:50, :33])
    if name == "multi":
        hm = synth_heightmap(128)
        return hm, synth_albedo(128, hm)
    if name == "fine":
        return synth_heightmap(256), synth_albedo(32, synth_heightmap(32))
    return np.ascontiguousarray(synth_heightmap(512)[:32, :512]), synth_albedo(32, synth_heightmap(32))


def max_height(name):
    return scaled_max_height(WORLD[name])


def staged_footprint(hm_shape, al_shape):
    """True where a 32 x 8 tile's footprint, (ceil(32 rx) + 4) x (ceil(8 rz) + 4) bytes, fits the 4 KiB the kernel stages in LDS."""
    rx, rz = float(F(hm_shape[1] / al_shape[1])), float(F(hm_shape[0] / al_shape[0]))
    return (int(np.ceil(32.0 * rx)) + 4) * (int(np.ceil(8.0 * rz)) + 4) <= 4096


def quantiles(hm, al_shape, mh, world):
    """What the layers are placed by: the model's own h (heightmap steps) and slope (degrees) under every albedo texel."""
    h, s2, _ = tm.sample(hm, al_shape, mh, world)
    return h, np.degrees(np.arctan(np.sqrt(s2.astype(np.float64))))


def four_layers(hm, al_shape, mh, world):
    """Grass on the low flats, sand in a narrow low band (two channels), rock on the steep half (hard altitude edges, every channel),
    snow above a line: bands placed at quantiles of the scene's own heights and slopes, so that every scene has texels in each band
    and on each fade."""
    h, deg = quantiles(hm, al_shape, mh, world)
    alt = lambda q: float(np.quantile(h, q)) * mh / 255.0               # world units of height
    slope = lambda q: min(float(np.quantile(deg, q)), 80.0)
    spread = max(alt(0.9) - alt(0.1), 1e-3)
    s_mid, s_fade = slope(0.55), max(0.25 * (slope(0.8) - slope(0.3)), 0.5)
    return [tm.layer((60.0, 140.0, 50.0, 255.0), 1.0, alt(0.0), alt(0.5), 0.25 * spread, 0.0, s_mid, s_fade, 0b0111),
            tm.layer((210.0, 190.5, 130.0, 9.0), 0.6, alt(0.2), alt(0.35), 0.1 * spread, 0.0, slope(0.7), s_fade, 0b0101),
            tm.layer((120.0, 110.0, 100.0, 200.0), 0.85, alt(0.1), alt(0.95), 0.0, s_mid, 89.0, s_fade, 0b1111),
            tm.layer((250.0, 250.0, 255.0, 255.0), 0.9, alt(0.7), alt(1.0) + 1.0, 0.3 * spread, 0.0, slope(0.85), s_fade, 0b0111)]


def zero_layers(mh):
    """Bands above every altitude a map can hold: every layer weighs 0 on every texel."""
    return [tm.layer((255.0, 0.0, 255.0, 0.0), 1.0, 1.5 * mh, 2.0 * mh, 0.25 * mh, 0.0, 89.0, 0.0, 0b1111),
            tm.layer((0.0, 255.0, 0.0, 255.0), 1.0, 1.3 * mh, 1.3 * mh, 0.0, 0.0, 89.0, 5.0, 0b1111)]


def dab(shape, world, tx, ty, r_tex, hardness, strength):
    """A dab whose centre is at texel coordinate (tx, ty) of a map of `shape` and whose radius is r_tex texels of the map's width."""
    h, w = shape[:2]
    return [(tx + 0.5) / w * world - world / 2, (ty + 0.5) / h * world - world / 2, r_tex * world / w, hardness, strength]


def five_dabs(shape, world, scale=1.0):
    """In the style of tests/test_terrain_brush_gpu.py's five_dabs, sized by the map: a wide soft dab, a hard-centred one, one on the
    map's corner, one outside the map that still overlaps it, one texel."""
    h, w = shape[:2]
    r = 0.5 * min(w, h) * scale
    return np.float32([dab(shape, world, 0.4 * w, 0.45 * h, 0.8 * r, 0.0, 0.9),
                       dab(shape, world, 0.7 * w + 0.37, 0.6 * h + 0.21, 0.45 * r, 0.7, 0.35),
                       dab(shape, world, -0.5, -0.5, 0.4 * r, 0.0, 0.8),                 # the map's corner
                       dab(shape, world, w + 2.0, 0.5 * h, 0.3 * r + 2.0, 0.7, 0.5),     # outside, overlapping
                       dab(shape, world, 10.1, 7.2, 0.4, 0.0, 1.0)])                     # one texel


def check_preconditions(al, out, layers, detail, what, reaches_edge=True):
    """Asserted on the model's output alone: the call can tell a wrong kernel from a right one.  At least 200 texels change and 30
    end strictly between 0 and 255 in a written channel; every layer is the last to change at least 10 texels; at least 10 masked
    texels lie on a fade - a ramp strictly between 0 and 1, in a layer that weighs there - for each of the four ramp kinds; at
    least 10 changed texels take a corner of their sample from a clamped edge of the heightmap (reaches_edge=False: none can, by the
    scene's geometry - REACHES_EDGE).  Returns the counts."""
    changed = (al != out).any(-1)
    written = np.zeros(al.shape, bool)
    for l in layers:
        for c in range(4):
            if l["channel_mask"] >> c & 1:
                written[..., c] = True
    between = (changed[..., None] & written & (out > 0) & (out < 255)).any(-1)
    m, h, s2 = detail["mask"], detail["h"], detail["s2"]
    # the last layer to change a texel: replay the composite and keep the index of the last step that moved a value
    val = al.astype(F)
    last = np.full(al.shape[:2], -1)
    for k, (p, wl) in enumerate(zip(detail["prepared"], detail["weights"])):
        a = m * wl
        moved = np.zeros(al.shape[:2], bool)
        for c in range(4):
            if p["channel_mask"] >> c & 1:
                new = np.minimum(np.maximum(val[..., c] + a * (p["color"][c] - val[..., c]), F(0)), F(255))
                moved |= new != val[..., c]
                val[..., c] = new
        last[moved & changed] = k
    per_layer = [int((last == k).sum()) for k in range(len(layers))]
    fades = [0, 0, 0, 0]
    for p, wl in zip(detail["prepared"], detail["weights"]):
        for r, v in enumerate(tm.ramps_of(p, h, s2)):
            fades[r] += int(((v > 0) & (v < 1) & (wl > 0) & (m > 0)).sum())
    pts = detail["points"]
    h0, w0 = detail["hm_shape"]
    edge_x = (pts["i0"] == 0) | (pts["i1"] == w0 - 1)
    edge_y = (pts["j0"] == 0) | (pts["j1"] == h0 - 1)
    on_edge = int((changed & (edge_x[None, :] | edge_y[:, None])).sum())
    counts = dict(changed=int(changed.sum()), between=int(between.sum()), per_layer=per_layer, fades=fades, on_edge=on_edge)
    assert counts["changed"] >= 200 and counts["between"] >= 30, (what, counts)
    assert min(per_layer) >= 10, (what, counts)
    assert min(fades) >= 10, (what, counts)
    assert on_edge >= 10 if reaches_edge else on_edge == 0, (what, counts)
    return counts


def model(hm, al, layers, mh, world, dabs=None, whole_map=False):
    """(albedo, rect, detail) of the model, the detail extended by what check_preconditions reads."""
    detail = {}
    out, rect = tm.texture(hm, al, layers, mh, world, dabs=dabs, whole_map=whole_map, detail=detail)
    detail["hm_shape"] = hm.shape
    return out, rect, detail
