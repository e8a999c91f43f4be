"""What the tests of the erosions' fp32 state share (tests/test_terrain_erosion_state_gpu.py on the device, tests/
test_terrain_erode_cpu.py on the host): the models' state by one call signature, the comparison on bit patterns, the wrong variants
of the models, and the precondition that a case can tell them from the right one.

A case is (kind, texels, dabs, world, iterations, params): kind "thermal" with params (talus, rate), or "hydraulic" with the keyword
dictionary of hydro_model.state.  The state is a dictionary: rect, mask, planes (h, or h, d, s) and bytes (the map after the call)."""
import numpy as np

from tests import erode_model as em
from tests import hydro_model as hm
from tests.level0_common import assert_bytes, level0

F = np.float32
WORLD = 64.0                                                         # of the CPU tests' seeded cases
FIELDS = {"thermal": ("h",), "hydraulic": ("h", "d", "s")}
SENSITIVE = 30                                                       # "at least 30 changed", as everywhere in this suite
# The swap every case is held to before it runs.  (-1,0) and (1,0) stand side by side in the thermal order: exchanging them changes one
# of a cell's seven partial sums, and h + acc then rounds the difference away in all but 3 .. 30 cells of the suite's smooth scenes,
# whatever the talus and the rate.  The first and the last neighbour change every partial sum.
PRECONDITION = "the first and the last neighbour swapped"


def swapped(order, a, b):
    """`order` with the neighbours a and b exchanged."""
    return tuple(b if n == a else a if n == b else n for n in order)


def ulp_up(x):
    return float(np.nextafter(F(x), F(np.inf)))


def state(kind, texels, dabs, world, iterations, params, neighbours=None, **wrong):
    """The model's final state of one call.  `neighbours` and `wrong` (talus=, keep=) select a wrong variant."""
    if kind == "thermal":
        talus, rate = params
        h, m, rect = em.state(texels, dabs, world, iterations, wrong.get("talus", talus), rate, neighbours or em.NEIGHBOURS)
        planes, settled = [h], h
    else:
        h, d, s, m, rect = hm.state(texels, dabs, world, iterations, neighbours=neighbours or hm.NEIGHBOURS, keep=wrong.get("keep"), **params)
        planes, settled = [h, d, s], h + s
    stored = np.floor(np.minimum(np.maximum(settled, F(0)), F(255)) + F(0.5)).astype(np.uint8)
    return dict(rect=tuple(int(v) for v in rect), mask=m, planes=planes, settled=settled, bytes=np.where(m > F(0), stored, texels).astype(np.uint8))


ITER = 20
_MODEL = {}


def model(kind, texels, dabs, world, iterations, params):
    """The model's state, computed once per distinct call and left unchanged."""
    key = (kind, texels.tobytes(), texels.shape, np.asarray(dabs, F).tobytes(), world, iterations, repr(params))
    if key not in _MODEL:
        _MODEL[key] = state(kind, texels, dabs, world, iterations, params)
    return _MODEL[key]


def assert_state(tp, want, what):
    """The planes the last call left are the model's, bit for bit, inside the model's rectangle; level 0 is the model's bytes."""
    rect, mask, planes = tp.ErosionState()
    assert rect == want["rect"], (what, rect, want["rect"])
    assert len(planes) == len(want["planes"]), (what, len(planes))
    assert_bits(mask, crop(want["mask"], rect), f"{what}: the mask plane")
    for name, got, ref in zip("hds", planes, want["planes"]):
        assert_bits(got, crop(ref, rect), f"{what}: {name}")
    assert_bytes(level0(tp, "height"), want["bytes"], f"{what}: level 0")


def wrong_variants(kind, params):
    """name -> keywords of state(): the models with one property of the definition broken."""
    order = em.NEIGHBOURS if kind == "thermal" else hm.NEIGHBOURS
    out = {PRECONDITION: dict(neighbours=swapped(order, order[0], order[-1])),
           "neighbours (-1,0) and (1,0) swapped": dict(neighbours=swapped(order, (-1, 0), (1, 0))),
           "neighbours in reverse order": dict(neighbours=order[::-1])}
    if kind == "thermal":
        out["talus one ULP up"] = dict(talus=ulp_up(params[0]))
    else:
        out["keep one ULP up"] = dict(keep=ulp_up(F(1.0) - F(params["evaporation"])))
    return out


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def cells_that_differ(a, b):
    """(cells in which any plane differs in its bit pattern, bytes that differ) between two states of one case."""
    cells = np.zeros(a["mask"].shape, bool)
    for pa, pb in zip(a["planes"], b["planes"]):
        cells |= bits(pa) != bits(pb)
    return int(cells.sum()), int((a["bytes"] != b["bytes"]).sum())


def sensitivity(kind, texels, dabs, world, iterations, params, right=None, variant=PRECONDITION):
    """How many fp32 cells, and how many bytes, of the case's final state the wrong variant changes."""
    right = right or state(kind, texels, dabs, world, iterations, params)
    return cells_that_differ(right, state(kind, texels, dabs, world, iterations, params, **wrong_variants(kind, params)[variant]))


def assert_sensitive(kind, texels, dabs, world, iterations, params, right=None):
    """On the model alone: the case tells the model from the one with two neighbours swapped, in at least 30 fp32 cells."""
    cells, _ = sensitivity(kind, texels, dabs, world, iterations, params, right)
    assert cells >= SENSITIVE, f"{kind}, {iterations} iterations: swapping two neighbours changes {cells} cells of the state"
    return cells


def crop(plane, rect):
    x, y, w, h = rect
    return plane[y:y + h, x:x + w]


def assert_bits(got, want, what):
    """Two float32 arrays of one shape are the same bit patterns."""
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    if not np.array_equal(g, w):
        at = np.argwhere(g != w)
        first = ", ".join(f"({y}, {x}): {g[y, x]:08x} for {w[y, x]:08x}" for y, x in at[:4].tolist())
        raise AssertionError(f"{what}: {len(at)} of {g.size} cells differ, first (row, column) {first}")


def subnormal(a):
    """Non-zero cells below the smallest normal fp32."""
    return (a != F(0)) & (np.abs(a) < np.finfo(F).tiny)


# ---- the cases, as plain data: a host test checks their preconditions without a device, the GPU module runs them ------------------------
THERMAL = (0.7, 0.1)                                                 # (talus, rate), neither dyadic: every product and most sums round
HYDRO = dict(rain=1.0, flow=0.5, capacity=8.0, dissolve=0.5, deposit=0.25, evaporation=0.05)       # tests/test_terrain_hydro_gpu.py's P
# Under a mask of 1 on a map of integers HYDRO's first sweep is exact (flow * difference >= 0.25 wherever there is one, so every share
# is 0.25 and every q is 0.25 * rain): no order can show.  A flow below 0.25 per step of height makes it round from the first sweep on.
HYDRO_SLOW = dict(HYDRO, flow=0.07)
PARAMS = {"thermal": THERMAL, "hydraulic": HYDRO}


def dab(shape, world, tx, ty, r_tex, hardness, strength):
    """tests/level0_common.py's: centre at texel coordinate (tx, ty), radius r_tex texels of the map's width."""
    h, w = shape[:2]
    return [(tx + 0.5) / w * world - world / 2, (ty + 0.5) / h * world - world / 2, r_tex * world / w, hardness, strength]


def five_dabs(shape, world):
    """tests/level0_common.py's five_dabs with opacities for strengths."""
    h, w = shape[:2]
    return np.float32([dab(shape, world, 0.3 * w, 0.4 * h, 12.0, 0.0, 0.6), dab(shape, world, 0.7 * w + 0.37, 0.6 * h + 0.21, 5.5, 0.7, 0.35),
                       dab(shape, world, -0.5, -0.5, 6.0, 0.0, 0.8), dab(shape, world, w + 2.0, 0.5 * h, 4.5, 0.7, 0.5),
                       dab(shape, world, 10.1, 7.2, 0.4, 0.0, 1.0)])


def full_mask(world=WORLD):
    return np.float32([[0.0, 0.0, 4.0 * world, 0.5, 1.0]])          # one hard-centred dab far larger than the map: mask 1 everywhere


def seeded_dabs(rng, h, w, n=12):
    """Centres inside and outside the map, radii from under a texel to a third of the map and more, hardness 0 and 0.7."""
    dabs = np.zeros((n, 5), np.float32)
    dabs[:, 0:2] = rng.uniform(-0.7 * WORLD, 0.7 * WORLD, (n, 2))
    dabs[:, 2] = np.exp(rng.uniform(np.log(0.3), np.log(25.0), n)) * WORLD / max(w, h)
    dabs[:, 3] = rng.choice([0.0, 0.7], n)
    dabs[:, 4] = rng.uniform(0.0, 1.0, n)
    dabs[0, 0:2] = (-0.6 * WORLD, 0.1 * WORLD)                       # a centre outside the map that still reaches it
    dabs[0, 2] = 0.25 * WORLD
    dabs[1, 2] = 0.4 * WORLD / max(w, h)                             # a sub-texel radius
    return dabs


def soft_mask(world):
    return np.float32([[0.0, 0.0, 0.8 * world, 0.0, 1.0]])          # one hardness-0 dab over the whole map: a fractional mask on every edge


def scene_maps(synth):
    """name -> (heightmap, world size) of tests/level0_common.py's scenes; synth(size): the synthetic heightmap."""
    return {"fast64": (synth(64), 64.0), "odd": (np.ascontiguousarray(synth(67)[:45, :67]), 64.0), "multi": (synth(128), 128.0)}


def borders(size, tile):
    return list(range(tile, size, tile))


def changes_on_both_sides_of_every_border(before, after, tile_w, tile_h):
    """The fp32 plane changed in the last row or column before every interior tile border and in the first one behind it."""
    changed = bits(before) != bits(after)
    rows = all(changed[b - 1, :].any() and changed[b, :].any() for b in borders(before.shape[0], tile_h))
    return rows and all(changed[:, b - 1].any() and changed[:, b].any() for b in borders(before.shape[1], tile_w))


ODD_SHAPE = (45, 67)


def rect_dabs(world):
    """name -> (dabs, the rectangle intended) of the rectangles that stress the load, the halo and the store, on the 67 x 45 map.

    A dab's span on an axis is [floor(c - r) - 1, ceil(c + r) + 2) clipped to the map, and a span of at most 5 x 5 texels that
    covers no texel is dropped.  So a rectangle one texel wide has c + r <= -1: its dab covers nothing, and one of 1 x 1 is
    dropped - the rectangle of a call that launches is never 1 x 1, and one a texel wide or a row high has mask 0 throughout.
    Those two are here with their masks of zeros (the planes are still filled, loaded, swept and stored); next to them the
    narrowest rectangles that hold masked texels: three wide with one masked column, three high with one masked row, 3 x 3 with one
    masked texel."""
    h, w = shape = ODD_SHAPE
    r = 20.0
    ry = r * h / w                                                   # the dab's radius in rows
    out = {
        "3 x 3, one masked texel": ([dab(shape, world, 0.1, 0.2, 0.4, 0.0, 1.0)], (0, 0, 3, 3)),
        "one texel wide, mask 0": ([dab(shape, world, -1.5 - r, 0.5 * h, r, 0.0, 1.0)], (0, 8, 1, 30)),
        "one row high, mask 0": ([dab(shape, world, 0.5 * w, -1.5 - ry, r, 0.0, 1.0)], (12, 0, 44, 1)),
        "three wide, one masked column": ([dab(shape, world, 0.5 - r, 0.5 * h, r, 0.0, 1.0)], (0, 8, 3, 30)),
        "three high, one masked row": ([dab(shape, world, 0.5 * w, 0.5 - ry, r, 0.0, 1.0)], (12, 0, 44, 3)),
        "the far corner, clipped": ([dab(shape, world, w - 2.0, h - 3.0, 9.0, 0.0, 1.0)], (54, 34, 13, 11)),
    }
    return {k: (np.float32(d), want) for k, (d, want) in out.items()}


def tile_wide_dabs(shape, world, width):
    """(dabs, rect): a hardness-0 dab centred on the map's origin corner whose rectangle is exactly `width` texels wide - the radius
    is the first of a fine scan at which the model says so."""
    for r in np.arange(width - 4.0, width + 1.0, 0.01):
        d = np.float32([dab(shape, world, 0.0, 0.0, r, 0.0, 1.0)])
        _, rect = em.mask_of(shape, d, world)
        if rect[2] == width:
            return d, tuple(int(v) for v in rect)
    raise AssertionError(f"no dab with a rectangle {width} wide")


# Over 1024 sweeps under a talus of 0.7 the slopes settle and few edges stay live; 0.3 keeps them moving.
THERMAL_LONG = (0.3, 0.1)


def _changed(plane, texels):
    return int((bits(plane) != bits(texels.astype(F))).sum())


def _holds_max(want, texels):
    assert _changed(want["planes"][0], texels) >= 30


def _holds_no_keep(want, texels):                                    # keep = 0: the water is the sweep's rain and nothing else
    h, d, s = want["planes"]
    assert np.array_equal(bits(d), bits((F(HYDRO["rain"]) * want["mask"]).astype(F))) and _changed(h, texels) >= 30


def _holds_no_rain(want, texels):
    h, d, s = want["planes"]
    assert not bits(d).any() and not bits(s).any() and _changed(h, texels) == 0                  # d and s all +0, h unchanged


def _holds_no_exchange(want, texels):                                # the water moves, the terrain and the sediment do not
    h, d, s = want["planes"]
    assert _changed(h, texels) == 0 and not bits(s).any() and len(np.unique(d[want["mask"] > 0])) >= 30


def _holds_subnormal_water(want, texels):
    assert int(subnormal(want["planes"][1]).sum()) >= 30


# name -> (parameters, what the model's state must show)
HYDRO_CORNERS = {
    "every maximum": (dict(rain=16.0, flow=1.0, capacity=64.0, dissolve=1.0, deposit=1.0, evaporation=0.0), _holds_max),
    "evaporation 1": (dict(HYDRO, evaporation=1.0), _holds_no_keep),
    "rain 0": (dict(HYDRO, rain=0.0), _holds_no_rain),
    "dissolve 0, deposit 0": (dict(HYDRO, dissolve=0.0, deposit=0.0), _holds_no_exchange),
    "a subnormal rain": (dict(HYDRO, rain=1e-39), _holds_subnormal_water),
}


def _as_it_is(texels):
    return texels


def _every_other_row_zero(texels):
    out = texels.copy()
    out[20:38:2, :] = 0
    return out


def _holds_moves(want, texels):
    assert _changed(want["planes"][0], texels) >= 30


def _holds_nothing_moves(want, texels):
    assert _changed(want["planes"][0], texels) == 0


def _holds_subnormal_heights(want, texels):
    assert int(subnormal(want["planes"][0]).sum()) >= 30


# name -> (parameters, the map from the scene's, what the model's state must show)
THERMAL_CORNERS = {
    "talus 0": ((0.0, 0.1), _as_it_is, _holds_moves),
    "talus 255": ((255.0, 0.1), _as_it_is, _holds_nothing_moves),
    "rate 0.125": ((0.7, 0.125), _as_it_is, _holds_moves),
    "a subnormal rate": ((0.0, 1e-42), _every_other_row_zero, _holds_subnormal_heights),
}


def clamp_case(world):
    """(texels, dabs, iterations, params): a 64^2 map whose left half is 0 and whose right half is 255 under the whole-map soft dab.
    What a texel dissolves leaves with the water, so h + s falls below 0 on the low half and rises above 255 on the high one."""
    x = np.arange(64)[None, :].repeat(64, 0)
    texels = np.where(x < 32, 0, 255).astype(np.uint8)
    return texels, soft_mask(world), 5, dict(rain=16.0, flow=1.0, capacity=64.0, dissolve=1.0, deposit=1.0, evaporation=0.0)


def suite_cases(maps, config):
    """Every case of the GPU module that is held to the sensitivity precondition, as (name, kind, texels, dabs, world, iterations,
    params); maps: scene_maps(); config: kind -> (tile width, tile height, sweeps per launch)."""
    out = []
    for name, (t, w) in maps.items():
        out += [(f"scene {name}", kind, t, five_dabs(t.shape, w), w, 20, PARAMS[kind]) for kind in FIELDS]
    t, w = maps["multi"]
    for kind in FIELDS:
        tw, th, k = config[kind]
        for mask, dabs in (("full", full_mask(w)), ("soft", soft_mask(w))):
            out += [(f"borders, {mask} mask", kind, t, dabs, w, n, THERMAL if kind == "thermal" else HYDRO_SLOW) for n in sorted({1, k - 1, k, k + 1, 2 * k + 1})]
        out += [(f"a rectangle {width} wide", kind, t, tile_wide_dabs(t.shape, w, width)[0], w, 20, PARAMS[kind]) for width in (tw, tw + 1)]
    t, w = maps["fast64"]
    out += [("1024 iterations", kind, t, np.float32([dab(t.shape, w, 30.0, 28.0, 10.0, 0.0, 1.0)]), w, 1024, THERMAL_LONG if kind == "thermal" else HYDRO) for kind in FIELDS]
    texels, dabs, n, params = clamp_case(64.0)
    return out + [("the clamp", "hydraulic", texels, dabs, 64.0, n, params)]
