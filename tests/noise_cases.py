"""The scenes, parameter sets, dabs and preconditions the vr_terrain_noise tests share (tests/test_noise_model_cpu.py checks the
preconditions on the oracle's synthetic maps, without a device; tests/test_terrain_noise_gpu.py asserts them again on the maps it runs
and holds the device to the model).

Scenes are those of tests/test_terrain_edit_gpu.py - 64^2 + 64^2, 67x45 height + 33x50 albedo, the 2x2-surface world of 128 on 128^2
maps - and tests/texture_cases.py's "wide", a 512x32 heightmap, for a non-square map with many tiles in a row and a clamped last row
of tiles.  They are the smallest at which a tile edge, a chunked dab list and a partial last tile all occur."""
import numpy as np

from tests import noise_model as nm
from tests import texture_cases as tc

F = np.float32
SCENES = ("fast64", "odd", "multi", "wide")
WORLD = {n: tc.WORLD[n] for n in SCENES}
GPU_OCTAVES = (4, 5, 6, 12)                 # every octave count a GPU case uses
COMBOS = [(b, f) for _, b in nm.BASES for _, f in nm.FRACTALS]
COMBO_IDS = [f"{bn}-{fn}" for bn, _ in nm.BASES for fn, _ in nm.FRACTALS]
scene_maps = tc.scene_maps
dab = tc.dab


def five_dabs(shape, world):
    """tests/texture_cases.py's five dabs, sized by the map's short side.  A dab's radius is given in texels of the map's WIDTH: on
    "wide" (512x32, a texel an eighth of a world unit wide and two tall) the radii are scaled by 8, so that the dabs, flat ellipses
    in texel space, still cover rows on either side of their centres."""
    h, w = shape[:2]
    return tc.five_dabs(shape, world, 8.0 if w >= 8 * h else 1.0)


def height_params(name, basis, fractal, op=nm.ADD, octaves=6):
    """A heightmap call of a scene: cells of 16 world units in the first octave, the lattice origin inside the map (so cells of both
    signs occur), an amplitude that reaches both clamps on the synthetic maps."""
    return nm.params(1.0 / 16.0, 150.0 if op == nm.ADD else -120.0, octaves=octaves, lacunarity=2.0, gain=0.5, offset=(3.3, -7.7), seed=20261 + 7 * basis + fractal,
                     basis=basis, fractal=fractal, op=op, base=128.0, channel_mask=1)


def scene_combo(name):
    """The one basis x fractal a scene other than fast64 runs under dabs."""
    return {"fast64": (nm.GRADIENT, nm.FBM), "odd": (nm.VALUE, nm.RIDGED), "multi": (nm.GRADIENT, nm.BILLOW), "wide": (nm.VALUE, nm.FBM)}[name]


def whole_params(name):
    """The whole-map call: BLEND about 128, 12 octaves; lacunarity 1.3 keeps the last octave (18 times the first: 0.56 cells per
    world unit) coarser than a texel, and gain 0.8 keeps its weight large enough to move bytes."""
    basis, fractal = scene_combo(name)
    return nm.params(1.0 / 32.0, 200.0, octaves=12, lacunarity=1.3, gain=0.8, offset=(-5.25, 9.5), seed=977, basis=basis, fractal=fractal, op=nm.BLEND,
                     base=128.0, channel_mask=1)


def albedo_params(name):
    """The albedo call: channels 0 and 2 (mask 5), gradient ridges added."""
    return nm.params(1.0 / 8.0, 90.0, octaves=4, lacunarity=2.0, gain=0.5, offset=(1.5, 2.5), seed=31337, basis=nm.GRADIENT, fractal=nm.RIDGED, op=nm.ADD,
                     channel_mask=5)


def model(texels, p, world, dabs=None, whole_map=False):
    """(texels, rect, detail) of the model."""
    detail = {}
    out, rect = nm.noise(texels, p, world, dabs=dabs, whole_map=whole_map, detail=detail)
    return out, rect, detail


def check_preconditions(before, out, p, detail, what, masked=True):
    """Asserted on the model's output alone: the call can tell a wrong kernel from a right one.  More than half of the texels with a
    positive mask change and at least 200 do; no texel with mask 0 and no unselected channel changes; the lattice cells of the first
    octave take both signs on both axes; dropping the last octave moves f at 200 texels or more (p["octaves"] > 1); a masked call leaves
    at least 10 texels with mask 0 inside its rectangle.  Returns the counts, with how many changed bytes ended at 0 and at 255."""
    m = detail["mask"]
    b3, o3 = before.reshape(m.shape + (-1,)), out.reshape(m.shape + (-1,))
    changed = (b3 != o3).any(-1)
    assert not changed[m == 0].any(), what
    for c in range(b3.shape[2]):
        if not p["channel_mask"] >> c & 1:
            assert np.array_equal(b3[..., c], o3[..., c]), (what, c)
    ix, iz = detail["cells"][0]
    counts = dict(masked=int((m > 0).sum()), changed=int(changed.sum()), at_0=int(((o3 == 0) & (b3 != 0)).sum()), at_255=int(((o3 == 255) & (b3 != 255)).sum()),
                  cells_x=(int(ix.min()), int(ix.max())), cells_z=(int(iz.min()), int(iz.max())))
    assert counts["changed"] >= 200 and 2 * counts["changed"] > counts["masked"], (what, counts)
    assert ix.min() < 0 <= ix.max() and iz.min() < 0 <= iz.max(), (what, counts)
    if p["octaves"] > 1:
        fewer = nm.fractal_of(dict(p, octaves=p["octaves"] - 1), detail["world"], m.shape[1], m.shape[0])
        counts["f_moved_by_last_octave"] = int((fewer != detail["f"]).sum())
        assert counts["f_moved_by_last_octave"] >= 200, (what, counts)
    if masked:
        x, y, w, h = detail["rect"]
        counts["mask_0_in_rect"] = int((m[y:y + h, x:x + w] == 0).sum())
        assert counts["mask_0_in_rect"] >= 10, (what, counts)
    return counts


def run_model(texels, p, world, dabs=None, whole_map=False):
    """model(), its detail extended by what check_preconditions reads."""
    out, rect, detail = model(texels, p, world, dabs=dabs, whole_map=whole_map)
    detail.update(world=world, rect=rect)
    return out, rect, detail
