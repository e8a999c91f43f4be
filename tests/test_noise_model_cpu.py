"""CPU tests of the noise model alone (tests/noise_model.py, tests/noise_cases.py): they need neither the library nor vr_noise.h.
The model has the properties the definition states, and the cases of tests/test_terrain_noise_gpu.py meet their preconditions on the
model's output, on the oracle's synthetic maps - so that no GPU test can pass emptily."""
import numpy as np
import pytest

from tests import noise_cases as nc
from tests import noise_model as nm

F = np.float32
WORLD = 128.0


def test_the_gradient_basis_is_zero_at_lattice_points():
    """Frequency 1/8 on a 128^2 map of a world of 128 with offset 0.5: texel i's centre is at lattice coordinate (i + 1) / 8 - 8, an exact
    fp32 value, so every eighth texel sits on a lattice point - there the gradient basis is 0, and the value basis is the corner's own
    value (not 0: the two bases differ there)."""
    p = nm.params(1.0 / 8.0, 100.0, octaves=1, offset=(0.5, 0.5), seed=3, basis=nm.GRADIENT)
    d = {}
    nm.fractal_of(p, WORLD, 128, 128, d)
    on = np.arange(7, 128, 8)
    assert np.array_equal(d["prepared"]["sx"], F([0.125])) and np.array_equal(d["prepared"]["ox"], F([-7.9375]))
    n = d["n"][0]
    assert not n[np.ix_(on, on)].any() and np.count_nonzero(n) > n.size // 2
    dv = {}
    nm.fractal_of(dict(p, basis=nm.VALUE), WORLD, 128, 128, dv)
    assert np.count_nonzero(dv["n"][0][np.ix_(on, on)]) >= 200


@pytest.mark.parametrize("basis", (nm.VALUE, nm.GRADIENT), ids=("value", "gradient"))
def test_neighbouring_texels_differ_by_a_bounded_step(basis):
    """One cell per 64 texels, one octave (a_0 = 1, so f = n).  Along an axis n is q_a + fade(t) (q_b - q_a) in each of the two rows it
    interpolates, so |dn/dt| <= max |fade'| * |q_b - q_a| plus, for the gradient basis, the corners' own slopes.  fade'(t) = 30 t^2
    (1 - t)^2 <= 30 / 16 = 1.875 (at t = 1/2).  VALUE: |q_b - q_a| <= 2, so |dn/dt| <= 3.75.  GRADIENT: a corner's dot product has
    slope |g| <= 1 and magnitude <= |offset| <= sqrt 2, so |dn/dt| <= sqrt 2 * (1 + 1.875 * 2 sqrt 2 + 1) < 10.4.  fade' is 0 at both
    ends of a cell and n is continuous across it, so a step of 1/64 cell changes n by at most bound / 64 anywhere (mean value
    theorem), plus 1e-5 for the roundings.  A lattice that broke at the cell edges would jump by up to 2."""
    bound = (3.75 if basis == nm.VALUE else 10.4) / 64.0 + 1e-5
    p = nm.params(1.0 / 64.0, 100.0, octaves=1, offset=(20.3, -11.7), seed=11, basis=basis)
    d = {}
    f = nm.fractal_of(p, WORLD, 128, 128, d).astype(np.float64)
    ix, iz = d["cells"][0]
    assert len(set(ix)) >= 3 and len(set(iz)) >= 3 and ix.min() < 0 <= ix.max()           # cell edges, of both signs, are crossed
    step = max(np.abs(np.diff(f, axis=0)).max(), np.abs(np.diff(f, axis=1)).max())
    assert 0.25 * bound / (1.0 if basis == nm.VALUE else 4.0) < step <= bound, (step, bound)


def test_every_octave_contributes():
    """Dropping the last octave changes bytes, for every octave count the GPU cases use (tests/noise_cases.py) and for 2.  The weakest
    is octave 12 at gain 0.5 and amplitude 150: it moves a value by about 150 / 2^12 * |n| ~ 0.01 stored units, so it flips about one
    byte in a hundred of the 4096 through the rounding - a few dozen; at least 10 are asked for."""
    rng = np.random.default_rng(9)
    hm = rng.integers(40, 216, (64, 64), dtype=np.uint8)
    for octaves in sorted(set(nc.GPU_OCTAVES + (2,)) - {1}):
        for p in (nc.height_params("fast64", nm.GRADIENT, nm.FBM, octaves=octaves), dict(nc.whole_params("fast64"), octaves=octaves)):
            full, _ = nm.noise(hm, p, 64.0, whole_map=True)
            fewer, _ = nm.noise(hm, dict(p, octaves=octaves - 1), 64.0, whole_map=True)
            assert (full != fewer).sum() >= 10, (octaves, (full != fewer).sum())
    assert {nc.height_params("fast64", 0, 0)["octaves"], nc.whole_params("fast64")["octaves"], nc.albedo_params("fast64")["octaves"]} <= set(nc.GPU_OCTAVES)


def test_the_six_combinations_differ():
    hm = np.full((64, 64), 128, np.uint8)
    outs = [nm.noise(hm, nc.height_params("fast64", b, f), 64.0, whole_map=True)[0] for b, f in nc.COMBOS]
    for i in range(len(outs)):
        for j in range(i):
            assert (outs[i] != outs[j]).sum() >= 1000, (nc.COMBO_IDS[i], nc.COMBO_IDS[j])


def test_a_texel_s_noise_does_not_depend_on_the_mask():
    """The same texel under two different dab sets - other rectangles, other masks - gets the same f; and where both masks are 1 the
    same byte."""
    rng = np.random.default_rng(10)
    hm = rng.integers(0, 256, (45, 67), dtype=np.uint8)
    p = nc.height_params("odd", nm.GRADIENT, nm.BILLOW)
    a, b = {}, {}
    one = np.float32([nc.dab(hm.shape, 64.0, 20.0, 20.0, 14.0, 0.9, 1.0)])
    two = np.float32([nc.dab(hm.shape, 64.0, 30.0, 25.0, 18.0, 0.9, 1.0), nc.dab(hm.shape, 64.0, 60.0, 5.0, 4.0, 0.0, 0.5)])
    oa, ra = nm.noise(hm, p, 64.0, dabs=one, detail=a)
    ob, rb = nm.noise(hm, p, 64.0, dabs=two, detail=b)
    assert ra != rb and np.array_equal(a["f"].view(np.uint32), b["f"].view(np.uint32))
    both = (a["mask"] == 1) & (b["mask"] == 1)
    assert both.sum() >= 100 and np.array_equal(oa[both], ob[both]) and (oa[both] != hm[both]).sum() >= 50


def test_zero_amplitude_and_misses_change_nothing():
    rng = np.random.default_rng(11)
    hm = rng.integers(0, 256, (45, 67), dtype=np.uint8)
    al = rng.integers(0, 256, (50, 33, 4), dtype=np.uint8)
    for texels, mask in ((hm, 1), (al, 15)):
        p = dict(nc.height_params("odd", nm.VALUE, nm.FBM), amplitude=0.0, channel_mask=mask)
        out, rect = nm.noise(texels, p, 64.0, whole_map=True)
        assert rect == (0, 0) + texels.shape[1::-1] and np.array_equal(out, texels)
        out, rect = nm.noise(texels, dict(p, amplitude=99.0), 64.0, dabs=np.float32([[5.0 * 64.0, 0.0, 3.0, 0.0, 1.0]]))
        assert rect == (0, 0, 0, 0) and np.array_equal(out, texels)
        out, rect = nm.noise(texels, dict(p, amplitude=99.0), 64.0, dabs=np.zeros((0, 5), np.float32))
        assert rect == (0, 0, 0, 0) and np.array_equal(out, texels)
    # BLEND with amplitude 0 and mask 1 puts `base` itself
    out, _ = nm.noise(hm, dict(nc.height_params("odd", nm.VALUE, nm.FBM, op=nm.BLEND), amplitude=0.0, base=77.0), 64.0, whole_map=True)
    assert (out == 77).all()


def test_the_range_refusal_is_the_stated_bound():
    p = nm.params(1.0, 1.0, octaves=12, lacunarity=4.0)                # octave 11: 4^11 cells per world unit, 32 units to the edge
    assert not nm.in_range(nm.prepare(p, 64.0, 64, 64), 64, 64)
    assert nm.in_range(nm.prepare(dict(p, octaves=8), 64.0, 64, 64), 64, 64)          # 4^7 * 31.5 = 516096 < 2^22


def test_the_gpu_cases_meet_their_preconditions_on_the_model(oracle):
    """The scenes of tests/test_terrain_noise_gpu.py made from the oracle's synthetic maps: in each case more than half of the masked
    texels change and cells of both signs occur, each masked case leaves mask-0 texels inside its rectangle, the last octave moves f;
    over all cases some byte clamps at 0 and some at 255."""
    at_0 = at_255 = 0
    for name in nc.SCENES:
        hm, al = nc.scene_maps(name, oracle.synth_heightmap, oracle.synth_albedo)
        S = nc.WORLD[name]
        cases = [(hm, nc.height_params(name, *combo), dict(dabs=nc.five_dabs(hm.shape, S))) for combo in (nc.COMBOS if name == "fast64" else [nc.scene_combo(name)])]
        cases += [(hm, nc.whole_params(name), dict(whole_map=True)), (al, nc.albedo_params(name), dict(dabs=nc.five_dabs(al.shape, S)))]
        for texels, p, kw in cases:
            out, rect, detail = nc.run_model(texels, p, S, **kw)
            counts = nc.check_preconditions(texels, out, p, detail, (name, p["basis"], p["fractal"], p["op"]), masked="dabs" in kw)
            at_0 += counts["at_0"]
            at_255 += counts["at_255"]
    assert at_0 >= 10 and at_255 >= 10, (at_0, at_255)
