"""CPU tests of the stamp model alone (tests/stamp_model.py, tests/stamp_cases.py): they need neither the library nor vr_stamp.h.
The model has the properties the definition states, and the cases of tests/test_terrain_stamp_gpu.py meet their preconditions on
the model's output, on the oracle's synthetic maps - so that no GPU test can pass emptily."""
import numpy as np
import pytest

from tests import stamp_cases as sc
from tests import stamp_model as sm


def test_model_properties():
    """A stamp that misses the map changes nothing and has a zero rectangle; opacity 0 keeps every byte; a stamp laid texel on texel
    with opacity 1 and a hard edge puts its own bytes, and nothing else changes; channels outside the mask keep their bytes."""
    rng = np.random.default_rng(3)
    hm = rng.integers(0, 256, (45, 67), dtype=np.uint8)
    st = rng.integers(0, 256, (16, 24), dtype=np.uint8)
    out, rect = sm.stamp(hm, st, sc.place(hm.shape, 64.0, -50.0, 10.0, 24.0, 16.0, 30.0), 64.0)
    assert rect == (0, 0, 0, 0) and np.array_equal(out, hm)
    out, rect = sm.stamp(hm, st, sc.place(hm.shape, 64.0, 30.0, 20.0, 24.0, 16.0, 30.0, opacity=0.0, feather=0.5), 64.0)
    assert rect != (0, 0, 0, 0) and np.array_equal(out, hm)
    sq = rng.integers(0, 256, (64, 64), dtype=np.uint8)                 # texel on texel needs a power-of-two map: every constant is exact
    out, rect = sm.stamp(sq, st, sc.place(sq.shape, 64.0, 10 + 12 - 0.5, 20 + 8 - 0.5, 24.0, 16.0, 0.0), 64.0)
    want = sq.copy()
    want[20:36, 10:34] = st
    assert np.array_equal(out, want) and rect == (8, 18, 28, 20)
    al = rng.integers(0, 256, (50, 33, 4), dtype=np.uint8)
    rgba = rng.integers(0, 256, (17, 33, 4), dtype=np.uint8)
    out, _ = sm.stamp(al, rgba, sc.place(al.shape, 64.0, 16.0, 25.0, 20.0, 20.0, 45.0, channel_mask=0b0101), 64.0)
    assert np.array_equal(out[..., 1], al[..., 1]) and np.array_equal(out[..., 3], al[..., 3]) and (out[..., 0] != al[..., 0]).sum() >= 30


def _maps(oracle, scene):
    return sc.scene_maps(scene, oracle.synth_heightmap, oracle.synth_albedo)


@pytest.mark.parametrize("scene", sc.SCENES)
def test_the_gpu_cases_meet_their_preconditions_on_the_model(oracle, scene):
    """Every call of tests/test_terrain_stamp_gpu.py on the oracle's synthetic maps: the model alone changes at least 30 texels, has
    fractional taps, weights on the feather, clamps that bind at both ends for ADD and SUB and uncovered texels in a rotated
    rectangle; the stamp outside the map has a zero rectangle."""
    hm, al = _maps(oracle, scene)
    world = sc.WORLD[scene]
    for op_index in range(len(sc.OPS)):
        cur = hm
        for call in sc.op_sequence(scene, op_index, hm.shape):
            out, rect, detail = sc.model(cur, call, world)
            sc.check_preconditions(cur, out, call, detail, f"{scene}, {call['name']}")
            cur = out
    for call in sc.albedo_calls(scene, al.shape):
        out, rect, detail = sc.model(al, call, world)
        sc.check_preconditions(al, out, call, detail, f"{scene}, {call['name']}")
    for call in sc.variant_calls(scene, hm.shape):
        out, rect, detail = sc.model(hm, call, world)
        sc.check_preconditions(hm, out, call, detail, f"{scene}, {call['name']}")
    out, rect = sm.stamp(hm, sc.stamp_texels(33, 17), sc.miss_params(scene, hm.shape), world)
    assert rect == (0, 0, 0, 0) and np.array_equal(out, hm)
