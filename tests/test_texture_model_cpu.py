"""CPU tests of the texturing model alone (tests/texture_model.py, tests/texture_cases.py): they need neither the library nor
vr_texture.h.  The model has the properties the definition states, and the cases of tests/test_terrain_texture_gpu.py meet their
preconditions on the model's output, on the oracle's synthetic maps - so that no GPU test can pass emptily."""
import numpy as np
import pytest

from tests import texture_cases as tc
from tests import texture_model as tm

WORLD, MAX_HEIGHT = 64.0, 12.5


def test_model_properties():
    """A mask of 0 writes nothing; layers that all weigh 0 keep every byte; opacity 1 in a hard band puts the colour itself."""
    rng = np.random.default_rng(5)
    hm = rng.integers(0, 256, (45, 67), dtype=np.uint8)
    al = rng.integers(0, 256, (50, 33, 4), dtype=np.uint8)
    out, rect = tm.texture(hm, al, tc.zero_layers(MAX_HEIGHT), MAX_HEIGHT, WORLD, whole_map=True)
    assert rect == (0, 0, 33, 50) and np.array_equal(out, al)
    everything = [tm.layer((7.0, 99.0, 200.0, 255.0), 1.0, -1.0, 2.0 * MAX_HEIGHT, 0.0, 0.0, 89.0, 0.0, 0b1010)]
    miss = np.float32([[5.0 * WORLD, 0.0, 3.0, 0.0, 1.0]])
    out, rect = tm.texture(hm, al, everything, MAX_HEIGHT, WORLD, dabs=miss)
    assert rect == (0, 0, 0, 0) and np.array_equal(out, al)
    out, rect = tm.texture(hm, al, everything, MAX_HEIGHT, WORLD, dabs=np.zeros((0, 5), np.float32))
    assert rect == (0, 0, 0, 0) and np.array_equal(out, al)
    out, _ = tm.texture(hm, al, everything, MAX_HEIGHT, WORLD, whole_map=True)
    steep = tm.sample(hm, al.shape, MAX_HEIGHT, WORLD)[1] > np.float32(np.tan(np.radians(89.0)) ** 2)
    assert (out[~steep][:, 1] == 99).all() and (out[~steep][:, 3] == 255).all() and np.array_equal(out[..., 0], al[..., 0]) and np.array_equal(out[..., 2], al[..., 2])


@pytest.mark.parametrize("name", tc.SCENES)
def test_the_gpu_cases_meet_their_preconditions_on_the_model(oracle, name):
    """The scenes of tests/test_terrain_texture_gpu.py made from the oracle's synthetic maps: under the five dabs and over the whole
    map the model alone changes at least 200 texels, leaves 30 between 0 and 255, lets every layer be the last to change 10 texels,
    puts 10 texels on each kind of fade and 10 on a clamped edge; the zero layers change nothing; the scenes reach both variants."""
    hm, al = tc.scene_maps(name, oracle.synth_heightmap, oracle.synth_albedo)
    mh, world = tc.max_height(name), tc.WORLD[name]
    layers = tc.four_layers(hm, al.shape, mh, world)
    for kw in (dict(dabs=tc.five_dabs(al.shape, world, tc.DAB_SCALE[name])), dict(whole_map=True)):
        out, _, detail = tc.model(hm, al, layers, mh, world, **kw)
        tc.check_preconditions(al, out, layers, detail, name, tc.REACHES_EDGE[name])
    out, _, _ = tc.model(hm, al, tc.zero_layers(mh), mh, world, whole_map=True)
    assert np.array_equal(out, al)
    assert tc.staged_footprint(hm.shape, al.shape) == (name not in ("fine", "wide"))
