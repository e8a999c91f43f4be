"""GPU tests of vr_terrain_texture.  The textured albedo must equal the numpy float32 model (tests/texture_model.py) in every byte - no
tolerance anywhere: vr_texture.h's arithmetic is IEEE fp32 in a fixed order, and a texel is a pure function of the two maps, so
neither the tile nor where the kernel reads its height bytes from (LDS or memory) may show.  Scenes and helpers are those of
tests/level0_common.py, with tests/texture_cases.py's two scenes that run the direct-load variant; the preconditions of
every case are asserted on the model's output (and, without a device, in tests/test_terrain_texture_cpu.py)."""
import numpy as np
import pytest

from tests import erode_model as em
from tests import texture_cases as tc
from tests.level0_common import assert_bytes, assert_chains_equal, assert_frames_equal, assert_tables_equal, level0, make_scenes, order_dabs, render, world_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scenes(gpu_ctx):
    out = make_scenes(gpu_ctx, tc.SCENES, tc.WORLD)
    for n, sc in out.items():
        assert sc.mh == tc.max_height(n)
        assert tc.staged_footprint(sc.hm.shape, sc.al.shape) == (n not in ("fine", "wide"))
    return out


_MODEL = {}


def model(sc, hm=None, layers=None, dabs=None, whole_map=False):
    """The model's (albedo, rect, detail, layers) of one call on scene `sc`, computed once per distinct call."""
    hm = sc.hm if hm is None else hm
    layers = tc.four_layers(sc.hm, sc.al.shape, sc.mh, world_of(sc)) if layers is None else layers
    key = (sc.name, hm.tobytes(), repr(layers), None if dabs is None else np.asarray(dabs, np.float32).tobytes(), whole_map)
    if key not in _MODEL:
        _MODEL[key] = tc.model(hm, sc.al, layers, sc.mh, world_of(sc), dabs=dabs, whole_map=whole_map) + (layers,)
    return _MODEL[key]


@pytest.mark.parametrize("name", tc.SCENES)
def test_bytes_equal_the_model_under_five_dabs(scenes, name):
    """1. Four layers under five dabs: the albedo's level 0 equals the model in every byte, the heightmap is untouched, the rectangle
    is the model's."""
    sc = scenes[name]
    dabs = tc.five_dabs(sc.al.shape, world_of(sc), tc.DAB_SCALE[name])
    want, want_rect, detail, layers = model(sc, dabs=dabs)
    print(name, tc.check_preconditions(sc.al, want, layers, detail, name, tc.REACHES_EDGE[name]))
    a = sc.terrain(sc.hm, sc.al, cast=False, render=False)
    rect = a.Texture(layers, dabs, max_height=sc.mh)
    assert rect == tuple(want_rect), (rect, want_rect)
    assert_bytes(level0(a, "albedo"), want, f"{name}, texture under five dabs")
    assert_bytes(level0(a, "height"), sc.hm, f"{name}, texture: the heightmap")
    b = sc.terrain(sc.hm, want, cast=False, render=False)
    assert_tables_equal(a, b, f"{name}, texture under five dabs")
    a.close(); b.close()


@pytest.mark.parametrize("name", tc.SCENES)
def test_bytes_equal_the_model_over_the_whole_map(scenes, name):
    """2. VR_TEXTURE_WHOLE_MAP: every byte equals the model, the rectangle is the whole map, and every mip level of the albedo is that
    of a terrain created from the model's albedo."""
    sc = scenes[name]
    want, want_rect, detail, layers = model(sc, whole_map=True)
    print(name, tc.check_preconditions(sc.al, want, layers, detail, name, tc.REACHES_EDGE[name]))
    a = sc.terrain(sc.hm, sc.al, cast=False, render=False)
    rect = a.Texture(layers, max_height=sc.mh, whole_map=True)
    assert rect == tuple(want_rect) == (0, 0, sc.al.shape[1], sc.al.shape[0]), (rect, want_rect)
    assert_bytes(level0(a, "albedo"), want, f"{name}, texture over the whole map")
    assert_bytes(level0(a, "height"), sc.hm, f"{name}, texture: the heightmap")
    b = sc.terrain(sc.hm, want, cast=False, render=False)
    assert_chains_equal(a, b, f"{name}, texture over the whole map")
    assert_tables_equal(a, b, f"{name}, texture over the whole map")
    a.close(); b.close()


def test_an_erode_then_a_texture_with_nothing_between(scenes):
    """3. Erode then Texture back to back, no host wait between: the texture kernel reads the eroded heightmap - the model applied to
    erode_model's map, which differs from the model applied to the map before the erosion - and a 256 x 144 frame has every G-buffer
    plane equal to that of a terrain created from the model's two maps."""
    sc = scenes["odd"]
    S = world_of(sc)
    mask = tc.five_dabs(sc.hm.shape, S)
    eroded, _ = em.erode(sc.hm, mask, S, 20, 0.5, 0.125)
    assert (eroded != sc.hm).sum() >= 30
    want, want_rect, detail, layers = model(sc, hm=eroded, whole_map=True)
    print(tc.check_preconditions(sc.al, want, layers, detail, "odd, eroded"))
    stale = model(sc, whole_map=True)[0]
    assert (stale != want).any(-1).sum() >= 30                       # a kernel that overtook the erosion would show
    a = sc.terrain(sc.hm, sc.al)
    a.Erode(mask, 20, 0.5, 0.125)
    assert a.Texture(layers, max_height=sc.mh, whole_map=True) == tuple(want_rect)
    assert_bytes(level0(a, "albedo"), want, "erode, texture")
    assert_bytes(level0(a, "height"), eroded, "erode, texture: the heightmap")
    b = sc.terrain(eroded, want)
    assert_frames_equal(render(sc, a, 0), render(sc, b, 0), "erode, texture: the frame")
    a.close(); b.close()


def test_history(scenes):
    """4. Enable, texture, commit, undo: the original albedo bytes; redo: the model's.  One call is one record and one step - under
    dabs and over the whole map."""
    sc = scenes["odd"]
    dabs = tc.five_dabs(sc.al.shape, world_of(sc))
    for kw in (dict(dabs=dabs), dict(whole_map=True)):
        want, _, _, layers = model(sc, **kw)
        assert (want != sc.al).any(-1).sum() >= 200
        a = sc.terrain(sc.hm, sc.al, cast=False, render=False)
        a.EnableHistory(1 << 20)
        a.Texture(layers, max_height=sc.mh, **kw)
        assert a.HistoryStatus()["open_records"] == 1
        a.CommitHistory()
        st = a.HistoryStatus()
        assert (st["undo_steps"], st["redo_steps"], st["open_records"]) == (1, 0, 0)
        assert_bytes(level0(a, "albedo"), want, "textured")
        assert a.Undo()
        assert_bytes(level0(a, "albedo"), sc.al, "undone")
        assert a.Redo() and not a.Redo()
        assert_bytes(level0(a, "albedo"), want, "redone")
        assert_bytes(level0(a, "height"), sc.hm, "the heightmap")
        a.close()


def test_three_hundred_dabs_in_either_order(scenes):
    """5. 300 dabs, which span two chunks of the walk, more than 256 of them on one tile: the model's bytes, and the same bytes from
    the reversed list - a mask texel is a maximum, which has no order."""
    sc = scenes["fast64"]
    S = world_of(sc)
    dabs = order_dabs(sc.al.shape, S, (0.9, 0.3, 0.65, 1.0, 0.15))
    want, want_rect, detail, layers = model(sc, dabs=dabs)
    m = detail["mask"]
    assert (want != sc.al).any(-1).sum() >= 200 and ((m > 0) & (m < 1)).sum() >= 100
    assert np.array_equal(want, model(sc, dabs=dabs[::-1])[0])
    got = []
    for rows in (dabs, dabs[::-1]):
        a = sc.terrain(sc.hm, sc.al, cast=False, render=False)
        assert a.Texture(layers, np.ascontiguousarray(rows), max_height=sc.mh) == tuple(want_rect)
        got.append(level0(a, "albedo"))
        a.close()
    assert_bytes(got[0], want, "300 dabs")
    assert_bytes(got[1], got[0], "300 dabs reversed")


def test_calls_that_change_nothing(scenes):
    """6. Dabs that all miss the map, and n == 0: VR_OK, a zero rectangle, nothing changed.  A whole-map call whose layers all weigh 0
    (bands above every altitude the map can hold): the whole rectangle, every byte as it was.  Then a good call still gives the model's
    bytes."""
    sc = scenes["odd"]
    S = world_of(sc)
    layers = tc.four_layers(sc.hm, sc.al.shape, sc.mh, S)
    a = sc.terrain(sc.hm, sc.al, cast=False, render=False)
    miss = np.float32([tc.dab(sc.al.shape, S, -40.0, 5.0, 3.0, 0.0, 1.0), tc.dab(sc.al.shape, S, 10.5, 12.5, 0.2, 0.0, 1.0)])
    assert tc.model(sc.hm, sc.al, layers, sc.mh, S, dabs=miss)[1] == (0, 0, 0, 0)
    assert a.Texture(layers, miss, max_height=sc.mh) == (0, 0, 0, 0)
    assert a.Texture(layers, np.zeros((0, 5), np.float32), max_height=sc.mh) == (0, 0, 0, 0)
    assert_bytes(level0(a, "albedo"), sc.al, "after calls that miss")
    zero = tc.zero_layers(sc.mh)
    assert np.array_equal(tc.model(sc.hm, sc.al, zero, sc.mh, S, whole_map=True)[0], sc.al)
    assert a.Texture(zero, max_height=sc.mh, whole_map=True) == (0, 0, sc.al.shape[1], sc.al.shape[0])
    assert_bytes(level0(a, "albedo"), sc.al, "after layers that all weigh 0")
    want, want_rect, _, _ = model(sc, whole_map=True)
    assert a.Texture(layers, max_height=sc.mh, whole_map=True) == tuple(want_rect)
    assert_bytes(level0(a, "albedo"), want, "after a good call")
    a.close()
