"""GPU tests of vr_terrain_occlusion.  The albedo with the occlusion baked in must equal the numpy float32 model
(tests/occlusion_model.py) in every byte - no tolerance anywhere: the march is integer arithmetic, vr_occlusion.h's fp32 runs in a
fixed order, and a texel is a pure function of the two maps, so neither the tile nor where the kernel reads its height bytes from
(LDS or memory) may show.  Scenes and test bodies are those of tests/level0_common.py where they fit; the calls are
tests/occlusion_cases.py's, whose preconditions are asserted on the model's output (and, without a device, in
tests/test_occlusion_model_cpu.py)."""
import numpy as np
import pytest

from tests import brush_model as bm
from tests import level0_common as lc
from tests import occlusion_cases as oc
from tests import occlusion_model as om
from tests import texture_cases as tc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scenes(gpu_ctx):
    out = lc.make_scenes(gpu_ctx, oc.SCENES, oc.WORLD)
    for n, sc in out.items():
        assert sc.mh == oc.max_height(n)
    return out


def apply(tp, which, call):
    """One vr_terrain_occlusion with the parameters of tests/occlusion_model.params."""
    assert which == "albedo"
    _, dabs, p, whole, mh = call
    return tp.Occlusion(dabs, radius=p["radius"], max_height=mh, gain=p["gain"], bias=p["bias"], opacity=p["opacity"], color=p["color"],
                        channels=p["channel_mask"], directions=p["directions"], mode=p["mode"], whole_map=whole)


OCCLUSION = lc.Level0Op("vr_terrain_occlusion", apply, oc.run_model)


def preconditions(sc, call, kind, staged):
    def check(before, want, detail, what):
        assert oc.staged(sc.hm.shape, sc.al.shape, call[2], call[4], lc.world_of(sc)) == staged, what
        return oc.check_preconditions(before, want, call, OCCLUSION.model(before, call, lc.world_of(sc))[1], detail, what, kind)
    return check


def check_call(sc, call, what, kind, staged):
    """One call: the model's rectangle and bytes, the heightmap untouched.  Returns the model's detail."""
    S = lc.world_of(sc)
    want, want_rect, detail = OCCLUSION.model(sc.al, call, S)
    print(what, preconditions(sc, call, kind, staged)(sc.al, want, detail, what))
    a = sc.terrain(sc.hm, sc.al, cast=False, render=False)
    assert apply(a, "albedo", call) == tuple(want_rect), what
    lc.assert_bytes(lc.level0(a, "albedo"), want, what)
    lc.assert_bytes(lc.level0(a, "height"), sc.hm, f"{what}: the heightmap")
    a.close()
    return detail


@pytest.mark.parametrize("name", oc.SCENES)
def test_bytes_equal_the_model_under_five_dabs(scenes, name):
    """1. TINT with 16 directions into channels 0 and 2 under five dabs: level 0 of the albedo equals the model in every byte, channels
    1 and 3 and the heightmap are untouched, the rectangle is the model's, and the mip chain is that of a terrain created from the
    model's albedo."""
    sc = scenes[name]
    call = oc.five_dabs_call(name, sc.hm, sc.al)
    lc.check_albedo_call(sc, OCCLUSION, call, f"{name}, occlusion under five dabs", preconditions(sc, call, "dabs", oc.STAGED[name]))


@pytest.mark.parametrize("name", oc.SCENES)
def test_the_whole_map_stored_into_one_channel(scenes, name):
    """2. VR_OCCLUSION_WHOLE_MAP, STORE into channel 3 alone: every byte equals the model, channels 0 .. 2 are untouched, and the
    rectangle is the whole map."""
    sc = scenes[name]
    call = oc.store_call(name, sc.hm)
    want = OCCLUSION.model(sc.al, call, lc.world_of(sc))
    assert np.array_equal(want[0][..., :3], sc.al[..., :3]) and want[1] == (0, 0, sc.al.shape[1], sc.al.shape[0])
    check_call(sc, call, f"{name}, stored", "whole", oc.STAGED[name])


@pytest.mark.parametrize("name,what", [("fast64", "4 directions"), ("fast64", "8 directions"), ("odd", "bias 0.25"), ("odd", "gain 4")])
def test_directions_bias_and_gain(scenes, name, what):
    """3. 4 and 8 directions on fast64; a bias of 0.25 and a gain of 4 on odd - where the model has texels with o = 1 and texels
    between."""
    sc = scenes[name]
    check_call(sc, oc.variant_calls(name, sc.hm)[what], f"{name}, {what}", "gain" if "gain" in what else "whole", oc.STAGED[name])


@pytest.mark.parametrize("name,radius,staged", oc.LONG)
def test_long_reach(scenes, name, radius, staged):
    """4. A reach of 64 height texels: on multi through the 161 x 137-byte staged footprint; on fine through direct loads, its
    footprint being above 32 KiB; on fast64 with every march leaving the map."""
    sc = scenes[name]
    d = check_call(sc, oc.long_call(name, sc.hm, radius), f"{name}, radius {radius:g}", "long", staged)
    assert max(d["prepared"]["reach"]) == 64
    if name == "fast64":
        assert (d["skipped"][[0, 4, 8, 12]] > 0).all()


def test_order_with_nothing_between(scenes):
    """5. A RAISE stroke on the heightmap, the occlusion, then a PAINT stroke on the albedo, queued back to back with no host wait:
    the bytes are the model's chain, which differs in at least 30 bytes from the chain with the occlusion computed on the unstroked
    heightmap."""
    sc = scenes["odd"]
    S = lc.world_of(sc)
    stroke = lc.five_dabs(sc.hm.shape, S, bm.RAISE)
    paint = lc.five_dabs(sc.al.shape, S, bm.PAINT)
    kw = lc.STROKE_KW[bm.PAINT]
    raised, _ = bm.stroke(sc.hm, bm.RAISE, stroke, S)
    call = oc.call(raised, sc.mh, whole_map=True, gain=2.0)
    occluded, rect, _ = OCCLUSION.model(sc.al, call, S)
    want, paint_rect = bm.stroke(occluded, bm.PAINT, paint, S, **kw)
    stale = bm.stroke(OCCLUSION.model(sc.al, oc.call(sc.hm, sc.mh, whole_map=True, gain=2.0), S)[0], bm.PAINT, paint, S, **kw)[0]
    assert (stale != want).sum() >= 30 and (want != occluded).sum() >= 30
    a = sc.terrain(sc.hm, sc.al)
    a.Brush("raise", stroke)
    assert apply(a, "albedo", call) == tuple(rect)
    assert a.Brush("paint", paint, color=kw["color"], channels=kw["channels"]) == tuple(paint_rect)
    lc.assert_bytes(lc.level0(a, "albedo"), want, "raise, occlusion, paint")
    lc.assert_bytes(lc.level0(a, "height"), raised, "raise, occlusion, paint: the heightmap")
    a.close()


def test_history(scenes):
    """6. Enable, occlusion, commit: one record and one step; undo restores the albedo's bytes and redo gives the model's; the
    heightmap is never touched - under dabs and over the whole map."""
    sc = scenes["odd"]
    S = lc.world_of(sc)
    for call in (oc.five_dabs_call("odd", sc.hm, sc.al), oc.call(sc.hm, sc.mh, whole_map=True)):
        want = OCCLUSION.model(sc.al, call, S)[0]
        assert (want != sc.al).any(-1).sum() >= 200
        a = sc.terrain(sc.hm, sc.al, cast=False, render=False)
        a.EnableHistory(1 << 20)
        apply(a, "albedo", call)
        assert a.HistoryStatus()["open_records"] == 1
        a.CommitHistory()
        st = a.HistoryStatus()
        assert (st["undo_steps"], st["redo_steps"], st["open_records"]) == (1, 0, 0)
        lc.assert_bytes(lc.level0(a, "albedo"), want, "occluded")
        assert a.Undo()
        lc.assert_bytes(lc.level0(a, "albedo"), sc.al, "undone")
        lc.assert_bytes(lc.level0(a, "height"), sc.hm, "undone: the heightmap")
        assert a.Redo() and not a.Redo()
        lc.assert_bytes(lc.level0(a, "albedo"), want, "redone")
        lc.assert_bytes(lc.level0(a, "height"), sc.hm, "the heightmap")
        a.close()


def test_calls_that_launch_nothing(scenes):
    """7. On a real terrain with history on: n == 0 and dabs beside the map return a zero rectangle; a radius that reaches 65 texels,
    directions = 5, mode 2 and a NaN gain are refused with the entry point's name; every byte and the history's status stay as they
    were.  Then a good call still gives the model's bytes."""
    sc = scenes["fast64"]
    S = lc.world_of(sc)
    good = oc.five_dabs_call("fast64", sc.hm, sc.al)
    hm, dabs, p, _, mh = good
    beside = np.float32([tc.dab(sc.al.shape, S, -40.0, 5.0, 3.0, 0.0, 1.0), tc.dab(sc.al.shape, S, 10.5, 12.5, 0.2, 0.0, 1.0)])
    a = sc.terrain(sc.hm, sc.al, cast=False, render=False)
    a.EnableHistory(1 << 20)
    before = a.HistoryStatus()
    for call in ((hm, np.zeros((0, 5), np.float32), p, False, mh), (hm, beside, p, False, mh)):
        assert oc.run_model(sc.al, call, S)[1] == (0, 0, 0, 0)
        assert apply(a, "albedo", call) == (0, 0, 0, 0)
    assert om.prepare(dict(p, radius=65.0), mh, S, sc.hm.shape[1], sc.hm.shape[0])["refused"]
    for bad in (dict(radius=65.0), dict(directions=5), dict(mode=2), dict(gain=float("nan"))):
        for d, whole in ((dabs, False), (None, True)):
            with pytest.raises(Exception) as e:
                apply(a, "albedo", (hm, d, dict(p, **bad), whole, mh))
            assert OCCLUSION.entry in str(e.value), e.value
    lc.assert_bytes(lc.level0(a, "albedo"), sc.al, "after calls that launch nothing")
    lc.assert_bytes(lc.level0(a, "height"), sc.hm, "after calls that launch nothing: the heightmap")
    assert a.HistoryStatus() == before
    want, want_rect, _ = OCCLUSION.model(sc.al, good, S)
    assert apply(a, "albedo", good) == tuple(want_rect)
    lc.assert_bytes(lc.level0(a, "albedo"), want, "after a good call")
    a.close()


def test_three_hundred_dabs_in_either_order(scenes):
    """8. 300 dabs, which span two chunks of the walk, in list order and reversed: the same bytes, which are the model's.  The
    rectangle holds tiles no dab meets: the tiles that stage nothing and march nothing."""
    sc = scenes["fast64"]
    S = lc.world_of(sc)
    dabs = lc.order_dabs(sc.al.shape, S, (0.9, 0.3, 0.65, 1.0, 0.15))
    call = oc.call(sc.hm, sc.mh, dabs=dabs, gain=2.0)
    want, want_rect, detail = OCCLUSION.model(sc.al, call, S)
    m = detail["mask"]
    assert (want != sc.al).any(-1).sum() >= 200 and ((m > 0) & (m < 1)).sum() >= 100
    x, y, w, h = want_rect
    empty = [(tx, ty) for ty in range(y, y + h, 8) for tx in range(x, x + w, 32) if not (m[ty:min(ty + 8, y + h), tx:min(tx + 32, x + w)] > 0).any()]
    assert empty, "every tile of the rectangle holds a masked texel"
    assert np.array_equal(want, OCCLUSION.model(sc.al, oc.call(sc.hm, sc.mh, dabs=dabs[::-1], gain=2.0), S)[0])
    got = []
    for rows in (dabs, dabs[::-1]):
        a = sc.terrain(sc.hm, sc.al, cast=False, render=False)
        assert apply(a, "albedo", oc.call(sc.hm, sc.mh, dabs=rows, gain=2.0)) == tuple(want_rect)
        got.append(lc.level0(a, "albedo"))
        a.close()
    lc.assert_bytes(got[0], want, "300 dabs")
    lc.assert_bytes(got[1], got[0], "300 dabs reversed")
