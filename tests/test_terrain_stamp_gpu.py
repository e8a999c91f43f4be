"""GPU tests of the stamps.  The stamped map must equal the numpy float32 model (tests/stamp_model.py) in every byte - no tolerance
anywhere: vr_stamp.h's arithmetic is IEEE fp32 in a fixed order, and a texel is a pure function of its own map texel and the stamp,
so neither the tile nor the order in which the device visits the texels may show.  Scenes and helpers are those of
tests/level0_common.py; the calls are tests/stamp_cases.py's, whose preconditions are asserted on the model's output (and,
without a device, in tests/test_stamp_model_cpu.py)."""
import numpy as np
import pytest

import vrenderer_amd as vr
from tests import brush_model as bm
from tests import erode_model as em
from tests import queries_common as qc
from tests import stamp_cases as sc
from tests import stamp_model as sm
from tests.f64_queries import Surface64
from tests.fusion_common import both, capture, terrain_fixture, views
from tests.level0_common import assert_bytes, assert_chains_equal, assert_frames_equal, assert_tables_equal, five_dabs, level0, make_scenes, render, world_of
from vrenderer_amd import capi

pytestmark = pytest.mark.gpu
OP_NAMES = [n for n, _ in sc.OPS]


@pytest.fixture(scope="module")
def scenes(gpu_ctx):
    return make_scenes(gpu_ctx, sc.SCENES, sc.WORLD)


def apply(tp, which, stamp, p):
    """One vr_terrain_stamp with a placement of tests/stamp_model.params."""
    return tp.Stamp(which, stamp, p["x"], p["z"], p["size_x"], p["size_z"], p["rotation"], p["opacity"], p["feather"], p["gain"], p["offset"], p["op"],
                    p["channel_mask"], bool(p["flags"] & sm.USE_ALPHA))


def run_calls(s, which, calls, tables=True):
    """The calls one after the other on a fresh terrain of scene `s`: after each, level 0 and the rectangle are the model's and the
    other map is untouched; at the end the chains and tables are those of a terrain created from the model's maps."""
    start = s.hm if which == "height" else s.al
    other, other_map = ("albedo", s.al) if which == "height" else ("height", s.hm)
    a = s.terrain(s.hm, s.al, cast=False, render=False)
    cur = start
    for call in calls:
        what = f"{s.name}, {call['name']}"
        want, want_rect, detail = sc.model(cur, call, world_of(s))
        print(what, sc.check_preconditions(cur, want, call, detail, what))
        st = vr.Stamp(s.ctx, call["stamp"])
        assert apply(a, which, st, call["params"]) == tuple(want_rect), what
        st.close()                                                   # (waits for the call that still reads it)
        assert_bytes(level0(a, which), want, what)
        assert_bytes(level0(a, other), other_map, f"{what}: the other map")
        cur = want
    if tables:
        b = s.terrain(cur, s.al, cast=False, render=False) if which == "height" else s.terrain(s.hm, cur, cast=False, render=False)
        assert_chains_equal(a, b, f"{s.name}, {calls[-1]['name']}")
        assert_tables_equal(a, b, f"{s.name}, {calls[-1]['name']}")
        b.close()
    a.close()
    return cur


@pytest.mark.parametrize("op", range(len(sc.OPS)), ids=OP_NAMES)
@pytest.mark.parametrize("name", sc.SCENES)
def test_each_op_on_the_heightmap(scenes, name, op):
    """1. One op, six calls - stamps of 5x3 and 33x17, angles 0, 30 and 180 degrees, feather 0 and 0.5, centres inside the map, across
    each edge and over a corner: level 0 equals the model after each, the albedo is untouched, the rectangle is the model's, and the
    chains and tables are those of a terrain created from the model's maps."""
    s = scenes[name]
    run_calls(s, "height", sc.op_sequence(name, op, s.hm.shape))


@pytest.mark.parametrize("name", sc.SCENES)
def test_the_albedo(scenes, name):
    """2. BLEND on the albedo with and without VR_STAMP_USE_ALPHA, channel masks 0x7 and 0xF, each on the original map."""
    s = scenes[name]
    for call in sc.albedo_calls(name, s.al.shape):
        run_calls(s, "albedo", [call], tables=call["params"]["flags"] != 0)


def test_the_extremes(scenes):
    """3. A 256^2 stamp squeezed onto 24 texels and turned, the same stamp over the whole map, a 1x1 stamp, a stamp larger than the map
    that covers every texel (the kernel has one variant: it reads the stamp from memory at every ratio).  A stamp wholly outside the
    map: a zero rectangle, no byte changed, no history record."""
    s = scenes["fast64"]
    for call in sc.variant_calls("fast64", s.hm.shape):
        run_calls(s, "height", [call])
    a = s.terrain(s.hm, s.al, cast=False, render=False)
    a.EnableHistory(1 << 20)
    st = vr.Stamp(s.ctx, sc.stamp_texels(33, 17))
    assert st.info() == (capi.VR_STAMP_R8, 33, 17)
    assert apply(a, "height", st, sc.miss_params("fast64", s.hm.shape)) == (0, 0, 0, 0)
    assert a.HistoryStatus()["open_records"] == 0
    assert_bytes(level0(a, "height"), s.hm, "a stamp outside the map")
    st.close(); a.close()


def test_clone(scenes):
    """4. vr_stamp_from_terrain of a 24x16 rectangle read back through vr_stamp_download equals the map's bytes; stamped back in place
    (BLEND, opacity 1, feather 0, angle 0) it changes no byte; stamped 8 texels to the right it is the numpy copy."""
    s = scenes["fast64"]
    S, (x, y, w, h) = world_of(s), (10, 20, 24, 16)
    a = s.terrain(s.hm, s.al, cast=False, render=False)
    st = a.CaptureStamp("height", x, y, w, h)
    assert st.info() == (capi.VR_STAMP_R8, w, h)
    patch = st.download()
    assert_bytes(patch, s.hm[y:y + h, x:x + w], "the captured rectangle")
    assert (patch != s.hm[y:y + h, x + 8:x + 8 + w]).sum() >= 30                 # the shifted copy will show
    in_place = sc.place(s.hm.shape, S, x + w / 2 - 0.5, y + h / 2 - 0.5, float(w), float(h), 0.0)
    want, want_rect = sm.stamp(s.hm, patch, in_place, S)
    assert np.array_equal(want, s.hm)
    assert apply(a, "height", st, in_place) == want_rect
    assert_bytes(level0(a, "height"), s.hm, "stamped back in place")
    shifted = sc.place(s.hm.shape, S, x + 8 + w / 2 - 0.5, y + h / 2 - 0.5, float(w), float(h), 0.0)
    copy = s.hm.copy()
    copy[y:y + h, x + 8:x + 8 + w] = patch
    want, want_rect = sm.stamp(s.hm, patch, shifted, S)
    assert np.array_equal(want, copy)
    assert apply(a, "height", st, shifted) == want_rect
    assert_bytes(level0(a, "height"), copy, "stamped 8 texels to the right")
    # the albedo's clone, from a device pointer with a wide pitch: the same stamp as from the host
    import torch
    rgba = np.ascontiguousarray(s.al[5:5 + 9, 3:3 + 13])
    wide = np.zeros((9, 13 * 4 + 12), np.uint8)
    wide[:, :13 * 4] = rgba.reshape(9, -1)
    t = torch.from_numpy(wide).to(f"cuda:{s.ctx.device}")
    torch.cuda.synchronize()
    d = vr.Stamp(s.ctx, device_ptr=t.data_ptr(), fmt="albedo", w=13, h=9, pitch=wide.shape[1])
    c = a.CaptureStamp("albedo", 3, 5, 13, 9)
    assert_bytes(d.download(), rgba, "a stamp from a device pointer")
    assert_bytes(c.download(), rgba, "a stamp from the albedo")
    for o in (d, c, st, a):
        o.close()


def test_order_with_nothing_between(scenes):
    """5. Erode then Stamp: the stamp's MAX sees the eroded map.  Brush then vr_stamp_from_terrain: the capture holds the brushed
    bytes.  Stamp then a 256x144 frame: every G-buffer plane is that of a terrain created from the model's maps."""
    s = scenes["odd"]
    S = world_of(s)
    mask = five_dabs(s.hm.shape, S, bm.FLATTEN)
    eroded, _ = em.erode(s.hm, mask, S, 20, 0.5, 0.125)
    assert (eroded != s.hm).sum() >= 30
    call = dict(name="max over the erosion", stamp=sc.stamp_texels(33, 17), rotated=True,
                params=sc.place(s.hm.shape, S, 0.5 * s.hm.shape[1], 0.5 * s.hm.shape[0], 52.0, 34.0, 30.0, feather=0.5, op=sm.MAX, gain=0.4, offset=20.0))
    want, want_rect, detail = sc.model(eroded, call, S)
    print(sc.check_preconditions(eroded, want, call, detail, "erode, stamp"))
    stale = sc.model(s.hm, call, S)[0]
    assert (stale != want).sum() >= 30                                # a kernel that overtook the erosion would show
    a = s.terrain(s.hm, s.al)
    st = vr.Stamp(s.ctx, call["stamp"])
    a.Erode(mask, 20, 0.5, 0.125)
    assert apply(a, "height", st, call["params"]) == tuple(want_rect)
    frame = render(s, a, 0)
    assert_bytes(level0(a, "height"), want, "erode, stamp")
    b = s.terrain(want, s.al)
    assert_frames_equal(frame, render(s, b, 0), "erode, stamp: the frame")
    b.close()
    # brush, capture
    stroke = five_dabs(s.hm.shape, S, bm.RAISE)
    brushed, _ = bm.stroke(want, bm.RAISE, stroke, S)
    x, y, w, h = 20, 12, 30, 22
    assert (brushed[y:y + h, x:x + w] != want[y:y + h, x:x + w]).sum() >= 30
    a.Brush("raise", stroke)
    cap = a.CaptureStamp("height", x, y, w, h)
    assert_bytes(cap.download(), brushed[y:y + h, x:x + w], "brush, capture")
    for o in (cap, st, a):
        o.close()


def test_a_stamp_with_a_lazily_fused_frame_pending():
    """5, last part.  A fused frame that left its colour planes to their first reader, then Stamp, then a G-buffer download: the planes
    are those of the eager path (VR_OPT_GBUFFER_LAZY off) - the frame on the terrain as it was; the next frame shows the stamp."""
    w, h = 96, 64
    with terrain_fixture(256) as fx:
        v = views(w, h)
        hm = fx["h"]
        st = vr.Stamp(fx["ctx"], sc.stamp_texels(33, 17))
        p = sc.place(hm.shape, 256.0, 128.0, 128.0, 120.0, 80.0, 30.0, feather=0.5, op=sm.MAX, offset=60.0)
        assert (sm.stamp(hm, sc.stamp_texels(33, 17), p, 256.0)[0] != hm).sum() >= 30

        def script(scn, lazy):
            out = {}
            try:
                scn.submit(v[1])
                apply(scn.tp, "height", st, p)
                out["before the stamp"] = capture(scn.rt, scn.hdr)
                scn.submit(v[1])
                out["after the stamp"] = capture(scn.rt, scn.hdr)
            finally:
                scn.tp.Edit("height", 0, 0, hm)
            return out
        want, _ = both(fx, w, h, script)
        assert not np.array_equal(want["before the stamp"]["normals"], want["after the stamp"]["normals"]), "the stamp is not in view"
        st.close()


def _queries(s, tp, rays):
    """1024 sampled heights and the hits of `rays` (origins, directions, t_max) on a terrain, as bytes."""
    pts = qc.uniform_points(s.world, 1024)
    return tp.SampleHeights(pts, s.mh).tobytes(), tp.CastRays(*rays, s.mh).tobytes()


def test_history(scenes):
    """6. Enable, stamp, commit: one call is one record and one step.  Undo restores every byte, redo gives the model's again; a ray
    cast and a height query after each agree with a terrain created from those maps."""
    s = scenes["fast64"]
    S = world_of(s)
    call = sc.op_sequence("fast64", 1, s.hm.shape)[0]
    want, want_rect, detail = sc.model(s.hm, call, S)
    sc.check_preconditions(s.hm, want, call, detail, "history")
    refs, rays = {}, None
    for key, m in (("original", s.hm), ("stamped", want)):
        b = s.terrain(m, s.al, render=False)
        if rays is None:                                             # aimed at the original surface: the same rays for every terrain
            rays = qc.make_rays(Surface64(b.download_mip("height", 0), b.download_mip("height", 1), s.world, s.mh), s.world, n=64)
        refs[key] = _queries(s, b, rays)
        b.close()
    assert refs["original"] != refs["stamped"]
    a = s.terrain(s.hm, s.al, render=False)
    st = vr.Stamp(s.ctx, call["stamp"])
    a.EnableHistory(1 << 20)
    assert apply(a, "height", st, call["params"]) == tuple(want_rect)
    assert a.HistoryStatus()["open_records"] == 1
    a.CommitHistory()
    hs = a.HistoryStatus()
    assert (hs["undo_steps"], hs["redo_steps"], hs["open_records"]) == (1, 0, 0)
    assert_bytes(level0(a, "height"), want, "stamped")
    assert _queries(s, a, rays) == refs["stamped"]
    assert a.Undo()
    assert_bytes(level0(a, "height"), s.hm, "undone")
    assert _queries(s, a, rays) == refs["original"]
    assert a.Redo() and not a.Redo()
    assert_bytes(level0(a, "height"), want, "redone")
    assert _queries(s, a, rays) == refs["stamped"]
    assert_bytes(level0(a, "albedo"), s.al, "the albedo")
    st.close(); a.close()
