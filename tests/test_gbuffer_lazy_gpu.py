"""VR_OPT_GBUFFER_LAZY: a fused frame leaves the G-buffer's colour planes to their first reader.  The same sequence of calls
with the option off (every fused frame writes the whole G-buffer: the reference) and on must leave the same bytes in every plane,
HdrColor and depth, the same region census and the same knowledge of the emissive plane, whichever call looks first and whatever
happened to the terrain or the target in between.  Which kernels ran comes from the dispatch-stamped timing records: the fused
frame is "k_raster (fused with lighting)" either way, a materialisation is the plain "k_raster"."""
import numpy as np
import pytest

import vrenderer_amd as vr
from tests.common import AMBIENT_BOTTOM, AMBIENT_TOP, flythrough_camera, scaled_camera
from tests.fusion_common import FUSED, PLANES, LazyScene, assert_same_bits, both, capture, terrain_fixture, timed, views

pytestmark = pytest.mark.gpu
PLAIN = "k_raster"
SIZES = [(68, 50), (96, 64), (256, 144)]      # partial tiles at the smallest size the fused plan takes; whole tiles; several tile rows


@pytest.fixture(scope="module")
def fx(product_lib):
    with terrain_fixture(256) as f:
        yield f


def test_the_views_show_sky_and_no_sky(fx):
    w, h = 96, 64
    sc = LazyScene(fx, 0, w, h)
    try:
        cov = []
        for v in views(w, h):
            sc.submit(v)
            cov.append((sc.rt.download("depth") < 1.0).mean())
        assert 0.2 < cov[0] < 1.0 and cov[1] == 1.0 and 0.2 < cov[2] < 1.0, cov
    finally:
        sc.close()


READERS = ("download", "census", "light", "upload", "describe")


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("reader", READERS)
def test_every_kind_of_reader_finds_the_eager_frame(fx, w, h, reader):
    """Two frames with nobody looking (sky, then no sky), the reader, everything the target holds; then a third frame and all
    of it again.  Lazy: the two frames queue no plain tile pass, the reader queues one, and from then on the target's frames
    keep their G-buffer - the capture behind the third frame queues nothing."""
    v = views(w, h)
    foreign = np.random.default_rng(7).integers(0, 1 << 32, (h, w), dtype=np.uint64).astype(np.uint32)

    def script(sc, lazy):
        out = {}
        ran = [sc.submit(v[0]), sc.submit(v[1])]
        assert all(PLAIN not in r and r[FUSED][1] == 1 for r in ran), ran      # no unfused tile pass, option on or off

        def read():
            if reader == "download":
                out["first"] = sc.rt.download("normals").copy()
            elif reader == "census":
                out["first"] = sc.rt.region_census()
            elif reader == "light":
                vr.DeferredLightingPass(sc.ctx).Render(v[1], sc.rt, sc.lights, AMBIENT_TOP, AMBIENT_BOTTOM, sc.hdr2)
                out["first"] = sc.hdr2.download().copy()
            elif reader == "upload":
                sc.rt.upload("specular", foreign)
            else:
                d = sc.rt.describe()
                out["first"] = (d.width, d.height)
        _, r = timed(sc.ctx, read)
        assert (PLAIN in r) == bool(lazy), (reader, sorted(r))                   # the one materialisation
        out["behind the reader"] = capture(sc.rt, sc.hdr)
        if reader == "light":      # the lighting pass over the materialised planes is the fused frame's HdrColor
            assert_same_bits(out["first"], out["behind the reader"]["hdr"], "vr_deferred_light against the fused frame")
        sc.submit(v[2], fused=reader != "describe")      # (the pointers have left the library: the two passes from now on)
        cap, r = timed(sc.ctx, lambda: capture(sc.rt, sc.hdr))
        assert PLAIN not in r, f"{reader}: the frame after a materialisation did not keep its G-buffer: {sorted(r)}"
        out["third frame"] = cap
        return out
    both(fx, w, h, script)


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("download_first", [False, True], ids=["edit-submit-download", "edit-download-submit"])
def test_an_edit_with_a_frame_pending(fx, w, h, download_first):
    """submit, edit, submit, download: the planes are the second frame's on the edited terrain; with the download between the
    edit and the second submit they are the first frame's on the terrain as it was."""
    v = views(w, h)
    hm = fx["h"]
    block = np.full((64, 64), 255, np.uint8)
    x0 = y0 = 96

    def script(sc, lazy):
        out = {}
        try:
            sc.submit(v[1])
            sc.tp.Edit("height", x0, y0, block)
            if download_first:
                out["before the edit"] = capture(sc.rt, sc.hdr)
            sc.submit(v[1])
            out["after the edit"] = capture(sc.rt, sc.hdr)
        finally:
            sc.tp.Edit("height", x0, y0, hm[y0:y0 + 64, x0:x0 + 64])
        return out
    want, _ = both(fx, w, h, script)
    if download_first:
        assert not np.array_equal(want["before the edit"]["normals"], want["after the edit"]["normals"]), "the edit is not in view"


def test_undo_and_redo_with_a_frame_pending(fx):
    w, h = 96, 64
    v = views(w, h)
    block = np.full((64, 64), 255, np.uint8)

    def script(sc, lazy):
        out = {}
        sc.tp.EnableHistory(1 << 20)
        try:
            sc.tp.Edit("height", 96, 96, block)
            sc.tp.CommitHistory()
            sc.submit(v[1])
            assert sc.tp.Undo() is True
            out["edited"] = capture(sc.rt, sc.hdr)          # the frame was submitted on the edited terrain
            sc = LazyScene(fx, lazy, w, h)                        # (a fresh target: the first one has given laziness up)
            try:
                sc.submit(v[1])
                assert sc.tp.Redo() is True
                out["original"] = capture(sc.rt, sc.hdr)
            finally:
                sc.tp.Undo()
                for o in (sc.hdr, sc.hdr2, sc.rt):
                    o.close()
        finally:
            sc.tp.EnableHistory(0)
        return out
    want, _ = both(fx, w, h, script)
    assert not np.array_equal(want["edited"]["normals"], want["original"]["normals"])


def test_resize_and_clear_with_a_frame_pending(fx):
    w, h = 96, 64
    v = views(w, h)

    def script(sc, lazy):
        out = {}
        sc.submit(v[0])
        sc.rt.Init(68, 50)                                    # the pending frame goes with the old target
        sc.hdr.upload(np.zeros(w * h * 4, np.uint16))
        sc.fr = vr.Frame(sc.tp, sc.rt, sc.rp, sc.lights, AMBIENT_TOP, AMBIENT_BOTTOM)
        sc.submit(vr.make_view(*scaled_camera(flythrough_camera(0), 256), 68, 50))
        out["resized"] = {p: sc.rt.download(p).copy() for p in PLANES}
        out["resized census"] = sc.rt.region_census()
        sc.rt.Init(w, h)
        sc.fr = vr.Frame(sc.tp, sc.rt, sc.rp, sc.lights, AMBIENT_TOP, AMBIENT_BOTTOM)
        sc.submit(v[0])
        sc.rt.Clear()                                         # the clear replaces the frame nobody looked at
        _, r = timed(sc.ctx, lambda: out.update(cleared=capture(sc.rt, sc.hdr)))
        assert PLAIN not in r, sorted(r)
        assert (out["cleared"]["depth"] == 1.0).all() and not out["cleared"]["diffuse"].any()
        sc.submit(v[1])
        sc.rp.assume_cleared = 0                              # keep-what-is-there over a pending frame: a partial writer
        sc.tp.Render(v[0], v[0], sc.rt, sc.rp)
        out["kept"] = capture(sc.rt, sc.hdr)
        return out
    both(fx, w, h, script)


def test_a_second_target_on_the_same_terrain(fx):
    """The terrain holds at most one pending target: a lazy frame into a second one produces the first one's planes."""
    w, h = 96, 64
    v = views(w, h)

    def script(sc, lazy):
        other = LazyScene(fx, lazy, w, h)
        try:
            sc.submit(v[0])
            other.submit(v[1])
            return {"first": capture(sc.rt, sc.hdr), "second": capture(other.rt, other.hdr)}
        finally:
            for o in (other.hdr, other.hdr2, other.rt):
                o.close()
    both(fx, w, h, script)


def test_a_pending_clear_belongs_to_the_frame_that_consumed_it(fx):
    """Clear, a frame without assume_cleared (the frame is that clear), then a keep-what-is-there pass: it keeps the FRAME's
    pixels where it draws nothing, not the clear's - the clear is not pending a second time behind a lazy frame."""
    w, h = 96, 64
    v = views(w, h)

    def script(sc, lazy):
        sc.rp.assume_cleared = 0
        sc.rt.Clear()
        sc.submit(v[1])
        sc.tp.Render(v[0], v[0], sc.rt, sc.rp)
        out = {"kept": capture(sc.rt, sc.hdr)}
        sc.rt.Clear()
        sc.submit(v[0])
        sc.rt.Clear()
        sc.submit(v[1])
        out["second clear"] = capture(sc.rt, sc.hdr)
        return out
    want, _ = both(fx, w, h, script)
    assert (want["kept"]["depth"] < 1.0).all(), "the top-down frame's pixels were not kept under the sky of the second view"


def test_a_second_terrain_takes_over_the_target(fx):
    """A change of level, then a resize: terrain A's frame is pending on the target, terrain B's frame replaces it - A lets go
    of the target - the target is destroyed and made again at another size, and A is edited.  The edit queues no tile pass (A
    holds nothing), and what B and A then draw is the eager world's.  Without the resize, an edit of A leaves B's frame pending:
    the target stays lazy until somebody looks."""
    from tests.common import params
    w, h = 96, 64
    v = views(w, h)
    ctx, hm = fx["ctx"], fx["h"]
    other = vr.TerrainPass(ctx, params(256)).Init(np.ascontiguousarray(hm[::-1]), vr.synth_albedo(ctx, 256, hm))
    block = np.full((64, 64), 255, np.uint8)

    def edit_a(sc):
        _, r = timed(sc.ctx, lambda: sc.tp.Edit("height", 96, 96, block))
        sc.tp.Edit("height", 96, 96, hm[96:160, 96:160])
        return r

    def script(sc, lazy):
        out = {}
        fr_b = vr.Frame(other, sc.rt, sc.rp, sc.lights, AMBIENT_TOP, AMBIENT_BOTTOM)
        sc.submit(v[0])                                       # terrain A
        timed(sc.ctx, lambda: fr_b.submit(v[1], sc.hdr))     # terrain B into the same target
        assert PLAIN not in edit_a(sc), "an edit of the first terrain drew the second terrain's frame"
        _, r = timed(sc.ctx, lambda: out.update(b=capture(sc.rt, sc.hdr)))
        assert (PLAIN in r) == bool(lazy), sorted(r)          # B's frame was still pending
        # again on a fresh target, with the resize in between
        sc.rt.Init(w, h)
        sc.fr = vr.Frame(sc.tp, sc.rt, sc.rp, sc.lights, AMBIENT_TOP, AMBIENT_BOTTOM)
        fr_b = vr.Frame(other, sc.rt, sc.rp, sc.lights, AMBIENT_TOP, AMBIENT_BOTTOM)
        sc.submit(v[0])
        timed(sc.ctx, lambda: fr_b.submit(v[1], sc.hdr))
        sc.rt.Init(68, 50)                                    # the target goes; neither terrain may still hold it
        assert PLAIN not in edit_a(sc)
        _, r = timed(sc.ctx, lambda: other.Edit("height", 96, 96, np.ascontiguousarray(hm[::-1])[96:160, 96:160]))
        assert PLAIN not in r
        sc.fr = vr.Frame(sc.tp, sc.rt, sc.rp, sc.lights, AMBIENT_TOP, AMBIENT_BOTTOM)
        sc.submit(vr.make_view(*scaled_camera(flythrough_camera(0), 256), 68, 50))
        out["a resized"] = {p: sc.rt.download(p).copy() for p in PLANES}
        return out
    try:
        both(fx, w, h, script)
    finally:
        other.close()


def test_a_materialising_pass_borrows_a_set_while_two_frames_are_prepared(fx):
    """A fused frame nobody has looked at, two frames prepared ahead for two other views, then the first reader: the materialising
    pass needs a geometry set while both sets other than the current one hold a prepared frame, so it takes the older one's
    (vr_geosets.h: the borrowed pass) and must leave the current set and the younger frame alone.  The two prepared views are then
    rendered - one from its prepared set, one built again - and a lock_view render reuses the last selection; every plane behind
    every step is the eager world's."""
    w, h = 320, 180
    v = views(w, h)

    def script(sc, lazy):
        out = {}
        assert PLAIN not in sc.submit(v[0])
        sc.tp.Prepare(v[1], sc.rt, sc.rp)
        sc.tp.Prepare(v[2], sc.rt, sc.rp)
        out["first"], r = timed(sc.ctx, lambda: sc.rt.download("diffuse").copy())
        assert (PLAIN in r) == bool(lazy), sorted(r)                             # the materialising pass, with two sets prepared
        out["the frame"] = capture(sc.rt, sc.hdr)
        for i in (1, 2):
            sc.tp.Render(v[i], v[i], sc.rt, sc.rp)
            out[f"prepared view {i}"] = capture(sc.rt, sc.hdr)
        sc.rp.lock_view = 1
        sc.tp.Render(v[0], v[0], sc.rt, sc.rp)
        out["lock_view"] = capture(sc.rt, sc.hdr)
        return out
    want, _ = both(fx, w, h, script)
    assert not np.array_equal(want["prepared view 1"]["depth"], want["prepared view 2"]["depth"])
