"""GPU tests of vr_terrain_edit: after an edit a terrain is indistinguishable from one freshly created from the edited
arrays.  Terrain A is created from the original maps, put into the state under test (SetHeight(True), one ray cast so the query
pyramid exists, one frame rendered) and edited; terrain B is created afresh from the edited arrays.  Everything the library
exposes is compared bit for bit - no tolerance anywhere: both sides run the same kernels' arithmetic.

The scenes, the state under test and the comparisons are tests/level0_common.py's."""
import ctypes as C

import numpy as np
import pytest

import vrenderer_amd as vr
from vrenderer_amd import capi
from tests.fusion_common import PLANES
from tests import queries_common as qc
from tests.f64_queries import Surface64
from tests.level0_common import (H, SCENES, W, Maps, assert_bytes, assert_chains_equal, assert_frames_equal, assert_pyramids_equal, assert_tables_equal, bits,
                                 five_dabs, level0, make_scenes, render, submit_frames, world_of)

pytestmark = pytest.mark.gpu

RENDER_CAMERAS = (0, 5, 7)


@pytest.fixture(scope="module")
def scenes(gpu_ctx):
    return make_scenes(gpu_ctx, SCENES)


def _edit_some(sc, tp, maps, seed=7):
    """A handful of edits of both maps that touch a corner, the interior and the right / bottom edges."""
    rng = np.random.default_rng(seed)
    for which, full in (("height", maps.hm), ("albedo", maps.al)):
        fh, fw = full.shape[:2]
        maps.random(tp, rng, which, 0, 0, 1, 1)
        maps.random(tp, rng, which, 3, 5, 7, 9)
        maps.random(tp, rng, which, fw - 6, fh - 4, 6, 4)
        maps.random(tp, rng, which, fw // 2 - 1, 0, 1, fh)


@pytest.mark.parametrize("name", SCENES)
def test_every_mip_level_after_every_kind_of_rectangle(scenes, name):
    """1x1 at the four corners and at an odd interior coordinate, (3, 5) 7x9, a full-width row, a full-height column, the
    rectangle that touches the right and bottom edges, the whole map, then 20 seeded random rectangles on height and albedo
    alternately: after each sequence every level of both chains of A is B's, byte for byte."""
    sc = scenes[name]
    a, maps, rng = sc.terrain(sc.hm, sc.al), Maps(sc), np.random.default_rng(2024)

    def both(fn):
        for which, full in (("height", maps.hm), ("albedo", maps.al)):
            fn(which, full.shape[1], full.shape[0])

    sequences = [
        ("corners", lambda wh, fw, fh: [maps.random(a, rng, wh, x, y, 1, 1) for x, y in ((0, 0), (fw - 1, 0), (0, fh - 1), (fw - 1, fh - 1))]),
        ("odd interior texel", lambda wh, fw, fh: maps.random(a, rng, wh, 11, 7, 1, 1)),
        ("(3, 5) 7x9", lambda wh, fw, fh: maps.random(a, rng, wh, 3, 5, 7, 9)),
        ("full-width row", lambda wh, fw, fh: maps.random(a, rng, wh, 0, 13, fw, 1)),
        ("full-height column", lambda wh, fw, fh: maps.random(a, rng, wh, 9, 0, 1, fh)),
        ("right and bottom edges", lambda wh, fw, fh: maps.random(a, rng, wh, fw - 5, fh - 3, 5, 3)),
        ("whole map", lambda wh, fw, fh: maps.random(a, rng, wh, 0, 0, fw, fh)),
    ]
    for what, fn in sequences:
        both(fn)
        b = sc.terrain(maps.hm, maps.al, cast=False, render=False)
        assert_chains_equal(a, b, f"{name}, {what}")
        b.close()
    for k in range(20):
        which = "height" if k % 2 == 0 else "albedo"
        fh, fw = (maps.hm if which == "height" else maps.al).shape[:2]
        x, y = int(rng.integers(0, fw)), int(rng.integers(0, fh))
        maps.random(a, rng, which, x, y, int(rng.integers(1, fw - x + 1)), int(rng.integers(1, fh - y + 1)))
    b = sc.terrain(maps.hm, maps.al, cast=False, render=False)
    assert_chains_equal(a, b, f"{name}, 20 random rectangles")
    a.close(); b.close()


@pytest.mark.parametrize("name", SCENES)
def test_every_gbuffer_plane(scenes, oracle, name):
    """All five planes of A and B at 256x144, depth as bits: three cameras x fill over a cleared target (the fast variant on
    the 64^2 scene), wireframe, depth_only and rank 1 of 3.  On the 64^2 scene A also equals the oracle on the edited arrays."""
    sc = scenes[name]
    a, maps = sc.terrain(sc.hm, sc.al), Maps(sc)
    _edit_some(sc, a, maps)
    b = sc.terrain(maps.hm, maps.al)
    assert_tables_equal(a, b, name)
    covered = 0
    for cam in RENDER_CAMERAS:
        for what, kw, part in (("fill", dict(assume_cleared=1), None), ("wireframe", dict(wireframe=1), None),
                               ("depth_only", dict(depth_only=1), None), ("rank 1 of 3", {}, vr.Partition(1, 3))):
            fa, fb = render(sc, a, cam, part, **kw), render(sc, b, cam, part, **kw)
            assert_frames_equal(fa, fb, f"{name}, camera {cam}, {what}")
            covered += int((fa["depth"] < 1.0).sum())
    assert covered > 0
    if name == "fast64":
        ot = oracle.OracleTerrain(sc.p, maps.hm, maps.al)
        ot.set_height(True)
        gb = oracle.GBufferHost(W, H)
        ot.render(sc.view(0), gb, vr.default_render_params(sc.mh, assume_cleared=1))
        fa = render(sc, a, 0, None, assume_cleared=1)
        assert_frames_equal(fa, {p: getattr(gb, p) for p in PLANES}, "64^2 against the oracle on the edited arrays")
        assert (fa["depth"] < 1.0).mean() > 0.05
        ot.close()
    a.close(); b.close()


@pytest.mark.parametrize("name", SCENES)
def test_node_heights_and_selection(scenes, name):
    """node_heights(0, all) as uint32 and NodeSelect's ids and instances for two cameras: the dyadic path (64^2), the full
    re-run (67x45) and the per-surface bases (2x2 surfaces)."""
    sc = scenes[name]
    a, maps = sc.terrain(sc.hm, sc.al), Maps(sc)
    _edit_some(sc, a, maps)
    # a tall spike and a pit, so that min and max of their nodes' ancestors move
    spike = np.full((2, 2), 255, np.uint8)
    maps.edit(a, "height", maps.hm.shape[1] // 2 + 1, maps.hm.shape[0] // 2 - 3, spike)
    maps.edit(a, "height", 5, maps.hm.shape[0] - 7, np.zeros((3, 3), np.uint8))
    b = sc.terrain(maps.hm, maps.al)
    surfaces = int(sc.p.world_size / sc.p.surface_size) ** 2
    nodes = (4 ** (a.GetNumLods() + 1) - 1) // 3 * surfaces
    ha, hb = a.node_heights(0, nodes), b.node_heights(0, nodes)
    assert np.array_equal(ha.view(np.uint32), hb.view(np.uint32)), f"{name}: {(ha.view(np.uint32) != hb.view(np.uint32)).any(1).sum()} of {nodes} nodes differ"
    for cam in (0, 5):
        v = sc.view(cam)
        na, ia, insta = a.NodeSelect(v, sc.mh)
        nb, ib, instb = b.NodeSelect(v, sc.mh)
        assert na == nb and na > 0 and np.array_equal(ia, ib) and np.array_equal(insta, instb), (name, cam, na, nb)
    a.close(); b.close()


@pytest.mark.parametrize("cast_first", (True, False))
@pytest.mark.parametrize("name", SCENES)
def test_queries(scenes, name, cast_first):
    """SampleHeights with normals at 4,096 seeded points and CastRays over queries_common.make_rays: the same bits, with the
    pyramid built before the edit and with no cast before the edit."""
    sc = scenes[name]
    a, maps = sc.terrain(sc.hm, sc.al, cast=cast_first), Maps(sc)
    _edit_some(sc, a, maps)
    maps.edit(a, "height", 20, 20, np.full((5, 4), 250, np.uint8))
    b = sc.terrain(maps.hm, maps.al, cast=False)
    pts = qc.uniform_points(sc.world)
    (h1, n1), (h2, n2) = a.SampleHeights(pts, sc.mh, normals=True), b.SampleHeights(pts, sc.mh, normals=True)
    assert np.array_equal(h1.view(np.uint32), h2.view(np.uint32)) and np.array_equal(n1.view(np.uint32), n2.view(np.uint32))
    surf = Surface64(b.download_mip("height", 0), b.download_mip("height", 1), sc.world, sc.mh)
    o, d, tm = qc.make_rays(surf, sc.world)
    ra, rb = a.CastRays(o, d, tm, sc.mh), b.CastRays(o, d, tm, sc.mh)
    assert ra.tobytes() == rb.tobytes(), f"{name}: {(ra != rb).sum()} of {len(ra)} hits differ"
    assert (ra["status"] == capi.VR_RAY_HIT).mean() > 0.2
    assert_pyramids_equal(sc, a, b, f"{name}, cast before the edits: {cast_first}")
    assert_tables_equal(a, b, f"{name}, cast before the edits: {cast_first}")
    a.close(); b.close()


def test_prepared_geometry_is_stale_after_an_edit(scenes):
    """Prepare(view), Edit, Render(view): A's frame is B's - for a height edit and for an albedo edit.  Under vr_frame_submit
    with prepare_views set, an edit between two submits gives B's second frame, fused and two-pass alike.  With lock_view the
    frame after the edit draws the nodes of the frame before it."""
    sc = scenes["fast64"]
    rng = np.random.default_rng(99)
    for which in ("height", "albedo"):
        a, maps = sc.terrain(sc.hm, sc.al), Maps(sc)
        rt = vr.RenderTargets(sc.ctx).Init(W, H)
        v, rp = sc.view(5), vr.default_render_params(sc.mh, assume_cleared=1)
        a.Prepare(v, rt, rp)
        maps.random(a, rng, which, 10, 12, 30, 25)
        rt.Clear(); a.Render(v, v, rt, rp)
        fa = {p: rt.download(p).copy() for p in PLANES}
        rt.close()
        b = sc.terrain(maps.hm, maps.al)
        assert_frames_equal(fa, render(sc, b, 5, None, assume_cleared=1), f"prepare, {which} edit, render")
        a.close(); b.close()
    views = [sc.view(5), sc.view(0), sc.view(0)]
    results = {}
    for fusion in (1, 0):
        a, maps = sc.terrain(sc.hm, sc.al), Maps(sc)
        erng = np.random.default_rng(5)
        fa = submit_frames(sc, a, views, fusion, edit=lambda: (maps.random(a, erng, "height", 8, 8, 40, 33), maps.random(a, erng, "albedo", 0, 30, 64, 9)))
        b = sc.terrain(maps.hm, maps.al)
        fb = submit_frames(sc, b, views, fusion)
        for p in PLANES + ("hdr",):
            assert np.array_equal(bits(fa[1][p]), bits(fb[1][p])), f"frame submit, fusion {fusion}: {p} of the frame after the edit differs"
        results[fusion] = fa
        a.close(); b.close()
    for p in PLANES + ("hdr",):
        assert np.array_equal(bits(results[1][1][p]), bits(results[0][1][p])), f"fused and two-pass frames after the edit differ in {p}"
    # lock_view: the frame after the edit draws the nodes of the frame before it (a node is named by two opposite corners of its
    # patch: vertices 0 and 1088, which no morph moves)
    a, maps = sc.terrain(sc.hm, sc.al), Maps(sc)
    rt = vr.RenderTargets(sc.ctx).Init(W, H)
    v0, v1 = sc.view(5), sc.view(0)

    def corners(lock, v):
        rt.Clear(); a.Render(v, v, rt, vr.default_render_params(sc.mh, lock_view=lock))
        n = a.num_chunks()
        return n, a.download_vertices(0, n)[:, [0, 1088], 4:6].copy()

    n0, c0 = corners(0, v0)
    maps.random(a, rng, "height", 0, 0, 64, 64)
    n1, c1 = corners(1, v1)
    assert n1 == n0 and np.array_equal(c0, c1)
    n2, c2 = corners(0, v1)
    assert n2 != n0 or not np.array_equal(c0, c2)                # (the unlocked frame of that view selects other nodes)
    rt.close(); a.close()


def test_device_pointer_mode_with_a_wide_pitch(scenes):
    """A rectangle out of a torch tensor on the device whose rows are wider than the rectangle == the same edit in host mode."""
    import torch
    sc = scenes["odd"]
    rng = np.random.default_rng(31)
    a, b = sc.terrain(sc.hm, sc.al), sc.terrain(sc.hm, sc.al)
    dev = f"cuda:{sc.ctx.device}"
    for which, tb, (x, y, w, h) in (("height", 1, (5, 3, 21, 17)), ("albedo", 4, (2, 29, 31, 21)), ("height", 1, (66, 44, 1, 1))):
        pitch = (w + 13) * tb
        host = rng.integers(0, 256, (h, pitch), dtype=np.uint8)
        t = torch.from_numpy(host).to(dev)
        torch.cuda.synchronize()
        a.Edit(which, x, y, device_ptr=t.data_ptr(), w=w, h=h, pitch=pitch)
        sc.ctx.synchronize()
        rect = host[:, :w * tb]
        b.Edit(which, x, y, rect.copy() if tb == 1 else rect.reshape(h, w, 4).copy())
    assert_chains_equal(a, b, "device-pointer mode")
    assert_frames_equal(render(sc, a, 0), render(sc, b, 0), "device-pointer mode")
    pts = qc.uniform_points(sc.world, 512)
    assert np.array_equal(a.SampleHeights(pts, sc.mh), b.SampleHeights(pts, sc.mh))
    a.close(); b.close()


def test_refusals_leave_the_terrain_alone(scenes):
    """Every invalid argument returns VR_ERR_INVALID_ARGUMENT, an empty rectangle VR_OK; the chains and a rendered frame of A
    are what they were."""
    import torch
    sc = scenes["odd"]
    a = sc.terrain(sc.hm, sc.al)
    lib, hnd = sc.ctx.lib, a.handle
    chains = {(wh, l): a.download_mip(wh, l) for wh in ("height", "albedo") for l in range(a.mip_levels(wh))}
    frame = render(sc, a, 0)
    buf = np.full((64, 64, 4), 77, np.uint8)
    p = buf.ctypes.data_as(C.c_void_p)
    dev = torch.full((4096,), 77, dtype=torch.uint8, device=f"cuda:{sc.ctx.device}")
    torch.cuda.synchronize()
    bad = [(0, 0, 0, 4, 4, None, 0, 0),                     # NULL with a non-empty rectangle
           (2, 0, 0, 4, 4, p, 0, 0), (-1, 0, 0, 4, 4, p, 0, 0),          # which
           (0, -1, 0, 4, 4, p, 0, 0), (0, 0, -1, 4, 4, p, 0, 0), (0, 0, 0, -4, 4, p, 0, 0), (0, 0, 0, 4, -4, p, 0, 0),
           (0, 64, 0, 4, 4, p, 0, 0), (0, 0, 42, 4, 4, p, 0, 0), (0, 0, 0, 68, 4, p, 0, 0), (0, 67, 45, 1, 1, p, 0, 0),     # outside 67 x 45
           (1, 30, 0, 4, 4, p, 0, 0), (1, 0, 0, 33, 51, p, 0, 0), (0, 2**31 - 1, 0, 2**31 - 1, 1, p, 0, 0),                 # outside 33 x 50
           (0, 0, 0, 8, 4, p, 7, 0), (1, 0, 0, 8, 4, p, 31, 0),          # pitch smaller than a row
           (1, 0, 0, 4, 4, C.c_void_p(dev.data_ptr() + 2), 0, 1)]        # device pointer not aligned to the texel
    for args in bad:
        assert lib.vr_terrain_edit(hnd, *args) == capi.VR_ERR_INVALID_ARGUMENT, args
    assert lib.vr_terrain_edit(None, 0, 0, 0, 1, 1, p, 0, 0) == capi.VR_ERR_INVALID_ARGUMENT
    for args in ((0, 3, 3, 0, 5, p, 0, 0), (1, 3, 3, 5, 0, p, 0, 0), (0, 0, 0, 0, 0, None, 0, 0), (0, 67, 45, 0, 0, None, 0, 1)):
        assert lib.vr_terrain_edit(hnd, *args) == capi.VR_OK, args
    for (wh, l), want in chains.items():
        assert np.array_equal(a.download_mip(wh, l), want), (wh, l)
    assert_frames_equal(render(sc, a, 0), frame, "after the refusals")
    a.close()


def test_side_resources_follow_the_context_across_two_streams(scenes, gpu_ctx):
    """The query pyramid, the journal and the brush buffers (vr_order.h's side resources) with the context moved between two streams
    and the host paying only what vr_context_set_stream asks of it - the new stream waits for the old one, nothing is synchronised.
    256 rays with host pointers on stream A (which builds the pyramid); on B a RAISE stroke with history on, then the rays through
    device pointers; back on A an undo, the rays again; on B a thermal erosion, and its planes read back on A.  The hits after each
    step are those of a fresh terrain created from the model's map for that step, byte for byte, level 0 is the model's, and the
    erosion's planes are the model's.  Checked first, on the references alone: the stroke changes at least 30 texels and at least 10
    rays hit another cell (or stop hitting) because of it - else a stale pyramid or map could not show."""
    import torch
    from tests import brush_model as bm
    from tests import erosion_state as es
    from tests.erosion_state import ITER, assert_state, model
    sc = scenes["fast64"]
    S, mh = world_of(sc), sc.mh
    stroke = five_dabs(sc.hm.shape, S, bm.RAISE)
    m1, _ = bm.stroke(sc.hm, bm.RAISE, stroke, S)
    mask = es.five_dabs(sc.hm.shape, S)
    eroded = model("thermal", sc.hm, mask, S, ITER, es.PARAMS["thermal"])
    assert (m1 != sc.hm).sum() >= 30

    def fresh_hits(hm, rays):
        b = sc.terrain(hm, sc.al, cast=False, render=False)
        try:
            return b.cast_ray_array(rays, mh)
        finally:
            b.close()

    b0 = sc.terrain(sc.hm, sc.al, cast=False, render=False)
    surf = Surface64(b0.download_mip("height", 0), b0.download_mip("height", 1), sc.world, mh)
    b0.close()
    o, d, tm = qc.make_rays(surf, sc.world, n=256)
    rays = np.zeros(256, vr.RAY_DTYPE)
    rays["origin"], rays["dir"], rays["t_max"] = o, d, tm
    ref0, ref1, ref2 = fresh_hits(sc.hm, rays), fresh_hits(m1, rays), fresh_hits(eroded["bytes"], rays)

    def cells(hits):
        xz = np.floor((hits["position"][:, [0, 2]].astype(np.float64) / S + 0.5) * sc.hm.shape[1]).astype(np.int64)
        return np.where((hits["status"] == capi.VR_RAY_HIT)[:, None], xz, -1)

    moved = (cells(ref0) != cells(ref1)).any(1).sum()
    print(f"stroke: {(m1 != sc.hm).sum()} texels changed, {moved} of 256 rays hit another cell")
    assert moved >= 10, moved

    dev = f"cuda:{gpu_ctx.device}"
    d_rays = torch.from_numpy(rays.view(np.uint8).reshape(-1).copy()).to(dev)
    d_hits = [torch.zeros(256 * 32, dtype=torch.uint8, device=dev) for _ in range(2)]
    a = sc.terrain(sc.hm, sc.al, cast=False, render=False)
    a.EnableHistory(1 << 20)
    gpu_ctx.synchronize()
    torch.cuda.synchronize()
    A, B = torch.cuda.Stream(), torch.cuda.Stream()

    def cast_on_device(out):
        capi.check(gpu_ctx.lib.vr_terrain_cast_rays(a.handle, C.c_void_p(d_rays.data_ptr()), 256, mh, C.c_void_p(out.data_ptr()), 1), "vr_terrain_cast_rays")

    try:
        gpu_ctx.set_stream(A.cuda_stream)
        assert a.cast_ray_array(rays, mh).tobytes() == ref0.tobytes(), "1. host pointers on A (the pyramid's build)"
        B.wait_stream(A)
        gpu_ctx.set_stream(B.cuda_stream)
        a.Brush("raise", stroke)
        a.CommitHistory()
        cast_on_device(d_hits[0])
        A.wait_stream(B)
        gpu_ctx.set_stream(A.cuda_stream)
        assert a.Undo()
        cast_on_device(d_hits[1])
        gpu_ctx.synchronize()
        assert d_hits[0].cpu().numpy().tobytes() == ref1.tobytes(), "4. device pointers on B behind the stroke"
        assert d_hits[1].cpu().numpy().tobytes() == ref0.tobytes(), "7. device pointers on A behind the undo"
        assert a.cast_ray_array(rays, mh).tobytes() == ref0.tobytes(), "7. host pointers on A behind the undo"
        assert_bytes(level0(a, "height"), sc.hm, "level 0 behind the undo")
        assert a.Redo()
        assert_bytes(level0(a, "height"), m1, "level 0 behind the redo")
        assert a.Undo()
        B.wait_stream(A)
        gpu_ctx.set_stream(B.cuda_stream)
        assert a.Erode(mask, ITER, *es.PARAMS["thermal"]) == eroded["rect"]
        A.wait_stream(B)
        gpu_ctx.set_stream(A.cuda_stream)
        assert_state(a, eroded, "8. sweep_state on A behind an erode on B")
        assert a.cast_ray_array(rays, mh).tobytes() == ref2.tobytes(), "8. host pointers on A behind the erode"
    finally:
        torch.cuda.synchronize()
        gpu_ctx.set_stream(0)
        a.close()
