"""GPU tests of the terrain history (vr_terrain_history_enable / commit / undo / redo / status).  After an undo or a redo the
terrain must be the one vr_terrain_create builds from the maps of that point in history; everything is compared bit for bit, with
no tolerance and no exclusions - the journal moves bytes, and the refresh is the one vr_terrain_edit runs.  Scenes and the state
under test are those of tests/level0_common.py (64^2 + 64^2; 67x45 height + 33x50 albedo, whose row pitches are no
multiples of 16, so that most rows take the kernels' texel-by-texel path and a few the vector path; 2x2 surfaces on 128^2), the
strokes tests/level0_common.py's five_dabs; frames are 256x144."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import vrenderer_amd as vr
from vrenderer_amd import capi
from tests import brush_model as bm
from tests import queries_common as qc
from tests.f64_queries import Surface64
from tests.fusion_common import PLANES
from tests.host_check import build_host_check
from tests.level0_common import (BRUSH_OPS, SCENES, STROKE_KW, assert_bytes, assert_chains_equal, assert_frames_equal, assert_pyramids_equal, assert_tables_equal, bits,
                                 check_stroke_preconditions, dab, five_dabs, level0, make_scenes, render, submit_frames, world_of)

pytestmark = pytest.mark.gpu

NODE_HEIGHTS = "k_node_heights (all levels)"


@pytest.fixture(scope="module")
def scenes(gpu_ctx):
    return make_scenes(gpu_ctx, SCENES)


@pytest.fixture(scope="module")
def record_bytes(tmp_path_factory):
    """history_record_bytes of vr_history.h, through the host check's `size` mode."""
    exe = build_host_check(tmp_path_factory.mktemp("history"), "history_check")

    def size(x0, w, h, texel_bytes):
        return int(subprocess.run([exe, "size", str(x0), str(w), str(h), str(texel_bytes)], capture_output=True, text=True, check=True).stdout)
    return size


def _assert_maps(tp, hm, al, what):
    assert_bytes(level0(tp, "height"), hm, f"{what}: height")
    assert_bytes(level0(tp, "albedo"), al, f"{what}: albedo")


def _assert_terrains_equal(sc, a, b, what):
    """Every mip level of both maps, the node heights, sampled heights with normals, ray hits, every G-buffer plane of a frame, the
    query pyramid and the hits under a negative max_height, the decoded tables of both maps."""
    assert_chains_equal(a, b, what)
    assert_tables_equal(a, b, what)
    surfaces = int(sc.p.world_size / sc.p.surface_size) ** 2
    nodes = (4 ** (a.GetNumLods() + 1) - 1) // 3 * surfaces
    ha, hb = a.node_heights(0, nodes).view(np.uint32), b.node_heights(0, nodes).view(np.uint32)
    assert np.array_equal(ha, hb), f"{what}: {(ha != hb).any(1).sum()} of {nodes} nodes differ"
    pts = qc.uniform_points(sc.world, 1024)
    (h1, n1), (h2, n2) = a.SampleHeights(pts, sc.mh, normals=True), b.SampleHeights(pts, sc.mh, normals=True)
    assert np.array_equal(h1.view(np.uint32), h2.view(np.uint32)) and np.array_equal(n1.view(np.uint32), n2.view(np.uint32)), f"{what}: sampled heights"
    surf = Surface64(b.download_mip("height", 0), b.download_mip("height", 1), sc.world, sc.mh)
    o, d, tm = qc.make_rays(surf, sc.world, n=64)
    ra, rb = a.CastRays(o, d, tm, sc.mh), b.CastRays(o, d, tm, sc.mh)
    assert ra.tobytes() == rb.tobytes(), f"{what}: {(ra != rb).sum()} of {len(ra)} hits differ"
    assert_frames_equal(render(sc, a, 0), render(sc, b, 0), what)
    assert_pyramids_equal(sc, a, b, what)


@pytest.mark.parametrize("name", SCENES)
def test_undo_restores_the_whole_terrain(scenes, name):
    """1. SetHeight on, one ray cast and one frame done first.  Each brush op (five_dabs), commit, undo: the terrain is the one
    created from the original maps - chains, node heights, queries, a frame.  Redo: the one created from the model's stroked maps."""
    sc = scenes[name]
    S = world_of(sc)
    a, orig = sc.terrain(sc.hm, sc.al), sc.terrain(sc.hm, sc.al)
    a.EnableHistory(1 << 20)
    for op in sorted(BRUSH_OPS):
        before = sc.al if op == bm.PAINT else sc.hm
        dabs = five_dabs(before.shape, S, op)
        want, _ = bm.stroke(before, op, dabs, S, **STROKE_KW[op])
        check_stroke_preconditions(before, want, op)
        a.Brush(BRUSH_OPS[op], dabs, **STROKE_KW[op])
        assert a.HistoryStatus()["open_records"] == 1
        a.CommitHistory()
        assert a.Undo() is True
        _assert_terrains_equal(sc, a, orig, f"{name}, {BRUSH_OPS[op]}, undo")
        assert a.Redo() is True
        b = sc.terrain(want if op != bm.PAINT else sc.hm, want if op == bm.PAINT else sc.al)
        _assert_terrains_equal(sc, a, b, f"{name}, {BRUSH_OPS[op]}, redo")
        b.close()
        assert a.Undo() is True                              # back to the original maps for the next op
    _assert_maps(a, sc.hm, sc.al, f"{name}: after the last undo")
    a.close(); orig.close()


def _stress_rects(fw, fh):
    return [("1 x 1", 11, 7, 1, 1), ("x = 3, w = 37 (clipped to the map)", 3, 2, min(37, fw - 3), 5), ("w = 16 at x = 0", 0, 9, 16, 3),
            ("w = 16 at x = 1", 1, 9, 16, 3), ("a full row", 0, 13, fw, 1), ("a full column", 9, 0, 1, fh), ("the whole map", 0, 0, fw, fh),
            ("left edge", 0, 5, 5, 7), ("right edge", fw - 5, 5, 5, 7), ("top edge", 7, 0, 9, 3), ("bottom edge", 7, fh - 3, 9, 3),
            ("the last texel", fw - 1, fh - 1, 1, 1), ("x = 15, w = 2", 15, 20, 2, 2), ("x = 17, w = 31", 17, 1, min(31, fw - 17), 4)]


@pytest.mark.parametrize("name", ("odd", "fast64"))
def test_rectangles_that_stress_the_vector_path(scenes, name):
    """2. Through vr_terrain_edit, both maps: ragged heads and tails, rows of exactly one vector, rectangles on every map edge.
    Edit with random bytes, undo: level 0 is the original in every byte; redo: the edited map.  Every edit changes at least one byte
    in the first and in the last column of its rectangle (asserted on the inputs).  `odd` is the issue's scene; the 64^2 scene runs
    the same rectangles with every row on the vector path (its row pitches are multiples of 16)."""
    sc = scenes[name]
    rng = np.random.default_rng(41)
    a = sc.terrain(sc.hm, sc.al, cast=False, render=False)
    a.EnableHistory(1 << 20)
    cur = {"height": sc.hm.copy(), "albedo": sc.al.copy()}
    for which in ("height", "albedo"):
        fh, fw = cur[which].shape[:2]
        for what, x, y, w, h in _stress_rects(fw, fh):
            old = cur[which][y:y + h, x:x + w].copy()
            new = rng.integers(0, 256, old.shape, dtype=np.uint8)
            for col in (0, w - 1):                           # a head or tail bug cannot hide behind an unchanged byte
                new[:, col] = old[:, col] + rng.integers(1, 256, old[:, col].shape, dtype=np.uint8)
            diff = (new != old) if which == "height" else (new != old).any(-1)
            assert diff[:, 0].any() and diff[:, -1].any()
            edited = {k: v.copy() for k, v in cur.items()}
            edited[which][y:y + h, x:x + w] = new
            a.Edit(which, x, y, new)
            a.CommitHistory()
            _assert_maps(a, edited["height"], edited["albedo"], f"{name}, {which}, {what}: edit")
            assert a.Undo() is True
            _assert_maps(a, cur["height"], cur["albedo"], f"{name}, {which}, {what}: undo")
            assert a.Redo() is True
            _assert_maps(a, edited["height"], edited["albedo"], f"{name}, {which}, {what}: redo")
            cur = edited
    b = sc.terrain(cur["height"], cur["albedo"], cast=False, render=False)
    assert_chains_equal(a, b, f"{name}: after all rectangles")
    a.close(); b.close()


def _timed(ctx, fn):
    ctx.timing_enable(1)
    out = fn()
    ctx.synchronize()
    ran = ctx.timing_collect()
    ctx.timing_enable(0)
    return out, ran


def test_a_step_of_overlapping_records(scenes):
    """3. Three overlapping RAISE strokes, one PAINT and one vr_terrain_edit inside the strokes form one step: one undo gives the
    original maps, one redo the final maps, applied == 1 both times.  A further call returns applied == 0 and queues nothing: the
    timing records are empty, where those of the undo that applied hold the refresh's node-height kernel."""
    sc = scenes["fast64"]
    S = world_of(sc)
    a = sc.terrain(sc.hm, sc.al)
    a.EnableHistory(1 << 20)
    hm, al = sc.hm, sc.al
    for k, (tx, ty) in enumerate(((20.0, 22.0), (26.5, 25.0), (23.0, 30.0))):
        dabs = np.float32([dab(hm.shape, S, tx, ty, 9.0, 0.3, 40.0 - 55.0 * (k == 1))])
        hm, _ = bm.stroke(hm, bm.RAISE, dabs, S)
        a.Brush("raise", dabs)
    pd = np.float32([dab(al.shape, S, 24.0, 24.0, 10.0, 0.5, 0.8)])
    al, _ = bm.stroke(al, bm.PAINT, pd, S, **STROKE_KW[bm.PAINT])
    a.Brush("paint", pd, **STROKE_KW[bm.PAINT])
    patch = np.random.default_rng(3).integers(0, 256, (11, 19), dtype=np.uint8)
    hm = hm.copy(); hm[18:29, 15:34] = patch
    a.Edit("height", 15, 18, patch)
    assert (hm != sc.hm).sum() >= 100 and (al != sc.al).any(-1).sum() >= 30
    st = a.HistoryStatus()
    assert (st["open_records"], st["undo_steps"], st["redo_steps"]) == (5, 0, 0)
    _assert_maps(a, hm, al, "the step")
    applied, ran = _timed(sc.ctx, a.Undo)                          # (undo closes the open step first)
    assert applied is True and NODE_HEIGHTS in ran, ran
    _assert_maps(a, sc.hm, sc.al, "one undo")
    orig = sc.terrain(sc.hm, sc.al)
    _assert_terrains_equal(sc, a, orig, "one undo of five overlapping records")
    orig.close()
    applied, ran = _timed(sc.ctx, a.Undo)
    assert applied is False and ran == {}, ran
    assert a.Redo() is True
    _assert_maps(a, hm, al, "one redo")
    b = sc.terrain(hm, al)
    _assert_terrains_equal(sc, a, b, "one redo of five overlapping records")
    b.close()
    applied, ran = _timed(sc.ctx, a.Redo)
    assert applied is False and ran == {}, ran
    st = a.HistoryStatus()
    assert (st["open_records"], st["undo_steps"], st["redo_steps"], st["dropped_steps"]) == (0, 1, 0, 0)
    a.close()


def test_redo_is_discarded_by_a_new_stroke(scenes):
    """4. Step 1 (RAISE), step 2 (PAINT), undo, a new RAISE stroke: redo_steps == 0 and redo applies nothing.  The two steps that
    remain undo and redo in order."""
    sc = scenes["fast64"]
    S = world_of(sc)
    a = sc.terrain(sc.hm, sc.al, cast=False, render=False)
    a.EnableHistory(1 << 20)
    d1, d2 = five_dabs(sc.hm.shape, S, bm.RAISE), five_dabs(sc.al.shape, S, bm.PAINT)
    d3 = np.float32([dab(sc.hm.shape, S, 40.0, 12.0, 8.0, 0.2, -35.0)])
    hm1, _ = bm.stroke(sc.hm, bm.RAISE, d1, S)
    al2, _ = bm.stroke(sc.al, bm.PAINT, d2, S, **STROKE_KW[bm.PAINT])
    hm3, _ = bm.stroke(hm1, bm.RAISE, d3, S)
    assert (hm3 != hm1).sum() >= 30
    a.Brush("raise", d1); a.CommitHistory()
    a.Brush("paint", d2, **STROKE_KW[bm.PAINT]); a.CommitHistory()
    _assert_maps(a, hm1, al2, "two steps")
    assert a.Undo() is True
    st = a.HistoryStatus()
    assert (st["undo_steps"], st["redo_steps"]) == (1, 1)
    used = st["bytes_used"]
    a.Brush("raise", d3)
    st = a.HistoryStatus()
    assert (st["undo_steps"], st["redo_steps"], st["open_records"], st["dropped_steps"]) == (1, 0, 1, 0)
    assert st["bytes_used"] != used                                   # the PAINT record's room went, the new record's came
    assert a.Redo() is False                                          # (closes the open step; there is nothing to redo)
    _assert_maps(a, hm3, sc.al, "after the new stroke")
    assert a.HistoryStatus()["undo_steps"] == 2
    assert a.Undo() is True; _assert_maps(a, hm1, sc.al, "first undo")
    assert a.Undo() is True; _assert_maps(a, sc.hm, sc.al, "second undo")
    assert a.Undo() is False
    assert a.Redo() is True; _assert_maps(a, hm1, sc.al, "first redo")
    assert a.Redo() is True; _assert_maps(a, hm3, sc.al, "second redo")
    assert a.Redo() is False
    a.close()


def test_budget(scenes, record_bytes):
    """5. An arena in which two records of a 37 x 9 rectangle at x = 3 fit and three do not (sized by vr_history.h's own function):
    after three steps dropped_steps == 1, two undos succeed, the third applies nothing and the maps are those after step 1.  An
    edit larger than the arena lands, leaves no undo step and raises dropped_steps by the steps lost (the two there were and the
    open one); the lost step records nothing until commit; later small steps record and undo normally."""
    sc = scenes["fast64"]
    rng = np.random.default_rng(12)
    one = record_bytes(3, 37, 9, 1)
    assert one == 48 * 9
    a = sc.terrain(sc.hm, sc.al, cast=False, render=False)
    a.EnableHistory(3 * one - 16)
    states = [sc.hm.copy()]
    for k in range(3):
        hm = states[-1].copy()
        hm[10 + 4 * k:19 + 4 * k, 3:40] = rng.integers(0, 256, (9, 37), dtype=np.uint8)
        a.Edit("height", 3, 10 + 4 * k, hm[10 + 4 * k:19 + 4 * k, 3:40])
        a.CommitHistory()
        states.append(hm)
        st = a.HistoryStatus()
        assert (st["undo_steps"], st["dropped_steps"], st["bytes_used"]) == (min(k + 1, 2), max(k - 1, 0), min(k + 1, 2) * one), st
    assert a.HistoryStatus()["bytes_budget"] == 3 * one - 16
    _assert_maps(a, states[3], sc.al, "three steps")
    assert a.Undo() is True and a.Undo() is True
    assert a.Undo() is False
    _assert_maps(a, states[1], sc.al, "two undos of three steps")
    assert a.Redo() is True and a.Redo() is True
    _assert_maps(a, states[3], sc.al, "two redos")
    # larger than the arena: 64 x 64 bytes
    assert record_bytes(0, 64, 64, 1) > 3 * one - 16
    big = rng.integers(0, 256, (64, 64), dtype=np.uint8)
    assert (big != states[3]).mean() > 0.9
    before = a.HistoryStatus()
    assert before["undo_steps"] == 2
    a.Edit("height", 0, 0, big)
    assert_bytes(level0(a, "height"), big, "the edit larger than the arena")
    st = a.HistoryStatus()
    assert (st["undo_steps"], st["redo_steps"], st["open_records"], st["bytes_used"]) == (0, 0, 0, 0), st
    assert st["dropped_steps"] == before["dropped_steps"] + 2 + 1
    small = rng.integers(0, 256, (3, 5), dtype=np.uint8)
    a.Edit("height", 30, 30, small)                                   # still inside the lost step: not recorded
    assert a.HistoryStatus()["open_records"] == 0
    assert a.Undo() is False                                          # (closes the lost step)
    cur = big.copy(); cur[30:33, 30:35] = small
    _assert_maps(a, cur, sc.al, "after the lost step")
    nxt = cur.copy(); nxt[5:8, 50:55] = cur[5:8, 50:55] ^ 0x5A
    a.Edit("height", 50, 5, nxt[5:8, 50:55])
    assert a.HistoryStatus()["open_records"] == 1
    a.CommitHistory()
    _assert_maps(a, nxt, sc.al, "a small step after the lost one")
    assert a.Undo() is True; _assert_maps(a, cur, sc.al, "its undo")
    assert a.Redo() is True; _assert_maps(a, nxt, sc.al, "its redo")
    assert a.HistoryStatus()["dropped_steps"] == before["dropped_steps"] + 3
    a.close()


def test_off_means_off(scenes):
    """6. With history never enabled, and again after enable(0), a stroke runs the timed kernels it runs with history on (the
    journal's kernels are untimed, the refresh is the same), undo applies nothing, the status is all zero, and
    vr_terrain_memory_bytes is what it was before enable-then-disable (and larger by the budget in between).  Argument refusals
    and a refused allocation leave maps, steps and status as they were."""
    sc = scenes["odd"]
    S = world_of(sc)
    lib = sc.ctx.lib
    dabs = five_dabs(sc.hm.shape, S, bm.RAISE)
    zero = dict(undo_steps=0, redo_steps=0, open_records=0, dropped_steps=0, bytes_used=0, bytes_budget=0)
    a = sc.terrain(sc.hm, sc.al)
    a.Brush("raise", dabs); a.Edit("height", 0, 0, sc.hm)              # the brush's own memory exists from here on
    sc.ctx.synchronize()
    mem = a.memory_bytes()
    _, never = _timed(sc.ctx, lambda: a.Brush("raise", dabs))
    assert never and a.HistoryStatus() == zero
    assert a.Undo() is False and a.Redo() is False
    a.CommitHistory()
    hm1 = level0(a, "height")
    a.EnableHistory(1 << 16)
    assert a.memory_bytes()["total"] == mem["total"] + (1 << 16)
    a.Edit("height", 0, 0, sc.hm)
    _, on = _timed(sc.ctx, lambda: a.Brush("raise", dabs))
    a.CommitHistory()
    st = a.HistoryStatus()
    assert (st["undo_steps"], st["bytes_budget"]) == (1, 1 << 16)
    # refusals: NULL arguments, and an arena the allocator refuses
    assert lib.vr_terrain_history_status(a.handle, None) == capi.VR_ERR_INVALID_ARGUMENT
    assert lib.vr_terrain_history_status(None, C.byref(capi.HistoryStatus())) == capi.VR_ERR_INVALID_ARGUMENT
    assert lib.vr_terrain_undo(None, None) == capi.VR_ERR_INVALID_ARGUMENT and lib.vr_terrain_history_enable(None, 64) == capi.VR_ERR_INVALID_ARGUMENT
    os.environ["VR_ALLOC_FAIL_ABOVE"] = "4096"
    try:
        assert lib.vr_terrain_history_enable(a.handle, 1 << 17) == capi.VR_ERR_OUT_OF_MEMORY
    finally:
        del os.environ["VR_ALLOC_FAIL_ABOVE"]
    assert a.HistoryStatus() == st
    assert_bytes(level0(a, "height"), hm1, "after the refusals")
    a.EnableHistory(1 << 16)                                          # the budget it has: the steps stay
    assert a.HistoryStatus() == st
    a.EnableHistory(0)
    assert a.HistoryStatus() == zero and a.memory_bytes() == mem
    assert a.Undo() is False
    assert_bytes(level0(a, "height"), hm1, "undo with history off")
    a.Edit("height", 0, 0, sc.hm)
    _, after = _timed(sc.ctx, lambda: a.Brush("raise", dabs))
    names = lambda ran: {k: n for k, (ms, n) in ran.items()}
    assert names(never) == names(after) == names(on), (never, on, after)
    assert_bytes(level0(a, "height"), hm1, "the stroke with history off again")
    a.close()


def test_frames_in_flight(scenes):
    """7. vr_frame_submit with the next view prepared ahead (the pattern of test_prepared_geometry_is_stale_after_an_edit): an undo
    between two submits gives the second frame of the restored terrain, with and without VR_OPT_FRAME_FUSION, and a redo the frame
    of the edited one."""
    sc = scenes["fast64"]
    views = [sc.view(5), sc.view(0), sc.view(0)]
    rng = np.random.default_rng(5)
    hm, al = sc.hm.copy(), sc.al.copy()
    hm[8:41, 8:48] = rng.integers(0, 256, (33, 40), dtype=np.uint8)
    al[30:39, 0:64] = rng.integers(0, 256, (9, 64, 4), dtype=np.uint8)
    results = {}
    for fusion in (1, 0):
        a = sc.terrain(sc.hm, sc.al)
        a.EnableHistory(1 << 20)
        a.Edit("height", 8, 8, hm[8:41, 8:48]); a.Edit("albedo", 0, 30, al[30:39, 0:64])
        a.CommitHistory()
        fa = submit_frames(sc, a, views, fusion, edit=lambda: a.Undo())
        b, e = sc.terrain(sc.hm, sc.al), sc.terrain(hm, al)
        fb = submit_frames(sc, b, views, fusion)
        fr = submit_frames(sc, a, views, fusion, edit=lambda: a.Redo())     # a is restored here: frame 0 of b, then frame 1 of e
        fe = submit_frames(sc, e, views, fusion)
        for p in PLANES + ("hdr",):
            assert np.array_equal(bits(fa[0][p]), bits(fe[0][p])), f"fusion {fusion}: {p} of the frame before the undo differs"
            assert np.array_equal(bits(fa[1][p]), bits(fb[1][p])), f"fusion {fusion}: {p} of the frame after the undo differs"
            assert np.array_equal(bits(fr[0][p]), bits(fb[0][p])), f"fusion {fusion}: {p} of the frame before the redo differs"
            assert np.array_equal(bits(fr[1][p]), bits(fe[1][p])), f"fusion {fusion}: {p} of the frame after the redo differs"
        assert (fa[1]["depth"] < 1.0).any() and any(not np.array_equal(bits(fb[1][p]), bits(fe[1][p])) for p in PLANES)
        results[fusion] = fa
        a.close(); b.close(); e.close()
    for p in PLANES + ("hdr",):
        assert np.array_equal(bits(results[1][1][p]), bits(results[0][1][p])), f"fused and two-pass frames after the undo differ in {p}"
