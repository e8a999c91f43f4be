"""What the GPU tests of the operations that write level 0 of a terrain map share (brush, the erosions, texture, stamp, noise, path,
region, and the edit, history and read-back tests beside them): the scenes and the state under test, dabs, comparison of two
terrains byte for byte, one adapter per operation (Level0Op) and the test bodies that differ between operations only in the call
they make.  Every reference is a numpy model of tests/*_model.py; no tolerance anywhere.

Scenes, the smallest at which each mechanism can go wrong: 64^2 + 64^2 (the tile pass's fast variant, the dyadic SetHeight
path), 67x45 height + 33x50 albedo (odd chains, the clamped last column, the non-dyadic SetHeight path, the general raster
variant) and a 2x2-surface world of 128 on 128^2 maps (per-surface node bases); tests/texture_cases.py adds two."""
import numpy as np
import pytest

import vrenderer_amd as vr
from vrenderer_amd import capi
from tests.common import AMBIENT_BOTTOM, AMBIENT_TOP, CAMERAS, params, scaled_camera
from tests.fusion_common import PLANES, LazyScene, assert_same_frame, both, capture, download_frame, terrain_fixture, views
from tests import brush_model as bm
from tests import erode_model as em
from tests import noise_cases as nc
from tests import pyramid_model as pm
from tests import queries_common as qc
from tests import tables_model as tm
from tests import texture_cases as tc
from tests.f64_queries import Surface64

W, H = 256, 144
SCENES = ("fast64", "odd", "multi")


def bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


class Scene:
    """The original maps of one scene, its terrain parameters and the world size its cameras are scaled to."""

    def __init__(self, ctx, name):
        self.ctx, self.name = ctx, name
        if name == "fast64":
            self.hm = vr.synth_heightmap(ctx, 64)
            self.al = vr.synth_albedo(ctx, 64, self.hm)
            self.p, self.world = params(64), 64
        elif name == "odd":
            self.hm = np.ascontiguousarray(vr.synth_heightmap(ctx, 67)[:45, :67])
            h50 = vr.synth_heightmap(ctx, 50)
            self.al = np.ascontiguousarray(vr.synth_albedo(ctx, 50, h50)[:50, :33])
            self.p, self.world = params(64), 64
        else:
            self.hm = vr.synth_heightmap(ctx, 128)
            self.al = vr.synth_albedo(ctx, 128, self.hm)
            self.p, self.world = params(64), 128
            self.p.world_size = 128.0
        self.mh = qc.scaled_max_height(self.world)

    def terrain(self, hm, al, cast=True, render=True):
        """A terrain of (hm, al) in the state under test: node heights on, the pyramid built by one cast, one frame rendered."""
        tp = vr.TerrainPass(self.ctx, self.p).Init(hm, al)
        tp.SetHeight(True)
        if cast:
            tp.CastRays(np.float32([[0.0, 4.0 * self.mh, 0.0]]), np.float32([[0.1, -1.0, 0.2]]), np.inf, self.mh)
        if render:
            rt = vr.RenderTargets(self.ctx).Init(W, H)
            v = self.view(0)
            tp.Render(v, v, rt, vr.default_render_params(self.mh))
            rt.close()
        return tp

    def view(self, cam, w=W, h=H):
        eye, tgt = scaled_camera(CAMERAS[cam], self.world)
        return vr.make_view(eye, tgt, w, h)


class ExtraScene(Scene):
    """A scene of tests/texture_cases.py that SCENES does not have."""

    def __init__(self, ctx, name):
        self.ctx, self.name = ctx, name
        self.hm, self.al = tc.scene_maps(name, lambda n: vr.synth_heightmap(ctx, n), lambda n, h: vr.synth_albedo(ctx, n, h))
        self.p, self.world = params(64), int(tc.WORLD[name])
        self.mh = qc.scaled_max_height(self.world)


def make_scenes(ctx, names, world=None):
    """name -> scene, for a module's `scenes` fixture; `world`: the world size the module's cases were written for, per name."""
    out = {n: (Scene if n in SCENES else ExtraScene)(ctx, n) for n in names}
    for n, sc in out.items():
        assert world is None or world_of(sc) == world[n]
    return out


class Maps:
    """Host copies of the two maps that follow every edit made to terrain A."""

    def __init__(self, sc):
        self.hm, self.al = sc.hm.copy(), sc.al.copy()

    def edit(self, tp, which, x, y, texels):
        tp.Edit(which, x, y, texels)
        dst = self.hm if which == "height" else self.al
        dst[y:y + texels.shape[0], x:x + texels.shape[1]] = texels

    def random(self, tp, rng, which, x, y, w, h):
        shape = (h, w) if which == "height" else (h, w, 4)
        self.edit(tp, which, x, y, rng.integers(0, 256, shape, dtype=np.uint8))


def world_of(sc):
    return float(sc.p.world_size)


def dab(shape, world, tx, ty, r_tex, hardness, strength):
    """A dab whose centre is at texel coordinate (tx, ty) of a map of `shape` (texel i has its centre at coordinate i) and whose
    radius is r_tex texels of the map's width."""
    h, w = shape[:2]
    return [(tx + 0.5) / w * world - world / 2, (ty + 0.5) / h * world - world / 2, r_tex * world / w, hardness, strength]


def five_dabs(shape, world, op):
    """Mixed radii (0.4 .. 12 texels), hardness 0 and 0.7, one centre on a map corner, one outside the map that still overlaps it."""
    h, w = shape[:2]
    s = {bm.RAISE: (37.3, -21.6, 60.5, 13.2, -90.0), bm.FLATTEN: (0.6, 0.35, 0.8, 0.5, 1.0),
         bm.SMOOTH: (1.0, 0.6, 0.8, 0.5, 1.0), bm.PAINT: (0.6, 0.35, 0.8, 0.5, 1.0)}[op]
    return np.float32([dab(shape, world, 0.3 * w, 0.4 * h, 12.0, 0.0, s[0]),
                       dab(shape, world, 0.7 * w + 0.37, 0.6 * h + 0.21, 5.5, 0.7, s[1]),
                       dab(shape, world, -0.5, -0.5, 6.0, 0.0, s[2]),                   # the map's corner
                       dab(shape, world, w + 2.0, 0.5 * h, 4.5, 0.7, s[3]),             # outside, overlapping
                       dab(shape, world, 10.1, 7.2, 0.4, 0.0, s[4])])                   # one texel


def order_dabs(shape, world, strengths):
    """300 dabs: 290 whose spans all meet the 32 x 8 tile at the map's origin, five near the top right corner and five near the
    left edge further down - so the stroke's rectangle holds tiles no dab meets - and none that reaches the bottom rows."""
    rows = []
    for i in range(300):
        if i % 30 == 7:
            tx, ty = 57.0 + (i % 4) * 0.5, 4.0
        elif i % 30 == 19:
            tx, ty = 4.0, 38.0 + (i % 4) * 0.5
        else:
            tx, ty = 8.0 + (i * 7 % 160) * 0.1, 2.0 + (i * 3 % 40) * 0.1
        rows.append(dab(shape, world, tx, ty, 2.0 + (i % 5) * 0.5, 0.7 if i % 2 else 0.0, strengths[i % len(strengths)]))
    return np.float32(rows)


def mask_dabs(shape, world):
    """five_dabs with opacities for strengths: radii 0.4 .. 12 texels, hardness 0 and 0.7, a centre on the map's corner, one outside."""
    return five_dabs(shape, world, bm.FLATTEN)


def full_mask(world):
    return np.float32([[0.0, 0.0, 4.0 * world, 0.5, 1.0]])          # mask 1 on every texel


def borders(size, tile):
    return list(range(tile, size, tile))


BRUSH_OPS = {bm.RAISE: "raise", bm.FLATTEN: "flatten", bm.SMOOTH: "smooth", bm.PAINT: "paint"}
STROKE_KW = {bm.RAISE: {}, bm.FLATTEN: dict(target=141.0), bm.SMOOTH: {}, bm.PAINT: dict(color=(200.0, 10.0, 35.5, 99.0), channels=0b0101)}


def check_stroke_preconditions(before, after, op):
    """Asserted on the model's output: the stroke can tell a wrong kernel from a right one."""
    changed = (before != after) if before.ndim == 2 else (before != after).any(-1)
    assert changed.sum() >= 30, changed.sum()
    vals = after[changed]
    assert ((vals > 0) & (vals < 255)).sum() >= 10
    if op == bm.PAINT:
        assert np.array_equal(before[..., 1], after[..., 1]) and np.array_equal(before[..., 3], after[..., 3])


def level0(tp, which):
    return tp.download_mip(which, 0)


def assert_bytes(got, want, what):
    assert np.array_equal(got, want), f"{what}: {(got != want).sum()} bytes differ, first {np.argwhere(got != want)[:4].tolist()}"


def assert_chains_equal(a, b, what):
    for which in ("height", "albedo"):
        n = a.mip_levels(which)
        assert n == b.mip_levels(which)
        for l in range(n):
            x, y = a.download_mip(which, l), b.download_mip(which, l)
            assert np.array_equal(x, y), f"{what}: {which} level {l} differs in {(x != y).sum()} bytes, first {np.argwhere(x != y)[:4].tolist()}"


def assert_terrains_equal(sc, a, b, what):
    """Everything the library exposes of terrains A and B of scene `sc`: every mip level, node heights and selections, every G-buffer
    plane for cameras 0 and 5, 1024 sampled heights with normals, 64 ray hits, then the query pyramid itself and 64 hits under a negative
    max_height (assert_pyramids_equal), and the decoded tables themselves (assert_tables_equal)."""
    assert_chains_equal(a, b, what)
    assert_tables_equal(a, b, what)
    surfaces = int(sc.p.world_size / sc.p.surface_size) ** 2
    nodes = (4 ** (a.GetNumLods() + 1) - 1) // 3 * surfaces
    ha, hb = a.node_heights(0, nodes), b.node_heights(0, nodes)
    assert np.array_equal(ha.view(np.uint32), hb.view(np.uint32)), f"{what}: {(ha.view(np.uint32) != hb.view(np.uint32)).any(1).sum()} of {nodes} nodes differ"
    for cam in (0, 5):
        v = sc.view(cam)
        na, ia, insta = a.NodeSelect(v, sc.mh)
        nb, ib, instb = b.NodeSelect(v, sc.mh)
        assert na == nb and na > 0 and np.array_equal(ia, ib) and np.array_equal(insta, instb), (what, cam, na, nb)
        assert_frames_equal(render(sc, a, cam), render(sc, b, cam), f"{what}, camera {cam}")
    pts = qc.uniform_points(sc.world, 1024)
    (h1, n1), (h2, n2) = a.SampleHeights(pts, sc.mh, normals=True), b.SampleHeights(pts, sc.mh, normals=True)
    assert np.array_equal(h1.view(np.uint32), h2.view(np.uint32)) and np.array_equal(n1.view(np.uint32), n2.view(np.uint32))
    surf = Surface64(b.download_mip("height", 0), b.download_mip("height", 1), sc.world, sc.mh)
    o, d, tm = qc.make_rays(surf, sc.world, n=64)
    ra, rb = a.CastRays(o, d, tm, sc.mh), b.CastRays(o, d, tm, sc.mh)
    assert ra.tobytes() == rb.tobytes(), f"{what}: {(ra != rb).sum()} of {len(ra)} hits differ"
    assert (ra["status"] == capi.VR_RAY_HIT).sum() > 0
    assert_pyramids_equal(sc, a, b, what)


def assert_tables_equal(a, b, what):
    """What frames and samples cannot show: they read only the entries some pixel or point selects, of the one raster variant the pair of
    maps takes.  Every decoded table (quad, quadf, fast; fast, rgbf) of every level of both maps of A equals B's and equals
    tests/tables_model.py's of the device's own level, bit for bit."""
    ta = tm.assert_tables_are_the_model(a, f"{what}: A")
    tm.assert_tables_equal(ta, tm.assert_tables_are_the_model(b, f"{what}: B"), f"{what}: A's tables against B's")


def assert_pyramids_equal(sc, a, b, what):
    """What the rays above cannot show.  The query pyramids of A and B (both have cast by now) are equal level by level, and equal to
    tests/pyramid_model.py's of B's maps, byte for byte: a bound left too loose by a refresh only makes a walk longer.  And 64 rays
    built for max_height = -sc.mh are cast with it - the one sign under which the walk reads the lo plane: the same bytes from A and B."""
    pa, pb = a.QueryPyramid(), b.QueryPyramid()
    assert pa is not None and pb is not None and len(pa) == len(pb), what
    l0 = b.download_mip("height", 0)
    model = pm.levels(l0, b.download_mip("height", 1) if b.mip_levels("height") > 1 else l0)
    assert len(pb) == len(model), (what, len(pb), len(model))
    for l, (x, y, m) in enumerate(zip(pa, pb, model)):
        assert x.shape == y.shape == m.shape, (what, l, x.shape, y.shape, m.shape)
        assert np.array_equal(x, y), f"{what}: pyramid level {l}: {(x != y).any(-1).sum()} cells of A differ from B's, first {np.argwhere((x != y).any(-1))[:4].tolist()}"
        assert np.array_equal(y, m), f"{what}: pyramid level {l}: {(y != m).any(-1).sum()} cells differ from the model, first {np.argwhere((y != m).any(-1))[:4].tolist()}"
    below = Surface64(l0, b.download_mip("height", 1) if b.mip_levels("height") > 1 else l0, sc.world, -sc.mh)
    o, d, tm = qc.make_rays(below, sc.world, n=64)
    ra, rb = a.CastRays(o, d, tm, -sc.mh), b.CastRays(o, d, tm, -sc.mh)
    assert ra.tobytes() == rb.tobytes(), f"{what}: {(ra != rb).sum()} of {len(ra)} hits differ under max_height = {-sc.mh}"
    assert (ra["status"] == capi.VR_RAY_HIT).sum() > 0


def render(sc, tp, cam, part=None, **rpkw):
    rt = vr.RenderTargets(sc.ctx).Init(W, H)
    if not rpkw.get("assume_cleared"):
        rt.Clear()
    v = sc.view(cam)
    tp.Render(v, v, rt, vr.default_render_params(sc.mh, **rpkw), part)
    out = {p: rt.download(p).copy() for p in PLANES}
    rt.close()
    return out


def assert_frames_equal(a, b, what):
    for p in PLANES:
        x, y = bits(a[p]), bits(b[p])
        assert np.array_equal(x, y), f"{what}: {p} differs in {(x != y).sum()} elements, first {np.argwhere(x != y)[:4].tolist()}"


def submit_frames(sc, tp, views, fusion, edit=None, lock_after=False):
    """Two vr_frame_submit frames with the next view prepared ahead; `edit` runs between them.  Returns per frame the planes,
    HdrColor and the selected node ids."""
    ctx = sc.ctx
    ctx.set_frame_fusion(fusion)
    rt, hdr = vr.RenderTargets(ctx).Init(W, H), vr.HdrImage(ctx, W, H)
    out = []
    try:
        for i in range(2):
            rp = vr.default_render_params(sc.mh, assume_cleared=1, lock_view=1 if (lock_after and i == 1) else 0)
            fr = vr.Frame(tp, rt, rp, [vr.reference_sun()], AMBIENT_TOP, AMBIENT_BOTTOM)
            rt.Clear()
            hdr.upload(np.zeros(W * H * 4, np.uint16))
            fr.submit(views[i], hdr, views[i + 1:i + 2])
            ctx.synchronize()
            f = download_frame(rt, hdr)
            f["chunks"] = tp.num_chunks()
            out.append(f)
            if i == 0 and edit is not None:
                edit()
    finally:
        ctx.set_frame_fusion(1)
        hdr.close(); rt.close()
    return out


class Level0Op:
    """One operation that writes level 0.  `entry`: the C entry point's name; apply(tp, which, call): the one binding call, returns
    the rectangle; run_model(texels, call, world): (texels, rect, detail) of the numpy model.  `call` is the tuple the operation's
    tests/*_cases.py produce - arrays, a dict of parameters, and whatever else is hashable."""

    def __init__(self, entry, apply, run_model):
        self.entry, self.apply, self.run_model = entry, apply, run_model
        self.cache = {}

    def model(self, texels, call, world):
        """run_model, computed once per distinct call and left unchanged."""
        parts = tuple(repr(sorted(c.items())) if isinstance(c, dict) else np.asarray(c, np.float32).tobytes() if isinstance(c, np.ndarray) else c for c in call)
        key = (texels.tobytes(), texels.shape, parts, world)
        if key not in self.cache:
            self.cache[key] = self.run_model(texels, call, world)
        return self.cache[key]


def check_height_call(sc, op, call, what, preconditions):
    """One call on the heightmap: the rectangle is the model's, level 0 equals the model in every byte, the albedo is untouched, and
    the decoded tables are those of a terrain created from the model's map.  preconditions(before, want, detail, what) asserts on the
    model's output that the call can tell a wrong kernel from a right one, and returns its counts."""
    want, want_rect, detail = op.model(sc.hm, call, world_of(sc))
    print(what, preconditions(sc.hm, want, detail, what))
    a = sc.terrain(sc.hm, sc.al, cast=False, render=False)
    rect = op.apply(a, "height", call)
    assert rect == tuple(want_rect), (rect, want_rect)
    assert_bytes(level0(a, "height"), want, what)
    assert_bytes(level0(a, "albedo"), sc.al, f"{what}: the albedo")
    b = sc.terrain(want, sc.al, cast=False, render=False)
    assert_tables_equal(a, b, what)
    a.close(); b.close()


def check_albedo_call(sc, op, call, what, preconditions):
    """One call on the albedo with channel_mask 5: channels 1 and 3 of the model are the original's, the rectangle and level 0 are
    the model's, the heightmap is untouched, and the mip chains are those of a terrain created from the model's albedo."""
    want, want_rect, detail = op.model(sc.al, call, world_of(sc))
    print(what, preconditions(sc.al, want, detail, what))
    assert np.array_equal(want[..., 1], sc.al[..., 1]) and np.array_equal(want[..., 3], sc.al[..., 3])
    a = sc.terrain(sc.hm, sc.al, cast=False, render=False)
    assert op.apply(a, "albedo", call) == tuple(want_rect)
    assert_bytes(level0(a, "albedo"), want, what)
    assert_bytes(level0(a, "height"), sc.hm, f"{what}: the heightmap")
    b = sc.terrain(sc.hm, want, cast=False, render=False)
    assert_chains_equal(a, b, what)
    a.close(); b.close()


def check_one_call(sc, op, call, what, min_changed=200):
    """One call on the heightmap that changes at least min_changed texels of the model: the model's rectangle and bytes.  Returns the
    model's (rect, detail)."""
    want, want_rect, detail = op.model(sc.hm, call, world_of(sc))
    assert (want != sc.hm).sum() >= min_changed, what
    a = sc.terrain(sc.hm, sc.al, cast=False, render=False)
    assert op.apply(a, "height", call) == tuple(want_rect), what
    assert_bytes(level0(a, "height"), want, what)
    a.close()
    return want_rect, detail


def check_history(sc, op, single_calls, first, second):
    """Each of single_calls: enable, call, commit, undo: the original bytes; redo: the model's; one call is one record and one step.
    Then `first` and `second` before one commit: two records, one step, undone and redone as one."""
    S = world_of(sc)
    for call in single_calls:
        want = op.model(sc.hm, call, S)[0]
        assert (want != sc.hm).sum() >= 200
        a = sc.terrain(sc.hm, sc.al, cast=False, render=False)
        a.EnableHistory(1 << 20)
        op.apply(a, "height", call)
        assert a.HistoryStatus()["open_records"] == 1
        a.CommitHistory()
        st = a.HistoryStatus()
        assert (st["undo_steps"], st["redo_steps"], st["open_records"]) == (1, 0, 0)
        assert_bytes(level0(a, "height"), want, "after the call")
        assert a.Undo()
        assert_bytes(level0(a, "height"), sc.hm, "undone")
        assert a.Redo() and not a.Redo()
        assert_bytes(level0(a, "height"), want, "redone")
        assert_bytes(level0(a, "albedo"), sc.al, "the albedo")
        a.close()
    want = op.model(sc.hm, first, S)[0]
    both_ = op.model(want, second, S)[0]
    assert (both_ != want).sum() >= 30
    a = sc.terrain(sc.hm, sc.al, cast=False, render=False)
    a.EnableHistory(1 << 20)
    op.apply(a, "height", first)
    op.apply(a, "height", second)
    assert a.HistoryStatus()["open_records"] == 2
    a.CommitHistory()
    st = a.HistoryStatus()
    assert (st["undo_steps"], st["redo_steps"], st["open_records"]) == (1, 0, 0)
    assert_bytes(level0(a, "height"), both_, "two calls")
    assert a.Undo() and not a.Undo()
    assert_bytes(level0(a, "height"), sc.hm, "two calls undone in one step")
    assert a.Redo()
    assert_bytes(level0(a, "height"), both_, "two calls redone")
    a.close()


def check_order_with_nothing_between(sc, op, call, noun):
    """A RAISE stroke, the call and a thermal erosion queued back to back, no host wait between: both rectangles and the final bytes
    are those of the model's chain.  Asserted on the models first, 30 bytes each: the called map differs from the call on the map
    before the stroke, with and without the stroke behind it; the chain differs from the chain with the call left out, from the
    chain with the call before the stroke, and from the called map."""
    S = world_of(sc)
    stroke = five_dabs(sc.hm.shape, S, bm.RAISE)
    mask = nc.five_dabs(sc.hm.shape, S)
    brushed, _ = bm.stroke(sc.hm, bm.RAISE, stroke, S)
    called, call_rect, _ = op.model(brushed, call, S)
    want, erode_rect = em.erode(called, mask, S, 20, 0.5, 0.125)
    stale = op.model(sc.hm, call, S)[0]
    assert (stale != called).sum() >= 30 and (em.erode(brushed, mask, S, 20, 0.5, 0.125)[0] != want).sum() >= 30 and (want != called).sum() >= 30
    first = bm.stroke(stale, bm.RAISE, stroke, S)[0]
    assert (first != called).sum() >= 30 and (em.erode(first, mask, S, 20, 0.5, 0.125)[0] != want).sum() >= 30
    a = sc.terrain(sc.hm, sc.al)
    a.Brush("raise", stroke)
    assert op.apply(a, "height", call) == tuple(call_rect)
    assert a.Erode(mask, 20, 0.5, 0.125) == tuple(erode_rect)
    assert_bytes(level0(a, "height"), want, f"brush, {noun}, erode")
    assert_bytes(level0(a, "albedo"), sc.al, f"brush, {noun}, erode: the albedo")
    a.close()


def check_calls_that_launch_nothing(sc, op, good, misses, refused):
    """With history on: every call of `misses` returns (0, 0, 0, 0), on the model and on the device; every call of `refused` raises
    with the entry point's name; both maps and the history's status stay as they were.  Then `good` still gives the model's bytes."""
    S = world_of(sc)
    a = sc.terrain(sc.hm, sc.al, cast=False, render=False)
    a.EnableHistory(1 << 20)
    before = a.HistoryStatus()
    for call in misses:
        assert op.model(sc.hm, call, S)[1] == (0, 0, 0, 0)
        assert op.apply(a, "height", call) == (0, 0, 0, 0)
    for call in refused:
        with pytest.raises(Exception) as e:
            op.apply(a, "height", call)
        assert op.entry in str(e.value), e.value
    assert_bytes(level0(a, "height"), sc.hm, "after calls that launch nothing")
    assert_bytes(level0(a, "albedo"), sc.al, "after calls that launch nothing: the albedo")
    assert a.HistoryStatus() == before
    want, want_rect, _ = op.model(sc.hm, good, S)
    assert op.apply(a, "height", good) == tuple(want_rect)
    assert_bytes(level0(a, "height"), want, "after a good call")
    a.close()


def check_with_a_lazily_fused_frame_pending(op, call, model_map, noun, min_changed):
    """On the 256^2 fixture at 96 x 64: a fused frame that left its colour planes to their first reader, then the call, then a
    G-buffer download: the planes are those of the eager path (VR_OPT_GBUFFER_LAZY off); the next frame shows the call, and is the
    frame of a terrain created from model_map(heightmap), which differs from the heightmap in at least min_changed texels."""
    w, h = 96, 64
    with terrain_fixture(256) as fx:
        v = views(w, h)
        hm = fx["h"]
        want_map = model_map(hm)
        assert (want_map != hm).sum() >= min_changed

        def script(scn, lazy):
            out = {}
            try:
                scn.submit(v[1])
                op.apply(scn.tp, "height", call)
                out[f"before the {noun}"] = capture(scn.rt, scn.hdr)
                scn.submit(v[1])
                out[f"after the {noun}"] = capture(scn.rt, scn.hdr)
            finally:
                scn.tp.Edit("height", 0, 0, hm)
            return out
        want, _ = both(fx, w, h, script)
        assert not np.array_equal(want[f"before the {noun}"]["normals"], want[f"after the {noun}"]["normals"]), f"the {noun} is not in view"
        fresh = vr.TerrainPass(fx["ctx"], params(256)).Init(want_map, vr.synth_albedo(fx["ctx"], 256, hm))
        scn = LazyScene(dict(ctx=fx["ctx"], tp=fresh), 1, w, h)
        try:
            scn.submit(v[1])
            assert_same_frame(want[f"after the {noun}"], capture(scn.rt, scn.hdr), "the frame of a terrain created from the model's map", PLANES + ("hdr",))
        finally:
            scn.close()
            fresh.close()
