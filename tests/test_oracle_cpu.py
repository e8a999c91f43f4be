"""CPU tests of the oracle itself: known answers, golden fixtures, structural properties.

The reference has no tests or fixtures; what pins the oracle is (i) the node counts the
survey measured on the reference's own QuadTree.cpp, (ii) closed-form
known answers, (iii) an independent float64 numpy restatement of the shading model, (iv) an exact-arithmetic
(float64 / rational) evaluation of the draw written from the HLSL / D3D semantics (tests/f64_model.py), against
which the oracle's raster / sampler model is BOUNDED - and, from round 4 on, FROZEN (model revision + digest).
"""
import hashlib
import os

import numpy as np
import pytest

import vrenderer_amd as vr
from tests import f64_shading, f64_tonemap
from tests.common import AMBIENT_BOTTOM, AMBIENT_TOP, CAMERAS, DEFAULT_EYE, DEFAULT_TARGET, params, scaled_camera

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def t256(oracle):
    h = oracle.synth_heightmap(256)
    a = oracle.synth_albedo(256, h)
    t = oracle.OracleTerrain(params(256), h, a)
    yield t
    t.close()


def test_reference_recorded_counts_256(oracle, t256):
    # reference QuadTree.cpp, surface 256: 87,381 nodes, 8 LODs, 28 selected at the
    # default camera with frustum.intersectsWith stubbed to "always intersects"
    assert t256.num_lods == 8
    assert t256.num_nodes == 87381
    v = oracle.view_from_camera(DEFAULT_EYE, DEFAULT_TARGET, 1920, 1080)
    n, ids, _ = t256.select(v, 400.0, stub_frustum=True)
    assert n == 28


def test_reference_recorded_counts_2048(oracle):
    # surface 2048: 5,592,405 nodes, 11 LODs, 562 selected (frustum stubbed)
    h = np.zeros((2048, 2048), np.uint8)
    a = np.zeros((8, 8, 4), np.uint8)
    t = oracle.OracleTerrain(params(2048), h, a)
    assert t.num_lods == 11
    assert t.num_nodes == 5592405
    v = oracle.view_from_camera(DEFAULT_EYE, DEFAULT_TARGET, 1920, 1080)
    n, _, _ = t.select(v, 400.0, stub_frustum=True)
    assert n == 562
    # watertightness: from the reference's default camera the 2048 terrain fills the frame, so
    # any pixel left at the clear depth would be a crack between triangles / LOD levels
    w, hh = 480, 270
    v = oracle.view_from_camera(DEFAULT_EYE, DEFAULT_TARGET, w, hh)
    gb = oracle.GBufferHost(w, hh)
    t.render(v, gb, vr.default_render_params(400.0))
    assert (gb.depth < 1.0).all()
    t.close()


def test_lod_ranges(t256):
    # QuadTree::InitLodRanges: 4 * 2^i (QuadTree.cpp:234-241)
    assert np.array_equal(t256.lod_ranges(), 4.0 * 2.0 ** np.arange(12, dtype=np.float32))


def test_golden_select_ids(oracle, t256):
    g = np.load(os.path.join(GOLD, "select_ids.npz"))
    for ci, cam in enumerate(CAMERAS):
        eye, tgt = scaled_camera(cam, 256)
        v = oracle.view_from_camera(eye, tgt, 1920, 1080)
        n, ids, _ = t256.select(v, 400.0)
        assert np.array_equal(ids, g[f"ids_256_{ci}"]), ci


def _decode_id(i):
    d = 0
    while (4 ** (d + 1) - 1) // 3 <= i:
        d += 1
    rel = i - (4 ** d - 1) // 3
    return d, rel % (1 << d), rel // (1 << d)


def test_selection_structure(oracle, t256):
    """Selected nodes are pairwise disjoint subtrees in depth-first (TL,TR,BL,BR) order and the
    instance transform is scaling(extents) * translation(position) (TerrainPass.cpp:245-249)."""
    L = t256.num_lods
    for cam in CAMERAS:
        eye, tgt = scaled_camera(cam, 256)
        v = oracle.view_from_camera(eye, tgt, 1920, 1080)
        n, ids, inst = t256.select(v, 400.0)
        keys = []
        for k, i in enumerate(ids):
            d, ix, iz = _decode_id(int(i))
            path = 0
            for l in range(d - 1, -1, -1):
                bx, bz = (ix >> l) & 1, (iz >> l) & 1
                c = (1 if bx else 0) if bz else (3 if bx else 2)
                path = (path << 2) | c
            keys.append((path << (2 * (L - d)), d))
            ext = 128.0 / (1 << d)
            tr = np.frombuffer(inst[k].tobytes(), np.float32, 12, 16)
            assert tr[0] == ext and tr[10] == ext and tr[5] == 0.0
            assert tr[3] == -128.0 + (ix + 0.5) * 2 * ext and tr[11] == -128.0 + (iz + 0.5) * 2 * ext
            hdr = np.frombuffer(inst[k].tobytes(), np.uint32, 4, 0)
            assert list(hdr) == [0, 0, 0, 1]
        assert keys == sorted(keys), "not in depth-first order"
        for (ka, da), (kb, db) in zip(keys, keys[1:]):
            assert kb >= ka + (1 << (2 * (L - da))), "overlapping subtrees selected"


def test_golden_frame_regression(oracle, t256):
    g = np.load(os.path.join(GOLD, "frame_256x144.npz"))
    w, h = 256, 144
    eye, tgt = scaled_camera(CAMERAS[0], 256)
    v = oracle.view_from_camera(eye, tgt, w, h)
    assert bytes(v) == g["view"].tobytes()
    gb = oracle.GBufferHost(w, h)
    t256.render(v, gb, vr.default_render_params(400.0))
    for name in ("depth", "diffuse", "specular", "normals", "emissive"):
        assert np.array_equal(getattr(gb, name), g[name]), name
    hdr = oracle.deferred(v, gb, [vr.reference_sun()], AMBIENT_TOP, AMBIENT_BOTTOM)
    assert np.array_equal(hdr, g["hdr"])


def _frame_digest(gb, hdr):
    m = hashlib.sha256()
    for a in (gb.depth, gb.diffuse, gb.specular, gb.normals, gb.emissive, hdr):
        m.update(np.ascontiguousarray(a).tobytes())
    return m.hexdigest()


def test_model_revision_is_frozen(oracle, t256):
    """From round 4 on the oracle's per-pixel results may only change together with its model revision: the golden frame
    carries the revision it was made with, and tests/golden/MODEL_REVISIONS.txt holds one digest per revision - a changed
    output under an old number fails here, and make_golden.py refuses to overwrite a revision's digest."""
    g = np.load(os.path.join(GOLD, "frame_256x144.npz"))
    rev = oracle.model_revision()
    assert int(g["model_revision"]) == rev, "tests/golden/frame_256x144.npz was made by another model revision"
    lines = [l.split() for l in open(os.path.join(GOLD, "MODEL_REVISIONS.txt")) if l.strip() and not l.startswith("#")]
    digests = {int(a): b for a, b in lines}
    assert rev in digests, f"revision {rev} has no digest line in tests/golden/MODEL_REVISIONS.txt"
    w, h = 256, 144
    v = oracle.view_from_camera(*scaled_camera(CAMERAS[0], 256), w, h)
    gb = oracle.GBufferHost(w, h)
    t256.render(v, gb, vr.default_render_params(400.0))
    hdr = oracle.deferred(v, gb, [vr.reference_sun()], AMBIENT_TOP, AMBIENT_BOTTOM)
    assert _frame_digest(gb, hdr) == digests[rev], ("the oracle's output changed without a new model revision "
                                                    "(oracle/vr_oracle.c: ORC_MODEL_REVISION; DESIGN.md 2)")


@pytest.mark.parametrize("cam", [0, 1, 5, 6])
def test_raster_and_sampler_model_is_bounded_by_exact_arithmetic(oracle, t256, cam):
    """The oracle's implementation choices (raster model revision 3: per-triangle plane equations set up in double and
    evaluated with two fmaf per pixel, fused sampler arithmetic, a pinned cubic for log2) against tests/f64_model.py - the
    same draw evaluated from the HLSL / D3D text with exact integer edge functions, rational barycentrics and float64
    everywhere.  Bounds (the golden 256x144 frame's camera and three more):
      coverage          identical, and no pixel whose depth test was decided by less than 4 fp32 ulps
      depth             within 1 fp32 ulp of the correctly rounded exact value (<= 1.5 ulp absolute)
      world xz          within 4 fp32 ulps (of the world's half size: 6e-5 units, 6e-5 texels) of the exact perspective-correct interpolation
      implicit LOD      within 2e-3 of log2(rho) (the pinned cubic's 1.1e-3 + fp32 rounding)
      albedo (SRGBA8)   at most one code, on at most 0.1 % of the covered pixels (sampled at the oracle's LOD)
      normal (SNORM16)  at most one code per component, on at most 2 % of the components
    The HIP path is then bit-exact against the oracle (tests/test_gpu_parity.py), so these bounds carry over to it."""
    from tests import f64_model as F
    w, h, size = 256, 144, 256
    v = oracle.view_from_camera(*scaled_camera(CAMERAS[cam], size), w, h)
    gb = oracle.GBufferHost(w, h)
    dbg = np.zeros((h, w, 3), np.float32)
    t256.render(v, gb, vr.default_render_params(400.0), debug_plane=dbg)
    hml = [t256.height_mip(l) for l in range(t256.height_levels())]
    alb = [t256.albedo_mip(l) for l in range(t256.albedo_levels())]
    fr = F.render(t256, v, w, h, 400.0, float(size), hml, alb, lod_for_sampling=dbg[..., 0])
    cov = gb.depth < 1.0
    assert cov.sum() > 4000 and fr.tri_count["rasterised"] > 2000
    assert np.array_equal(cov, fr.covered), f"coverage differs at {(cov != fr.covered).sum()} pixels"
    assert fr.ambiguous.sum() == 0 and fr.from_clipper.sum() == 0
    m = cov
    exact32 = fr.depth.astype(np.float32)
    ulps = np.abs(gb.depth.view(np.int32).astype(np.int64) - exact32.view(np.int32).astype(np.int64))
    assert ulps[m].max() <= 1, f"depth: {ulps[m].max()} ulps from the rounded exact value"
    err = np.abs(gb.depth.astype(np.float64) - fr.depth) / np.spacing(exact32).astype(np.float64)
    assert err[m].max() <= 1.5
    for k, exact in ((1, fr.wx), (2, fr.wz)):
        e = np.abs(dbg[..., k].astype(np.float64) - exact) / float(np.spacing(np.float32(size / 2)))
        assert e[m].max() <= 4.0, f"world {'xz'[k - 1]}: {e[m].max():.2f} ulps of the world's half size"
    assert fr.lod[m].min() < 0.0 and fr.lod[m].max() > 2.0, "the frame must hold magnified and minified pixels"
    dl = np.abs(dbg[..., 0].astype(np.float64) - fr.lod)
    assert dl[m].max() <= 2e-3, f"implicit LOD: {dl[m].max():.5f}"
    rgb = np.stack([(gb.diffuse >> (8 * k)) & 255 for k in range(3)], -1).astype(np.int64)
    dc = np.abs(rgb - fr.albedo_codes)[m]
    assert dc.max() <= 1 and (dc.max(-1) > 0).mean() <= 1e-3, (dc.max(), (dc.max(-1) > 0).mean())
    nn = gb.normals[..., :3].view(np.int16).astype(np.int64)
    dn = np.abs(nn - fr.normal_codes)[m]
    assert dn.max() <= 1 and (dn > 0).mean() <= 0.02, (dn.max(), (dn > 0).mean())
    assert np.all(gb.normals[..., 3][m] == 32767) and np.all(gb.emissive[m] == 0)
    spec = int(oracle.lib().orc_linear_to_srgb8(np.float32(0.01)))                    # terrain_ps.hlsl:76
    assert np.all(gb.specular[m] == (spec | spec << 8 | spec << 16 | 0xff000000))


def test_flat_terrain_known_answers(oracle):
    """Flat heightmap => normal (0,1,0) and depth of a plane; constant albedo survives the sRGB round trip."""
    size = 256
    h = np.full((size, size), 77, np.uint8)
    a = np.zeros((size, size, 4), np.uint8)
    a[...] = (128, 64, 200, 255)
    t = oracle.OracleTerrain(params(size), h, a)
    w, hh = 320, 180
    v = oracle.view_from_camera((0.0, 160.0, 30.0), (0.0, 120.0, 0.0), w, hh)
    gb = oracle.GBufferHost(w, hh)
    t.render(v, gb, vr.default_render_params(400.0))
    cov = gb.depth < 1.0
    assert cov.mean() > 0.9
    n = gb.normals.view(np.int16)[cov]
    assert (n[:, 0] == 0).all() and (n[:, 1] == 32767).all() and (n[:, 2] == 0).all() and (n[:, 3] == 32767).all()
    assert (gb.diffuse[cov] == (128 | (64 << 8) | (200 << 16) | (255 << 24))).all()
    assert (gb.specular[cov] == (25 | (25 << 8) | (25 << 16) | (255 << 24))).all()   # sRGB8(0.01) = 25
    assert not gb.emissive.any()
    # world height of the plane is 77/255*400; reconstruct it from depth at the image centre
    y_plane = np.float32(77) / np.float32(255) * np.float32(400)
    c2w = np.array(v.clip_to_world[:], np.float64).reshape(4, 4)
    py, px = hh // 2, w // 2
    clip = np.array([(px + 0.5) * 2 / w - 1, 1 - (py + 0.5) * 2 / hh, float(gb.depth[py, px]), 1.0])
    wp = clip @ c2w
    assert abs(wp[1] / wp[3] - float(y_plane)) < 0.05
    # Lambert known answer: sun straight down, irradiance 1 -> diffuse = albedo / pi (+ ambient top)
    sun = vr.directional_light((0.0, -1.0, 0.0), 1.0, 0.0)
    out = oracle.deferred(v, gb, [sun], (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), f32=True)
    alb = np.array([oracle.lib().orc_srgb8_to_linear(c) for c in (128, 64, 200)])
    # what is left after the Lambert term is the GGX lobe: F0 is grey (25,25,25), so it is the
    # same small positive number in every channel
    rest = out[py, px, :3].astype(np.float64) - alb / np.pi
    assert np.all(rest > 0) and np.all(rest < 2e-3) and np.ptp(rest) < 1e-6
    t.close()


def test_deferred_matches_independent_float64_model(oracle):
    """The C oracle's closed-form area-light correction equals the slerp formulation (float64 numpy)."""
    g = np.load(os.path.join(GOLD, "frame_256x144.npz"))
    gb = oracle.GBufferHost(256, 144)
    for name in ("depth", "diffuse", "specular", "normals", "emissive"):
        getattr(gb, name)[...] = g[name]
    v = vr.View.from_buffer_copy(g["view"].tobytes())
    lights = [vr.reference_sun(), vr.point_light((10.0, 40.0, -5.0), 3000.0, 120.0, (1.0, 0.5, 0.25)),
              vr.spot_light((-20.0, 60.0, 10.0), (0.3, -1.0, -0.2), 6000.0, 200.0, 12.0, 25.0, (0.2, 1.0, 0.4)),
              vr.point_light((30.0, 35.0, -30.0), 2000.0, 150.0, (0.9, 0.9, 1.0), radius=6.0),
              vr.spot_light((0.0, 80.0, -40.0), (0.0, -1.0, 0.3), 9000.0, 0.0, 5.0, 40.0, (1.0, 0.2, 0.2), radius=3.0)]
    got = oracle.deferred(v, gb, lights, AMBIENT_TOP, AMBIENT_BOTTOM, f32=True)[..., :3]
    only_sun = oracle.deferred(v, gb, lights[:1], AMBIENT_TOP, AMBIENT_BOTTOM, f32=True)[..., :3]
    assert np.abs(got - only_sun).max() > 1e-3, "the local lights must reach the terrain"
    want = f64_shading.shade_frame(v, gb, lights, AMBIENT_TOP, AMBIENT_BOTTOM)
    assert np.abs(got - want).max() < 2e-5 * max(1.0, np.abs(want).max())


def test_half_and_srgb_conversions(oracle):
    rng = np.random.default_rng(7)
    x = np.concatenate([rng.normal(0, 1, 4000), rng.uniform(-70000, 70000, 2000), 10.0 ** rng.uniform(-9, 5, 3000),
                        [0.0, -0.0, 65504.0, 65520.0, 1e-8, 6e-8, 5.96e-8, 2.98e-8, np.inf, -np.inf]]).astype(np.float32)
    ours = np.array([oracle.lib().orc_float_to_half(float(v)) for v in x], np.uint16)
    with np.errstate(over="ignore"):
        ref = x.astype(np.float16).view(np.uint16)
    assert np.array_equal(ours, ref)
    back = np.array([oracle.lib().orc_half_to_float(int(v)) for v in range(0, 65536, 7)], np.float32)
    refb = np.arange(0, 65536, 7, dtype=np.uint16).view(np.float16).astype(np.float32)
    assert np.array_equal(back.view(np.uint32)[~np.isnan(refb)], refb.view(np.uint32)[~np.isnan(refb)])
    for c in range(256):
        lin = oracle.lib().orc_srgb8_to_linear(c)
        assert oracle.lib().orc_linear_to_srgb8(lin) == c
    assert oracle.lib().orc_linear_to_srgb8(0.01) == 25
    assert oracle.lib().orc_linear_to_srgb8(-1.0) == 0 and oracle.lib().orc_linear_to_srgb8(2.0) == 255


def test_view_helper_sanity(oracle):
    v = oracle.view_from_camera(DEFAULT_EYE, DEFAULT_TARGET, 1920, 1080)
    m = np.array(v.world_to_view[:], np.float64).reshape(4, 4)
    assert np.allclose(m[:3, :3].T @ m[:3, :3], np.eye(3), atol=1e-6)
    assert v.mirrored == 1          # right = dir x up: left-handed view space (front = CCW)
    tgt = np.array(DEFAULT_TARGET + (1.0,), np.float64)
    for p in v.planes:
        assert np.dot(p[:3], tgt[:3]) - p[3] < 0, "look-at target must be inside the frustum"
    eye = np.array(DEFAULT_EYE)
    assert np.dot(np.array(v.planes[0][:3]), eye) - v.planes[0][3] > 0, "eye is behind the near plane"
    c2w = np.array(v.clip_to_world[:], np.float64).reshape(4, 4)
    w2c = np.array(v.world_to_clip[:], np.float64).reshape(4, 4)
    for p in ((1.0, 1.8, 0.0, 1.0), (-200.0, 50.0, -300.0, 1.0), (30.0, 120.0, 100.0, 1.0)):
        c = np.array(p) @ w2c
        q = (c / c[3]) @ c2w            # clip_to_world is stored in fp32: round trip to ~1e-3 relative
        assert np.allclose(q[:3] / q[3], p[:3], rtol=2e-3, atol=0.3)


def test_partitioned_render_equals_unsplit(oracle, t256):
    from vrenderer_amd import partition as pt
    w, h = 300, 260     # not a multiple of the tile size: exercises ragged edge tiles
    eye, tgt = scaled_camera(CAMERAS[5], 256)
    v = oracle.view_from_camera(eye, tgt, w, h)
    rp = vr.default_render_params(400.0)
    full = oracle.GBufferHost(w, h)
    t256.render(v, full, rp)
    world = 3
    seen = np.zeros((h, w), np.int32)
    for r in range(world):
        gb = oracle.GBufferHost(w, h)
        t256.render(v, gb, rp, vr.Partition(r, world))
        tx, _ = pt.owner_grid(w, h)
        own = np.zeros((h, w), bool)
        for t in pt.owned_tiles(w, h, r, world):
            own[(t // tx) * 128:(t // tx) * 128 + 128, (t % tx) * 128:(t % tx) * 128 + 128] = True
        seen += own
        assert np.array_equal(gb.depth[own], full.depth[own]) and np.array_equal(gb.diffuse[own], full.diffuse[own])
        assert (gb.depth[~own] == 1.0).all() and not gb.diffuse[~own].any(), "a rank touched pixels it does not own"
    assert (seen == 1).all()


def test_set_height_known_answers(oracle, t256):
    """QuadTree::SetHeight (QuadTree.cpp:164-208): the root spans the whole heightmap, a leaf one texel."""
    h = oracle.synth_heightmap(256)
    try:
        t256.set_height(True)
        nh = t256.node_heights()
        mn, mx = np.float32(h.min()) / np.float32(255), np.float32(h.max()) / np.float32(255)
        ext = (mx - mn) / np.float32(2)
        assert nh[0, 1] == ext and nh[0, 0] == mn + ext
        L = t256.num_lods
        base = (4 ** L - 1) // 3
        for (ix, iz) in ((0, 0), (17, 200), (255, 255)):
            py, ey = nh[base + iz * 256 + ix]
            # single texel: max - min == 0 -> min forced to 0 (QuadTree.cpp:186), so the box is [0, h]
            half = (np.float32(h[iz, ix]) / np.float32(255)) / np.float32(2)
            assert ey == half and py == half
        d = L - 1                                    # 2x2 texel nodes
        b1 = (4 ** d - 1) // 3
        blk = h[0:2, 0:2].astype(np.float32) / np.float32(255)
        e1 = (blk.max() - blk.min()) / np.float32(2)
        lo = np.float32(0) if blk.max() == blk.min() else blk.min()
        e1 = (blk.max() - lo) / np.float32(2)
        assert nh[b1, 1] == e1 and nh[b1, 0] == lo + e1
    finally:
        t256.set_height(False)


def test_wireframe_structure(oracle, t256):
    """RasterFillMode::Wireframe: line pixels hug the filled surface and leave the interiors open."""
    w, h = 480, 270
    eye, tgt = scaled_camera(CAMERAS[0], 256)
    v = oracle.view_from_camera(eye, tgt, w, h)
    fill = oracle.GBufferHost(w, h)
    t256.render(v, fill, vr.default_render_params(400.0))
    wire = oracle.GBufferHost(w, h)
    t256.render(v, wire, vr.default_render_params(400.0, wireframe=1))
    f, l = fill.depth < 1.0, wire.depth < 1.0
    assert 0 < l.sum() < f.sum()
    grown = f.copy()                                   # a line pixel contains a point of a filled triangle's edge
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            grown |= np.roll(np.roll(f, dy, 0), dx, 1)
    assert not (l & ~grown).any()
    # a line pixel samples its triangle's plane: the nearest surface there is at most a pixel's slope away
    both = f & l
    assert np.median(np.abs(wire.depth[both] - fill.depth[both])) < 1e-5
    assert (wire.specular[l] == wire.specular[l][0]).all() and not wire.specular[~l].any()
    # triangles here are only a few pixels across, yet a good part of their interiors stays open
    assert l[f].mean() < 0.9


def test_tonemap_known_answers(oracle):
    """ToneMappingPass restatement (f3): closed-form checks of the three stages."""
    p = vr.default_tonemap_params()
    L = oracle.lib()
    # pinned log2 / exp2: accurate enough for 256 bins over 14 stops (bin width 0.055)
    xs = np.exp2(np.linspace(-12, 6, 2001)).astype(np.float32)
    assert max(abs(L.orc_log2_pinned(float(x)) - np.log2(float(x))) for x in xs) < 2e-3
    es = np.linspace(-11, 5, 2001).astype(np.float32)
    assert max(abs(L.orc_exp2_pinned(float(e)) / 2.0 ** float(e) - 1.0) for e in es) < 2e-4
    assert L.orc_exp2_pinned(3.0) == 8.0 and L.orc_log2_pinned(0.25) == -2.0

    def frame(values, counts):
        px = np.concatenate([np.full(c, v, np.float16) for v, c in zip(values, counts)])
        img = np.zeros((1, px.size, 4), np.float16)
        img[0, :, :3] = px[:, None]
        return img.view(np.uint16)

    # uniform mid grey: all weight (64 per pixel) in the two bins around log2(0.18); exposure = its luminance
    tm = oracle.ToneMapper()
    g = frame([0.18], [4096])
    ldr = tm.SimpleRender(p, g)
    lum = float(np.float16(0.18)) * (0.2126 + 0.7152 + 0.0722)
    t = (np.log2(lum) + 10.0) / 14.0 * 255.0
    assert tm.hist.sum() == 64 * 4096 and set(tm.hist.nonzero()[0]) == {int(t), int(t) + 1}
    assert abs(tm.adapted / lum - 1.0) < 0.02
    scaled = 2.0 ** -0.5 * lum / tm.adapted
    mapped = scaled * (1 + scaled / 9.0) / (1 + scaled)
    srgb = 1.055 * mapped ** (1 / 2.4) - 0.055
    assert abs(int(ldr[0, 0, 0]) - srgb * 255.0) <= 1.0 and (ldr[..., 3] == 255).all()
    assert (ldr[..., 0] == ldr[..., 1]).all() and (ldr[..., 1] == ldr[..., 2]).all()

    # percentile window [0.8, 0.95]: 90 % of the pixels at 0.1, 10 % at 10 -> 2/3 of the window is dark, 1/3 bright
    tm = oracle.ToneMapper()
    tm.SimpleRender(p, frame([0.1, 10.0], [9000, 1000]))
    expect = 2.0 ** ((2.0 / 3.0) * np.log2(0.1) + (1.0 / 3.0) * np.log2(10.0))
    assert abs(tm.adapted / expect - 1.0) < 0.05
    # clamps: a black frame adapts to the minimum, a very bright one to the maximum
    tm = oracle.ToneMapper(); tm.SimpleRender(p, frame([0.0], [256])); assert tm.adapted == pytest.approx(0.02)
    tm = oracle.ToneMapper(); tm.SimpleRender(p, frame([100.0], [256])); assert tm.adapted == pytest.approx(0.5)

    # eye adaptation: the first frame jumps, later frames move by (1 - exp(-dt * speed)) of the gap
    tm = oracle.ToneMapper()
    tm.AdvanceFrame(1.0 / 60.0)
    tm.SimpleRender(p, frame([0.05], [1024])); a0 = tm.adapted
    tm.SimpleRender(p, frame([0.4], [1024])); a1 = tm.adapted
    target = float(np.float16(0.4))
    assert a0 < a1 < target
    assert abs((a1 - a0) / (target - a0) - (1 - np.exp(-1.0 / 60.0 * 1.0))) < 2e-3      # brighter: eyeAdaptationSpeedUp = 1
    tm.SimpleRender(p, frame([0.05], [1024])); a2 = tm.adapted
    assert abs((a1 - a2) / (a1 - a0) - (1 - np.exp(-1.0 / 60.0 * 0.5))) < 2e-2         # darker: speedDown = 0.5
    # black pixels stay black; an inf pixel has L = inf, s = inf and mapped = inf / inf = NaN in the written order (the
    # float64 model, tests/f64_tonemap.py): it encodes to black
    img = np.zeros((1, 2, 4), np.float16); img[0, 1, :3] = np.inf
    tm = oracle.ToneMapper()
    out = tm.SimpleRender(p, img.view(np.uint16))
    model = f64_tonemap.operator(img.view(np.uint16)[0, :, :3], tm.adapted, p)
    assert model["lo"].tolist() == model["hi"].tolist() == [[0, 0, 0], [0, 0, 0]]
    assert out[0, 0].tolist() == [0, 0, 0, 255] and out[0, 1].tolist() == [0, 0, 0, 255]


def test_shadow_view_and_shadow_term_known_answers(oracle, t256):
    """Row f1: the one-cascade "stable" light view (Renderer.cpp:345-352) and the PCF shadow term."""
    import ctypes as C
    lib = vr.load_library()
    sun = vr.reference_sun()
    eye, tgt = scaled_camera(CAMERAS[0], 256)
    cam = oracle.view_from_camera(eye, tgt, 480, 270)
    p = vr.default_shadow_params(256.0, resolution=256)
    lv = oracle.shadow_view(sun, cam, p)
    host = vr.View()
    assert lib.vr_shadow_view_setup(C.byref(sun), C.byref(cam), C.byref(p), C.byref(host)) == 0
    for f in ("world_to_view", "view_to_clip", "world_to_clip", "clip_to_world", "camera_pos"):
        assert np.array_equal(np.array(getattr(host, f)[:]), np.array(getattr(lv, f)[:])), f      # library host code == restatement
    w2v = np.array(lv.world_to_view[:], np.float64).reshape(4, 4)
    d = np.array(sun.direction[:], np.float64)
    assert np.allclose(w2v[:3, 2], d / np.linalg.norm(d), atol=1e-6)                 # looks along the light
    assert np.allclose(w2v[:3, :3].T @ w2v[:3, :3], np.eye(3), atol=1e-5) and lv.mirrored == 0
    radius = 1.0 / lv.view_to_clip[0]
    # in x and y the box holds the camera and the four corners of the frustum slice at maxShadowDistance
    c2w = np.array(cam.clip_to_world[:], np.float64).reshape(4, 4)
    w2c_l = np.array(lv.world_to_clip[:], np.float64).reshape(4, 4)
    fwd = np.array(cam.world_to_view[:], np.float64).reshape(4, 4)[:3, 2]
    pts = [np.array(cam.camera_pos[:3], np.float64)]
    for sx in (-1, 1):
        for sy in (-1, 1):
            q = np.array([sx, sy, 1.0, 1.0]) @ c2w
            far = q[:3] / q[3]
            ray = far - pts[0]
            pts.append(pts[0] + ray * (256.0 / (ray @ fwd)))
    texel = 2.0 * radius / 256
    for q in pts:
        ndc = np.append(q, 1.0) @ w2c_l
        assert abs(ndc[0]) <= 1.0 + 2 * texel / radius and abs(ndc[1]) <= 1.0 + 2 * texel / radius      # z: the caller's zUp / zDown, not the sphere
    # stable: the light-space origin sits on the texel grid, so a small camera move shifts it by whole texels
    cam2 = oracle.view_from_camera((eye[0] + 0.37, eye[1], eye[2] - 0.21), tgt, 480, 270)
    lv2 = oracle.shadow_view(sun, cam2, p)
    shift = (np.array(lv2.camera_pos[:3], np.float64) - np.array(lv.camera_pos[:3], np.float64)) @ w2v[:3, :2] / texel
    assert np.allclose(shift, np.round(shift), atol=2e-3)

    # shadow term on a lit frame
    gb = oracle.GBufferHost(480, 270)
    t256.render(cam, gb, vr.default_render_params(400.0))
    plain = oracle.deferred(cam, gb, [sun], AMBIENT_TOP, AMBIENT_BOTTOM, f32=True)
    none = oracle.deferred(cam, gb, [], AMBIENT_TOP, AMBIENT_BOTTOM, f32=True)
    covered = gb.depth < 1.0
    open_map = np.ones((256, 256), np.float32)                                   # nothing between the light and anything
    lit = oracle.deferred(cam, gb, [sun], AMBIENT_TOP, AMBIENT_BOTTOM, f32=True, shadow=(lv, open_map, 0, 0.0))
    assert np.array_equal(lit, plain)
    blocked = np.zeros((256, 256), np.float32)                                   # an occluder at depth 0 everywhere
    dark = oracle.deferred(cam, gb, [sun], AMBIENT_TOP, AMBIENT_BOTTOM, f32=True, shadow=(lv, blocked, 0, 0.0))
    assert np.array_equal(dark[covered], none[covered])                          # only the ambient term is left
    # block the map's columns left of the middle of what the camera sees: dark side, lit side, and a PCF ramp between
    ys, xs = np.nonzero(covered)
    clip = np.stack([(xs + 0.5) * 2 / 480 - 1, 1 - (ys + 0.5) * 2 / 270, gb.depth[ys, xs].astype(np.float64), np.ones(len(xs))], 1)
    wpos = clip @ c2w
    u_tex = ((wpos / wpos[:, 3:4]) @ w2c_l)[:, 0] * 0.5 + 0.5
    split = int(np.median(u_tex) * 256)
    half = np.ones((256, 256), np.float32); half[:, :split] = 0.0
    mixed = oracle.deferred(cam, gb, [sun], AMBIENT_TOP, AMBIENT_BOTTOM, f32=True, shadow=(lv, half, 0, 0.0))
    sunlit = covered & np.any(plain != none, axis=-1)                            # pixels the sun reaches at all
    is_dark = np.all(mixed == none, axis=-1) & sunlit
    is_lit = np.all(mixed == plain, axis=-1) & sunlit
    partial = sunlit & ~is_dark & ~is_lit
    assert is_dark.sum() > 100 and is_lit.sum() > 100 and 0 < partial.sum() < 0.5 * sunlit.sum()
    assert (mixed[partial] <= plain[partial] + 1e-7).all() and (mixed[partial] >= none[partial] - 1e-7).all()
    u_img = np.zeros(covered.shape); u_img[ys, xs] = u_tex * 256
    assert u_img[is_dark].max() < split + 1.5 and u_img[is_lit].min() > split - 2.5     # the ramp is the 4-texel footprint
    # outside the map the light's outOfBoundsShadow applies
    tiny = vr.default_shadow_params(256.0, resolution=256, max_shadow_distance=1.0)
    lv_t = oracle.shadow_view(sun, cam, tiny)
    sun_oob = vr.reference_sun(); sun_oob.out_of_bounds_shadow = 1.0
    out = oracle.deferred(cam, gb, [sun_oob], AMBIENT_TOP, AMBIENT_BOTTOM, f32=True, shadow=(lv_t, blocked, 0, 0.0))
    far_px = gb.depth > np.quantile(gb.depth[covered], 0.5)
    assert np.array_equal(out[far_px & covered], plain[far_px & covered])


def test_oracle_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """`make -C oracle asan` (sanitizers on the CPU build - GPU AddressSanitizer is not available on the pool) and one
    small frame through the instrumented library: select, raster, pixel shader, lighting, tone map.  `make -C oracle asan-test`
    runs the whole oracle-driven suites the same way; this keeps the target from rotting."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run(["make", "-C", os.path.join(root, "oracle"), "asan"], check=True, capture_output=True, text=True)
    cc = os.environ.get("CC", "gcc")
    pre = " ".join(subprocess.run([cc, f"-print-file-name={n}"], capture_output=True, text=True, check=True).stdout.strip()
                   for n in ("libasan.so", "libubsan.so"))
    env = dict(os.environ, LD_PRELOAD=pre, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1",
               VR_ORACLE_LIB=os.path.join(root, "oracle", "_build", "libvroracle_asan.so"))
    code = ("import numpy as np\n"
            "import vrenderer_amd as vr\n"
            "from oracle import pyoracle as o\n"
            "from vrenderer_amd.scene import params, scaled_camera, DEFAULT_EYE, DEFAULT_TARGET, AMBIENT_TOP, AMBIENT_BOTTOM\n"
            "o.lib()\n"
            "h = o.synth_heightmap(64); a = o.synth_albedo(64, h)\n"
            "t = o.OracleTerrain(params(64), h, a)\n"
            "v = o.view_from_camera(*scaled_camera((DEFAULT_EYE, DEFAULT_TARGET), 64), 96, 54)\n"
            "gb = o.GBufferHost(96, 54)\n"
            "n = t.render(v, gb, vr.default_render_params(400.0))\n"
            "assert n > 0 and (gb.depth < 1.0).any()\n"
            "print('sanitized frame ok', n)\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "sanitized frame ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


EDGE_W, EDGE_H = 512, 128


@pytest.mark.parametrize("lights_name", ["suns", "points", "extra", "max", "tiled"])
def test_oracle_within_the_float64_bound_on_the_edge_case_frame(oracle, lights_name):
    """The fp32 oracle's half output against the float64 model (tests/f64_shading.py) on the edge-case frame: every
    unflagged value within its bound, flagged ones in their envelope, NaN / infinity where the model has them."""
    view, planes, rows = f64_shading.edge_case_frame(vr, EDGE_W, EDGE_H)
    lights = f64_shading.edge_lights(vr, view, planes, rows)[lights_name]
    gb = oracle.GBufferHost(EDGE_W, EDGE_H)
    for k, a in planes.items():
        getattr(gb, k)[...] = a
    got = oracle.half_to_float(oracle.deferred(view, gb, lights, AMBIENT_TOP, AMBIENT_BOTTOM))[..., :3]
    pix = f64_shading.Pixels.from_planes(planes)
    r = f64_shading.check(got.astype(np.float64).reshape(-1, 3),
                          f64_shading.reference(pix, view, lights, AMBIENT_TOP, AMBIENT_BOTTOM), pix, f"oracle, {lights_name}",
                          caps=f64_shading.EDGE_CAPS)
    assert r["checked"] > 0.9 * got.size
    if not any(l.type == vr.VR_LIGHT_DIRECTIONAL for l in lights):
        return
    y0, y1 = rows["far_plane"]
    amb_only = f64_shading.reference(f64_shading.Pixels.from_planes(planes, np.arange(EDGE_W), np.full(EDGE_W, y0)), view, [],
                                     AMBIENT_TOP, AMBIENT_BOTTOM)["ref"]
    assert (np.abs(got[y0, :, :3] - amb_only) > 1e-3).mean() > 0.2, "texels at depth 1.0 with real planes are lit"


@pytest.mark.parametrize("width,w_scale", [(2048, 1.0), (2048, 2.0), (2047, 1.0)])
def test_oracle_shadowed_within_the_float64_bound(oracle, width, w_scale):
    """The shadowed oracle on the PCF frame (tests/f64_shading.py: pcf_frame): receivers over the map's ramp,
    checkerboard, constants 0 and 1 and exactly on a stored depth, footprints over every edge and corner, u / v / zc
    exactly 0 and 1, an orthographic (w = 1) and a general (w = 2) light matrix; every pixel checked."""
    cam, lv, smap, planes = f64_shading.pcf_frame(vr, w_scale, width)
    sun = vr.reference_sun()
    lights = [sun, vr.directional_light((0.3, -1.0, 0.2), 0.5, 0.0)]
    gb = oracle.GBufferHost(width, f64_shading.PCF_H)
    for k, a in planes.items():
        getattr(gb, k)[...] = a
    got = oracle.half_to_float(oracle.deferred(cam, gb, lights, AMBIENT_TOP, AMBIENT_BOTTOM,
                                               shadow=(lv, smap, 0, f64_shading.PCF_BIAS)))[..., :3]
    pix = f64_shading.Pixels.from_planes(planes)
    sh = (lv, smap, 0, f64_shading.PCF_BIAS, sun.out_of_bounds_shadow)
    r = f64_shading.reference(pix, cam, lights, AMBIENT_TOP, AMBIENT_BOTTOM, shadow=sh,
                              exact_geometry=True if width == 2048 else "vz")
    res = f64_shading.check(got, r, pix, f"oracle, PCF frame {width}, w = {w_scale}")
    assert res["checked"] > 0.99 * got.size
    cov = f64_shading.pcf_coverage(r["shadow_geo"], W=width)
    for k in ("v0", "v1", "z0", "z1", "edge", "outside") + (("u0", "u1") if width == 2048 else ()):
        assert cov[k] > 0, cov
    assert cov["clamp_path"] > 1000 and cov["row_path"] > 1000, cov


# ---- the tone mapper against its float64 model (tests/f64_tonemap.py) ----------------------------------------------
def _oracle_step(oracle, tm, p, frame, dt, what, old):
    tm.AdvanceFrame(dt)
    ldr = tm.SimpleRender(p, frame)
    rgb = frame[..., :3].reshape(-1, 3)
    return f64_tonemap.check_step(tm.hist, tm.adapted, ldr[..., :3].reshape(-1, 3), f64_tonemap.PixelSet.from_frame(frame), p, dt,
                                  old, what, codes=rgb)


@pytest.mark.parametrize("w", [512, 509])
def test_oracle_tonemap_within_the_float64_bound_on_the_edge_frame(oracle, w):
    """Bin boundaries k + j/Q and fp32 ulps around them, the range ends and beyond, every half code in each channel,
    negative channels, OETF thresholds and the white point: histogram envelope, exposure bounds, LDR bytes."""
    p = vr.default_tonemap_params()
    frame = f64_tonemap.as_frame(f64_tonemap.edge_pixels(p), w)
    r = _oracle_step(oracle, oracle.ToneMapper(), p, frame, 1 / 60, f"oracle edge frame, w {w}", 0.0)
    print(r)
    tm = oracle.ToneMapper(); tm.adapted = 0.18                  # the operator at the adapted value the frame was built for
    ldr = tm.Render(p, frame)
    worst, counts, checked = f64_tonemap.check_ldr(ldr[..., :3].reshape(-1, 3), frame[..., :3].reshape(-1, 3), 0.18, p, "oracle, A = 0.18")
    print(worst, counts)
    assert checked > 0.99 * frame[..., :3].size and counts["rounding"] > 0 and counts["saturated"] > 0 and counts["inf_nan"] > 0


def test_oracle_tonemap_within_the_float64_bound_on_the_golden_frame(oracle):
    p = vr.default_tonemap_params()
    hdr = np.load(os.path.join(GOLD, "frame_256x144.npz"))["hdr"]
    tm = oracle.ToneMapper()
    old = 0.0
    for i in range(3):                                          # the first frame jumps, the next two adapt from it
        r = _oracle_step(oracle, tm, p, hdr, 1 / 60, f"golden frame, step {i}", old)
        old = tm.adapted
        print(r)


@pytest.mark.parametrize("case", [c[0] for c in f64_tonemap.adaptation_cases()])
def test_oracle_tonemap_adaptation_sequences(oracle, case):
    """Each step from the oracle's own previous value; the two rules of the header (old <= 0 jumps, speed <= 0 jumps)."""
    name, kw, steps = next(c for c in f64_tonemap.adaptation_cases() if c[0] == case)
    p = vr.default_tonemap_params(**kw)
    tm = oracle.ToneMapper()
    old = 0.0
    for i, (kind, dt) in enumerate(steps):
        _oracle_step(oracle, tm, p, f64_tonemap.sequence_frame(kind, i), dt, f"{case} step {i}", old)
        if dt == 0.0 and old > 0.0 and (kw.get("eye_adaptation_speed_up", 1.0) > 0.0 and kw.get("eye_adaptation_speed_down", 1.0) > 0.0):
            assert tm.adapted == old, "dt = 0 holds the adapted value"
        old = tm.adapted


def test_oracle_tonemap_does_not_wrap_above_2_26_pixels(oracle):
    """16384 x 4200 (68.8 M pixels): 4100 black rows, 100 rows at 0.3.  Q drops to 32; the black bin holds 32 * 67.2 M
    (64 * 67.2 M wrapped to 4.2 M before, and the window landed in the bright band).  Closed-form model; also a world-2
    share (the whole frame's Q)."""
    w, h, rows = 16384, 4200, 100
    p = vr.default_tonemap_params()
    g = f64_tonemap._to_half(0.3)
    frame = np.zeros((h, w, 4), np.uint16)
    frame[h - rows:, :, :3] = g
    tm = oracle.ToneMapper()
    tm.AddFrameToHistogram(p, frame)
    tm.ComputeExposure(p)
    ps = f64_tonemap.banded(w, h, rows, 0.3)
    hm = f64_tonemap.histogram_model(ps, p)
    assert hm["q"] == 32
    f64_tonemap.check_histogram(tm.hist, hm, "banded 16384x4200")
    f64_tonemap.check_exposure(tm.adapted, tm.hist, hm, p, 0.0, 0.0, "banded 16384x4200")
    assert tm.adapted == pytest.approx(0.02), "the 0.8..0.95 window lies in the black rows: minimum adapted luminance"
    ldr = tm.Render(p, frame[h - rows - 2:h - rows + 2])
    f64_tonemap.check_ldr(ldr[..., :3].reshape(-1, 3), frame[h - rows - 2:h - rows + 2, :, :3].reshape(-1, 3), tm.adapted, p, "banded LDR")
    part = vr.Partition(1, 2)
    tm2 = oracle.ToneMapper()
    tm2.AddFrameToHistogram(p, frame, part)
    share = f64_tonemap.banded_share(w, h, rows, 0.3, 1, 2)
    f64_tonemap.check_histogram(tm2.hist, f64_tonemap.histogram_model(share, p, frame_pixels=w * h), "banded, rank 1 of 2")


@pytest.mark.parametrize("how", ["reset_exposure", "min_adapted"])
def test_oracle_tonemap_extreme_exposure_saturates(oracle, how):
    """adapted = 1e-30: the fused mapped / src overflows (inf / inf); bright pixels must come out 255, not black."""
    vals = [60000.0, 1.0, 1e-4, 0.0]
    codes = [[f64_tonemap._to_half(v)] * 3 for v in vals] + [[f64_tonemap._to_half(0.5), 0, 0], [0, f64_tonemap._to_half(65504.0), 0]]
    frame = f64_tonemap.as_frame(np.array(codes, np.uint16), len(codes))
    p = vr.default_tonemap_params(**({"min_adapted_luminance": 1e-30, "max_adapted_luminance": 1e-30} if how == "min_adapted" else {}))
    tm = oracle.ToneMapper()
    if how == "reset_exposure":
        tm.adapted = 1e-30
    else:
        tm.ComputeExposure(p)                                     # empty histogram: min_log -> clamp to [1e-30, 1e-30]
        assert np.float32(tm.adapted) == np.float32(1e-30)
    ldr = tm.Render(p, frame)[0, :, :3]
    f64_tonemap.check_ldr(ldr, frame[0, :, :3], tm.adapted, p, f"extreme exposure ({how})")
    assert ldr[:3].tolist() == [[255] * 3] * 3 and ldr[3].tolist() == [0, 0, 0]
    assert ldr[4].tolist() == [255, 0, 0] and ldr[5].tolist() == [0, 255, 0]


def test_tonemap_model_constants():
    """The derived constants of tests/f64_tonemap.py: position delta over every fp32 luminance of the range, the exp2
    cubic's error, the weight quantum."""
    d = f64_tonemap.position_delta(-10.0, 4.0)
    assert 0.005 < d < 0.03, d                                   # 1/64 of a bin is 0.0156: the split's resolution
    assert 1e-5 < f64_tonemap.exp2_error() < 2e-4
    assert f64_tonemap.quantum(2 ** 26 - 1) == 64 and f64_tonemap.quantum(2 ** 26) == 32
    assert f64_tonemap.quantum(16384 * 4200) == 32 and f64_tonemap.quantum(2 ** 32 - 1) == 1 and f64_tonemap.quantum(2 ** 32) == 0
