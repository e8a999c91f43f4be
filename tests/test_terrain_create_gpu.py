"""GPU tests of vr_terrain_create on the smallest maps at which covering a WHOLE level can go wrong.  Creating a terrain derives
everything - mip chains, decoded tables, node heights, the query pyramid - through the kernels of an in-place edit, with the
rectangle of the whole map (vrenderer_amd/csrc/vr_derive.hip); tests/host/dirty_check.cpp shows that this rectangle is all of
every structure, these tests that the device then holds what the models say, out to the rim of every table.

Maps (tests/frontend_common.py: CREATE_SHAPES, random bytes, on a world of 64): 1 x 1, the smallest pair create accepts; 5 x 5,
odd with every level ragged; 7 x 2 and 2 x 7, where one side reaches one texel levels before the other; 33 x 17.  Each is the
heightmap of one case and the albedo of the case before, so every case pairs two shapes (the general raster variant: quadf and
rgbf); a second terrain with an albedo of the heightmap's own shape takes the fast variant (fast).  create refuses none of them.

Every bound is one the project already has: the mip model of test_mip_chains_follow_the_box_filter, the exact min / max of
tests/f64_frontend.py, Surface64's height_tol / ray_tol, and bit-exact G-buffer planes against the oracle."""
import numpy as np
import pytest

import vrenderer_amd as vr
from tests import f64_frontend as fe
from tests import frontend_common as fc
from tests import queries_common as qc
from tests.common import CAMERAS, params, scaled_camera
from tests.f64_queries import Surface64

pytestmark = pytest.mark.gpu

WORLD = fc.CREATE_WORLD
MH = qc.scaled_max_height(WORLD)
PLANES = ("depth", "diffuse", "specular", "normals", "emissive")
FRAME_W, FRAME_H = 64, 36
CASES = [f"{w}x{h}" for w, h in fc.CREATE_SHAPES]


@pytest.fixture(scope="module")
def maps():
    return [fc.random_texture(w, h, fc.CREATE_SEED) for w, h in fc.CREATE_SHAPES]


@pytest.fixture(scope="module")
def terrains(gpu_ctx, maps):
    """Case k: heightmap k with the albedo of shape k + 1, created once and shared."""
    made = {}

    def get(case):
        k = CASES.index(case)
        if k not in made:
            hm, al = maps[k][0], maps[(k + 1) % len(maps)][1]
            made[k] = dict(hm=hm, al=al, tp=vr.TerrainPass(gpu_ctx, params(WORLD)).Init(hm, al))
        return made[k]
    yield get
    for sc in made.values():
        sc["tp"].close()


@pytest.mark.parametrize("case", CASES)
def test_both_chains_are_the_box_filter_byte_for_byte(case, terrains):
    """Every level of both chains equals the model of the level below; nothing is flagged on these maps
    (tests/test_frontend_cpu.py), so equal means every byte."""
    sc, rows = terrains(case), []
    assert np.array_equal(sc["tp"].download_mip("height", 0), sc["hm"]) and np.array_equal(sc["tp"].download_mip("albedo", 0), sc["al"])
    fc.check_chain(sc["tp"], case, rows, flag_cap=0.0)
    fc.report(f"mip chains of a created terrain, {case}", rows)


@pytest.mark.parametrize("case", CASES)
def test_node_heights_are_the_exact_min_max(case, terrains):
    sc = terrains(case)
    tp, tree = sc["tp"], fe.Tree(WORLD, WORLD)
    model = fe.set_height(tree, sc["hm"])
    assert tp.GetNumLods() == tree.num_lods and not model.flagged.any()
    tp.SetHeight(True)
    try:
        r = fe.check_node_heights(model, tp.node_heights(0, tree.num_nodes))
    finally:
        tp.SetHeight(False)
    fc.report(f"SetHeight of a created terrain, {case}", [("worst |error| / bound", f"{r['worst']:.3f}")])
    assert r["bad"] == 0, f"{r['bad']} nodes outside the bound, first ids {r['first']}; worst ratio {r['worst']:.2f}"


@pytest.mark.parametrize("case", CASES)
def test_heights_and_rays_read_the_rim(case, terrains):
    """Heights at every texel centre and every texel boundary of level 0, the four borders of the world included, and a step
    outside them (clamp addressing): the quad table out to its clamped rim.  128 rays of tests/queries_common.py: the pyramid
    at every ragged level."""
    sc = terrains(case)
    tp = sc["tp"]
    l0 = tp.download_mip("height", 0)
    surf = Surface64(l0, tp.download_mip("height", 1) if tp.mip_levels("height") > 1 else l0, WORLD, MH)
    h, w = sc["hm"].shape
    xs = np.concatenate([[-0.5 - 1.0 / w], np.arange(2 * w + 1) / (2.0 * w) - 0.5, [0.5 + 1.0 / w]]) * WORLD
    zs = np.concatenate([[-0.5 - 1.0 / h], np.arange(2 * h + 1) / (2.0 * h) - 0.5, [0.5 + 1.0 / h]]) * WORLD
    pts = np.stack(np.meshgrid(xs, zs), -1).reshape(-1, 2).astype(np.float32)
    got = tp.SampleHeights(pts, MH)
    x, z = pts[:, 0].astype(np.float64), pts[:, 1].astype(np.float64)
    ratio = np.abs(got - surf.H(x, z)) / surf.height_tol(x, z)
    o, d, tm = qc.make_rays(surf, WORLD, 128)
    worst = qc.check_ray_hits(surf, o, d, tm, tp.CastRays(o, d, tm, MH), label=case)
    print(f"\n{case}: {len(pts)} heights, worst |h - H64| / tol = {ratio.max():.4f}; rays: worst ratios {worst}")
    assert (ratio <= 1.0).all(), (case, ratio.max(), pts[ratio.argmax()].tolist())


def _frame(gpu_ctx, oracle, hm, al, cam, what):
    eye, tgt = scaled_camera(CAMERAS[cam], WORLD)
    v = vr.make_view(eye, tgt, FRAME_W, FRAME_H)
    rp = vr.default_render_params(MH)
    ot = oracle.OracleTerrain(params(WORLD), hm, al)
    tp = vr.TerrainPass(gpu_ctx, params(WORLD)).Init(hm, al)
    rt = vr.RenderTargets(gpu_ctx).Init(FRAME_W, FRAME_H)
    try:
        gb = oracle.GBufferHost(FRAME_W, FRAME_H)
        n_o = ot.render(v, gb, rp)
        rt.Clear()
        tp.Render(v, v, rt, rp)
        assert tp.num_chunks() == n_o and n_o > 0, what
        covered = int((gb.depth < 1.0).sum())
        assert covered > FRAME_W * FRAME_H // 8, (what, covered)          # the terrain is in the picture
        for name in PLANES:
            got, ref = rt.download(name), getattr(gb, name)
            if name == "depth":
                got, ref = got.view(np.uint32), ref.view(np.uint32)
            mis = np.argwhere(got != ref)
            assert mis.size == 0, f"{what}: {name} differs at {len(mis)} entries, first {mis[:5].tolist()}"
    finally:
        rt.close(); tp.close(); ot.close()


@pytest.mark.parametrize("case", CASES)
def test_a_frame_matches_the_oracle_bit_for_bit(case, maps, gpu_ctx, oracle):
    """A 64 x 36 frame from across the world (its far rim in view), every G-buffer plane bit for bit as the parity tests ask:
    with the other shape's albedo (the general variant reads quadf and rgbf) and with an albedo of the heightmap's own shape
    (the fast variant reads fast)."""
    k = CASES.index(case)
    _frame(gpu_ctx, oracle, maps[k][0], maps[(k + 1) % len(maps)][1], 1, f"{case}, general variant")
    _frame(gpu_ctx, oracle, maps[k][0], maps[k][1], 7, f"{case}, fast variant")
