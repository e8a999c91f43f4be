"""The HIP front end - k_derive_mip_*, k_node_heights_* / k_derive_minmax_*, k_select, k_vertex - against the model of
tests/f64_frontend.py directly, not through the oracle.  tests/test_frontend_cpu.py checks the conditions this file relies
on (flagged shares, unambiguous views, real ties, vertex classes).  Every test prints its worst |error| / bound (-rA)."""
import numpy as np
import pytest

import vrenderer_amd as vr
from tests import f64_frontend as fe
from tests import frontend_common as fc
from tests.common import params
from tests.f64_queries import Surface64

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def worlds(gpu_ctx):
    """Device terrains by world size, built from the device's own synthetic textures: 256, 2048 (one surface), 512 (two surfaces
    of 256 per side, the world of test_multi_surface_world)."""
    made = {}

    def get(world):
        if world not in made:
            h = vr.synth_heightmap(gpu_ctx, world)
            a = vr.synth_albedo(gpu_ctx, world, h)
            p = params(world) if world != 512 else fc.world_params(256, 512)
            made[world] = dict(tp=vr.TerrainPass(gpu_ctx, p).Init(h, a), tree=fe.Tree(256 if world == 512 else world, world), h=h, a=a,
                               heights=None)
        return made[world]
    yield get
    for sc in made.values():
        sc["tp"].close()


def _heights(sc):
    if sc["heights"] is None:
        sc["heights"] = fe.set_height(sc["tree"], sc["h"])
    return sc["heights"]


def test_mip_chains_follow_the_box_filter(gpu_ctx, worlds):
    """The synthetic 256^2 pair, random bytes with random alpha at 129 x 129 and 67 x 41 (odd sizes: clamped last row and
    column, sides that reach one texel before the other), the strips 64 x 1 and 1 x 37, and 256 x 64 - all sizes
    vr_terrain_create accepts as they are.  R8 and alpha are exact; sRGB equal outside the flagged components."""
    rows = []
    sc = worlds(256)
    assert np.array_equal(sc["tp"].download_mip("height", 0), sc["h"]) and np.array_equal(sc["tp"].download_mip("albedo", 0), sc["a"])
    fc.check_chain(sc["tp"], "synthetic 256", rows)
    for name, w, h, seed in fc.MIP_TEXTURES:
        hm, al = fc.random_texture(w, h, seed)
        tp = vr.TerrainPass(gpu_ctx, params(256)).Init(hm, al)
        try:
            assert np.array_equal(tp.download_mip("albedo", 0), al)
            fc.check_chain(tp, name, rows)
        finally:
            tp.close()
    fc.report("mip chains, device vs model", rows)


@pytest.mark.parametrize("name", ["256", "two surfaces", "ragged 200x200 on 256", "420x300 on 200", "2048"])
def test_set_height_is_the_exact_min_max(name, gpu_ctx, worlds):
    """All nodes through node_heights(0, num_nodes).  The 256, two-surface and 2048 worlds sample one texel per world unit and take
    the k_derive_minmax_leaf / k_derive_minmax_up pyramid (2048: twelve levels of it); the ragged maps take the per-node scan:
    k_node_heights_block while a node covers 512 texels or more (depths 0-3 of the 200 x 200 map), k_node_heights_thread
    below.  No node of the dyadic worlds is flagged, at most 1 % of the ragged one; the 420 x 300 map on the 200 world
    exercises the flagged branch (tests/test_frontend_cpu.py says why up to 10 %)."""
    if name in ("256", "two surfaces", "2048"):
        sc = worlds({"256": 256, "two surfaces": 512, "2048": 2048}[name])
        tp, tree, model, cap, own = sc["tp"], sc["tree"], _heights(sc), 0.0, False
    else:
        surface, world, hm, cap = (256, 256, fc.ragged_heightmap(), 0.01) if name.startswith("ragged") else (200, 200, fc.world200_heightmap(), 0.10)
        tp = vr.TerrainPass(gpu_ctx, fc.world_params(surface, world)).Init(hm, np.zeros((4, 4, 4), np.uint8))
        tree, own = fe.Tree(surface, world), True
        model = fe.set_height(tree, hm)
    try:
        assert tp.GetNumLods() == tree.num_lods
        tp.SetHeight(True)
        r = fe.check_node_heights(model, tp.node_heights(0, tree.num_nodes))
        fc.report(f"SetHeight, {name}, device vs model", [("worst |error| / bound", f"{r['worst']:.3f}"), ("flagged share", f"{r['flagged']:.4f}")])
        assert r["bad"] == 0, f"{r['bad']} nodes outside the bound, first ids {r['first']}; worst ratio {r['worst']:.2f}"
        assert r["flagged"] <= cap, r["flagged"]
    finally:
        tp.SetHeight(False)
        if own:
            tp.close()


@pytest.mark.parametrize("loaded", [False, True])
def test_select_is_the_exact_recursion(loaded, gpu_ctx, worlds):
    """Ids, count and instance fields equal the model's, in both modes of m_HeightLoaded: the eight cameras on the 256 world
    (three of them moved where the model alone finds them ambiguous, tests/frontend_common.py), two on the 2048 world, a
    camera far outside and one below the world, one on a node boundary, the two `<=` ties on the squared range, and the
    orthographic light view of SetupForPlanarViewStable, whose six planes are a box."""
    rows = []
    for world, views in ((256, fc.SELECT_VIEWS_256[loaded]), (2048, fc.SELECT_VIEWS_2048)):
        sc = worlds(world)
        tp = sc["tp"]
        assert np.array_equal(tp.GetLodRanges(), np.array(fe.lod_ranges(), np.float32))
        tp.SetHeight(loaded)
        try:
            cases = [(name, fc.make_view(*cam)) for name, cam in views]
            if world == 256:
                sm = vr.CascadedShadowMap(gpu_ctx, vr.default_shadow_params(256.0, resolution=512))
                cases.append(("light view", fc.light_view_of(lambda light, cam, p: sm.SetupForPlanarViewStable(light, cam), 256)))
            for name, view in cases:
                model = fe.node_select(sc["tree"], view, fc.MAX_HEIGHT, _heights(sc) if loaded else None)
                n, ids, inst = tp.NodeSelect(view, fc.MAX_HEIGHT)
                diff = fe.check_selection(model, n, ids, inst)
                assert diff is None, f"{world} {name}: {diff}"
                rows.append((f"{world} {name}", f"{n} nodes equal; ties {model.ties}"))
            if world == 256:
                sm.close()
        finally:
            tp.SetHeight(False)
    fc.report(f"NodeSelect, heights loaded = {loaded}, device vs model", rows)


@pytest.mark.parametrize("case", fc.VERTEX_CASES)
def test_vertex_stage_is_within_the_model_s_bounds(case, gpu_ctx, worlds):
    """All 1,089 vertices of the five instances test_vertex_stage_bit_exact picks (nearest, morph band, coarsest, first, last),
    through download_vertices: world xz and the clip position within the model's bound for that vertex.  The device keeps no
    height of its own; a height outside its bound moves the clip position outside its own, which is the height's bound
    through the two matrices plus their rounding.  The light view is the orthographic case: w = 1, camera position far
    away."""
    world, view = None, None
    sm = vr.CascadedShadowMap(gpu_ctx, vr.default_shadow_params(256.0, resolution=512))
    try:
        world, view = fc.vertex_case_view(case, lambda light, cam, p: sm.SetupForPlanarViewStable(light, cam))
        sc = worlds(world)
        tp = sc["tp"]
        surf = Surface64(tp.download_mip("height", 0), tp.download_mip("height", 1), world, fc.MAX_HEIGHT)
        n, ids, inst = tp.NodeSelect(view, fc.MAX_HEIGHT)
        if case == "256 light view":
            sm.Clear()
            sm.RenderTerrain(tp, fc.MAX_HEIGHT)
        else:
            rt = vr.RenderTargets(gpu_ctx).Init(view.viewport_w, view.viewport_h)
            tp.Render(view, view, rt, vr.default_render_params(fc.MAX_HEIGHT))
        assert tp.num_chunks() == n and n > 0
        fields, _ = fe.instance_fields(inst)
        eye = [float(view.camera_pos[k]) for k in range(3)]
        worst, models = dict(xz=0.0, clip=0.0), []
        for i in fc.chosen_instances(fields, eye, fe.lod_ranges()):
            m = fe.main_vs(fields[i], view, surf)
            models.append(m)
            got = tp.download_vertices(i, 1)[0].astype(np.float64)
            r = fe.check_vertices(m, got[:, :4], got[:, 4:6])
            for key in worst:
                worst[key] = max(worst[key], r[key])
            assert max(r.values()) <= 1.0, f"{case}, instance {i} (node {ids[i]}): worst |error| / bound {r}"
        fc.report(f"main_vs, {case}, device vs model", [("worst |error| / bound", ", ".join(f"{k} {v:.3f}" for k, v in worst.items())),
                                                         ("vertex classes", fc.morph_classes(models))])
        if case == "256 light view":
            assert (np.abs(models[-1]["clip"][:, 3] - 1.0) < 1e-6).all()
        else:
            rt.close()
    finally:
        sm.close()
