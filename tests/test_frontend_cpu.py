"""The C oracle's front end - mip chains, SetHeight, NodeSelect, the vertex stage - against the model of
tests/f64_frontend.py, which is written from the reference's text alone, and the conditions tests/test_frontend_f64.py relies
on, checked here for the model by itself: flagged shares under their caps, no ambiguous view, real ties, all morph classes
and border samples among the chosen instances."""
import numpy as np
import pytest

from tests import f64_frontend as fe
from tests import frontend_common as fc
from tests.common import params
from tests.f64_queries import Surface64


@pytest.fixture(scope="module")
def worlds(oracle, product_lib):
    """Oracle terrains by world size: 256 and 2048 (one surface), 512 (two surfaces of 256 per side)."""
    made = {}

    def get(world):
        if world not in made:
            h = oracle.synth_heightmap(world)
            p = params(world) if world != 512 else fc.world_params(256, 512)
            tree = fe.Tree(256 if world == 512 else world, world)
            made[world] = dict(ot=oracle.OracleTerrain(p, h, oracle.synth_albedo(world, h)), tree=tree, h=h, heights=None)
        return made[world]
    yield get
    for sc in made.values():
        sc["ot"].close()


def _heights(sc):
    if sc["heights"] is None:
        sc["heights"] = fe.set_height(sc["tree"], sc["h"])
    return sc["heights"]


def test_mip_chains_of_the_oracle_follow_the_box_filter(oracle, worlds):
    """Every level of every texture the GPU test uses is the model's of the level below: R8 and alpha equal, sRGB equal
    outside the flagged texels, whose share stays at or below 0.5 % on every level."""
    sc = worlds(256)
    textures = [("synthetic 256", sc["h"], oracle.synth_albedo(256, sc["h"]))] + [(n,) + fc.random_texture(w, h, s) for n, w, h, s in fc.MIP_TEXTURES]
    rows = []
    for name, hm, al in textures:
        ot = oracle.OracleTerrain(params(256), hm, al)
        assert ot.height_levels() == fe.num_mip_levels(hm.shape[1], hm.shape[0]) == ot.albedo_levels(), name
        flagged = 0.0
        for l in range(1, ot.height_levels()):
            r = fe.check_mip(ot.height_mip(l - 1), ot.height_mip(l), srgb=False)
            assert r["bad"] == 0, f"{name}: height level {l}: {r['bad']} texels differ from the model"
            r = fe.check_mip(ot.albedo_mip(l - 1), ot.albedo_mip(l), srgb=True)
            assert r["bad"] == 0, f"{name}: albedo level {l}: {r['bad']} components differ from the model"
            assert r["flagged"] <= fc.MIP_FLAG_CAP, f"{name}: albedo level {l}: {r['flagged']:.4f} of the components are flagged"
            flagged = max(flagged, r["flagged"])
        rows.append((name, f"levels {ot.height_levels()}, largest flagged share {flagged:.5f}"))
        ot.close()
    fc.report("mip chains, oracle vs model", rows)


def test_create_shapes_leave_nothing_open_to_the_model(oracle):
    """What tests/test_terrain_create_gpu.py relies on: no colour component of any level of its maps is flagged, so "equal to
    the model" is byte for byte there (and the oracle's chains are); on the 64 world their texel sizes w / 64 are dyadic, every
    footprint bound is an exact fp32 product and no node is flagged either."""
    maps = [fc.random_texture(w, h, fc.CREATE_SEED) for w, h in fc.CREATE_SHAPES]
    for k, (hm, _) in enumerate(maps):
        al = maps[(k + 1) % len(maps)][1]
        ot = oracle.OracleTerrain(params(fc.CREATE_WORLD), hm, al)
        try:
            for l in range(1, ot.height_levels()):
                assert fe.check_mip(ot.height_mip(l - 1), ot.height_mip(l), srgb=False)["bad"] == 0, (hm.shape, l)
            for l in range(1, ot.albedo_levels()):
                r = fe.check_mip(ot.albedo_mip(l - 1), ot.albedo_mip(l), srgb=True)
                assert r["bad"] == 0 and r["flagged"] == 0.0, (al.shape, l, r)
        finally:
            ot.close()
        assert not fe.set_height(fe.Tree(fc.CREATE_WORLD, fc.CREATE_WORLD), hm).flagged.any(), hm.shape


def test_mip_model_known_answers():
    """The model itself: round-half-up, the clamp at odd sizes, a strip, and sRGB averaging in linear light."""
    assert fe.mip_r8(np.array([[1, 2, 9], [2, 1, 9], [7, 7, 3]], np.uint8)).tolist() == [[2]]                 # 6 / 4 = 1.5 -> 2; 3 x 3 -> 1 x 1
    assert fe.mip_r8(np.array([[0, 1, 2, 3, 250]], np.uint8)).tolist() == [[1, 3]]                            # a strip: rows clamp
    assert fe.mip_r8(np.array([[255, 254], [254, 254]], np.uint8)).tolist() == [[254]]                        # 1017 / 4 = 254.25
    px = np.zeros((2, 2, 4), np.uint8); px[0, 0] = (255, 255, 255, 255)
    lo, hi = fe.mip_srgb(px)
    assert lo.tolist() == hi.tolist() == [[[137, 137, 137]]]                                                  # OETF(1/4) 255 = 136.98, not 64
    assert fe.mip_r8(px[..., 3]).tolist() == [[64]]


@pytest.mark.parametrize("name", ["256", "two surfaces", "ragged 200x200 on 256", "420x300 on 200", "2048"])
def test_set_height_of_the_oracle_is_the_exact_min_max(name, oracle, worlds):
    """Every node's (position.y, extents.y) within the derived fp32 bound of the exact rationals; no node flagged on the dyadic
    scenes, at most 1 % on the ragged one.  The 420 x 300 map on the 200 world is there for the flagged branch: its texel
    size 2.1 is no fp32 number while 105 k / 32 is an integer for every 32nd node edge, so about a twelfth of the nodes may
    take either footprint - at least one and at most 10 % are, and each of them must match one of the footprints."""
    if name in ("256", "two surfaces", "2048"):
        sc = worlds({"256": 256, "two surfaces": 512, "2048": 2048}[name])
        ot, tree, model, cap = sc["ot"], sc["tree"], _heights(sc), 0.0
    else:
        surface, world, hm, cap = (256, 256, fc.ragged_heightmap(), 0.01) if name.startswith("ragged") else (200, 200, fc.world200_heightmap(), 0.10)
        ot = oracle.OracleTerrain(fc.world_params(surface, world), hm, np.zeros((4, 4, 4), np.uint8))
        tree = fe.Tree(surface, world)
        model = fe.set_height(tree, hm)
    try:
        assert tree.num_nodes == ot.num_nodes and tree.num_lods == ot.num_lods
        ot.set_height(True)
        r = fe.check_node_heights(model, ot.node_heights())
        fc.report(f"SetHeight, {name}", [("worst |error| / bound", f"{r['worst']:.3f}"), ("flagged share", f"{r['flagged']:.4f}")])
        assert r["bad"] == 0, f"{r['bad']} nodes outside the bound, first ids {r['first']}; worst ratio {r['worst']:.2f}"
        assert r["flagged"] <= cap, r["flagged"]
        if name.startswith("420"):
            assert model.flagged.any()
        if name.startswith("ragged"):
            assert (model.mn == model.mx).sum() > 100 and (model.pos[model.mn == model.mx] > 0).any(), "no flat node takes the min = 0 branch"
    finally:
        ot.set_height(False)
        if name not in ("256", "two surfaces", "2048"):
            ot.close()


def _select_case(sc, view, loaded, oracle_terrain):
    model = fe.node_select(sc["tree"], view, fc.MAX_HEIGHT, _heights(sc) if loaded else None)
    n, ids, inst = oracle_terrain.select(view, fc.MAX_HEIGHT)
    return model, fe.check_selection(model, n, ids, inst)


@pytest.mark.parametrize("loaded", [False, True])
def test_select_of_the_oracle_is_the_exact_recursion(loaded, oracle, worlds):
    """Ids, count and instance fields equal the model's for every view of the list, in both modes of m_HeightLoaded; every view
    is unambiguous under the model alone; the tie views really hold zero-margin decisions of both kinds, and comparing with
    `<` in either use alone changes what the model selects for one of them."""
    rows = []
    for world, views in ((256, fc.SELECT_VIEWS_256[loaded]), (2048, fc.SELECT_VIEWS_2048)):
        sc = worlds(world)
        sc["ot"].set_height(loaded)
        try:
            cases = [(name, fc.make_view(*cam)) for name, cam in views]
            if world == 256:
                cases.append(("light view", fc.light_view_of(oracle.shadow_view, 256)))
            told_apart = set()
            for name, view in cases:
                model, diff = _select_case(sc, view, loaded, sc["ot"])
                assert model.ambiguous == 0, f"{world} {name}: {model.ambiguous} decisions within tau - replace the view"
                assert diff is None, f"{world} {name}: {diff}"
                rows.append((f"{world} {name}", f"{model.count} nodes, {model.decisions} decisions, ties {model.ties}"))
                if name in fc.TIE_VIEWS:
                    assert model.ties["range_first"] > 0 and model.ties["range_finer"] > 0, (name, model.ties)
                    for use in ("range_first", "range_finer"):
                        other = fe.node_select(sc["tree"], view, fc.MAX_HEIGHT, _heights(sc) if loaded else None, strict=(use,))
                        if not np.array_equal(other.ids, model.ids):
                            told_apart.add(use)
                if name == "far outside":
                    assert model.count == 0
                if name == "light view":
                    assert view.view_to_clip[15] == 1.0 and model.count > 0            # orthographic: w = 1
            if world == 256:
                assert told_apart == {"range_first", "range_finer"}, told_apart
        finally:
            sc["ot"].set_height(False)
    fc.report(f"NodeSelect, heights loaded = {loaded}", rows)


def test_vertex_stage_of_the_oracle_is_within_the_model_s_bounds(oracle, worlds):
    """World xz, height and clip position of all 1,089 vertices of the five chosen instances of every case within the bound the
    model derives for that vertex; the chosen instances hold partially morphed, fully morphed and unmorphed vertices and
    vertices that sample the clamp border at uv = 0 and at uv = 1."""
    models, rows = [], []
    for case in fc.VERTEX_CASES:
        world, view = fc.vertex_case_view(case, oracle.shadow_view)
        sc = worlds(world)
        ot = sc["ot"]
        surf = Surface64(ot.height_mip(0), ot.height_mip(1), world, fc.MAX_HEIGHT)
        n, ids, inst = ot.select(view, fc.MAX_HEIGHT)
        fields, _ = fe.instance_fields(inst)
        eye = [float(view.camera_pos[k]) for k in range(3)]
        worst = dict(xz=0.0, clip=0.0, h=0.0)
        for i in fc.chosen_instances(fields, eye, fe.lod_ranges()):
            m = fe.main_vs(fields[i], view, surf)
            models.append(m)
            got = np.array([np.concatenate(ot.vertex(view, fc.MAX_HEIGHT, inst[i], k % 33, k // 33)) for k in range(1089)], np.float64)
            r = fe.check_vertices(m, got[:, :4], got[:, [4, 6]], got[:, 5])
            for key in worst:
                worst[key] = max(worst[key], r[key])
            assert max(r.values()) <= 1.0, f"{case}, instance {i} (node {ids[i]}): worst |error| / bound {r}"
        rows.append((case, ", ".join(f"{k} {v:.3f}" for k, v in worst.items())))
        if case == "256 light view":
            assert (np.abs(models[-1]["clip"][:, 3] - 1.0) < 1e-6).all()
    classes = fc.morph_classes(models)
    fc.report("main_vs, oracle vs model: worst |error| / bound", rows + [("vertex classes", classes)])
    assert min(classes.values()) > 0, classes
