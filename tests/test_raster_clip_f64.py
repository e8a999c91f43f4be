"""The HIP tile pass's downloaded G-buffer planes on clipped and edge views, held to tests/f64_model.py directly - not
through the oracle, which supplies only what the model takes as given: the selection, the vertex stage and the LOD to
sample at (views and comparison: tests/raster_clip_common.py)."""
import numpy as np
import pytest

import vrenderer_amd as vr
from tests import raster_clip_common as RC
from tests.common import params

pytestmark = pytest.mark.gpu

_frames = {}


@pytest.fixture(scope="module")
def scene(oracle, gpu_ctx):
    h = oracle.synth_heightmap(RC.SIZE)
    a = oracle.synth_albedo(RC.SIZE, h)
    ot = oracle.OracleTerrain(params(RC.SIZE), h, a)
    tp = vr.TerrainPass(gpu_ctx, params(RC.SIZE)).Init(h, a)
    yield dict(ot=ot, tp=tp)
    tp.close()
    ot.close()
    _frames.clear()


def _model(oracle, scene, name):
    """The model's frame of a view, computed once and shared by the tile sizes."""
    if name not in _frames:
        spec = RC.VIEWS[name]
        w, h = spec["w"], spec["h"]
        v = RC.make_view(spec)
        gb = oracle.GBufferHost(w, h)
        dbg = np.zeros((h, w, 3), np.float32)
        part = vr.Partition(*spec["part"]) if "part" in spec else None
        scene["ot"].render(v, gb, vr.default_render_params(400.0), part, debug_plane=dbg)
        _frames[name] = (v, RC.model_frame(scene["ot"], spec, v, dbg[..., 0]))
    return _frames[name]


@pytest.mark.parametrize("name,edge", [(n, 0) for n in RC.VIEWS] + [("near-45", 32), ("near-45", 64), ("guard-band", 32), ("guard-band", 64)])
def test_tile_pass_pixels_of_clipped_and_edge_views_are_bounded_by_the_exact_model(oracle, scene, gpu_ctx, name, edge):
    """TerrainPass.Render's planes: coverage by class, depth within the bound derived per parent triangle, albedo and
    normal codes, the other planes exact; on the frame's own raster tile size and, for two views, on 32- and 64-pixel tiles."""
    spec = RC.VIEWS[name]
    w, h = spec["w"], spec["h"]
    v, fr = _model(oracle, scene, name)
    part = vr.Partition(*spec["part"]) if "part" in spec else None
    rt = vr.RenderTargets(gpu_ctx).Init(w, h)
    try:
        gpu_ctx.set_raster_tile(edge)
        scene["tp"].Render(v, v, rt, vr.default_render_params(400.0), part)
        st = scene["tp"].render_stats()
        planes = {k: rt.download(k) for k in ("depth", "diffuse", "specular", "normals", "emissive")}
    finally:
        gpu_ctx.set_raster_tile(0)
        rt.close()
    print(f"{name}, tile {edge}: device {st}")
    assert st["clipped_tris"] > 0 and st["flags"] == 0, st
    # the clipper's structure against the model's exact polygons: which triangles it takes, how many vertices and fan triangles it makes
    tc = fr.tri_count
    assert (st["clipped_tris"], st["clip_verts"], st["clip_subtris"]) == (tc["clipped"], tc["poly_verts"], tc["poly_subtris"]), (st, tc)
    RC.check_planes(f"{name}, tile {edge}", spec, fr, planes, int(oracle.lib().orc_linear_to_srgb8(np.float32(0.01))))
