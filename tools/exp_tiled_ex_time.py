"""Scratch (GPU box): k_light_cull and k_deferred_tiled at 7680x4320 with the seed-9001 1024-light set, through the context's
kernel timing, over 8 flythrough frames (2 warm-up + REPS timed calls each; per case the median frame and the min..max spread):
  old      vr_deferred_light_tiled                                   (VARIANT=<name>: the same on another build of the library,
                                                                      vrenderer_amd/lib/variants/<name>/libvrterrain.so, e.g. the parent's)
  ex       vr_deferred_light_tiled_ex, same list (runs the plain kernels)
  shadow   the same list with the sun's shadow binding (2048^2 map)
  spots    every fourth light turned into a 25-degree spot, no binding
"""
import os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vrenderer_amd import capi
variant = os.environ.get("VARIANT")
if variant:
    capi.LIB_PATH = os.path.join(ROOT, "vrenderer_amd", "lib", "variants", variant, "libvrterrain.so")
    capi.EXPORTS = [e for e in capi.EXPORTS if e not in ("vr_deferred_light_tiled_ex", "vr_debug_tile_light_list")]
import torch  # noqa: F401
import vrenderer_amd as vr
from vrenderer_amd.scene import params, AMBIENT_TOP, AMBIENT_BOTTOM, flythrough_camera
size, w, h = 2048, int(os.environ.get("W", 7680)), int(os.environ.get("H", 4320))
reps = int(os.environ.get("REPS", 5))
ctx = vr.Context(0)
hm = vr.synth_heightmap(ctx, size); al = vr.synth_albedo(ctx, size, hm)
tp = vr.TerrainPass(ctx, params(size)).Init(hm, al)
rt = vr.RenderTargets(ctx).Init(w, h)
hdr = vr.HdrImage(ctx, w, h)
lights = [vr.reference_sun()] + vr.synthetic_point_lights(1023, 2048.0, hm, 400.0, seed=9001)
spots = list(lights)
for i in range(4, 1024, 4):
    l = lights[i]
    spots[i] = vr.spot_light(l.position[:], (0.2, -1.0, 0.1), l.intensity, 1.0 / l.angular_size_or_inv_range, 12.0, 25.0, l.color[:])
tl = vr.TiledDeferredLightingPass(ctx)
sm = vr.CascadedShadowMap(ctx, vr.default_shadow_params(2048.0))
cases = [("old", lights, {})]
if not variant:
    cases += [("ex", lights, dict(all_light_types=True)), ("shadow", lights, dict(shadow_map=sm)), ("spots", spots, dict(all_light_types=True))]
res = {name: {"k_light_cull": [], "k_deferred_tiled": []} for name, _, _ in cases}
for f in range(0, 120, 15):
    v = vr.make_view(*flythrough_camera(f), w, h)
    sm.SetupForPlanarViewStable(lights[0], v); sm.Clear(); sm.RenderTerrain(tp)
    rt.Clear(); tp.Render(v, v, rt, vr.default_render_params(400.0))
    for name, ls, kw in cases:
        arr = vr.passes.light_array(ls)
        for _ in range(2): tl.Render(v, rt, arr, AMBIENT_TOP, AMBIENT_BOTTOM, hdr, None, len(ls), **kw)
        ctx.synchronize()
        ctx.timing_enable(True)
        for _ in range(reps): tl.Render(v, rt, arr, AMBIENT_TOP, AMBIENT_BOTTOM, hdr, None, len(ls), **kw)
        ctx.synchronize()
        t = ctx.timing_collect(); ctx.timing_enable(False)
        for k, (ms, n) in t.items():
            if k in res[name]: res[name][k].append(ms / n * 1e3)
tl.Status()
for name, ks in res.items():
    print(variant or "this build", name, "  ".join("%s median %.1f us (frames %.1f..%.1f)" % (k, statistics.median(v), min(v), max(v)) for k, v in ks.items() if v), flush=True)
