"""Terrain-query rates on the 2048^2 synthetic map: 2^20 height queries and 2^20 rays (the pixel rays of the default camera's
1024 x 1024 view, and as many uniformly random rays), device-pointer mode, HIP-event timing through vr_timing_*, warm, median
of 20.  The same rays are then cast by a variant build whose walk is pinned to level 0 of the bound pyramid
(tools/build_variant.py query_level0 vr_query.hip=-DVR_EXP_QUERY_LEVEL0), in a child process, so that the output shows
whether the pyramid pays.  No rate is asserted anywhere.

    python tools/exp_queries.py [--size 2048] [--reps 20]       (recorded as profiles/r05_queries.txt)
"""
import argparse
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
VARIANT = os.path.join(ROOT, "vrenderer_amd", "lib", "variants", "query_level0", "libvrterrain.so")


def pixel_rays(view, w, h):
    """vr_view_pixel_ray for every pixel, vectorised (without its fp32 polish of the origin)."""
    M = np.array(view.clip_to_world[:], np.float64).reshape(4, 4)
    px, py = np.meshgrid(np.arange(w) + 0.5, np.arange(h) + 0.5)
    ndc = np.stack([px.ravel() / w * 2 - 1, 1 - py.ravel() / h * 2], 1)
    ends = []
    for z in (0.0, 1.0):
        c = np.concatenate([ndc, np.full((len(ndc), 1), z), np.ones((len(ndc), 1))], 1) @ M
        ends.append(c[:, :3] / c[:, 3:])
    return ends[0], ends[1] - ends[0], np.ones(len(ndc))


def measure(args):
    import torch
    import vrenderer_amd as vr
    from vrenderer_amd import capi
    from vrenderer_amd.scene import DEFAULT_EYE, DEFAULT_TARGET, params, scaled_camera
    size, n, mh = args.size, 1 << 20, 400.0 * args.size / 2048.0
    ctx = vr.Context(0)
    hm = vr.synth_heightmap(ctx, size)
    tp = vr.TerrainPass(ctx, params(size)).Init(hm, vr.synth_albedo(ctx, size, hm))
    rng = np.random.default_rng(2025)
    dev = f"cuda:{ctx.device}"

    def to_dev(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)

    def pack(o, d, tm):
        r = np.zeros(len(o), vr.RAY_DTYPE)
        r["origin"], r["dir"], r["t_max"] = o, d, tm
        return r

    eye, tgt = scaled_camera((DEFAULT_EYE, DEFAULT_TARGET), size)
    sets = {"pixel rays 1024x1024": pack(*pixel_rays(vr.make_view(eye, tgt, 1024, 1024), 1024, 1024))}
    o = np.stack([rng.uniform(-0.5, 0.5, n) * size, rng.uniform(1.0, 2.0, n) * mh, rng.uniform(-0.5, 0.5, n) * size], 1)
    tgt_pt = np.stack([rng.uniform(-0.5, 0.5, n) * size, np.zeros(n), rng.uniform(-0.5, 0.5, n) * size], 1)
    sets["uniformly random rays"] = pack(o, tgt_pt - o, np.full(n, np.inf))
    label = "walk pinned to level 0 (variant build)" if ctx.lib.vr_build_experiments() else "product build"
    print(f"--- {label}: {size}^2 synthetic map, max_height {mh:g}, n = 2^20, median of {args.reps} warm launches")

    def timed(kernel, call):
        for _ in range(3):
            call()
        ctx.synchronize()
        ms = []
        for _ in range(args.reps):
            ctx.timing_enable(1)
            call()
            t = ctx.timing_collect()
            ms.append(t[kernel][0])
        ctx.timing_enable(0)
        return float(np.median(ms))

    if not ctx.lib.vr_build_experiments():
        xz = to_dev(rng.uniform(-0.5 * size, 0.5 * size, (n, 2)).astype(np.float32))
        d_h, d_n = torch.zeros(n * 4, dtype=torch.uint8, device=dev), torch.zeros(n * 12, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        for name, nrm in (("heights", None), ("heights + normals", C.c_void_p(d_n.data_ptr()))):
            ms = timed("k_query_heights", lambda: capi.check(ctx.lib.vr_terrain_query_heights(
                tp.handle, C.c_void_p(xz.data_ptr()), n, mh, C.c_void_p(d_h.data_ptr()), nrm, 1), "vr_terrain_query_heights"))
            print(f"{name:28s} {ms * 1e3:9.1f} us  {n / ms / 1e3:9.1f} Mqueries/s")
    for name, rays in sets.items():
        d_r, d_o = to_dev(rays), torch.zeros(n * 32, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        ms = timed("k_query_rays", lambda: capi.check(ctx.lib.vr_terrain_cast_rays(
            tp.handle, C.c_void_p(d_r.data_ptr()), n, mh, C.c_void_p(d_o.data_ptr()), 1), "vr_terrain_cast_rays"))
        st = np.bincount(d_o.cpu().numpy().view(vr.RAY_HIT_DTYPE)["status"], minlength=4)
        print(f"{name:28s} {ms * 1e3:9.1f} us  {n / ms / 1e3:9.1f} Mrays/s   miss / hit / invalid / step limit = {st.tolist()}")
    tp.close(); ctx.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    measure(a)
    if not a.child:
        sys.stdout.flush()
        csrc = os.path.join(ROOT, "vrenderer_amd", "csrc")
        sources = [os.path.join(csrc, f) for f in os.listdir(csrc)] + [os.path.join(ROOT, "include", "vrterrain.h"), os.path.join(ROOT, "vrenderer_amd", "build.py")]
        if not os.path.exists(VARIANT) or os.path.getmtime(VARIANT) < max(os.path.getmtime(f) for f in sources):      # never time a stale variant
            subprocess.run([sys.executable, os.path.join(ROOT, "tools", "build_variant.py"), "query_level0", "vr_query.hip=-DVR_EXP_QUERY_LEVEL0", "-DVR_EXPERIMENT_BUILD"],
                           check=True, stdout=subprocess.DEVNULL)
        env = dict(os.environ, VRTERRAIN_LIB=VARIANT)
        subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--size", str(a.size), "--reps", str(a.reps)], check=True, env=env)
