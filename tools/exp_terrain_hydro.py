"""Cost of vr_terrain_erode_hydraulic on the bench's 2048^2 pair, with SetHeight on and the query pyramid built, under a mask that
covers the whole map: time per call and per sweep and texel, at the build's sweeps per launch and at ONE sweep per launch
(vr_debug_hydro_sweeps_per_launch: the same kernel, the same bytes, a launch and a trip through memory per sweep - the figure the
temporal blocking is judged against), beside vr_terrain_erode (thermal) of the same rectangle and iteration count.  Each figure is
the median (min .. max) of --reps (>= 31) warm repeats of the device time between two HIP events recorded around the call on the
context's stream; the variants alternate repeat by repeat inside one process.  The per-sweep figure of a call still holds the
call's fixed part (the mask, the final store, the refresh); the second line of each variant gives the slope between the two
iteration counts, which does not.  --thermal-lib times vr_terrain_erode with ANOTHER build of the library (the parent commit's) in a
process of its own.  Nothing is asserted; the output goes into DESIGN.md 4v.

    python tools/exp_terrain_hydro.py [--size 2048] [--iterations 64] [--reps 31] [--thermal-lib PATH]
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HYDRO = dict(rain=1.0, flow=0.5, capacity=8.0, dissolve=0.5, deposit=0.25, evaporation=0.05)
TALUS, RATE = 1.0, 0.125


def measure(args, thermal_only):
    import torch                                                       # first: the process then holds one HIP runtime (capi.load_library)
    from vrenderer_amd import capi
    if thermal_only:                                                   # an older build: it lacks the entry points under test
        lib = ctypes.CDLL(capi.LIB_PATH)
        capi.EXPORTS[:] = [n for n in capi.EXPORTS if hasattr(lib, n)]
    import vrenderer_amd as vr
    from vrenderer_amd.scene import params
    size, reps, mh = args.size, max(args.reps, 31), 400.0 * args.size / 2048.0
    ctx = vr.Context(0)
    hm = vr.synth_heightmap(ctx, size)
    al = vr.synth_albedo(ctx, size, hm)
    tp = vr.TerrainPass(ctx, params(size)).Init(hm, al)
    tp.SetHeight(True)
    tp.CastRays(np.float32([[0.0, 4.0 * mh, 0.0]]), np.float32([[0.1, -1.0, 0.2]]), np.inf, mh)
    dabs = np.zeros((1, 8), np.float32)
    dabs[0, 2:5] = 4.0 * size, 0.5, 1.0                                # mask 1 on every texel
    few, many = max(1, args.iterations // 8), args.iterations

    def hydro(n, per_launch):
        def run():
            ctx.lib.vr_debug_hydro_sweeps_per_launch(per_launch)
            tp.ErodeHydraulic(dabs, n, **HYDRO)
        return run

    variants = {}
    if not thermal_only:
        for n in (few, many):
            variants[f"hydraulic|K|{n}"] = hydro(n, 0)
            variants[f"hydraulic|1|{n}"] = hydro(n, 1)
    for n in (few, many):
        variants[f"thermal|K|{n}"] = (lambda n=n: tp.Erode(dabs, n, TALUS, RATE))
    times = {name: [] for name in variants}
    for k in range(3 + reps):                                          # three warm rounds, then the variants in turn, repeat by repeat
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ctx.synchronize()
            e0.record(torch.cuda.default_stream())
            fn()
            e1.record(torch.cuda.default_stream())
            e1.synchronize()
            if k >= 3:
                times[name].append(e0.elapsed_time(e1) * 1e3)
    if not thermal_only:
        ctx.lib.vr_debug_hydro_sweeps_per_launch(0)
    cfg = (ctypes.c_int32 * 4)()
    if not thermal_only:
        ctx.lib.vr_debug_hydro_config(cfg)
    tp.close()
    ctx.close()
    return {"config": list(cfg), "few": few, "many": many, "us": {name: [statistics.median(t), min(t), max(t)] for name, t in times.items()}}


def report(res, size, label=""):
    texels, few, many = size * size, res["few"], res["many"]
    for kind in ("hydraulic|K", "hydraulic|1", "thermal|K"):
        if f"{kind}|{many}" not in res["us"]:
            continue
        a, b = res["us"][f"{kind}|{few}"], res["us"][f"{kind}|{many}"]
        name = {"hydraulic|K": f"hydraulic, {res['config'][2]} sweeps per launch", "hydraulic|1": "hydraulic, 1 sweep per launch", "thermal|K": "thermal" + label}[kind]
        for n, m in ((few, a), (many, b)):
            print(f"    {name:36s} {n:4d} iterations: {m[0]:10.1f} us ({m[1]:.1f} .. {m[2]:.1f}) per call   {m[0] * 1e3 / (n * texels):8.4f} ns per sweep and texel", flush=True)
        print(f"    {name:36s} slope {few} -> {many}: {(b[0] - a[0]) / (many - few):9.2f} us per sweep   {(b[0] - a[0]) * 1e3 / ((many - few) * texels):8.4f} ns per sweep and texel", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--iterations", type=int, default=64)
    ap.add_argument("--reps", type=int, default=31)
    ap.add_argument("--thermal-lib", default="", help="another build of the library (the parent commit's) whose vr_terrain_erode is timed in a process of its own")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        print("RESULT " + json.dumps(measure(args, True)), flush=True)
        return
    res = measure(args, False)
    print(f"--- vr_terrain_erode_hydraulic on the {args.size}^2 pair, whole-map mask, SetHeight on, pyramid built, median (min .. max) of {max(args.reps, 31)} warm repeats; "
          f"tile {res['config'][0]} x {res['config'][1]}")
    report(res, args.size)
    if args.thermal_lib:
        env = dict(os.environ, VRTERRAIN_LIB=args.thermal_lib)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--size", str(args.size), "--iterations", str(args.iterations), "--reps", str(args.reps)],
                           env=env, capture_output=True, text=True, timeout=900)
        lines = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not lines:
            raise SystemExit(f"the thermal child failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
        report(json.loads(lines[-1][7:]), args.size, f" ({os.path.basename(os.path.dirname(args.thermal_lib)) or 'other'} build)")


if __name__ == "__main__":
    main()
