"""Cost of vr_terrain_erode on the bench's 2048^2 pair, with SetHeight on and the query pyramid built: masks whose rectangles are
67 x 67, 579 x 67 and the whole map, for 8, 64 and 512 iterations.  Each figure is the median (min .. max) of --reps (>= 31) warm
repeats: device time between two HIP events recorded around the call on the context's stream, and host microseconds of the call
itself (tools/exp_terrain_edit.py's scheme).  Beside each stands the device-pointer vr_terrain_edit of the same rectangle measured
with ANOTHER build of the library (--parent-lib: the parent commit's) - the refresh alone, the cost any route to the same map pays -
and the difference per iteration.  The two libraries alternate process by process (--rounds of each) in one session.  Nothing is
asserted; the output goes into DESIGN.md 4u.

    python tools/exp_terrain_erode.py --parent-lib PATH [--erode-lib PATH] [--size 2048] [--reps 31] [--rounds 2]
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

ITERATIONS = (8, 64, 512)
TALUS, RATE = 1.0, 0.125


def masks(size):
    """name -> dabs laid out as vr_brush_dab: a radius of 31.5 texels about a texel centre has a span of 67 texels"""
    c = size // 2

    def dabs(n, r_tex, x0, x1):
        t = np.linspace(0.0, 1.0, n) if n > 1 else np.float64([0.5])
        out = np.zeros((n, 8), np.float32)
        out[:, 0] = (x0 + (x1 - x0) * t + 0.5) - size / 2            # a texel is one world unit here
        out[:, 1] = (c + 0.5) - size / 2
        out[:, 2], out[:, 3], out[:, 4] = r_tex, 0.5, 1.0
        return out

    return (("67 x 67", dabs(1, 31.5, c, c)), ("579 x 67", dabs(33, 31.5, c - 256, c + 256)), ("whole map", dabs(1, 4.0 * size, c, c)))


def child(args):
    """One process, one library: mode 'erode' times vr_terrain_erode, mode 'edit' the device-pointer edit of the same rectangles."""
    import torch                                                       # first: the process then holds one HIP runtime (capi.load_library)
    from vrenderer_amd import capi
    if args.child == "edit":                                           # an older build: it lacks the entry points under test
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

    def timed(fn, warm=3):
        dev_ms, host_us = [], []
        for k in range(warm + reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ctx.synchronize()
            e0.record(torch.cuda.default_stream())
            t0 = time.perf_counter()
            fn()
            t1 = time.perf_counter()
            e1.record(torch.cuda.default_stream())
            e1.synchronize()
            if k >= warm:
                dev_ms.append(e0.elapsed_time(e1) * 1e3); host_us.append((t1 - t0) * 1e6)
        return [statistics.median(dev_ms), min(dev_ms), max(dev_ms), statistics.median(host_us)]

    out = {}
    rng = np.random.default_rng(79)
    for name, d in masks(size):
        if args.child == "erode":
            for n in ITERATIONS:
                out[f"{name}|{n}"] = timed(lambda: tp.Erode(d, n, TALUS, RATE))
        else:
            flat = d.copy()
            flat[:, 4] = 0.0                                           # an opacity of 0 changes nothing and returns the rectangle
            x, y, w, h = tp.Brush("flatten", flat, target=0.0)
            src = torch.from_numpy(rng.integers(0, 256, (h, w), dtype=np.uint8)).to(f"cuda:{ctx.device}")
            torch.cuda.synchronize()
            out[f"{name}|rect"] = [w, h]
            out[name] = timed(lambda: tp.Edit("height", x, y, device_ptr=src.data_ptr(), w=w, h=h, pitch=w))
    tp.close()
    ctx.close()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=31)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--erode-lib", default="", help="another build with vr_terrain_erode to time instead of the product's (tools/build_variant.py)")
    ap.add_argument("--child", choices=("erode", "edit"), default="")
    args = ap.parse_args()
    if args.child:
        return child(args)
    from exp_terrain_edit import clocks

    def run(mode, lib):
        env = dict(os.environ)
        if lib:
            env["VRTERRAIN_LIB"] = lib
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, "--size", str(args.size), "--reps", str(args.reps)],
                           env=env, capture_output=True, text=True, timeout=900)
        lines = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not lines:
            raise SystemExit(f"{mode} child failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
        return json.loads(lines[-1][7:])

    print(f"--- vr_terrain_erode on the {args.size}^2 pair, SetHeight on, pyramid built, median (min .. max) of {max(args.reps, 31)} warm repeats, "
          f"talus {TALUS}, rate {RATE}")
    print(f"    clocks: {clocks() or 'rocm-smi not available'}")
    for rnd in range(args.rounds):
        erode = run("erode", args.erode_lib)
        edit = run("edit", args.parent_lib) if args.parent_lib else None
        for name, _ in masks(args.size):
            e = edit[name] if edit else None
            rect = "x".join(str(v) for v in edit[f"{name}|rect"]) if edit else "?"
            for n in ITERATIONS:
                m = erode[f"{name}|{n}"]
                line = f"    round {rnd}  {name:9s} rect {rect:9s} {n:4d} iterations: device {m[0]:9.1f} us ({m[1]:.1f} .. {m[2]:.1f})  host {m[3]:7.1f} us"
                if e:
                    line += f"    edit on the parent build: device {e[0]:8.1f} us ({e[1]:.1f} .. {e[2]:.1f})  host {e[3]:6.1f} us    per iteration {(m[0] - e[0]) / n:7.2f} us"
                print(line, flush=True)


if __name__ == "__main__":
    main()
