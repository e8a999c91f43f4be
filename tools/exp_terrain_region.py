"""Cost of vr_terrain_region on a 4096^2 heightmap (under a 256^2 albedo): a 64-edge polygon that covers about a quarter of the map -
few edges, most tiles deep inside and reached by the edges left of them through their spans alone - and a closed coastline of 4096
edges with a feather of 24 world units, 16 chunks of the walk.  Next to each stands a vr_terrain_edit of the same rectangle from a
device pointer - the refresh alone, the floor of any write of that rectangle - and the calls alternate inside one session: each
figure is the median of --reps (>= 5) warm repeats of the device time between two HIP events recorded around the call on the
context's stream (tools/exp_terrain_path.py's scheme), with the spread (max - min) of the repeats beside it.  region - edit is what
the kernel, the upload and the history-free call frame cost.  tools/exp_terrain_path.py's two cases follow, from the same session:
region against path at a comparable rectangle.  Nothing is asserted; the output goes into DESIGN.md 4ac.

(An earlier revision of the library could be built without the skip of the distance chain where an edge's distance box misses the
tile; the two builds' lines, taken alternately with VRTERRAIN_LIB, are profiles/terrain_region_variants.txt.)

    python tools/exp_terrain_region.py [--size 4096] [--reps 7] [--label NAME] [--no-path]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def polygon(world, edges=64):
    """A wavy 64-gon of mean radius 0.28 world sizes: pi * 0.28^2 is about a quarter of the map."""
    a = np.arange(edges) * (2.0 * np.pi / edges)
    r = 0.28 * world * (1.0 + 0.12 * np.sin(5.0 * a))
    return np.float32(np.stack([r * np.cos(a), r * np.sin(a)], 1))


def coastline(world, points=4096):
    a = np.arange(points) * (2.0 * np.pi / points)
    r = 0.33 * world * (1.0 + 0.3 * np.sin(24.0 * a) + 0.02 * np.sin(311.0 * a))
    return np.float32(np.stack([r * np.cos(a), r * np.sin(a)], 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--label", default="")
    ap.add_argument("--no-path", action="store_true")
    args = ap.parse_args()
    reps = max(args.reps, 5)
    import torch
    import vrenderer_amd as vr
    from vrenderer_amd.scene import params
    from exp_terrain_edit import clocks
    from exp_terrain_path import diagonal, meander
    size = args.size
    ctx = vr.Context(0)
    hm = vr.synth_heightmap(ctx, size)
    small = vr.synth_heightmap(ctx, 256)
    al = vr.synth_albedo(ctx, 256, small)
    dev = f"cuda:{ctx.device}"
    tp = vr.TerrainPass(ctx, params(size)).Init(hm, al)
    world = float(size)                                              # a texel is one world unit here

    def once(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ctx.synchronize()
        e0.record(torch.cuda.default_stream())
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        e1.record(torch.cuda.default_stream())
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3, (t1 - t0) * 1e6

    def alternating(fns, warm=2):
        dev_us = {n: [] for n in fns}
        host_us = {n: [] for n in fns}
        for k in range(warm + reps):
            for n, fn in fns.items():
                d, h = once(fn)
                if k >= warm:
                    dev_us[n].append(d); host_us[n].append(h)
        return {n: (statistics.median(dev_us[n]), max(dev_us[n]) - min(dev_us[n]), statistics.median(host_us[n])) for n in fns}

    rng = np.random.default_rng(83)
    src = torch.from_numpy(rng.integers(0, 256, (size, size), dtype=np.uint8)).to(dev)
    torch.cuda.synchronize()

    def line(name, what, call):
        x, y, w, h = call()
        res = alternating({what: call, "edit": lambda: tp.Edit("height", x, y, device_ptr=src.data_ptr() + y * size + x, w=w, h=h, pitch=size)})
        cells = "  ".join(f"{n} {res[n][0]:8.1f} ({res[n][1]:6.1f})" for n in (what, "edit"))
        print(f"    {name:36s} rect {w:4d} x {h:<4d}  {cells}  {what} - edit {res[what][0] - res['edit'][0]:8.1f}  host {res[what][2]:6.1f} us")

    print(f"--- vr_terrain_region {args.label} on the {size}^2 heightmap, median (spread) of {reps} warm repeats, device us")
    print(f"    clocks: {clocks() or 'rocm-smi not available'}")
    for name, pts, kw in (("polygon, 64 edges, feather 24", polygon(world), dict(feather=24.0)),
                          ("polygon, 64 edges, hard edge", polygon(world), dict(feather=0.0)),
                          ("coastline, 4096 edges, feather 24", coastline(world), dict(feather=24.0))):
        line(name, "region", lambda: tp.Region("height", pts, op="level", target=90.0, opacity=0.8, **kw))
    if not args.no_path:
        for name, pts, kw in (("path: diagonal, 64 segments, radius 24", diagonal(world), dict(radius=24.0)),
                              ("path: meander, 4096 segments, radius 24", meander(world), dict(radius=24.0, closed=True))):
            line(name, "path", lambda: tp.Path("height", pts, hardness=0.5, opacity=0.8, op="level", **kw))
    tp.close()
    ctx.close()


if __name__ == "__main__":
    main()
