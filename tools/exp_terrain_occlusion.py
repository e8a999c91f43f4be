"""Cost of vr_terrain_occlusion over the whole map on 4096^2 maps (a height texel per albedo texel, a texel one world unit): a radius
of 16 and of 64 texels, with 16 and with 4 directions.  Next to each stands vr_terrain_texture with four layers over the whole map -
the same albedo bytes written and the same refresh of the albedo chain behind it - and the calls alternate inside one session: each
figure is the median of --reps (>= 5) warm repeats of the device time between two HIP events recorded around the call on the
context's stream (tools/exp_terrain_path.py's scheme), with the spread (max - min) of the repeats beside it.  occlusion - texture is
what the march costs over a kernel that reads a 4 x 4 footprint; from it and the steps a texel marches (the sum of n_d over the
directions, one LDS byte read each) the line gives the LDS byte reads per second the loop sustains.  One process; every case runs
under --step-limit seconds and the tool ends at the first that overruns; nothing is tried twice.  Nothing is asserted; the output
goes into profiles/terrain_occlusion.txt.

    python tools/exp_terrain_occlusion.py [--size 4096] [--reps 7] [--step-limit 120] [--label NAME]
"""
import argparse
import os
import signal
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def overrun(signum, frame):
    print("    a case ran past its time limit: stopping here", flush=True)
    os._exit(124)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--step-limit", type=int, default=120)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    reps = max(args.reps, 5)
    import torch
    import vrenderer_amd as vr
    from vrenderer_amd.scene import params
    from exp_terrain_edit import clocks
    signal.signal(signal.SIGALRM, overrun)
    signal.alarm(args.step_limit)
    size = args.size
    ctx = vr.Context(0)
    hm = vr.synth_heightmap(ctx, size)
    al = vr.synth_albedo(ctx, size, hm)
    tp = vr.TerrainPass(ctx, params(size)).Init(hm, al)
    mh = 400.0 * size / 2048.0
    layers = [dict(color=(60.0, 140.0, 50.0, 255.0), opacity=1.0, alt_lo=0.0, alt_hi=0.5 * mh, alt_fade=0.1 * mh, slope_lo=0.0, slope_hi=30.0, slope_fade=8.0, channel_mask=7),
              dict(color=(210.0, 190.0, 130.0, 9.0), opacity=0.6, alt_lo=0.1 * mh, alt_hi=0.2 * mh, alt_fade=0.05 * mh, slope_lo=0.0, slope_hi=40.0, slope_fade=8.0, channel_mask=5),
              dict(color=(120.0, 110.0, 100.0, 200.0), opacity=0.85, alt_lo=0.05 * mh, alt_hi=0.95 * mh, alt_fade=0.0, slope_lo=30.0, slope_hi=89.0, slope_fade=8.0, channel_mask=15),
              dict(color=(250.0, 250.0, 255.0, 255.0), opacity=0.9, alt_lo=0.7 * mh, alt_hi=1.5 * mh, alt_fade=0.1 * mh, slope_lo=0.0, slope_hi=50.0, slope_fade=8.0, channel_mask=7)]

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

    dir16 = ((1, 0), (2, 1), (1, 1), (1, 2), (0, 1), (-1, 2), (-1, 1), (-2, 1), (-1, 0), (-2, -1), (-1, -1), (-1, -2), (0, -1), (1, -2), (1, -1), (2, -1))
    print(f"--- vr_terrain_occlusion {args.label} over the whole {size}^2 map, median (spread) of {reps} warm repeats, device us")
    print(f"    clocks: {clocks() or 'rocm-smi not available'}")
    texture = lambda: tp.Texture(layers, max_height=mh, whole_map=True)
    for radius in (16.0, 64.0):
        for D in (16, 4):
            signal.alarm(args.step_limit)
            steps = sum(int(radius / float(np.hypot(dx, dz))) for dx, dz in dir16[::16 // D])
            res = alternating({"occlusion": lambda: tp.Occlusion(radius=radius, max_height=mh, directions=D, whole_map=True), "texture": texture})
            o, t = res["occlusion"], res["texture"]
            extra = o[0] - t[0]
            reads = float(size) * size * steps
            print(f"    radius {radius:3.0f}, {D:2d} directions, {steps:4d} steps a texel  occlusion {o[0]:9.1f} ({o[1]:7.1f})  texture {t[0]:8.1f} ({t[1]:6.1f})  "
                  f"occlusion / texture {o[0] / t[0]:6.2f}  occlusion - texture {extra:9.1f} us = {reads / (extra * 1e-6) / 1e12 if extra > 0 else float('nan'):6.3f} T LDS byte reads/s  "
                  f"host {o[2]:6.1f} us", flush=True)
    signal.alarm(0)
    tp.close()
    ctx.close()


if __name__ == "__main__":
    main()
