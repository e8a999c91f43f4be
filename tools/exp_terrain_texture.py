"""Cost of vr_terrain_texture on the bench's 2048^2 pair, with SetHeight on and the query pyramid built: four layers (grass, sand,
rock, snow) under 1 dab of radius 32 texels, under a 64-dab stroke, and over the whole map.  Each figure is the median of --reps
(>= 31) warm repeats: device time between two HIP events recorded around the call on the context's stream, and host microseconds of
the call itself (tools/exp_terrain_edit.py's scheme).  Next to each stands the only route to the same map before the entry point
existed, less the download and the work of computing the texels on the host: a vr_terrain_edit of the same albedo rectangle from a
device pointer, which is the refresh alone.  Nothing is asserted; the output goes into DESIGN.md 4x.

    python tools/exp_terrain_texture.py [--size 2048] [--reps 31]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=31)
    args = ap.parse_args()
    reps = max(args.reps, 31)
    import torch
    import vrenderer_amd as vr
    from vrenderer_amd.scene import params
    from exp_terrain_edit import clocks
    size, mh = args.size, 400.0 * args.size / 2048.0
    ctx = vr.Context(0)
    hm = vr.synth_heightmap(ctx, size)
    al = vr.synth_albedo(ctx, size, hm)
    dev = f"cuda:{ctx.device}"
    tp = vr.TerrainPass(ctx, params(size)).Init(hm, al)
    tp.SetHeight(True)
    tp.CastRays(np.float32([[0.0, 4.0 * mh, 0.0]]), np.float32([[0.1, -1.0, 0.2]]), np.inf, mh)

    def timed(fn, warm=5):
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
                dev_ms.append(e0.elapsed_time(e1)); host_us.append((t1 - t0) * 1e6)
        return statistics.median(dev_ms), statistics.median(host_us)

    def dabs(n, r_tex, x0, y0, x1, y1, strength):
        """n dabs of r_tex texels, evenly spaced from texel (x0, y0) to (x1, y1), laid out as vr_brush_dab"""
        t = np.linspace(0.0, 1.0, n) if n > 1 else np.float64([0.5])
        out = np.zeros((n, 8), np.float32)
        out[:, 0] = (x0 + (x1 - x0) * t + 0.5) - size / 2            # a texel is one world unit here
        out[:, 1] = (y0 + (y1 - y0) * t + 0.5) - size / 2
        out[:, 2], out[:, 3], out[:, 4] = r_tex, 0.5, strength
        return out

    layers = [dict(color=(60.0, 140.0, 50.0, 255.0), opacity=1.0, alt_lo=0.0, alt_hi=0.45 * mh, alt_fade=0.1 * mh, slope_lo=0.0, slope_hi=25.0, slope_fade=10.0, channel_mask=7),
              dict(color=(210.0, 190.0, 130.0, 255.0), opacity=0.6, alt_lo=0.1 * mh, alt_hi=0.2 * mh, alt_fade=0.05 * mh, slope_lo=0.0, slope_hi=15.0, slope_fade=8.0, channel_mask=7),
              dict(color=(120.0, 110.0, 100.0, 255.0), opacity=0.85, alt_lo=0.0, alt_hi=mh, alt_fade=0.0, slope_lo=30.0, slope_hi=89.0, slope_fade=12.0, channel_mask=15),
              dict(color=(250.0, 250.0, 255.0, 255.0), opacity=0.9, alt_lo=0.6 * mh, alt_hi=mh, alt_fade=0.15 * mh, slope_lo=0.0, slope_hi=50.0, slope_fade=15.0, channel_mask=7)]
    c = size // 2
    cases = (("1 dab, r 32", dict(dabs=dabs(1, 32.0, c, c, c, c, 1.0))),
             ("64 dabs, r 32, 512 long", dict(dabs=dabs(64, 32.0, c - 256, c, c + 256, c, 1.0))),
             ("whole map", dict(whole_map=True)))
    print(f"--- vr_terrain_texture, 4 layers, on the {size}^2 pair, SetHeight on, pyramid built, median of {reps} warm repeats")
    print(f"    clocks: {clocks() or 'rocm-smi not available'}")
    rng = np.random.default_rng(78)
    for what, kw in cases:
        rect = tp.Texture(layers, max_height=mh, **kw)
        ms, us = timed(lambda: tp.Texture(layers, max_height=mh, **kw))
        x, y, w, h = rect
        src = torch.from_numpy(rng.integers(0, 256, (h, w * 4), dtype=np.uint8)).to(dev)
        torch.cuda.synchronize()
        ems, eus = timed(lambda: tp.Edit("albedo", x, y, device_ptr=src.data_ptr(), w=w, h=h, pitch=w * 4))
        print(f"    {what:26s} rect {w:4d} x {h:<4d}  texture: device {ms * 1e3:8.1f} us  host {us:7.1f} us    "
              f"edit of the rectangle (refresh alone): device {ems * 1e3:8.1f} us  host {eus:7.1f} us")
    tp.close()
    ctx.close()


if __name__ == "__main__":
    main()
