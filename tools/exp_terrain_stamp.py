"""Cost of vr_terrain_stamp on the bench's 2048^2 pair, with SetHeight on and the query pyramid built: stamps of 256^2, 1024^2 and
2048^2 texels on the heightmap (R8) and on the albedo (SRGBA8), at 0 and 30 degrees, at one and at four stamp texels per map texel
(BLEND, feather 0.25).  Next to each stands a vr_terrain_edit of the same rectangle from a device pointer - the refresh alone, the
floor of any write of that rectangle - and the two alternate inside one session: each figure is the median of --reps (>= 5) warm
repeats of the device time between two HIP events recorded around the call on the context's stream (tools/exp_terrain_edit.py's
scheme), with the spread (max - min) of the repeats beside it.  Nothing is asserted; the output goes into DESIGN.md 4y.  (An earlier
revision of this tool also forced an LDS-staged variant of the kernel against the direct one; those lines are
profiles/terrain_stamp_variants.txt, and the staged kernel was not kept.)

    python tools/exp_terrain_stamp.py [--size 2048] [--reps 5]
"""
import argparse
import math
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
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    reps = max(args.reps, 5)
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
        """fns: name -> callable; `warm` + reps rounds, each running every callable once, in turn"""
        dev_us = {n: [] for n in fns}
        host_us = {n: [] for n in fns}
        for k in range(warm + reps):
            for n, fn in fns.items():
                d, h = once(fn)
                if k >= warm:
                    dev_us[n].append(d); host_us[n].append(h)
        return {n: (statistics.median(dev_us[n]), max(dev_us[n]) - min(dev_us[n]), statistics.median(host_us[n])) for n in fns}

    rng = np.random.default_rng(79)
    print(f"--- vr_terrain_stamp on the {size}^2 pair, SetHeight on, pyramid built, median (spread) of {reps} warm repeats, device us")
    print(f"    clocks: {clocks() or 'rocm-smi not available'}")
    for which, channels in (("height", 1), ("albedo", 4)):
        for n in (256, 1024, 2048):
            texels = rng.integers(0, 256, (n, n) if channels == 1 else (n, n, 4), dtype=np.uint8)
            st = vr.Stamp(ctx, texels)
            for ratio in (1, 4):
                for deg in (0.0, 30.0):
                    extent = float(n // ratio)                   # a texel is one world unit here
                    kw = dict(x=3.3, z=-7.7, size_x=extent, size_z=extent, rotation=math.radians(deg), opacity=0.8, feather=0.25)

                    def stamp():
                        return tp.Stamp(which, st, **kw)
                    x, y, w, h = stamp()
                    src = torch.from_numpy(rng.integers(0, 256, (h, w * channels), dtype=np.uint8)).to(dev)
                    torch.cuda.synchronize()
                    res = alternating({"stamp": stamp, "edit": lambda: tp.Edit(which, x, y, device_ptr=src.data_ptr(), w=w, h=h, pitch=w * channels)})
                    cells = "  ".join(f"{name} {res[name][0]:8.1f} ({res[name][1]:6.1f})" for name in ("stamp", "edit"))
                    print(f"    {which:6s} stamp {n:4d}^2  {ratio}:1  {deg:4.0f} deg  rect {w:4d} x {h:<4d}  {cells}  host {res['stamp'][2]:6.1f} us")
            st.close()
    tp.close()
    ctx.close()


if __name__ == "__main__":
    main()
