"""Cost of vr_terrain_noise on the bench's 2048^2 pair, with SetHeight on and the query pyramid built: the whole heightmap (R8) at 1, 6
and 12 octaves for both bases, the whole albedo (SRGBA8) and a masked call of five dabs at 6 octaves.  Next to each stands a
vr_terrain_edit of the same rectangle from a device pointer - the refresh alone, the floor of any write of that rectangle - and the
calls alternate inside one session: each figure is the median of --reps (>= 5) warm repeats of the device time between two HIP events
recorded around the call on the context's stream (tools/exp_terrain_edit.py's scheme), with the spread (max - min) of the repeats
beside it.  Nothing is asserted; the output goes into DESIGN.md 4z.

(An earlier revision of this tool also forced a variant of the kernel for the whole R8 map - four texels per lane, one dword load and
store - against the one-texel kernel; those lines are profiles/terrain_noise_variants.txt, and the variant was not kept.)

    python tools/exp_terrain_noise.py [--size 2048] [--reps 5]
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

    rng = np.random.default_rng(83)
    world = float(size)                                              # a texel is one world unit here
    src = {w: torch.from_numpy(rng.integers(0, 256, (size, size * c), dtype=np.uint8)).to(dev) for w, c in (("height", 1), ("albedo", 4))}
    torch.cuda.synchronize()

    def edit(which):
        c = 1 if which == "height" else 4
        return lambda: tp.Edit(which, 0, 0, device_ptr=src[which].data_ptr(), w=size, h=size, pitch=size * c)

    def noise(which, octaves, basis, **kw):
        def fn():
            return tp.Noise(which, 1.0 / 256.0, 60.0, octaves=octaves, lacunarity=2.0, gain=0.5, offset=(3.3, -7.7), seed=5, basis=basis, fractal="fbm", op="blend",
                            base=128.0, **kw)
        return fn

    print(f"--- vr_terrain_noise on the {size}^2 pair, SetHeight on, pyramid built, median (spread) of {reps} warm repeats, device us")
    print(f"    clocks: {clocks() or 'rocm-smi not available'}")
    dabs = np.float32([[0.1 * world, -0.05 * world, 0.3 * world, 0.0, 0.9], [-0.2 * world, 0.2 * world, 0.15 * world, 0.7, 0.5],
                       [-0.5 * world, -0.5 * world, 0.1 * world, 0.0, 0.8], [0.52 * world, 0.0, 0.1 * world, 0.7, 0.5], [0.3 * world, 0.3 * world, 0.002 * world, 0.0, 1.0]])
    for which in ("height", "albedo"):
        for basis in ("value", "gradient"):
            for octaves in ((1, 6, 12) if which == "height" else (6,)):
                res = alternating({"noise": noise(which, octaves, basis, whole_map=True), "edit": edit(which)})
                cells = "  ".join(f"{name} {res[name][0]:8.1f} ({res[name][1]:6.1f})" for name in ("noise", "edit"))
                print(f"    {which:6s} whole map  {basis:8s} {octaves:2d} octaves  {cells}  host {res['noise'][2]:6.1f} us")
        x, y, w, h = noise(which, 6, "gradient", dabs=dabs)()
        c = 1 if which == "height" else 4
        res = alternating({"noise": noise(which, 6, "gradient", dabs=dabs),
                           "edit": lambda: tp.Edit(which, x, y, device_ptr=src[which].data_ptr(), w=w, h=h, pitch=size * c)})
        cells = "  ".join(f"{name} {res[name][0]:8.1f} ({res[name][1]:6.1f})" for name in ("noise", "edit"))
        print(f"    {which:6s} five dabs  gradient  6 octaves  rect {w:4d} x {h:<4d}  {cells}  host {res['noise'][2]:6.1f} us")
    tp.close()
    ctx.close()


if __name__ == "__main__":
    main()
