"""Cost of bringing a terrain up: vr_terrain_create + vr_terrain_update_heights(1) + the first ray cast (which builds the query
pyramid), wall clock with the context's stream drained, on the 2048^2 pair (the bench's own maps, and tools/exp_terrain_edit.py's)
and on an 8192^2 pair - the largest the library takes.  Median and min..max of --reps rounds after one unrecorded round; nothing
is asserted.  The figures belong in DESIGN.md 7 (row f2).

    python tools/exp_create_time.py [--reps 7]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    import vrenderer_amd as vr
    from vrenderer_amd.scene import params
    ctx = vr.Context(0)
    for size in (2048, 8192):
        hm = vr.synth_heightmap(ctx, size)
        al = vr.synth_albedo(ctx, size, hm)
        mh = 400.0 * size / 2048.0
        ms = {"create": [], "update_heights": [], "first ray cast": [], "all three": []}
        for k in range(args.reps + 1):
            ctx.synchronize()
            t0 = time.perf_counter()
            tp = vr.TerrainPass(ctx, params(size)).Init(hm, al)
            ctx.synchronize(); t1 = time.perf_counter()
            tp.SetHeight(True)
            ctx.synchronize(); t2 = time.perf_counter()
            tp.CastRays(np.float32([[0.0, 4.0 * mh, 0.0]]), np.float32([[0.1, -1.0, 0.2]]), np.inf, mh)
            ctx.synchronize(); t3 = time.perf_counter()
            tp.close()
            if k:
                for key, dt in zip(ms, (t1 - t0, t2 - t1, t3 - t2, t3 - t0)):
                    ms[key].append(dt * 1e3)
        print(f"{size}^2: " + "; ".join(f"{key} {statistics.median(v):.2f} ({min(v):.2f}..{max(v):.2f}) ms" for key, v in ms.items()), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
