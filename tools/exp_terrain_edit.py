"""Cost of vr_terrain_edit on the bench's 2048^2 pair, with SetHeight on and the query pyramid built: a 1x1, a 64x64, a
512x512 and a whole-map edit of the heightmap and of the albedo, device-pointer mode.  Each figure is the median of --reps
(>= 30) warm repeats: device time between two HIP events recorded around the call on the context's stream, and host
microseconds of the call itself.  The yardstick is what the library offered before the entry point existed -
vr_terrain_destroy + vr_terrain_create + vr_terrain_update_heights(1) + one ray cast - timed the same way.  Nothing is asserted;
the output goes into DESIGN.md 4r.

    python tools/exp_terrain_edit.py [--size 2048] [--reps 31]
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def clocks():
    """Current shader / memory clocks as rocm-smi reports them (read only); '' when the tool is not there."""
    try:
        r = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20)
        keep = [l.strip() for l in r.stdout.splitlines() if "sclk" in l or "mclk" in l]
        return "; ".join(keep[:4])
    except Exception:
        return ""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=31)
    args = ap.parse_args()
    reps = max(args.reps, 30)
    import torch
    import vrenderer_amd as vr
    from vrenderer_amd.scene import params
    size, mh = args.size, 400.0 * args.size / 2048.0
    ctx = vr.Context(0)
    hm = vr.synth_heightmap(ctx, size)
    al = vr.synth_albedo(ctx, size, hm)
    dev = f"cuda:{ctx.device}"
    ray_o, ray_d = np.float32([[0.0, 4.0 * mh, 0.0]]), np.float32([[0.1, -1.0, 0.2]])

    def fresh():
        tp = vr.TerrainPass(ctx, params(size)).Init(hm, al)
        tp.SetHeight(True)
        tp.CastRays(ray_o, ray_d, np.inf, mh)
        return tp

    def timed(fn, warm=5):
        """(median device ms, median host us) of fn() over `reps` repeats after `warm` unrecorded ones; the events sit on the
        legacy default stream, which is the context's stream here."""
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

    print(f"--- vr_terrain_edit on the {size}^2 pair, SetHeight on, pyramid built, device-pointer mode, median of {reps} warm repeats")
    print(f"    clocks: {clocks() or 'rocm-smi not available'}")
    tp = fresh()
    rng = np.random.default_rng(77)
    rows = {}
    for which, tb in (("height", 1), ("albedo", 4)):
        for edge in (1, 64, 512, size):
            src = torch.from_numpy(rng.integers(0, 256, (edge, edge * tb), dtype=np.uint8)).to(dev)
            torch.cuda.synchronize()
            x = y = (size - edge) // 2 if edge < size else 0
            x |= 1 if edge == 1 else 0                   # an odd coordinate for the single texel
            ms, us = timed(lambda: tp.Edit(which, x, y, device_ptr=src.data_ptr(), w=edge, h=edge, pitch=edge * tb))
            rows[(which, edge)] = (ms, us)
            print(f"    {which:6s} {edge:5d} x {edge:<5d}  device {ms * 1e3:9.1f} us   host {us:9.1f} us per call{'   (host-issue bound)' if us > 0.8 * ms * 1e3 else ''}")
    state = {"tp": tp}

    def recreate():
        state["tp"].close()
        state["tp"] = fresh()

    ms, us = timed(recreate, warm=2)
    print(f"    yardstick: destroy + create + update_heights(1) + one ray cast   device+host {ms * 1e3:9.1f} us   host {us:9.1f} us per round")
    for which in ("height", "albedo"):
        whole, small = rows[(which, size)][0], rows[(which, 64)][0]
        print(f"    {which}: whole-map edit / yardstick = {whole / ms:.3f}; 64x64 edit / whole-map edit = {small / whole:.4f}")
    state["tp"].close()
    ctx.close()


if __name__ == "__main__":
    main()
