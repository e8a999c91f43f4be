"""Cost of the terrain history on the bench's 2048^2 pair, with SetHeight on and the query pyramid built: tools/exp_terrain_brush.py's
64-dab RAISE stroke (rectangle ~576 x 64) and a single dab 64 texels across, plus a PAINT of the same dabs (4-byte texels) and a
whole-map edit (the copy-bandwidth figure).  Per case: the stroke with history off, the stroke with history on, and undo and redo
of that step.  Each figure is the median of --reps (>= 30) warm rounds, with the spread (min .. max): device time between two HIP
events recorded around the call on the context's stream, and host microseconds of the call itself (tools/exp_terrain_edit.py's
scheme) - the journal's kernels are untimed, so the context's kernel timing does not see them; it is printed next to the event
time for the refresh it does see (node heights + pyramid).  Nothing is asserted; the output goes into DESIGN.md 4t.

    python tools/exp_terrain_history.py [--size 2048] [--reps 31] [--off-only]

--off-only measures the history-off strokes alone and needs none of the history entry points, so that VRTERRAIN_LIB may name the
build of the parent commit: alternate the two builds, process by process, in one session (measuring: A/B in the same session).
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
    ap.add_argument("--off-only", action="store_true")
    args = ap.parse_args()
    reps = max(args.reps, 30)
    import torch
    from vrenderer_amd import capi
    if args.off_only:
        capi.EXPORTS = [n for n in capi.EXPORTS if "history" not in n and n not in ("vr_terrain_undo", "vr_terrain_redo")]
    import vrenderer_amd as vr
    from vrenderer_amd.scene import params
    from exp_terrain_edit import clocks
    size, mh = args.size, 400.0 * args.size / 2048.0
    ctx = vr.Context(0)
    hm = vr.synth_heightmap(ctx, size)
    al = vr.synth_albedo(ctx, size, hm)
    tp = vr.TerrainPass(ctx, params(size)).Init(hm, al)
    tp.SetHeight(True)
    tp.CastRays(np.float32([[0.0, 4.0 * mh, 0.0]]), np.float32([[0.1, -1.0, 0.2]]), np.inf, mh)

    def timed(fn, warm=5, between=None):
        """(median, min, max) device us, median host us, median us of the context's timed kernels"""
        dev, host, timed_k = [], [], []
        for k in range(warm + reps):
            if between is not None:
                between()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ctx.synchronize()
            e0.record(torch.cuda.default_stream())
            t0 = time.perf_counter()
            fn()
            t1 = time.perf_counter()
            e1.record(torch.cuda.default_stream())
            e1.synchronize()
            if k >= warm:
                dev.append(e0.elapsed_time(e1) * 1e3); host.append((t1 - t0) * 1e6)
        for k in range(5):                                            # the context's own kernel timing, in rounds of its own (its events cost time)
            if between is not None:
                between()
            ctx.timing_enable(1)
            fn()
            ctx.synchronize()
            timed_k.append(sum(ms for ms, n in ctx.timing_collect().values()) * 1e3)
            ctx.timing_enable(0)
        return (statistics.median(dev), min(dev), max(dev)), statistics.median(host), statistics.median(timed_k)

    def show(what, r):
        (med, lo, hi), host, tk = r
        print(f"      {what:28s} device {med:8.1f} us ({lo:7.1f} .. {hi:7.1f})  host {host:7.1f} us  timed kernels {tk:7.1f} us", flush=True)
        return med

    def dabs(n, r_tex, x0, y0, x1, y1, strength):
        t = np.linspace(0.0, 1.0, n) if n > 1 else np.float64([0.5])
        out = np.zeros((n, 8), np.float32)
        out[:, 0] = (x0 + (x1 - x0) * t + 0.5) - size / 2            # a texel is one world unit here
        out[:, 1] = (y0 + (y1 - y0) * t + 0.5) - size / 2
        out[:, 2], out[:, 3], out[:, 4] = r_tex, 0.5, strength
        return out

    c = size // 2
    cases = (("raise, 1 dab, r 32", "raise", 1, dabs(1, 32.0, c, c, c, c, 0.3), {}),
             ("raise, 64 dabs, r 32, 512 long", "raise", 1, dabs(64, 32.0, c - 256, c, c + 256, c, 0.3), {}),
             ("paint, 64 dabs, r 32, 512 long", "paint", 4, dabs(64, 32.0, c - 256, c, c + 256, c, 0.5), dict(color=(200.0, 120.0, 40.0, 255.0))))
    print(f"--- terrain history on the {size}^2 pair, SetHeight on, pyramid built, median (min .. max) of {reps} warm rounds"
          f"{', history-off strokes only' if args.off_only else ''}; library {capi.LIB_PATH}")
    print(f"    clocks: {clocks() or 'rocm-smi not available'}")
    for what, op, tb, d, kw in cases:
        x, y, w, h = tp.Brush(op, d, **kw)
        print(f"    {what}: rect {w} x {h}, {w * h * tb} bytes")
        show("stroke, history off", timed(lambda: tp.Brush(op, d, **kw)))
        if args.off_only:
            continue
        tp.EnableHistory(256 << 20)
        show("stroke, history on", timed(lambda: tp.Brush(op, d, **kw), between=tp.CommitHistory))
        tp.CommitHistory()
        show("undo", timed(tp.Undo, between=lambda: tp.Redo()))
        tp.Undo()
        show("redo", timed(tp.Redo, between=lambda: tp.Undo()))
        tp.EnableHistory(0)
    if not args.off_only:
        # the two kernels alone, by difference: a device-pointer edit of a rectangle with history on and off (the edit's own copy
        # and refresh are the same in both), and an undo against that edit - for rectangles from launch-bound to the whole map
        print("    capture and swap by difference (device-pointer edit, R8 and SRGBA8): rectangle, bytes, capture us, swap us, GB/s moved")
        for which, tb in (("height", 1), ("albedo", 4)):
            for side in (64, 256, 1024, size):
                src = torch.randint(0, 256, (side, side * tb), dtype=torch.uint8, device=f"cuda:{ctx.device}")
                torch.cuda.synchronize()
                x0 = 0 if side == size else 16
                edit = lambda: tp.Edit(which, x0, x0, device_ptr=src.data_ptr(), w=side, h=side, pitch=side * tb)
                off = timed(edit, warm=3)[0][0]
                tp.EnableHistory(512 << 20)
                on = timed(edit, warm=3, between=tp.CommitHistory)[0][0]
                tp.CommitHistory()
                undo = timed(tp.Undo, warm=3, between=lambda: tp.Redo())[0][0]
                tp.EnableHistory(0)
                nbytes = side * side * tb
                cap, swap = on - off, undo - off                       # undo = swap + refresh; the edit = copy + refresh (the copy moves as much as a capture)
                print(f"      {which:6s} {side:4d}^2 {nbytes:10d} B  edit off {off:8.1f}  on {on:8.1f}  undo {undo:8.1f} us   capture {cap:7.1f} us "
                      f"({2 * nbytes / max(cap, 1e-3) / 1e3:7.1f} GB/s read+written)   undo - edit {swap:7.1f} us", flush=True)
    tp.close()
    ctx.close()


if __name__ == "__main__":
    main()
