#!/usr/bin/env python3
"""bench.py — shaded Gpixels/s of the terrain + deferred-shading hot path at 8K on MI355X.

One "step" = one frame of the hot path on synthetic input already resident in HBM:
quadtree LOD select -> vertex transform -> triangle setup/binning -> tile raster + pixel
shader into the G-buffer -> deferred lighting into HdrColor (RGBA16F).  With N > 1 the
frame is partitioned into interleaved 128x128 screen tiles (owner = (tx+ty) mod N), each
rank renders and lights only its tiles, and the packed tiles are all-gathered over
RCCL/xGMI and de-tiled into the full frame on every rank (strong scaling: the frame is
fixed, the ranks split it).

Prints ONE JSON line on rank 0 (see the driver contract in the task description).

A plain run (`bench.py --gpus 1 --steps K --warmup W`) sets up, renders W warm-up frames, times K frames and prints the
line (`value`, `ms_per_step` and the per-launch figures of the timed frames).  `--full` adds everything else the bench
measures, each in timed regions or child processes of its own: `sustained`, `without_plane_tracking`, the small kernels'
timings and the geometry chain alone, the `frames_4k` / `lights_1024` / `shadows` / `fused` sub-records and `cpu_baseline`.
`--dump-outputs DIR` writes what the last timed frame computed as DIR/<name>.npy (see dump_outputs).
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# HIP multiplexes streams onto 4 hardware queues by default; the N-rank loop uses 5 (render, exchange, de-tile, two geometry
# streams) and streams that share a queue serialise.  Must be set before the runtime initialises.
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

WRITE_STREAM_GBS = 5700.0      # a write-only stream of the tile pass's shape: profiles/r03_fill_rate.txt
HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: 8.0 TB/s spec (6.29 TB/s measured copy ceiling)
DEFERRED_BYTES_PER_PX = 36     # 28 B G-buffer read + 8 B RGBA16F write
GBUFFER_BYTES_PER_PX = 28      # G-buffer fill, per covered pixel


from vrenderer_amd.scene import flythrough_camera  # noqa: E402


def cpu_baseline(size, hm, al, params_fn, ambient, cam_fn):
    """The oracle ("port") timed on this box's host cores on a bounded sample; rank 0, N=1 only."""
    import numpy as np
    from oracle import pyoracle as po
    import vrenderer_amd as vr
    po.build()
    w, h = 1920, 1080
    p = params_fn(size)
    t0 = time.perf_counter()
    ot = po.OracleTerrain(p, hm, al)
    t_create = time.perf_counter() - t0
    gb = po.GBufferHost(w, h)
    rp = vr.default_render_params(400.0)
    frames = 16                                    # every 7th flythrough frame: ~10 s of single-core work
    n = 0
    t0 = time.perf_counter()
    for k in range(frames):
        view = po.view_from_camera(*cam_fn(7 * k), w, h)
        gb.clear()
        n = ot.render(view, gb, rp)
        po.deferred(view, gb, [vr.reference_sun()], ambient[0], ambient[1])
    t_frame = (time.perf_counter() - t0) / frames
    # the reference's own CPU-side terrain work, single-threaded like its main thread
    import ctypes as C
    t_build = po.lib().orc_time_tree_build(C.byref(p), hm.ctypes.data_as(C.c_void_p), hm.shape[1], hm.shape[0])
    views = (vr.View * 120)(*[po.view_from_camera(*cam_fn(i), 7680, 4320) for i in range(120)])
    sel = C.c_int()
    reps = 200
    t_sel = po.lib().orc_time_select(ot.handle, views, 120, 400.0, reps, C.byref(sel))
    t_seth = po.lib().orc_time_set_height(ot.handle)
    ot.close()
    return {
        "value": round(w * h / t_frame / 1e9, 6), "unit": "Gpixels/s", "cores": 1, "kind": "port",
        "sample": f"{frames} flythrough frames at {w}x{h} (1/16 of the 8K frame's pixels each), same scene: oracle "
                  f"clear+select+raster+pixel shader+deferred, {t_frame:.2f} s per frame, {frames * t_frame:.1f} s in all",
        "host_cores": os.cpu_count(),
        "reference_cpu_side": {
            "quadtree_build_s": round(t_build, 4), "nodes": int((4 ** (ot_num_lods(size) + 1) - 1) // 3),
            "select_plus_update_transforms_us_per_frame": round(t_sel / (reps * 120) * 1e6, 3),
            "selected_nodes_sum_over_120_frames": int(sel.value),
            "set_height_minmax_s": round(t_seth, 4),
            "oracle_terrain_create_s": round(t_create, 3),
            "note": "restatement of QuadTree::Split / NodeSelect / UpdateTransforms / SetHeight, 1 core (reference runs them on the main thread)",
        },
    }


def cpu_quadtree_line(args):
    """BASELINE config 1: source/terrain's quadtree LOD update on a 256^2 heightmap, fixed (reference default) camera,
    CPU only - the oracle's restatement of QuadTree::Split / NodeSelect / UpdateTransforms / SetHeight timed on this
    host's cores, single-threaded like the reference's main thread.  No GPU call is made."""
    import ctypes as C
    import numpy as np
    from oracle import pyoracle as po
    from vrenderer_amd import capi
    from vrenderer_amd.scene import DEFAULT_EYE, DEFAULT_TARGET, params, scaled_camera
    po.build()
    size = 256
    hm = po.synth_heightmap(size)
    al = po.synth_albedo(size, hm)
    p = params(size)
    eye, tgt = scaled_camera((DEFAULT_EYE, DEFAULT_TARGET), size)
    reps = max(1, args.steps) * 1000
    t_build = min(po.lib().orc_time_tree_build(C.byref(p), hm.ctypes.data_as(C.c_void_p), size, size) for _ in range(5))
    ot = po.OracleTerrain(p, hm, al)
    views = (capi.View * 1)(po.view_from_camera(eye, tgt, 1920, 1080))
    sel = C.c_int()
    po.lib().orc_time_select(ot.handle, views, 1, 400.0, max(1, args.warmup) * 100, C.byref(sel))          # warm-up
    t_sel = min(po.lib().orc_time_select(ot.handle, views, 1, 400.0, reps, C.byref(sel)) for _ in range(3))
    t_seth = min(po.lib().orc_time_set_height(ot.handle) for _ in range(5))
    n_sel = int(sel.value)                      # orc_time_select reports the per-repetition count
    ot.close()
    us = t_sel / reps * 1e6
    print(json.dumps({
        "metric": "quadtree LOD update (NodeSelect + UpdateTransforms) per frame, CPU", "value": round(us, 4), "unit": "us/frame",
        "n_gpus": 0, "steps": reps, "warmup": max(1, args.warmup) * 100, "ms_per_step": round(us * 1e-3, 7), "higher_is_better": False,
        "scaling": "none", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": "BASELINE config 1: source/terrain quadtree LOD update, 256^2 heightmap (8 LODs, 87,381 nodes), reference "
                               "default camera scaled to the surface, 1920x1080 view, CPU only; restatement (oracle/vr_oracle.c) of "
                               "QuadTree.cpp:80-131,164-232 + TerrainPass.cpp:234-256", "heightmap": size,
                   "selected_nodes": n_sel},
        "cpu_baseline": {"value": round(us, 4), "unit": "us/frame", "cores": 1, "kind": "port", "host_cores": os.cpu_count(),
                         "sample": f"best of 3 x {reps} NodeSelect+UpdateTransforms calls; tree build (Split) best of 5; SetHeight best of 5",
                         "quadtree_build_s": round(t_build, 5), "set_height_minmax_s": round(t_seth, 5)},
        "roofline": None,
        "note": "parity unpinned (no reference fixtures exist); the device counterpart of this work is k_select (~22 us, latency-bound) "
                "and the mip-style SetHeight reduction",
    }), flush=True)


def ot_num_lods(size):
    return min(11, int(math.log2(size)))


DUMP_SAMPLE_PX = 1 << 21        # at most this many pixels of an image are written (seeded sample): 32 MB of RGBA float32
DUMP_SEED = 20261016


def dump_outputs(out_dir, images):
    """Writes each (name, HxWxC array) of `images` as out_dir/<name>.npy in float32, one row per pixel.  An image of more
    than DUMP_SAMPLE_PX pixels is reduced to the same fixed, seeded set of pixel indices (ascending) for every image of that
    size, so two builds' files compare element for element."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    picks = {}
    for name, a in images:
        a = a.reshape(a.shape[0] * a.shape[1], -1)
        n = a.shape[0]
        if n > DUMP_SAMPLE_PX:
            if n not in picks:
                picks[n] = np.sort(np.random.default_rng(DUMP_SEED).choice(n, size=DUMP_SAMPLE_PX, replace=False))
            a = a[picks[n]]
        if a.dtype == np.uint16:            # RGBA16F bits
            a = a.view(np.float16)
        np.save(os.path.join(out_dir, f"{name}.npy"), np.ascontiguousarray(a, dtype=np.float32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=120, help="timed frames; the default is one whole lap of the 120-frame flythrough")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--width", type=int, default=7680)
    ap.add_argument("--height", type=int, default=4320)
    ap.add_argument("--size", type=int, default=2048, help="heightmap / world size")
    ap.add_argument("--full", action="store_true",
                    help="measure everything beside the headline figure (module docstring); a plain run only times the --steps frames")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed frames, write what the last one computed as DIR/<name>.npy (float32)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--fixed-camera", action="store_true", help="reference default camera instead of the flythrough")
    ap.add_argument("--no-prepare", action="store_true",
                    help="do not build frame i+1's geometry ahead (vr_terrain_prepare) under frame i's tile pass")
    ap.add_argument("--raster-tile", type=int, default=0, choices=[0, 32, 64],
                    help="pin the tile pass's raster tile edge (VR_OPT_RASTER_TILE); 0 = by frame size and split (default)")
    ap.add_argument("--no-depth-ranges", action="store_true",
                    help="--lights N: the tiled pass's culling stage reads the depth plane instead of the ranges the tile pass leaves")
    ap.add_argument("--prewarm-laps", type=int, default=0,
                    help="untimed laps of the 120-frame camera path rendered during set-up, before the warm-up steps (device clock ramp); "
                         "0 (default): --warmup means exactly what it says and the figure after a lap of load is reported beside it ('sustained')")
    ap.add_argument("--no-submit", action="store_true",
                    help="queue a frame through the per-call entry points (Render, Prepare x 2, Light, tone-map stage: ~9 calls) instead of "
                         "vr_frame_submit (one call); A/B of the host's cost per frame")
    ap.add_argument("--fused", action="store_true",
                    help="opt-in fused variant (vr_terrain_render_lit, SURVEY 7 step 6): the tile pass shades what it rasterises and writes depth + "
                         "HdrColor only - same bits as the two passes; reported as the `fused` sub-record of the default run, never as the headline")
    ap.add_argument("--no-sustained", action="store_true", help="skip the second timed region (the same K frames after one more lap of load)")
    ap.add_argument("--no-plane-tracking", action="store_true",
                    help="the whole run with vr_context_set_option(VR_OPT_PLANE_TRACKING, 0): every plane of every pixel written and read")
    ap.add_argument("--timing-level", type=int, default=2, choices=[0, 1, 2],
                    help="vr_timing_enable level inside the timed region: 2 = dispatch-stamped events on the two big kernels (default), "
                         "1 = event records around every kernel, 0 = none (no per-kernel figures; measures what the stamps cost)")
    ap.add_argument("--prepare-depth", type=int, default=2, choices=[1, 2],
                    help="how many frames ahead vr_terrain_prepare builds geometry (three geometry sets, one stream each: two chains in flight)")
    ap.add_argument("--no-overlap", action="store_true",
                    help="N>1: run the all-gather + de-tile of frame i on the render stream instead of overlapping it with frame i+1")
    ap.add_argument("--verify", action="store_true", help="after timing, compare the assembled frame with an unsplit render")
    ap.add_argument("--force-dist", action="store_true",
                    help="run the N>1 code path (process group, packed tiles, all-gather, de-tile) even with one rank")
    ap.add_argument("--no-4k", action="store_true", help="skip the additional 3840x2160 measurement (N=1, default resolution only)")
    ap.add_argument("--shadows", action="store_true",
                    help="add row f1 to every step: the 2048^2 terrain shadow pass from the sun + the PCF shadow term in the "
                         "lighting pass (Renderer.cpp:333-367); not part of the default workload")
    ap.add_argument("--exchange", choices=["ldr", "hdr"], default="ldr",
                    help="N>1: what the all-gather carries. ldr (default): each rank tone-maps its tiles (ToneMappingPass, "
                         "histogram all-reduced over the ranks) and RGB8 tiles are gathered, 3 B/px; hdr: RGB16F tiles, 6 B/px")
    ap.add_argument("--no-dispatch-events", action="store_true",
                    help="explicit hipEventRecord packets around the tile pass instead of the dispatch-stamped events (A/B of the launch gap)")
    ap.add_argument("--lights", type=int, default=1,
                    help="BASELINE config 5: N > 1 lights the frame with 1 sun + N-1 point lights (seed 9001, ranges 20-80) through "
                         "the tiled pass (per-tile LDS light culling) instead of the streaming pass")
    ap.add_argument("--emulate-rank", type=int, default=None,
                    help="with --emulate-world N: no process group; this one GPU renders and lights rank R's share of the N-way "
                         "screen-tile split (what one rank of an N-GPU job computes per frame, without the exchange)")
    ap.add_argument("--emulate-world", type=int, default=None)
    ap.add_argument("--config", choices=["gpu", "cpu-quadtree"], default="gpu",
                    help="cpu-quadtree = BASELINE config 1: the reference's CPU-side quadtree work on a 256^2 heightmap, "
                         "fixed camera, no GPU call at all")
    ap.add_argument("--rehearse-on-one-gpu", action="store_true",
                    help="debug: all ranks share cuda:0 and the exchange goes through gloo on host copies (RCCL refuses "
                         "two ranks on one device); exercises the N>1 control flow on a one-GPU box, timings are meaningless")
    args = ap.parse_args()
    if args.config == "cpu-quadtree":
        return cpu_quadtree_line(args)

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus > 1 and world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} needs WORLD_SIZE={args.gpus} (launch with torch.distributed.run)")
    if args.gpus == 1 and not args.force_dist:
        world, rank, local_rank = 1, 0, 0
    use_dist = world > 1 or args.force_dist

    import numpy as np
    torch = None
    dist = None
    comm = None            # this rank's ncclComm_t for the C-ABI exchange (vrenderer_amd.rccl.Communicator)
    if use_dist:
        import torch
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29531")
        if args.rehearse_on_one_gpu:
            local_rank = 0
            torch.cuda.set_device(0)
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            torch.cuda.set_device(local_rank)
            # RCCL prints a version banner on stdout when the communicator comes up (at the first collective): keep stdout
            # for the one JSON line by pointing fd 1 at stderr until then
            sys.stdout.flush()
            saved_stdout = os.dup(1)
            os.dup2(2, 1)
            try:
                dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
                warm = torch.zeros(1, device="cuda")
                dist.all_reduce(warm)
                torch.cuda.synchronize()
                # The exchange of the timed loop goes through the library's own entry points (vr_tonemap_allreduce_histogram,
                # vr_frame_allgather[_tiles/_ldr]: include/vrterrain.h), which take the host's ncclComm_t: one communicator of
                # this job's ranks, made from the RCCL already in the process; rank 0's unique id travels over the process group.
                from vrenderer_amd import rccl
                uid = torch.zeros(rccl.NCCL_UNIQUE_ID_BYTES, dtype=torch.uint8, device="cuda")
                if rank == 0:
                    uid.copy_(torch.frombuffer(bytearray(rccl.get_unique_id()), dtype=torch.uint8))
                dist.broadcast(uid, 0)
                comm = rccl.Communicator(world, rank, uid.cpu().numpy().tobytes())
                torch.cuda.synchronize()
            finally:
                sys.stdout.flush()
                os.dup2(saved_stdout, 1)
                os.close(saved_stdout)

    import vrenderer_amd as vr
    from vrenderer_amd.passes import (frame_allgather, frame_allgather_ldr, frame_allgather_tiles, frame_detile, frame_detile_ldr, partition_info,
                                      partition_prepare)
    from vrenderer_amd.scene import AMBIENT_BOTTOM, AMBIENT_TOP, DEFAULT_EYE, DEFAULT_TARGET, params

    W, H, size = args.width, args.height, args.size
    # host housekeeping first, device set-up last: a full collection takes ~40 ms, and a device that sits idle for that long right
    # before the warm-up frames starts them from its idle clocks (the same 20 frames: 0.49 ms each then, 0.44 at sustained clocks)
    import gc
    gc.collect()
    ctx = vr.Context(local_rank)
    if args.raster_tile:
        ctx.set_raster_tile(args.raster_tile)
    if torch is not None:
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)

    if args.no_dispatch_events:
        ctx.set_dispatch_events(False)
    if args.no_plane_tracking:
        ctx.set_plane_tracking(False)
    hm = vr.synth_heightmap(ctx, size, 1337)
    al = vr.synth_albedo(ctx, size, hm, 4242)
    tp = vr.TerrainPass(ctx, params(size)).Init(hm, al)
    rt = vr.RenderTargets(ctx).Init(W, H)
    lights = [vr.reference_sun()]
    tiled = args.lights > 1
    if tiled:
        lights += vr.synthetic_point_lights(args.lights - 1, float(size), hm, 400.0, seed=9001)
    deferred = vr.TiledDeferredLightingPass(ctx) if tiled else vr.DeferredLightingPass(ctx)
    tiled_lights = vr.light_array(lights) if tiled else None        # the vr_light[] the C ABI takes, built once
    light_kernel = "k_deferred_tiled" if tiled else "k_deferred"
    # Clear fused into the tile pass (same result as Clear + Render); with the tiled lighting pass behind it, the tile pass also
    # leaves the light tiles' depth ranges for its culling stage (--no-depth-ranges: the stage reads the depth plane again)
    rp = vr.default_render_params(400.0, assume_cleared=1, depth_ranges=1 if (tiled and not args.no_depth_ranges) else 0)

    shadow_map = None
    if args.shadows:
        shadow_map = vr.CascadedShadowMap(ctx, vr.default_shadow_params(float(size), depth_bias=0.002))
    part = None
    ctx_comm = ctx
    emu = args.emulate_world is not None
    if emu:
        # one rank's share of an N-way split on this one GPU: packed tiles out of the lighting pass, tone-mapped to the
        # RGB8 tiles the rank would hand to the all-gather (histogram of its own pixels only: no all-reduce here)
        if use_dist or args.emulate_rank is None or not (0 <= args.emulate_rank < args.emulate_world):
            raise SystemExit("--emulate-rank R --emulate-world N (0 <= R < N) runs without a process group")
        part = vr.Partition(args.emulate_rank, args.emulate_world)
        info = partition_info(W, H, args.emulate_rank, args.emulate_world)
        rows = (info["packed_bytes"] + vr.VR_OWNER_TILE * 8 - 1) // (vr.VR_OWNER_TILE * 8)
        emu_hdr = [vr.HdrImage(ctx, vr.VR_OWNER_TILE, rows) for _ in range(2)]
        hdr = frame = emu_hdr[0]
        emu_ldr = args.exchange == "ldr"
        if emu_ldr:
            # as in the N-rank loop: the tone-map stage of frame i runs on the exchange stream under the rendering of frame i+1
            import torch
            torch.cuda.set_device(local_rank)
            main_stream = torch.cuda.current_stream()
            ctx.set_stream(main_stream.cuda_stream)
            comm_stream = torch.cuda.Stream()
            ctx_comm = vr.Context(local_rank)
            ctx_comm.set_stream(comm_stream.cuda_stream)
            tmp = vr.default_tonemap_params()
            tm = vr.ToneMappingPass(ctx_comm)
            tm.AdvanceFrame(1.0 / 60.0)
            ldr_img = vr.LdrImage(ctx_comm, W, H)     # capacity of a whole frame; the packed RGB8 tiles use the front of it
            emu_render_done = [torch.cuda.Event() for _ in range(2)]
            emu_tm_done = [torch.cuda.Event() for _ in range(2)]
        from vrenderer_amd import partition as pt
        tx_ = pt.owner_grid(W, H)[0]
        owned_px = sum(min(128, W - (t % tx_) * 128) * min(128, H - (t // tx_) * 128)
                       for t in pt.owned_tiles(W, H, args.emulate_rank, args.emulate_world))
    if use_dist:
        part = vr.Partition(rank, world)
        info = partition_info(W, H, rank, world)
        # Double-buffered exchange: frame i's all-gather + de-tile run on a side stream while frame
        # i+1 is rendered (the collective reads packed[b] / writes gathered[b], the renderer does not).
        nbuf = 1 if args.no_overlap else 2
        half_elems = info["packed_bytes"] // 2
        gathered = [torch.empty(world * half_elems, dtype=torch.float16, device="cuda") for _ in range(nbuf)]
        # packed tile-major buffer: max_owned tiles of 128x128 RGB16F (6 B/px), equal on every rank
        rows = (info["packed_bytes"] + vr.VR_OWNER_TILE * 8 - 1) // (vr.VR_OWNER_TILE * 8)     # image wrapper sized in 8-B pixels
        packed = [torch.empty(rows * vr.VR_OWNER_TILE * 4, dtype=torch.float16, device="cuda") for _ in range(nbuf)]
        hdr_bufs = [vr.HdrImage(ctx, vr.VR_OWNER_TILE, rows, external_ptr=t.data_ptr()) for t in packed]
        main_stream = torch.cuda.current_stream()
        ctx_post = ctx
        if nbuf > 1:
            comm_stream = torch.cuda.Stream()
            ctx_comm = vr.Context(local_rank)
            ctx_comm.set_stream(comm_stream.cuda_stream)
            # the de-tile of frame i has no part in the exchange itself: on a third stream it runs under frame i+1's all-gather
            post_stream = torch.cuda.Stream()
            ctx_post = vr.Context(local_rank)
            ctx_post.set_stream(post_stream.cuda_stream)
        else:
            comm_stream = post_stream = main_stream
        partition_prepare(ctx_comm, W, H, part)
        if ctx_post is not ctx_comm:
            partition_prepare(ctx_post, W, H, part)
        ldr = args.exchange == "ldr"
        one_call = nbuf == 1 and comm is not None       # everything on one stream: vr_frame_allgather[_ldr] (gather + de-tile)
        if ldr:
            # f3: the frame leaves each rank tone-mapped (Renderer.cpp:430-431); all of it runs on the exchange stream
            tmp = vr.default_tonemap_params()
            tm = vr.ToneMappingPass(ctx_comm)
            tm.AdvanceFrame(1.0 / 60.0)

            class _DevArray:        # the pass's 256 histogram bins as a tensor for the all-reduce
                def __init__(self, ptr, n):
                    self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<i4", "data": (ptr, False), "version": 2}
            hist_t = torch.as_tensor(_DevArray(tm.histogram_device_ptr, 256), device="cuda")
            ldr_bytes = info["packed_bytes_ldr"]
            packed_ldr = [torch.empty(ldr_bytes, dtype=torch.uint8, device="cuda") for _ in range(nbuf)]
            ldr_bufs = [vr.LdrImage(ctx_comm, W, H, external_ptr=t.data_ptr(), capacity_bytes=ldr_bytes) for t in packed_ldr]
            gathered_ldr = [torch.empty(world * ldr_bytes, dtype=torch.uint8, device="cuda") for _ in range(nbuf)]
            frame = vr.LdrImage(ctx_post, W, H)
        else:
            frame = vr.HdrImage(ctx_post, W, H)
        # event pairs around the collectives themselves (on the exchange stream): the first multi-GPU run can then separate
        # the exchange from the compute it hides behind
        xch_events = []                                            # (start, stop) per timed frame
        xch_timed = [False]
        render_done = [torch.cuda.Event() for _ in range(nbuf)]
        comm_done = [torch.cuda.Event() for _ in range(nbuf)]       # the send buffers of slot b are free again
        gather_done = [torch.cuda.Event() for _ in range(nbuf)]     # gathered[b] is complete
        post_done = [torch.cuda.Event() for _ in range(nbuf)]       # gathered[b] has been consumed by the de-tile
        from vrenderer_amd import partition as pt
        tx_ = pt.owner_grid(W, H)[0]
        owned_px = sum(min(128, W - (t % tx_) * 128) * min(128, H - (t // tx_) * 128) for t in pt.owned_tiles(W, H, rank, world))
    elif not emu:
        hdr = vr.HdrImage(ctx, W, H)
        frame = hdr
        owned_px = W * H

    def camera(i):
        return (DEFAULT_EYE, DEFAULT_TARGET) if args.fixed_camera else flythrough_camera(i)

    views = [vr.make_view(*camera(i), W, H) for i in range(120)]

    def allgather(dst_u8, src_u8):
        """This rank's packed tiles -> every rank's `gathered` buffer, on the exchange stream: ncclAllGather through the C ABI
        (vr_frame_allgather_tiles; RCCL over xGMI, equal send counts)."""
        if args.rehearse_on_one_gpu:                                       # (debug: gloo on host copies stands in for RCCL)
            comm_stream.synchronize()
            host = torch.empty(dst_u8.numel(), dtype=torch.uint8)
            dist.all_gather_into_tensor(host, src_u8.cpu())
            dst_u8.copy_(host)
        else:
            frame_allgather_tiles(ctx_comm, comm, src_u8.data_ptr(), dst_u8.data_ptr(), world, src_u8.numel())

    def allreduce(t_i32):
        """The tone mapper's 256 histogram bins summed over the ranks: vr_tonemap_allreduce_histogram (ncclAllReduce)."""
        if args.rehearse_on_one_gpu:
            comm_stream.synchronize()
            host = t_i32.cpu()
            dist.all_reduce(host)
            t_i32.copy_(host)
        else:
            tm.AllReduceHistogram(comm)

    def light(v, out_img, p):
        if tiled:
            deferred.Render(v, rt, tiled_lights, AMBIENT_TOP, AMBIENT_BOTTOM, out_img, p)
        else:
            deferred.Render(v, rt, lights, AMBIENT_TOP, AMBIENT_BOTTOM, out_img, p, shadow_map=shadow_map)

    def prepare_ahead(i, p):
        tp.Prepare(views[(i + 1) % 120], rt, rp, p)          # frame i+1's geometry is built under frame i's tile pass
        if args.prepare_depth > 1:
            tp.Prepare(views[(i + 2) % 120], rt, rp, p)      # ... and frame i+2's: a second chain in flight (a no-op for a frame already prepared)

    # one call per frame (vr_frame_submit: Render [+ Clear] -> Prepare x 2 -> lighting [-> tone-map stage]); the shadow path keeps
    # the per-call sequence (its shadow-map pass sits between frames)
    if args.fused and (tiled or shadow_map is not None or use_dist):
        raise SystemExit("--fused: the fused kernel takes the streaming pass's plain case (<= 16 lights, no shadow term) on one GPU or an emulated rank")
    use_submit = not args.no_submit and shadow_map is None and not args.no_prepare and not args.fused
    frame_call = None
    if use_submit:
        stage = dict(tonemap=tm, tonemap_params=tmp, ldr=ldr_img) if (emu and emu_ldr) else {}
        frame_call = vr.Frame(tp, rt, rp, tiled_lights if tiled else lights, AMBIENT_TOP, AMBIENT_BOTTOM, part, tiled, **stage)

    def submit(i, out_img):
        ahead = [views[(i + 1) % 120]] + ([views[(i + 2) % 120]] if args.prepare_depth > 1 else [])
        frame_call.submit(views[i % 120], out_img, ahead)

    def step(i):
        v = views[i % 120]
        if shadow_map is not None:                  # every rank renders the whole (small) shadow map
            shadow_map.SetupForPlanarViewStable(lights[0], v)
            shadow_map.RenderTerrain(tp)
        if use_submit and not use_dist:
            submit(i, emu_hdr[i % 2] if emu else hdr)        # (an emulated rank rotates two tile buffers; the library orders the two streams)
            return
        if not use_dist:
            out_img = emu_hdr[i % 2] if emu else hdr
            if emu and emu_ldr:
                main_stream.wait_event(emu_tm_done[i % 2])         # the packed tiles of two frames ago have been consumed
            if args.fused:
                tp.RenderLit(v, rt, rp, lights, AMBIENT_TOP, AMBIENT_BOTTOM, out_img, part)
            else:
                tp.Render(v, v, rt, rp, part)
            if not args.no_prepare:
                if shadow_map is None:
                    prepare_ahead(i, part)
                else:                                # both passes of frame i+1: its shadow map's geometry, then its main view's
                    shadow_map.PrepareTerrain(tp, lights[0], views[(i + 1) % 120])
                    tp.Prepare(views[(i + 1) % 120], rt, rp, part)
            if not args.fused:
                light(v, out_img, part)
            if emu and emu_ldr:
                emu_render_done[i % 2].record(main_stream)
                with torch.cuda.stream(comm_stream):
                    comm_stream.wait_event(emu_render_done[i % 2])
                    tm.ResetHistogram()
                    tm.AddFrameToHistogram(tmp, out_img, W, H, part)
                    tm.ComputeExposure(tmp)
                    tm.Render(tmp, out_img, ldr_img, W, H, part)
                    emu_tm_done[i % 2].record(comm_stream)
            return
        b = i % nbuf
        main_stream.wait_event(comm_done[b])        # packed[b] / gathered[b] are free again (no-op before first use)
        if use_submit:
            submit(i, hdr_bufs[b])
        else:
            tp.Render(v, v, rt, rp, part)
            if not args.no_prepare and shadow_map is None:
                prepare_ahead(i, part)
            light(v, hdr_bufs[b], part)
        render_done[b].record(main_stream)
        with torch.cuda.stream(comm_stream):
            comm_stream.wait_event(render_done[b])
            comm_stream.wait_event(post_done[b])                           # gathered[b] is free (no-op before first use)
            ev = None
            if xch_timed[0]:
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
                xch_events.append(ev)
            if ldr:
                tm.ResetHistogram()
                tm.AddFrameToHistogram(tmp, hdr_bufs[b], W, H, part)       # this rank's pixels
                if ev: ev[0].record(comm_stream)
                allreduce(hist_t)                                          # the real exchange step of f3: 1 KiB
                if ev: ev[1].record(comm_stream)
                tm.ComputeExposure(tmp)
                tm.Render(tmp, hdr_bufs[b], ldr_bufs[b], W, H, part)       # packed RGB16F tiles -> packed RGB8 tiles
                if ev: ev[2].record(comm_stream)
                if one_call:         # --no-overlap: all-gather + de-tile as ONE call of the C ABI, on the one stream
                    frame_allgather_ldr(ctx_comm, comm, packed_ldr[b].data_ptr(), gathered_ldr[b].data_ptr(), world, W, H, frame)
                else:
                    allgather(gathered_ldr[b], packed_ldr[b])
                if ev: ev[3].record(comm_stream)
            else:
                if ev: ev[0].record(comm_stream); ev[1].record(comm_stream); ev[2].record(comm_stream)
                if one_call:
                    frame_allgather(ctx_comm, comm, packed[b].data_ptr(), gathered[b].data_ptr(), world, frame)
                else:
                    allgather(gathered[b].view(torch.uint8), packed[b][:half_elems].view(torch.uint8))
                if ev: ev[3].record(comm_stream)
            gather_done[b].record(comm_stream)
            comm_done[b].record(comm_stream)
        with torch.cuda.stream(post_stream):
            post_stream.wait_event(gather_done[b])
            if not one_call:         # the de-tile of frame i on its own stream, under the all-gather of frame i+1
                if ldr:
                    frame_detile_ldr(ctx_post, gathered_ldr[b].data_ptr(), world, W, H, frame)
                else:
                    frame_detile(ctx_post, gathered[b].data_ptr(), world, frame)
            post_done[b].record(post_stream)

    def sync():
        if emu and emu_ldr:
            torch.cuda.synchronize()
        elif use_dist:
            torch.cuda.synchronize()
            dist.barrier()
            torch.cuda.synchronize()
        else:
            ctx.synchronize()

    # The contract: W untimed warm-up steps, then exactly K timed steps - `value`.  The device idles through the seconds of
    # host-side set-up above (context, textures, tables) and needs ~15 ms of load to return to its sustained clocks; the W = 5
    # warm-up frames of the driver's command are 3 ms, so `value` contains that ramp (same 20 frames: 0.584-0.590 ms straight
    # after 5 warm-up frames, 0.547-0.550 ms after a lap; profiles/r03_clock_ramp.txt).  Round 3 rendered an untimed lap here
    # by default; now --prewarm-laps defaults to 0 and the figure after a lap of load is measured in a SECOND timed region
    # behind the first and reported beside it ("sustained").
    gc.disable()                             # (collected before the device set-up, above) no collector pause while the host queues the warm-up and timed frames (20 frames are 11 ms);
                                             # here, not between warm-up and timed region: a collection there idles the device for tens of
                                             # milliseconds and the timed frames then measure its clock ramp (0.54 -> 0.61 ms, measured)
    for i in range(120 * args.prewarm_laps):
        step(i)
    sync()
    for i in range(args.warmup):
        step(i)
    sync()
    # HIP events on the stream each kernel is launched on.  The timed region times the launches whose events the dispatch
    # itself stamps - the tile pass and the lighting pass (level 2: no host call, no extra packet) - and the small kernels
    # (geometry chain, tone-map stage, de-tile) are timed with event records around every launch in a separate pass behind
    # it: two hipEventRecord calls around each of a frame's dozen small kernels cost the 8K frame 30 us (557 -> 590 us) and
    # make a rank's loop of an 8-way split, whose frame period is near 0.1 ms, host-bound (host 164 us per frame with
    # them, 60 without; tools/exp_host_cost.py).
    timing_level = args.timing_level
    ctx.timing_enable(timing_level)
    side_ctxs = [c for c in dict.fromkeys((ctx_comm, ctx_post if use_dist else ctx_comm)) if c is not ctx]
    for c in side_ctxs:
        c.timing_enable(timing_level)
    if use_dist:
        xch_timed[0] = True
    t0 = time.perf_counter()
    for i in range(args.steps):
        step(args.warmup + i)
    t_issue = time.perf_counter() - t0       # host time to queue the timed frames (the device runs behind it)
    gc.enable()
    sync()
    elapsed = time.perf_counter() - t0
    if use_dist:
        xch_timed[0] = False
    timings = ctx.timing_collect()
    ctx.timing_enable(False)
    for c in side_ctxs:
        timings.update(c.timing_collect())
        c.timing_enable(False)
    if args.dump_outputs and rank == 0:
        # the last timed frame as its caller receives it: HdrColor (packed tiles of the emulated rank's share, or the
        # assembled frame of an N-rank run), with the depth plane of an unsplit frame beside it
        if use_dist:
            dump = [("ldr_color" if ldr else "hdr_color", frame.download())]
        elif emu:
            # the rank's owned pixels in packed order (the padding of partial and missing tiles is never written)
            packed = (ldr_img.download(info["packed_bytes_ldr"]) if emu_ldr else
                      emu_hdr[(args.warmup + args.steps - 1) % 2].download(info["packed_bytes"])).reshape(-1, 128, 128, 3)
            px = []
            for j, t in enumerate(pt.owned_tiles(W, H, args.emulate_rank, args.emulate_world)):
                px.append(packed[j, :min(128, H - (t // tx_) * 128), :min(128, W - (t % tx_) * 128)].reshape(-1, 1, 3))
            dump = [("ldr_tiles" if emu_ldr else "hdr_tiles", np.concatenate(px))]
        else:
            dump = [("hdr_color", hdr.download()), ("depth", rt.download("depth")[..., None])]
        dump_outputs(args.dump_outputs, dump)
    # the same K frames once more after a further lap of load (clocks ramped): reported beside `value`, never instead of it
    sustained = None
    if args.full and args.prewarm_laps == 0 and not args.no_sustained:
        gc.collect(); gc.disable()
        for i in range(120):
            step(args.warmup + args.steps + i)
        sync()
        t1 = time.perf_counter()
        for i in range(args.steps):
            step(args.warmup + args.steps + 120 + i)
        gc.enable()
        sync()
        el2 = time.perf_counter() - t1
        if use_dist:
            t2 = torch.tensor([el2], dtype=torch.float64, device="cpu" if args.rehearse_on_one_gpu else "cuda")
            dist.all_reduce(t2, op=dist.ReduceOp.MAX)
            el2 = float(t2.item())
        sustained = {"value": round(W * H * args.steps / el2 / 1e9, 3), "unit": "Gpixels/s", "ms_per_step": round(el2 / args.steps * 1e3, 4),
                     "what": f"the same {args.steps} steps timed again behind one further lap (120 frames) of load, when the device has returned to its "
                             "sustained clocks after the idle set-up phase (round 3's `value` was measured like this: its bench rendered an untimed lap first)"}
    # ... and once more with the plane-state tracking off (VR_OPT_PLANE_TRACKING = 0): every tile pass writes all five planes of
    # every pixel and the lighting pass reads them all, as a renderer without clear / constant metadata would.  Same frames, same
    # bits in the G-buffer and in HdrColor; reported beside `value` so that the tracking's share of it is on the page.
    untracked = None
    if args.full and not args.no_sustained and not args.fused and not args.no_plane_tracking:
        ctx.set_plane_tracking(False)
        gc.collect(); gc.disable()
        for i in range(20):
            step(args.warmup + i)
        sync()
        ctx.timing_enable(2)
        t1 = time.perf_counter()
        for i in range(args.steps):
            step(args.warmup + args.steps + 120 + i)
        gc.enable()
        sync()
        el3 = time.perf_counter() - t1
        t_off = ctx.timing_collect()
        ctx.timing_enable(False)
        ctx.set_plane_tracking(True)
        if use_dist:
            t3 = torch.tensor([el3], dtype=torch.float64, device="cpu" if args.rehearse_on_one_gpu else "cuda")
            dist.all_reduce(t3, op=dist.ReduceOp.MAX)
            el3 = float(t3.item())
        untracked = {"value": round(W * H * args.steps / el3 / 1e9, 3), "unit": "Gpixels/s", "ms_per_step": round(el3 / args.steps * 1e3, 4),
                     "kernels": {k: {"avg_us": round(ms / n * 1e3, 2), "launches": n} for k, (ms, n) in t_off.items()},
                     "what": f"the same {args.steps} steps as `sustained` with vr_context_set_option(VR_OPT_PLANE_TRACKING, 0): 28 B/px written by "
                             "the tile pass and 28 B/px read by the lighting pass whatever the planes hold"}
        for i in range(3):                   # (back on: the states are rebuilt by the next frames)
            step(args.warmup + i)
        sync()
    kernels_note = None
    if args.full and timing_level == 2:
        # the small kernels (geometry chain, tone-map stage, de-tile), timed with events around every launch over a few
        # more frames OUTSIDE the timed region
        extra = min(args.steps, 20)
        for c in [ctx] + side_ctxs:
            c.timing_enable(1)
        for i in range(extra):
            step(args.warmup + args.steps + i)
        sync()
        diag = ctx.timing_collect()
        ctx.timing_enable(False)
        for c in side_ctxs:
            diag.update(c.timing_collect())
            c.timing_enable(False)
        for k, v in diag.items():
            timings.setdefault(k, v)
        # ... and the geometry chain with the device to itself: beside the tile pass its kernels' durations are residence times
        # (below ~9.6K x 5.4K the tile pass runs six waves of 80 VGPRs per SIMD and leaves a geometry wave 32), not costs
        chain_alone = None
        if shadow_map is None:
            try:
                ctx.timing_enable(1)
                for i in range(8):
                    tp.Prepare(views[(args.warmup + args.steps + extra + 31 + 13 * i) % 120], rt, rp, part)
                    ctx.synchronize()
                alone = ctx.timing_collect()
                ctx.timing_enable(False)
                chain_alone = {k: round(ms / n * 1e3, 2) for k, (ms, n) in alone.items()
                               if k in ("k_select", "k_vertex", "k_setup", "k_clip", "k_scan", "k_fill")}
            except Exception:
                chain_alone = None
        kernels_note = (f"k_raster and the lighting kernel from the {args.steps} timed frames (dispatch-stamped events); every other kernel from "
                        f"{extra} further frames timed with events around every launch, outside the timed region - beside the tile pass, "
                        "whose waves leave the geometry kernels few registers: their figures there are residence times, "
                        "geometry_chain_alone_us has them with the device to themselves")
    n_nodes = tp.num_chunks()
    if tiled:
        deferred.Status()            # raises if a tile kept more than VR_TILE_LIGHT_CAP lights (the result would be truncated)

    verified = None
    if args.verify:
        idx = args.warmup + args.steps - 1
        if use_dist and ldr:
            tm.ResetExposure(0.0)       # the adapted luminance has a history; restart it for the comparison frame
        idx += 1                        # (other frames may have been rendered since the timed region: render the comparison frame now)
        step(idx)
        sync()
        last = views[idx % 120]
        got = frame.download()
        ref_img = vr.HdrImage(ctx, W, H)
        tp.Render(last, last, rt, rp, None)                 # (the comparison frame is always the unfused pair)
        if shadow_map is not None:
            shadow_map.SetupForPlanarViewStable(lights[0], last)
            shadow_map.RenderTerrain(tp)
        light(last, ref_img, None)
        if use_dist and ldr:
            tm_ref = vr.ToneMappingPass(ctx)
            tm_ref.AdvanceFrame(1.0 / 60.0)
            ldr_ref = vr.LdrImage(ctx, W, H)
            tm_ref.SimpleRender(tmp, ref_img, ldr_ref)
            verified = bool(np.array_equal(got, ldr_ref.download()))
            ldr_ref.close(); tm_ref.close()
        else:
            verified = bool(np.array_equal(got, ref_img.download()))
        ref_img.close()
        if not verified:
            raise SystemExit(f"rank {rank}: assembled frame differs from the unsplit frame")

    if use_dist:
        tmax = torch.tensor([elapsed], dtype=torch.float64, device="cpu" if args.rehearse_on_one_gpu else "cuda")
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        elapsed = float(tmax.item())

    if rank == 0:
        ms_per_step = elapsed / args.steps * 1e3
        value = W * H * args.steps / elapsed / 1e9
        kern = {k: {"avg_us": round(ms / n * 1e3, 2), "launches": n} for k, (ms, n) in timings.items()}
        total_kernel_ms = sum(ms for ms, _ in timings.values())
        dominant = max(timings.items(), key=lambda kv: kv[1][0])[0] if timings else None

        # HBM bytes per launch measured with rocprofv3 PMC passes (FETCH_SIZE x2 on gfx950 for wide
        # reads, + WRITE_SIZE; see tools/summarize_pmc.py).  They were taken on the N=1 8K workload.
        pmc, sq = {}, {}
        def newest(stem):
            for rnd in ("r04", "r03", "r02"):
                f = f"profiles/{rnd}_{stem}"
                if os.path.exists(os.path.join(ROOT, f)):
                    return f
            return f"profiles/r02_{stem}"
        pmc_file = newest("pmc_traffic_lights.json" if tiled else "pmc_traffic.json")
        sq_file = newest("pmc_sq_lights.json" if tiled else "pmc_sq.json")
        # the counter passes were taken on the default workload's launches only: with the shadow pass in the frame, on a
        # partitioned frame or at another size the per-launch instruction counts are not those of the timed launches
        counters_apply = world == 1 and not emu and (W, H) == (7680, 4320) and not args.shadows
        if counters_apply:
            try:
                pmc = json.load(open(os.path.join(ROOT, pmc_file)))
            except Exception:
                pmc = {}
            try:
                sq = json.load(open(os.path.join(ROOT, sq_file)))
            except Exception:
                sq = {}

        def roof(name, bytes_per_px, px, moved_per_px=None, moved_note=None):
            """achieved = ALGORITHMIC bytes per launch (SURVEY 8d's per-pixel figure x the launch's pixels) / the launch's HIP-event
            duration.  With the plane-state tracking on, the launch MOVES fewer bytes than that (it does not rewrite / re-read what
            the library knows the planes hold): `moved` has that figure and the rate it corresponds to."""
            if name not in timings:
                return None
            ms, n = timings[name]
            avg_s = ms / n * 1e-3
            ach = bytes_per_px * px / avg_s / 1e9
            out = {"kernel": name, "bound": "hbm", "achieved": round(ach, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                   "frac": round(ach / HBM_PEAK_GBS, 4),
                   "traffic": pmc.get(name, {}).get("hbm_bytes_per_launch"),
                   "traffic_source": (pmc_file + " (separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this command, "
                                                 "not measured in this run)") if name in pmc else None,
                   "avg_us": round(avg_s * 1e6, 2), "bytes_per_launch": bytes_per_px * px,
                   "note": f"{bytes_per_px} algorithmic B/pixel (SURVEY 8d) x {px} pixels per launch / HIP-event duration"
                           + ("; a kernel that only moves the same bytes reaches 5.6-5.9 TB/s on this part (profiles/r01_stream_layout_ceiling.txt)"
                              if name == "k_deferred" else "; runs at ~80 % of the per-CU memory pipeline (fetches and stores in series) and at half of a store-only kernel's rate, "
                                   "see write_stream_ceiling, roofline_l1, roofline_valu and DESIGN.md 4")}
            if moved_per_px is not None:
                mv = moved_per_px * px / avg_s / 1e9
                out["moved"] = {"bytes_per_pixel": moved_per_px, "bytes_per_launch": round(moved_per_px * px), "achieved": round(mv, 1),
                                "frac": round(mv / HBM_PEAK_GBS, 4), "note": moved_note}
            return out

        def roof_valu(name):
            """Vector-instruction issue of the tile pass / the tiled lighting pass.  achieved = wave-instructions per launch
            (SQ_INSTS_VALU from the committed PMC pass of this command) / the live HIP-event duration.  peak = one wave64
            instruction per TWO cycles and SIMD: the cheapest class (v_mul / v_add / v_fma_f32, moves, 32-bit integer adds and
            logic with register operands) occupies a SIMD-32 for 2 cycles - round 4's calibration by wall time x the launch's
            clock (tools/micro/valu_cost.hip, profiles/r04_valu_issue_costs.txt; round 3's table read 1 cycle from a median
            wave's ticks, which the age-based arbitration halves).  Conversions, v_med3, 24-bit mads, shifts, compares,
            selects and anything with a scalar operand cost 4, transcendentals 8.  pipe_busy = the launch's class counters
            priced with those costs / (1024 SIMDs x clock x duration): the share of the vector pipes' cycles that are taken,
            with the 32-bit integer class (adds and logic at 2, the rest at 4: not split by the counters) at both ends."""
            if name not in timings or name not in sq:
                return None
            ms, n = timings[name]
            avg_s = ms / n * 1e-3
            c = sq[name]
            ach = c["SQ_INSTS_VALU"] / avg_s / 1e9
            peak = 1024 * 2.4 / 2.0
            out = {"kernel": name, "bound": "valu", "achieved": round(ach, 1), "peak": round(peak, 1), "unit": "G wave-instr/s",
                   "frac": round(ach / peak, 4), "insts_per_launch": c["SQ_INSTS_VALU"], "avg_us": round(avg_s * 1e6, 2),
                   "peak_note": "1024 SIMDs x 2.4 GHz / 2 cycles per cheap wave64 instruction; under this load the part runs at 1.9-2.2 GHz",
                   "source": sq_file + ", profiles/r04_valu_issue_costs.txt"}
            if "SQ_INSTS_VALU_FMA_F32" in c:
                f32 = c["SQ_INSTS_VALU_ADD_F32"] + c["SQ_INSTS_VALU_MUL_F32"] + c["SQ_INSTS_VALU_FMA_F32"]
                i32, i64, cvt, trans = c["SQ_INSTS_VALU_INT32"], c.get("SQ_INSTS_VALU_INT64", 0.0), c["SQ_INSTS_VALU_CVT"], c["SQ_INSTS_VALU_TRANS_F32"]
                rest = max(c["SQ_INSTS_VALU"] - f32 - i32 - i64 - cvt - trans, 0.0)          # moves, compares, selects, lane ops, ...
                lo = 2 * f32 + 2 * i32 + 4 * i64 + 4 * cvt + 8 * trans + 2 * rest
                hi = 2 * f32 + 4 * i32 + 4 * i64 + 4 * cvt + 8 * trans + 4 * rest
                out["class_mix"] = {"f32_add_mul_fma": f32, "int32": i32, "int64": i64, "cvt": cvt, "transcendental": trans, "other": rest}
                if "GRBM_GUI_ACTIVE" in c and c.get("GRBM_duration_us"):
                    # GRBM_GUI_ACTIVE is summed over the 8 XCDs; the counter pass runs every kernel alone (serialised launches), so
                    # the busy share is taken against that pass's own cycles, not against the live duration
                    xcd_cycles = c["GRBM_GUI_ACTIVE"] / 8.0
                    out["pipe_busy"] = {"low": round(lo / (1024 * xcd_cycles), 3), "high": round(hi / (1024 * xcd_cycles), 3),
                                        "of": "the counter pass's launch (kernel alone)", "duration_us": c["GRBM_duration_us"],
                                        "clock_ghz": round(xcd_cycles / c["GRBM_duration_us"] / 1e3, 2)}
            return out

        def roof_l1(name):
            """The tile pass's other bound: the L1's tag look-ups (one cache line per clock per CU).  achieved = look-ups per
            launch (TCP_TOTAL_CACHE_ACCESSES from the committed PMC pass of the 8K tile pass) / the live HIP-event duration;
            peak = 256 L1s x 2.4 GHz.  Only quoted for the frame the counters were collected on (8K, unsplit)."""
            tcp_file = newest("pmc_tcp.json")
            try:
                with open(os.path.join(ROOT, tcp_file)) as f:
                    tcp = json.load(f)
            except OSError:
                return None
            if name not in timings or name not in tcp or not counters_apply or part is not None or tiled:
                return None
            ms, n = timings[name]
            avg_s = ms / n * 1e-3
            ach = tcp[name]["TCP_TOTAL_CACHE_ACCESSES"] / avg_s / 1e9
            peak = 256 * 2.4
            return {"kernel": name, "bound": "l1-tags", "achieved": round(ach, 1), "peak": round(peak, 1), "unit": "G look-ups/s",
                    "frac": round(ach / peak, 4), "lookups_per_launch": tcp[name]["TCP_TOTAL_CACHE_ACCESSES"],
                    "pending_stall_cycles_per_launch": tcp[name]["TCP_PENDING_STALL_CYCLES"], "source": tcp_file}

        # bytes the lighting pass really moves per pixel: 8 written; read 28, less the emissive plane (8) while it is known zero,
        # less the specular plane (4) in regions known to hold the shader's constant, nothing in regions known clear (sky)
        census_l = rt.region_census()
        emi_zero = bool(rt.plane_known_zero("emissive"))
        fl_clear = census_l["clear"] / max(census_l["total"], 1)
        fl_spec = census_l["specular_constant"] / max(census_l["total"], 1)
        read_px = (28 - (8 if emi_zero else 0)) * (1.0 - fl_clear) - 4.0 * fl_spec
        deferred_moved = round(8 + read_px, 2) if (light_kernel == "k_deferred") else None
        roof_deferred = roof(light_kernel, DEFERRED_BYTES_PER_PX, owned_px, deferred_moved,
                             "8 B/px written; of the G-buffer's 28 B/px the pass reads what the plane-state tracking does not already know: no emissive "
                             "plane while it is zero, no specular plane in regions that hold the shader's constant, nothing in regions that are "
                             "clear (region states after the last frame; `traffic` is the HBM-side measurement)")
        if tiled and roof_deferred and "k_light_cull" in timings:      # config 5's lighting is two launches: price the pair
            pair_s = (timings[light_kernel][0] / timings[light_kernel][1] + timings["k_light_cull"][0] / timings["k_light_cull"][1]) * 1e-3
            ach = DEFERRED_BYTES_PER_PX * owned_px / pair_s / 1e9
            roof_deferred.update({"kernel": "k_light_cull + k_deferred_tiled", "achieved": round(ach, 1), "frac": round(ach / HBM_PEAK_GBS, 4),
                                  "avg_us": round(pair_s * 1e6, 2)})
        # bytes the tile pass really writes per pixel: 28, or 20 while the library knows the emissive plane is all zero and does not
        # rewrite it (VR_OPT_PLANE_TRACKING: main_ps's o_channel3 = 0 lands on zeros)
        emissive_skipped = bool(rt.plane_known_zero("emissive"))
        plane_bytes = GBUFFER_BYTES_PER_PX - (8 if emissive_skipped else 0)
        # ... and per region (8 rows x 32 pixels): a sky region known clear is not written, a terrain region known to hold the
        # shader's specular constant keeps that plane.  The states after the last frame say what a frame of this flythrough skips
        # (consecutive views differ little); the HBM-side truth is WRITE_SIZE in `traffic`.
        census = rt.region_census()
        f_clear = census["clear"] / max(census["total"], 1)
        f_spec = census["specular_constant"] / max(census["total"], 1)
        raster_moved = round(plane_bytes * (1.0 - f_clear) - 4.0 * f_spec, 2)
        roof_raster = roof("k_raster", GBUFFER_BYTES_PER_PX, owned_px, raster_moved,
                           "the frame's average over all pixels: 28 B/px less the emissive plane (8) while it is known zero, less the specular plane (4) "
                           "in regions known to hold the shader's constant, nothing in regions known clear")
        if roof_raster:
            roof_raster["emissive_plane"] = ("known zero (cleared at creation, only zeros written since): not rewritten" if emissive_skipped else "written")
            roof_raster["regions"] = dict(census, note="8x32-pixel regions by what the library knows they hold after the last frame: `clear` regions "
                                          "(sky) were not written, `specular_constant` regions (terrain) kept their specular plane")
        if roof_raster:
            # the tile pass only writes: what a store-only kernel of its own pattern reaches on this part (tools/micro/fill_rate.hip:
            # 929 MB in 156-163 us), next to the 8 TB/s of reads and writes together that `peak` is
            roof_raster["write_stream_ceiling"] = {"gbs": WRITE_STREAM_GBS, "frac": round(roof_raster["moved"]["achieved"] / WRITE_STREAM_GBS, 4),
                                                   "source": "profiles/r03_fill_rate.txt (measured, not a datasheet figure)"}
        out = {
            "metric": "shaded Gpixels/s at 8K terrain", "value": round(value, 3), "unit": "Gpixels/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms_per_step, 4),
            "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "untimed_setup": (f"{args.prewarm_laps} lap(s) of the 120-frame camera path rendered before the {args.warmup} warm-up steps: the device "
                              "needs ~15 ms of load after the host-side set-up to reach its sustained clocks (same 20 frames: 0.585 ms straight "
                              "after 5 warm-up frames, 0.549 ms after a lap; --prewarm-laps 0 for the raw figure)") if args.prewarm_laps else None,
            "sustained": sustained,
            "without_plane_tracking": (dict(untracked, roofline=(lambda us: {"kernel": light_kernel, "bound": "hbm", "avg_us": us,
                                                   "achieved": round(DEFERRED_BYTES_PER_PX * owned_px / (us * 1e-6) / 1e9, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                                   "frac": round(DEFERRED_BYTES_PER_PX * owned_px / (us * 1e-6) / 1e9 / HBM_PEAK_GBS, 4),
                                                   "note": "all 36 B/pixel moved: the lighting pass as a pure stream"})(untracked["kernels"][light_kernel]["avg_us"]))
                                       if untracked and light_kernel in untracked.get("kernels", {}) else untracked),
            "config": {"workload": f"{W}x{H} terrain flythrough (120-frame circle r=600 y=250), heightmap {size}^2, "
                                   + (f"1 sun + {args.lights - 1} point lights (seed 9001, range 20-80) through the tiled pass; " if tiled
                                      else "1 directional light; ")
                                   + "full path select+vertex+setup/bin+tile raster(PS)+deferred"
                                   + ("; +terrain shadow pass 2048^2 and PCF shadow term" if args.shadows else "")
                                   + (("+tone map (histogram all-reduce)+all-gather of RGB8 tiles+detile" if ldr else
                                       "+all-gather of RGB16F tiles+detile") if use_dist else ""),
                       "resolution": [W, H], "heightmap": size, "nodes_last_frame": n_nodes,
                       "parallelism": f"screen tiles {vr.VR_OWNER_TILE}x{vr.VR_OWNER_TILE}, owner=(tx+ty)%{world}"
                                      + (", tone map + all-gather of frame i under the rendering of frame i+1, de-tile of frame i under the all-gather of frame i+1"
                                         if use_dist and not args.no_overlap else "")},
            # the north-star kernel (>= 60 % HBM roofline target on the 8K deferred-lighting pass)
            "roofline": roof_deferred,
            "roofline_gbuffer_fill": roof_raster,
            "roofline_valu": [r for r in (roof_valu("k_raster"), roof_valu(light_kernel) if tiled else None) if r] if counters_apply else [],
            "roofline_l1": roof_l1("k_raster"),
            "dominant_kernel_by_time": dominant,
            "kernels": kern,
            "kernel_time_ms_per_step": round(total_kernel_ms / args.steps, 4),
            # how long the host needed to queue a frame: if this approaches ms_per_step the loop is host-bound, not device-bound
            "host_issue_ms_per_step": round(t_issue / args.steps * 1e3, 4),
            "host_calls_per_frame": "1 (vr_frame_submit)" if use_submit and not use_dist else ("vr_frame_submit + the exchange stage's calls" if use_submit else "per-call API"),
        }
        if kernels_note:
            out["kernels_note"] = kernels_note
            if chain_alone:
                out["geometry_chain_alone_us"] = dict(chain_alone, sum=round(sum(chain_alone.values()), 1))
        if emu:
            out["emulation"] = {"rank": args.emulate_rank, "world": args.emulate_world, "owned_pixels": owned_px,
                                "what": "one GPU computes this rank's share of the N-way screen-tile split per frame (geometry replicated, "
                                        "tile pass + lighting" + (" + tone map to packed RGB8 tiles" if emu_ldr else "") + " of owned tiles); "
                                        "no exchange. value = frame pixels / this rank's frame period = what N such ranks deliver when the "
                                        "all-gather is fully hidden; unmeasured on N GPUs",
                                "rank_frame_us": round(ms_per_step * 1e3, 1)}
        if use_dist and xch_events:
            # rank 0's own view of the exchange: event pairs on the exchange stream around the collectives themselves
            def span(i, j):
                return sum(ev[i].elapsed_time(ev[j]) for ev in xch_events) / len(xch_events) * 1e3
            allreduce_us = span(0, 1) if ldr else 0.0
            allgather_us = span(2, 3)
            compute_us = sum(timings[k][0] / timings[k][1] * 1e3 for k in ("k_raster", light_kernel, "k_light_cull") if k in timings)
            period_us = ms_per_step * 1e3
            exchange_us = allreduce_us + allgather_us
            hidden = max(0.0, min(exchange_us, compute_us + exchange_us - period_us))
            out["exchange"] = {"exchange_us": round(exchange_us, 1), "allgather_us": round(allgather_us, 1), "allreduce_us": round(allreduce_us, 1),
                               "rank_compute_us": round(compute_us, 1), "frame_period_us": round(period_us, 1),
                               "overlap": round(hidden / exchange_us, 3) if exchange_us > 0 else None,
                               "bytes_received_per_rank": int((world - 1) * (info["packed_bytes_ldr"] if ldr else info["packed_bytes"])),
                               "through": ("gloo on host copies (rehearsal)" if comm is None else
                                           "the C ABI: vr_tonemap_allreduce_histogram + " + ("vr_frame_allgather_ldr / vr_frame_allgather (gather + de-tile in one call)" if one_call
                                                                                             else "vr_frame_allgather_tiles, vr_frame_detile[_ldr] on a third stream")
                                           + ", ncclComm_t of this job's ranks (vrenderer_amd/rccl.py)"),
                               "what": "HIP events on rank 0's exchange stream around the all-reduce (256 histogram bins) and the all-gather "
                                       "(packed tiles) of every timed frame, including the wait for the slowest peer; rank_compute_us = tile pass + "
                                       "lighting of rank 0's tiles; overlap = share of the exchange hidden behind the next frame's rendering"}
        if verified is not None:
            out["frame_verified_against_unsplit"] = verified
        if args.full and world == 1 and not use_dist and not emu and (W, H) == (7680, 4320) and not args.no_4k and not args.shadows:
            # the north star asks for 4K next to 8K: the same workload at 3840x2160, measured by a child process
            # (same code path, its own context) after this process has gone idle
            try:
                import subprocess
                ctx.synchronize()
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--width", "3840", "--height", "2160", "--steps", str(args.steps),
                                    "--warmup", str(args.warmup), "--full", "--no-cpu-baseline", "--no-4k", "--lights", str(args.lights)]
                                   + (["--fixed-camera"] if args.fixed_camera else []),
                                   capture_output=True, text=True, timeout=300)
                j = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
                out["frames_4k"] = {"resolution": [3840, 2160], "value": j["value"], "unit": j["unit"], "ms_per_step": j["ms_per_step"],
                                    "roofline": {k: j["roofline"][k] for k in ("kernel", "achieved", "peak", "unit", "frac", "avg_us")},
                                    "k_raster_avg_us": j["kernels"]["k_raster"]["avg_us"]}
            except Exception as e:
                out["frames_4k"] = {"error": repr(e)}
        if args.full and world == 1 and not use_dist and not emu and (W, H) == (7680, 4320) and not args.no_4k and not args.shadows and not tiled:
            # BASELINE config 5 on one GPU: the same frame lit by 1 sun + 1023 point lights through the tiled pass (child process)
            try:
                import subprocess
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--lights", "1024", "--steps", str(args.steps),
                                    "--warmup", str(args.warmup), "--full", "--no-cpu-baseline", "--no-4k"] + (["--fixed-camera"] if args.fixed_camera else []),
                                   capture_output=True, text=True, timeout=300)
                j = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
                pair_us = sum(j["kernels"][k]["avg_us"] for k in ("k_light_cull", "k_deferred_tiled") if k in j["kernels"])
                out["lights_1024"] = {"lights": 1024, "value": j["value"], "unit": j["unit"], "ms_per_step": j["ms_per_step"],
                                      "roofline": {"kernel": "k_light_cull + k_deferred_tiled", "bound": "hbm",
                                                   "achieved": round(DEFERRED_BYTES_PER_PX * W * H / (pair_us * 1e-6) / 1e9, 1) if pair_us else None,
                                                   "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                                   "frac": round(DEFERRED_BYTES_PER_PX * W * H / (pair_us * 1e-6) / 1e9 / HBM_PEAK_GBS, 4) if pair_us else None,
                                                   "avg_us": round(pair_us, 2)},
                                      "roofline_valu": j.get("roofline_valu"),
                                      "kernels": {k: j["kernels"][k]["avg_us"] for k in ("k_raster", "k_light_cull", "k_deferred_tiled") if k in j["kernels"]},
                                      "note": "not bandwidth-bound (SURVEY 7): 1.6 lights reach a covered pixel on average, ~85 instructions each"}
            except Exception as e:
                out["lights_1024"] = {"error": repr(e)}
        if args.full and world == 1 and not use_dist and not emu and (W, H) == (7680, 4320) and not args.no_4k and not args.shadows and not tiled and not args.fused:
            # row f1 (Renderer.cpp:333-372, :427): the same frame with the sun's terrain shadow map (2048^2, depth-only pass per frame)
            # and the 4x4 PCF term in the lighting pass (child process)
            try:
                import subprocess
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--shadows", "--steps", str(args.steps), "--warmup", str(args.warmup),
                                    "--full", "--no-cpu-baseline", "--no-4k"] + (["--fixed-camera"] if args.fixed_camera else []),
                                   capture_output=True, text=True, timeout=300)
                j = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
                out["shadows"] = {"value": j["value"], "unit": j["unit"], "ms_per_step": j["ms_per_step"],
                                  "sustained": (j.get("sustained") or {}).get("value"),
                                  "kernels": {k: v["avg_us"] for k, v in j["kernels"].items() if k in ("k_raster", "k_raster (depth only)", "k_deferred")},
                                  "note": "terrain shadow pass (depth only, 2048^2) + shadowed lighting pass (sixteen PCF taps per pixel) in every frame"}
            except Exception as e:
                out["shadows"] = {"error": repr(e)}
        if args.fused:
            out["config"]["workload"] += "; FUSED variant (vr_terrain_render_lit): lighting inside the tile pass, depth + HdrColor written (12 B/px)"
            out["roofline"] = None
            out["roofline_gbuffer_fill"] = None
            fk = "k_raster (fused with lighting)"
            if fk in timings:
                ms_f, n_f = timings[fk]
                out["roofline_fused"] = {"kernel": fk, "bound": "hbm", "bytes_per_pixel": 12, "achieved": round(12 * owned_px / (ms_f / n_f * 1e-3) / 1e9, 1),
                                         "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(12 * owned_px / (ms_f / n_f * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                                         "avg_us": round(ms_f / n_f * 1e3, 2),
                                         "note": "depth 4 B + HdrColor 8 B written per pixel, nothing read back; bound by the tile pass's own work, not by HBM"}
        if args.full and world == 1 and not use_dist and not emu and (W, H) == (7680, 4320) and not args.no_4k and not args.shadows and not tiled and not args.fused:
            # the opt-in fused variant on the same workload (child process): reported beside the graded path, never instead of it
            try:
                import subprocess
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--fused", "--steps", str(args.steps), "--warmup", str(args.warmup),
                                    "--full", "--no-cpu-baseline", "--no-4k", "--verify"] + (["--fixed-camera"] if args.fixed_camera else []),
                                   capture_output=True, text=True, timeout=300)
                j = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
                out["fused"] = {"what": "vr_terrain_render_lit (opt-in, SURVEY 7 step 6): TerrainPass::Render + DeferredLightingPass::Render in one pass over the pixels; "
                                        "HdrColor and depth bit-identical to the two passes (frame_verified_against_unfused), the other G-buffer planes not written",
                                "value": j["value"], "unit": j["unit"], "ms_per_step": j["ms_per_step"], "sustained": j.get("sustained"),
                                "roofline_fused": j.get("roofline_fused"), "frame_verified_against_unfused": j.get("frame_verified_against_unsplit"),
                                "kernels": {k: v["avg_us"] for k, v in j["kernels"].items() if k.startswith("k_raster")}}
            except Exception as e:
                out["fused"] = {"error": repr(e)}
        if args.full and world == 1 and not emu and not args.no_cpu_baseline:
            try:
                out["cpu_baseline"] = cpu_baseline(size, hm, al, params, (AMBIENT_TOP, AMBIENT_BOTTOM), camera)
                # the device counterpart of the reference's (disabled) heightmap update, for the same heightmap
                ctx.timing_enable(True)
                tp.SetHeight(True)
                th = ctx.timing_collect()
                tp.SetHeight(False)
                ctx.timing_enable(False)
                out["cpu_baseline"]["reference_cpu_side"]["device_set_height_minmax_us"] = round(
                    sum(ms for ms, _ in th.values()) * 1e3, 1)
            except Exception as e:  # the baseline is reported, never required for the GPU number
                out["cpu_baseline"] = {"error": repr(e)}
        print(json.dumps(out), flush=True)

    if use_dist:
        dist.barrier()
        if comm is not None:
            comm.close()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
