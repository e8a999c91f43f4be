"""Shared scene definitions for the parity tests."""
import numpy as np

import vrenderer_amd as vr

from vrenderer_amd.scene import (AMBIENT_BOTTOM, AMBIENT_TOP, DEFAULT_EYE, DEFAULT_TARGET, flythrough_camera,  # noqa: F401
                                 params, scaled_camera)

# a handful of cameras: the reference default, the flythrough circle, low/grazing, inside terrain
CAMERAS = [
    (DEFAULT_EYE, DEFAULT_TARGET),
    ((600.0, 250.0, 0.0), (0.0, 0.0, 0.0)),
    ((0.0, 250.0, -600.0), (0.0, 0.0, 0.0)),
    ((-424.26, 250.0, 424.26), (0.0, 0.0, 0.0)),
    ((10.0, 900.0, 10.0), (0.0, 0.0, 1.0)),
    ((-300.0, 120.0, 80.0), (200.0, 60.0, -40.0)),
    ((50.0, 40.0, -20.0), (300.0, 80.0, 200.0)),
    ((900.0, 500.0, 900.0), (0.0, 0.0, 0.0)),
]


def upload_planes(gpu_ctx, planes):
    """A G-buffer of the planes' size with the five planes (dict name -> array) uploaded."""
    h, w = planes["depth"].shape
    rt = vr.RenderTargets(gpu_ctx).Init(w, h)
    for k, a in planes.items():
        rt.upload(k, a)
    return rt


def hdr_rgb(hdr, w, h):
    """An HdrImage's RGB as (h, w, 3) float64."""
    return hdr.download().view(np.float16).reshape(h, w, 4)[..., :3].astype(np.float64)


def packed_hdr(ctx, w, h, part):
    """An HdrImage that holds a rank's packed RGB16F tiles of a w x h frame (VR_OWNER_TILE pixels wide, as many rows as
    vr_partition_packed_bytes() needs), and the number of bytes of it that `part`'s own tiles occupy."""
    from vrenderer_amd.passes import partition_info
    info = partition_info(w, h, part.rank, part.world_size)
    rows = (info["packed_bytes"] + vr.VR_OWNER_TILE * 8 - 1) // (vr.VR_OWNER_TILE * 8)
    return vr.HdrImage(ctx, vr.VR_OWNER_TILE, rows), info["owned"] * 128 * 128 * 6


def packed_frame(gpu_ctx, w, h, world, render):
    """Each rank's packed tile-major output (vr_partition; render(buffer, partition) queues one rank's pass), de-tiled on the
    host into an (h, w, 3) image."""
    from vrenderer_amd import partition as pt
    from vrenderer_amd.passes import partition_info
    info = partition_info(w, h, 0, world)
    got = np.full((h, w, 3), np.nan)
    tx, _ = pt.owner_grid(w, h)
    for r in range(world):
        part = vr.Partition(r, world)
        buf, _ = packed_hdr(gpu_ctx, w, h, part)
        render(buf, part)
        packed = buf.download(info["packed_bytes"]).view(np.float16).reshape(-1, 128, 128, 3)
        for lt, tile in enumerate(pt.owned_tiles(w, h, r, world)):
            y0, x0 = (tile // tx) * 128, (tile % tx) * 128
            hh, ww = min(128, h - y0), min(128, w - x0)
            got[y0:y0 + hh, x0:x0 + ww] = packed[lt, :hh, :ww]
        buf.close()
    return got
