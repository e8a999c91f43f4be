"""The maps, frames and cameras of tests/test_packed_texels_gpu.py, and what each camera has to show - counted on the CPU from the
oracle's per-pixel plane (main_ps's implicit LOD before the sampler's clamp and the interpolated world x, z), so that a camera which
misses its case fails the test instead of passing it silently.

The fused tile pass addresses the albedo's packed footprint table with the offsets it forms for the height taps (pixel_shader_fast,
vr_raster.hip): the footprint's floor comes from the UNSHIFTED u, v of the pixel, the height taps from u +- 0.1, v +- 0.1, which leave
[0, 1] near the terrain's edges and land in the tables' clamp padding; a wave skips the second mip level where all of its pixels are
magnified; the coarser level is min(floor(lod) + 1, last level)."""
import numpy as np

import vrenderer_amd as vr
from tests.common import params

FRAMES = ((256, 144), (333, 211))          # whole tiles of both edges / partial edge tiles of both
OFFSET = 0.1                               # terrain_ps.hlsl:59

# Cameras by world size s (the terrain spans [-s / 2, s / 2]^2 and a texel is one world unit; the test's own maps keep the heights
# below 100 world units).  Chosen with the oracle; what each has to show is asserted from the oracle again when the test runs (CLAIMS).
CAMERAS = {
    # down on the terrain from beyond one corner: all four edges in view, so u +- 0.1 and v +- 0.1 leave [0, 1] on all four sides
    "corner and edges": lambda s: dict(eye=(0.62 * s, 700.0, 0.66 * s), target=(0.3 * s, 0.0, 0.3 * s)),
    # straight down from close by through a narrow lens: every pixel magnified, no wave takes the second level
    "near": lambda s: dict(eye=(0.1 * s, 100.0, -0.07 * s), target=(0.1 * s, 0.0, -0.07 * s), up=(0.0, 0.0, 1.0), vfov_deg=20.0),
    # straight down through a very wide lens: the whole terrain inside a few pixels, the implicit LOD at and beyond the last level,
    # where min(lf + 1, max_level) clamps.  (The quadtree's LOD ranges end a few world sizes out: the lens, not the distance.)
    "high and far": lambda s: dict(eye=(0.0, 100.0 + (s if s < 128 else 2.0 * s), 0.0), target=(0.0, 0.0, 0.0), up=(0.0, 0.0, 1.0), vfov_deg=176.0),
    # low over one edge towards the other: magnified in front, minified towards the far side - waves that hold both
    "grazing": lambda s: dict(eye=(-0.6 * s, 110.0, 0.1 * s), target=(0.5 * s, 0.0, 0.0)),
}

# What a camera has to show, as a predicate on facts(); None: the frame is compared all the same, without a claim.  The few pixels of
# "high and far" and the last magnified pixels of "near" depend on the frame's size: the claim names the frames it was chosen for.
def claim(name, size, w, h):
    if name == "corner and edges":
        return lambda f: min(f["u_lo"], f["u_hi"], f["v_lo"], f["v_hi"]) > 0
    if name == "near":
        return (lambda f: f["covered"] > 10000 and f["second_level"] == 0) if (size, (w, h)) != (64, (256, 144)) else None
    if name == "high and far":
        return (lambda f: f["last_level"] > 0) if (w, h) == (256, 144) else None
    if name == "grazing":
        return lambda f: f["mixed_steps_32"] > 0 and f["mixed_steps_64"] > 0
    raise KeyError(name)


def view(name, size, w, h):
    kw = dict(CAMERAS[name](float(size)))
    return vr.make_view(kw.pop("eye"), kw.pop("target"), w, h, **kw)


def maps(size_w, size_h=None, seed=3):
    """(heightmap (h, w), albedo (h, w, 4)): a gentle synthetic relief (heights below 100 world units, so that the cameras above see
    what they are meant to) under an albedo of random bytes - every sRGB8 code in every channel, neighbours unrelated, so that a
    footprint fetched from the wrong entry or a code decoded from the wrong field shows in the filtered colour."""
    from oracle import pyoracle as po
    size_h = size_w if size_h is None else size_h
    n = max(size_w, size_h)
    hm = (po.synth_heightmap(n)[:size_h, :size_w] // max(4, 1024 // n)).astype(np.uint8)     # (a texel is one world unit at either size)
    al = np.random.default_rng(seed).integers(0, 256, (size_h, size_w, 4), dtype=np.uint8)
    return np.ascontiguousarray(hm), al


def facts(po, ot, size, v, w, h, levels):
    """What one frame shows, from the oracle's render of it: covered pixels, the implicit LOD's range, pixels whose height taps leave
    [0, 1] on each of the four sides, pixels at or beyond the last level, and waves of the resolve (both tile edges) that hold
    magnified and minified pixels in one step."""
    gb = po.GBufferHost(w, h)
    plane = np.zeros((h, w, 3), np.float32)
    ot.render(v, gb, vr.default_render_params(400.0), debug_plane=plane)
    cov = gb.depth < 1.0
    lod, u, vv = plane[..., 0], (plane[..., 1] + size / 2) / size, (plane[..., 2] + size / 2) / size
    f = dict(covered=int(cov.sum()), lod_min=float(lod[cov].min()) if cov.any() else None, lod_max=float(lod[cov].max()) if cov.any() else None,
             u_hi=int((cov & (u + OFFSET > 1.0)).sum()), u_lo=int((cov & (u - OFFSET < 0.0)).sum()),
             v_hi=int((cov & (vv + OFFSET > 1.0)).sum()), v_lo=int((cov & (vv - OFFSET < 0.0)).sum()),
             last_level=int((cov & (lod >= levels - 1)).sum()), second_level=int((cov & (lod > 0.0)).sum()))
    mag, mini = cov & (lod <= 0.0), cov & (lod > 0.0)

    def mixed_steps(tile):
        # a wave's step: 32-pixel tiles - rows y and y + 4 of an 8-row region, 32 columns; 64-pixel tiles - one row of 64 columns
        n = 0
        for y0 in range(0, h, 8 if tile == 32 else 1):
            for x0 in range(0, w, tile):
                rows = [(y0 + k, y0 + k + 4) for k in range(4)] if tile == 32 else [(y0,)]
                for rr in rows:
                    rr = [r for r in rr if r < h]
                    if rr and mag[rr, x0:x0 + tile].any() and mini[rr, x0:x0 + tile].any():
                        n += 1
        return n
    f["mixed_steps_32"], f["mixed_steps_64"] = mixed_steps(32), mixed_steps(64)
    return f


def oracle_terrain(po, size, hm, al):
    return po.OracleTerrain(params(size), hm, al)
