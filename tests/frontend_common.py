"""Shared by tests/test_frontend_cpu.py and tests/test_frontend_f64.py: the textures, worlds, views and instances the front-end
tests use.  Everything is fixed here; the CPU tests verify, for the model alone and for the oracle, every condition the GPU
tests rely on (flagged shares, unambiguous views, real ties, morph classes, border samples)."""
import numpy as np

import vrenderer_amd as vr
from tests import f64_frontend as fe
from tests.common import CAMERAS, params, scaled_camera

MAX_HEIGHT = 400.0
VIEW_W, VIEW_H = 1920, 1080


def random_texture(w, h, seed):
    """Random bytes with random alpha; the seeds keep the flagged share of every sRGB level at or below 0.5 %."""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h, w, 4), dtype=np.uint8)


# (name, width, height, seed) of the random textures of the mip tests; the synthetic 256^2 pair is added by the tests
MIP_TEXTURES = [("129x129", 129, 129, 11), ("67x41", 67, 41, 12), ("64x1", 64, 1, 13), ("1x37", 1, 37, 14), ("256x64", 256, 64, 15)]
MIP_FLAG_CAP = 0.005
# (width, height) of the maps of tests/test_terrain_create_gpu.py: the smallest pair vr_terrain_create accepts, then odd sizes
# whose every level is ragged, sizes of which one side reaches one texel levels before the other, and 33 x 17.  Map k is the
# heightmap of case k and the albedo of case k - 1.  With CREATE_SEED no colour component of any level of any of them is
# flagged (tests/test_frontend_cpu.py), so their chains are the model's byte for byte.
CREATE_SHAPES = [(1, 1), (5, 5), (7, 2), (2, 7), (33, 17)]
CREATE_SEED = 100
CREATE_WORLD = 64


def check_chain(tp, name, rows, flag_cap=MIP_FLAG_CAP):
    """Every level of both chains of a device terrain against the model applied to the device's own previous level."""
    for which, srgb in (("height", False), ("albedo", True)):
        levels = tp.mip_levels(which)
        prev = tp.download_mip(which, 0)
        assert levels == fe.num_mip_levels(prev.shape[1], prev.shape[0]), (name, which, levels)
        flagged = 0.0
        for l in range(1, levels):
            got = tp.download_mip(which, l)
            r = fe.check_mip(prev, got, srgb)
            assert r["bad"] == 0, f"{name}: {which} level {l} ({got.shape[1]}x{got.shape[0]}): {r['bad']} components differ from the model"
            assert r["flagged"] <= flag_cap, (name, which, l, r["flagged"])
            flagged = max(flagged, r["flagged"])
            prev = got
        rows.append((f"{name} {which}", f"{levels} levels equal; largest flagged share {flagged:.5f}"))


def ragged_heightmap():
    """200 x 200 random bytes with two plateaus (flat nodes take the `max == min -> min = 0` branch) on a 256 world: the
    texel size 200 / 256 is no integer, so footprints overlap and no kernel of the dyadic path applies."""
    rng = np.random.default_rng(2001)
    t = rng.integers(0, 256, (200, 200), dtype=np.uint8)
    t[0:50, 0:75] = 77
    t[120:200, 100:200] = (t[120:200, 100:200] // 16) + 180
    return t


def world200_heightmap():
    """420 x 300 random bytes on a 200 world: texel sizes 2.1 and 1.5 - 2.1 is no fp32 number, footprint bounds round."""
    return np.random.default_rng(2002).integers(0, 256, (300, 420), dtype=np.uint8)


def world_params(surface, world):
    p = params(surface)
    p.world_size = float(world)
    return p


def make_view(eye, tgt, w=VIEW_W, h=VIEW_H):
    return vr.make_view(tuple(float(c) for c in eye), tuple(float(c) for c in tgt), w, h)


# ---- select views ------------------------------------------------------------------------------------------------------
# Ties on the 256 world (lod ranges 4 2^i, nodes of lod L are 2^L wide and aligned to multiples of 2^L).  Every coordinate of a
# tie position is a multiple of 2^-4 with at most 12 significant bits and node edges are integers below 2^8: position - edge
# is exact and has at most 12 bits, its square at most 24 - every product and the sum dx^2 + 0 in the decision are exact in
# fp32 by construction, so `<=` against r^2 = 2^(2 i + 4) is decided on an exact equality.  z = 4.5 lies inside the rows of
# nodes [0, 2^L], so the distance is dx alone: x = 16 is exactly r_2 from the edge x = 0 (and r_3 = 32 from x = -16, ...), x =
# 48 exactly r_2 from x = 32 and r_3 from x = 16.  A node of lod L at exactly r_(L-1) is a tie of the finer-range test
# (QuadTree.cpp:113: `<=` descends, `<` selects the node), its children at the same edge are ties of the first test (:82: `<=`
# goes on to the frustum test, `<` has the parent push the child unculled).
TIE_A = ((16.0, 40.0, 4.5), (-40.0, 0.0, 19.25))
TIE_B = ((48.0, 40.0, 4.5), (40.0, 0.0, 57.25))
# Without heights the cull box is y in [0, camera.y] (QuadTree.cpp:92-96) and the top and bottom planes of a roll-free
# camera contain the horizontal line through the eye: with an eye on whole coordinates, box corners (x, camera.y, z) fall on
# that line and their plane test is a true zero evaluated with rounded planes.  The model finds cameras 1, 2 and 7 ambiguous
# for that reason in that mode; there they are replaced by the same cameras moved by (0.37, 0, 0.21).
_NUDGE = (0.37, 0.0, 0.21)


def _nudged(cam):
    return tuple(a + b for a, b in zip(cam[0], _NUDGE)), cam[1]


_CAMS_256 = [scaled_camera(c, 256) for c in CAMERAS]
_COMMON_256 = [
    ("far outside", ((2000.0, 100.0, 1500.0), (0.0, 0.0, 0.0))),
    ("below", ((10.0, -30.0, 5.0), (60.0, 0.0, 40.0))),
    ("on a node boundary", ((32.0, 450.0, -48.0), (-17.75, 200.0, 22.5))),
    ("tie A", TIE_A),
    ("tie B", TIE_B),
]
# mode (heights loaded or not) -> [(name, (eye, target))]
SELECT_VIEWS_256 = {
    False: [(f"camera {i}" + (" moved" if i in (1, 2, 7) else ""), _nudged(c) if i in (1, 2, 7) else c) for i, c in enumerate(_CAMS_256)] + _COMMON_256,
    True: [(f"camera {i}", c) for i, c in enumerate(_CAMS_256)] + _COMMON_256,
}
TIE_VIEWS = ("tie A", "tie B")
SELECT_VIEWS_2048 = [("camera 0", CAMERAS[0]), ("camera 3", CAMERAS[3])]        # the two of the eight without ambiguity in either mode


def light_view_of(shadow_view_fn, size=256):
    """The orthographic light view SetupForPlanarViewStable gives for the reference sun and camera 0 of the `size` world."""
    eye, tgt = scaled_camera(CAMERAS[0], size)
    cam = make_view(eye, tgt, 640, 360)
    return shadow_view_fn(vr.reference_sun(), cam, vr.default_shadow_params(float(size), resolution=512))


# ---- vertex cases ------------------------------------------------------------------------------------------------------
def chosen_instances(fields, eye, ranges):
    """The five instances test_vertex_stage_bit_exact picks: the nearest, one in the morph band, the coarsest, first, last."""
    ext, pos = fields[:, 0], fields[:, [3, 5]]
    dist = np.hypot(pos[:, 0] - eye[0], pos[:, 1] - eye[2])
    lod = np.clip(np.floor(np.log2(2.0 * ext)).astype(int), 0, 11)
    band = np.abs(dist - 0.925 * np.asarray(ranges)[lod]) - ext
    return sorted({int(np.argmin(dist)), int(np.argmin(band)), int(np.argmax(ext)), len(ext) - 1, 0})


VERTEX_CASES = ["2048 camera 0", "256 grazing", "two surfaces", "256 light view"]


def vertex_case_view(name, shadow_view_fn):
    """(world size, view) of a vertex case; the terrain is the synthetic one of that world size (surface 256 for two surfaces)."""
    if name == "2048 camera 0":
        return 2048, make_view(*CAMERAS[0], 960, 540)
    if name == "256 grazing":
        return 256, make_view(*scaled_camera(CAMERAS[6], 256), 960, 540)
    if name == "two surfaces":
        return 512, make_view(*scaled_camera(CAMERAS[1], 512), 960, 540)
    return 256, light_view_of(shadow_view_fn, 256)


def morph_classes(models):
    """Counts over a list of main_vs results: vertices that can move (odd grid index) with 0 < morphK < 1, with morphK = 1,
    with morphK = 0, and vertices that sample the clamp border at uv = 0 / uv = 1."""
    c = dict(partial=0, full=0, none=0, uv0=0, uv1=0)
    for m in models:
        k, odd = m["morph"], m["odd"]
        c["partial"] += int((odd & (k > 0) & (k < 1)).sum()); c["full"] += int((odd & (k == 1)).sum()); c["none"] += int((odd & (k == 0)).sum())
        c["uv0"] += int((m["uv"] == 0.0).any(1).sum()); c["uv1"] += int((m["uv"] == 1.0).any(1).sum())
    return c


def report(title, rows):
    """Prints a small table of worst error / bound ratios (read it with -rA or -s)."""
    print(f"\n{title}")
    for name, val in rows:
        print(f"  {name:<44} {val}")
