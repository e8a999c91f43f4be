"""CPU test of the terrain's surface constants (vrenderer_amd/csrc/vr_terrain_surface.h) through tests/host/terrain_surface_check.cpp."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_terrain_surface_constants_and_the_facts_the_folds_rest_on(tmp_path):
    """vr_terrain_surface.h compiles without HIP (its static_asserts hold for the host compiler too).  The constants equal
    decode_surface's generic expressions evaluated in float at run time; the normal decode's fmaxf(., -1) is an identity for all
    65,535 codes in [-32767, 32767]; x * 0 + 1 == 1, separately rounded and fused, over a dense sweep of [0, 1] with both
    endpoints, the denormals and the last floats below 1."""
    exe = os.path.join(str(tmp_path), "terrain_surface_check")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off", "-I", os.path.join(ROOT, "vrenderer_amd", "csrc"),
           os.path.join(ROOT, "tests", "host", "terrain_surface_check.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
    m = re.search(r"(\d+) cases", r.stdout)
    assert m and int(m.group(1)) == 11, r.stdout[-400:]           # 7 on the constants, 3 on the normal decode, 1 on the sweep
