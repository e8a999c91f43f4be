"""CPU tests of vr_terrain_region's entry point: it is declared, mirrored and exported, its structs have the header's layout, and it
refuses bad arguments without a device.  (The definition against the model: tests/test_region_model_cpu.py.)"""
import ctypes as C
import os
import re
import subprocess

from tests import region_model as rm
from vrenderer_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_region_is_declared_mirrored_and_exported(product_lib, tmp_path):
    header = open(os.path.join(ROOT, "include", "vrterrain.h")).read()
    assert re.search(r"VR_API\s+int\s+vr_terrain_region\s*\(\s*vr_terrain\*\s*t,\s*int which,\s*const vr_region_params\*\s*p,"
                     r"\s*const vr_region_point\*\s*points,\s*uint32_t n,\s*const uint32_t\*\s*contour_counts,\s*uint32_t num_contours,\s*int32_t out_rect\[4\]\)", header)
    assert re.search(r"#define\s+VR_MAX_REGION_POINTS\s+4096\b", header) and capi.VR_MAX_REGION_POINTS == 4096 == rm.MAX_POINTS
    assert capi.VR_MAX_REGION_POINTS <= capi.VR_MAX_BRUSH_DABS               # a contour has as many edges as points: they fit the brush's list buffers
    assert re.search(r"VR_REGION_LEVEL = 0, VR_REGION_CUT = 1, VR_REGION_FILL = 2, VR_REGION_RAISE = 3, VR_REGION_PAINT = 4\b", header)
    assert (capi.VR_REGION_LEVEL, capi.VR_REGION_CUT, capi.VR_REGION_FILL, capi.VR_REGION_RAISE, capi.VR_REGION_PAINT) == \
        (rm.LEVEL, rm.CUT, rm.FILL, rm.RAISE, rm.PAINT) == (0, 1, 2, 3, 4)
    assert re.search(r"VR_REGION_FEATHER_INSIDE = 1\b", header) and capi.VR_REGION_FEATHER_INSIDE == 1 == rm.FEATHER_INSIDE
    assert C.sizeof(capi.RegionPoint) == 8 and C.sizeof(capi.RegionParams) == 64
    assert "vr_terrain_region" in capi.EXPORTS and len(product_lib.vr_terrain_region.argtypes) == 8
    # a call adds no kernel id: its kernel is untimed, like the brush's
    assert capi.VR_K_COUNT == 22 and product_lib.vr_timing_kernel_count() == 22
    hpp = open(os.path.join(ROOT, "include", "vrterrain.hpp")).read()
    assert "Region(" in hpp and "vr_terrain_region" in hpp
    for word in ("sloped target plane", "per-vertex heights", "non-zero winding", "curves", "both maps in one call"):       # what the header says is out of scope
        assert word in header, word
    # the ctypes sizes and offsets against the header's, and the declarations in C and in C++
    pf, qf = [n for n, _ in capi.RegionParams._fields_], [n for n, _ in capi.RegionPoint._fields_]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include <vrterrain.h>\n'
                   'int (*region_fn(void))(vr_terrain*, int, const vr_region_params*, const vr_region_point*, uint32_t, const uint32_t*, uint32_t, int32_t*) '
                   '{ return vr_terrain_region; }\n'
                   '#ifdef WITH_MAIN\nint main(void) { printf("%zu %zu", sizeof(vr_region_params), sizeof(vr_region_point));\n'
                   + "".join(f'printf(" %zu", offsetof(vr_region_params, {n}));\n' for n in pf)
                   + "".join(f'printf(" %zu", offsetof(vr_region_point, {n}));\n' for n in qf)
                   + 'printf(" %d %d\\n", (int)VR_MAX_REGION_POINTS, (int)VR_REGION_FEATHER_INSIDE); return 0; }\n#endif\n')
    inc = os.path.join(ROOT, "include")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", inc, "-c", str(src), "-o", str(tmp_path / "sizes.o")], check=True, capture_output=True, text=True)
    exe, lib_dir = str(tmp_path / "sizes"), os.path.join(ROOT, "vrenderer_amd", "lib")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-DWITH_MAIN", "-I", inc, str(src), "-o", exe, "-L", lib_dir, "-lvrterrain", f"-Wl,-rpath,{lib_dir}",
                    "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"], check=True, capture_output=True, text=True)
    got = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    want = ["64", "8"] + [str(getattr(capi.RegionParams, n).offset) for n in pf] + [str(getattr(capi.RegionPoint, n).offset) for n in qf] + ["4096", "1"]
    assert got == want, got
    cpp = tmp_path / "region.cpp"
    cpp.write_text('#include <vrterrain.hpp>\nbool region(vRenderer::TerrainPass& tp, const vr_region_params& p, const vr_region_point* q, const uint32_t* c, int32_t r[4]) '
                   '{ return tp.Region(0, p, q, 8, c, 2, r) && tp.Region(1, p, q, 5); }\n'
                   'static_assert(sizeof(vr_region_params) == 64 && sizeof(vr_region_point) == 8, "vr_region_params / vr_region_point");\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", inc, "-c", str(cpp), "-o", str(tmp_path / "region_cpp.o")], check=True, capture_output=True, text=True)


GOOD = dict(op=0, channel_mask=1, target=100.0, feather=3.0, opacity=0.8, color=(10.0, 20.0, 30.0, 40.0), flags=0, reserved=(0,) * 6)


def test_refusals_answer_without_a_device(product_lib):
    """Every refusal of the header's list comes before any use of the device: a handle that is no terrain is never looked into, and
    out_rect - which the siblings zero only past the last argument refusal - keeps what it held."""
    lib = product_lib
    fake = C.create_string_buffer(1 << 16)                          # stands in for a terrain; a refused call does not read it
    nan, inf = float("nan"), float("inf")

    def call(t=True, p=True, which=0, points=True, n=6, pt=(1.0, 2.0), bad_at=None, counts=None, num_contours=None, **kw):
        f = dict(GOOD, **kw)
        pp = capi.RegionParams(**{k: v for k, v in f.items() if k not in ("reserved", "color")})
        pp.color[:] = f["color"]
        pp.reserved[:] = f["reserved"]
        arr = (capi.RegionPoint * max(n, 1))(*[capi.RegionPoint(0.5 * i, -0.25 * i * i) for i in range(max(n, 1))])
        arr[(max(n, 1) - 1) if bad_at is None else bad_at] = capi.RegionPoint(*pt)
        cc = (C.c_uint32 * len(counts))(*counts) if counts else None
        nc = num_contours if num_contours is not None else (len(counts) if counts else 0)
        rect = (C.c_int32 * 4)(7, 7, 7, 7)
        rc = lib.vr_terrain_region(C.cast(fake, C.c_void_p) if t else None, which, C.byref(pp) if p else None, arr if points else None, n, cc, nc, rect)
        assert tuple(rect) == (7, 7, 7, 7), kw
        return rc

    bad = [dict(t=False), dict(p=False), dict(points=False), dict(points=False, n=3), dict(n=capi.VR_MAX_REGION_POINTS + 1),
           dict(which=2), dict(which=-1),
           dict(op=5), dict(op=-1), dict(op=4), dict(op=4, channel_mask=5),                        # PAINT on the heightmap
           dict(which=1, op=0, channel_mask=1), dict(which=1, op=1), dict(which=1, op=2), dict(which=1, op=3),     # the height ops on the albedo
           dict(flags=2), dict(flags=3), dict(flags=0x80000000), dict(flags=0x100),
           dict(counts=(4, 2)), dict(counts=(2, 4)), dict(counts=(3, 2, 1)), dict(counts=(3,)), dict(counts=(3, 4)), dict(counts=(6, 3)),
           dict(num_contours=1), dict(num_contours=2),                                             # counts missing
           dict(n=1), dict(n=2), dict(n=2, counts=(2,)), dict(n=0, counts=(3,)),
           dict(feather=-0.5), dict(opacity=-0.01), dict(opacity=1.01),
           dict(target=-0.5), dict(target=255.5), dict(op=3, target=-255.5), dict(op=3, target=256.0),
           dict(color=(256.0, 0.0, 0.0, 0.0)), dict(color=(0.0, 0.0, 0.0, -1.0)), dict(which=1, op=4, channel_mask=15, color=(0.0, 300.0, 0.0, 0.0)),
           dict(channel_mask=0), dict(channel_mask=16), dict(channel_mask=2), dict(channel_mask=15),      # the heightmap has the one channel
           dict(which=1, op=4, channel_mask=0), dict(which=1, op=4, channel_mask=16),
           dict(pt=(nan, 0.0)), dict(pt=(0.0, inf)), dict(pt=(-inf, 0.0)), dict(pt=(0.0, nan), bad_at=0)]
    for i in range(6):
        bad.append(dict(reserved=tuple(1 if k == i else 0 for k in range(6))))
    for field in ("target", "feather", "opacity"):
        bad += [{field: nan}, {field: inf}, {field: -inf}]
    for c in range(4):
        bad += [dict(color=tuple(v if k == c else 0.0 for k in range(4))) for v in (nan, inf)]
    for kw in bad:
        assert call(**kw) == capi.VR_ERR_INVALID_ARGUMENT, kw
    assert bytes(fake) == bytes(1 << 16)
