"""CPU tests of vr_terrain_path's entry point: it is declared, mirrored and exported, its structs have the header's layout, and it
refuses bad arguments without a device.  (The definition against the model: tests/test_path_model_cpu.py.)"""
import ctypes as C
import os
import re
import subprocess

from tests import path_model as pm
from vrenderer_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_path_is_declared_mirrored_and_exported(product_lib, tmp_path):
    header = open(os.path.join(ROOT, "include", "vrterrain.h")).read()
    assert re.search(r"VR_API\s+int\s+vr_terrain_path\s*\(\s*vr_terrain\*\s*t,\s*int which,\s*const vr_path_params\*\s*p,"
                     r"\s*const vr_path_point\*\s*points,\s*uint32_t n,\s*int32_t out_rect\[4\]\)", header)
    assert re.search(r"#define\s+VR_MAX_PATH_POINTS\s+4096\b", header) and capi.VR_MAX_PATH_POINTS == 4096 == pm.MAX_POINTS
    assert capi.VR_MAX_PATH_POINTS <= capi.VR_MAX_BRUSH_DABS                  # a closed path's segments fit the brush's list buffers
    assert re.search(r"VR_PATH_LEVEL = 0, VR_PATH_CUT = 1, VR_PATH_FILL = 2, VR_PATH_PAINT = 3\b", header)
    assert (capi.VR_PATH_LEVEL, capi.VR_PATH_CUT, capi.VR_PATH_FILL, capi.VR_PATH_PAINT) == (pm.LEVEL, pm.CUT, pm.FILL, pm.PAINT) == (0, 1, 2, 3)
    assert re.search(r"VR_PATH_CLOSED = 1\b", header) and capi.VR_PATH_CLOSED == 1 == pm.CLOSED
    assert C.sizeof(capi.PathPoint) == 16 and C.sizeof(capi.PathParams) == 64
    assert "vr_terrain_path" in capi.EXPORTS and len(product_lib.vr_terrain_path.argtypes) == 6
    # a call adds no kernel id: its kernel is untimed, like the brush's
    assert capi.VR_K_COUNT == 22 and product_lib.vr_timing_kernel_count() == 22
    hpp = open(os.path.join(ROOT, "include", "vrterrain.hpp")).read()
    assert "Path(" in hpp and "vr_terrain_path" in hpp
    for lists in re.findall(r"vr_terrain_edit[^\n]*_texture[^\n]*", header):          # the history paragraph's lists, and the stream's
        assert "_path" in lists, lists
    for word in ("width per point", "splines", "vr_terrain_query_heights", "both maps in one call"):       # what the header says is out of scope
        assert word in header, word
    # the ctypes sizes and offsets against the header's, and the declarations in C and in C++
    pf, qf = [n for n, _ in capi.PathParams._fields_], [n for n, _ in capi.PathPoint._fields_]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include <vrterrain.h>\n'
                   'int (*path_fn(void))(vr_terrain*, int, const vr_path_params*, const vr_path_point*, uint32_t, int32_t*) { return vr_terrain_path; }\n'
                   '#ifdef WITH_MAIN\nint main(void) { printf("%zu %zu", sizeof(vr_path_params), sizeof(vr_path_point));\n'
                   + "".join(f'printf(" %zu", offsetof(vr_path_params, {n}));\n' for n in pf)
                   + "".join(f'printf(" %zu", offsetof(vr_path_point, {n}));\n' for n in qf)
                   + 'printf(" %d %d\\n", (int)VR_MAX_PATH_POINTS, (int)VR_PATH_CLOSED); return 0; }\n#endif\n')
    inc = os.path.join(ROOT, "include")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", inc, "-c", str(src), "-o", str(tmp_path / "sizes.o")], check=True, capture_output=True, text=True)
    exe, lib_dir = str(tmp_path / "sizes"), os.path.join(ROOT, "vrenderer_amd", "lib")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-DWITH_MAIN", "-I", inc, str(src), "-o", exe, "-L", lib_dir, "-lvrterrain", f"-Wl,-rpath,{lib_dir}",
                    "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"], check=True, capture_output=True, text=True)
    got = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    want = ["64", "16"] + [str(getattr(capi.PathParams, n).offset) for n in pf] + [str(getattr(capi.PathPoint, n).offset) for n in qf] + ["4096", "1"]
    assert got == want, got
    cpp = tmp_path / "path.cpp"
    cpp.write_text('#include <vrterrain.hpp>\nbool path(vRenderer::TerrainPass& tp, const vr_path_params& p, const vr_path_point* q, int32_t r[4]) '
                   '{ return tp.Path(0, p, q, 5, false, r) && tp.Path(1, p, q, 5, true); }\n'
                   'static_assert(sizeof(vr_path_params) == 64 && sizeof(vr_path_point) == 16, "vr_path_params / vr_path_point");\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", inc, "-c", str(cpp), "-o", str(tmp_path / "path_cpp.o")], check=True, capture_output=True, text=True)


GOOD = dict(op=0, channel_mask=1, radius=4.0, hardness=0.5, opacity=0.8, color=(10.0, 20.0, 30.0, 40.0), flags=0, reserved=(0,) * 6)


def test_refusals_answer_without_a_device(product_lib):
    """Every refusal of the header's list comes before any use of the device: a handle that is no terrain is never looked into, and
    out_rect - which the siblings zero only past the last argument refusal - keeps what it held."""
    lib = product_lib
    fake = C.create_string_buffer(1 << 16)                          # stands in for a terrain; a refused call does not read it
    nan, inf = float("nan"), float("inf")

    def call(t=True, p=True, which=0, points=True, n=3, pt=(1.0, 2.0, 100.0, 0.0), bad_at=None, **kw):
        f = dict(GOOD, **kw)
        pp = capi.PathParams(**{k: v for k, v in f.items() if k not in ("reserved", "color")})
        pp.color[:] = f["color"]
        pp.reserved[:] = f["reserved"]
        arr = (capi.PathPoint * max(n, 1))(*[capi.PathPoint(0.5 * i, -0.25 * i, 50.0, 0.0) for i in range(max(n, 1))])
        arr[(max(n, 1) - 1) if bad_at is None else bad_at] = capi.PathPoint(*pt)
        rect = (C.c_int32 * 4)(7, 7, 7, 7)
        rc = lib.vr_terrain_path(C.cast(fake, C.c_void_p) if t else None, which, C.byref(pp) if p else None, arr if points else None, n, rect)
        assert tuple(rect) == (7, 7, 7, 7), kw
        return rc

    bad = [dict(t=False), dict(p=False), dict(points=False), dict(points=False, n=1), dict(n=capi.VR_MAX_PATH_POINTS + 1),
           dict(which=2), dict(which=-1),
           dict(op=4), dict(op=-1), dict(op=3), dict(op=3, channel_mask=5),                        # PAINT on the heightmap
           dict(which=1, op=0, channel_mask=1), dict(which=1, op=1), dict(which=1, op=2),          # LEVEL, CUT, FILL on the albedo
           dict(flags=2), dict(flags=3), dict(flags=0x80000000),
           dict(flags=1, n=2), dict(flags=1, n=1), dict(flags=1, n=0), dict(flags=1, n=0, points=False),       # CLOSED needs three points
           dict(radius=0.0), dict(radius=-1.0), dict(hardness=1.0), dict(hardness=-0.01), dict(opacity=-0.01), dict(opacity=1.01),
           dict(color=(256.0, 0.0, 0.0, 0.0)), dict(color=(0.0, 0.0, 0.0, -1.0)), dict(which=1, op=3, channel_mask=15, color=(0.0, 300.0, 0.0, 0.0)),
           dict(channel_mask=0), dict(channel_mask=16), dict(channel_mask=2), dict(channel_mask=15),      # the heightmap has the one channel
           dict(which=1, op=3, channel_mask=0), dict(which=1, op=3, channel_mask=16),
           dict(pt=(nan, 0.0, 1.0, 0.0)), dict(pt=(0.0, inf, 1.0, 0.0)), dict(pt=(0.0, 0.0, nan, 0.0)), dict(pt=(0.0, 0.0, -inf, 0.0)),
           dict(pt=(0.0, 0.0, 1.0, nan)), dict(pt=(0.0, 0.0, 1.0, 1.0)),                            # a point's reserved word
           dict(pt=(0.0, 0.0, -0.5, 0.0)), dict(pt=(0.0, 0.0, 255.5, 0.0)), dict(pt=(0.0, 0.0, 255.5, 0.0), bad_at=0),
           dict(which=1, op=3, channel_mask=15, pt=(0.0, 0.0, 256.0, 0.0))]                         # PAINT ignores heights but takes no bad ones
    for i in range(6):
        bad.append(dict(reserved=tuple(1 if k == i else 0 for k in range(6))))
    for field in ("radius", "hardness", "opacity"):
        bad += [{field: nan}, {field: inf}, {field: -inf}]
    for c in range(4):
        bad += [dict(color=tuple(v if k == c else 0.0 for k in range(4))) for v in (nan, inf)]
    for kw in bad:
        assert call(**kw) == capi.VR_ERR_INVALID_ARGUMENT, kw
    assert bytes(fake) == bytes(1 << 16)
