"""CPU tests of vr_terrain_occlusion's entry point: it is declared, mirrored and exported, its struct has the header's layout, and it
refuses bad arguments without a device.  (The definition against the model: tests/test_occlusion_model_cpu.py.)"""
import ctypes as C
import os
import re
import subprocess

from tests import occlusion_model as om
from vrenderer_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_occlusion_is_declared_mirrored_and_exported(product_lib, tmp_path):
    header = open(os.path.join(ROOT, "include", "vrterrain.h")).read()
    assert re.search(r"VR_API\s+int\s+vr_terrain_occlusion\s*\(\s*vr_terrain\*\s*t,\s*const vr_occlusion_params\*\s*p,\s*const vr_brush_dab\*\s*dabs,"
                     r"\s*uint32_t n,\s*int32_t out_rect\[4\]\)", header)
    assert re.search(r"#define\s+VR_OCCLUSION_MAX_REACH\s+64\b", header) and capi.VR_OCCLUSION_MAX_REACH == 64 == om.MAX_REACH
    assert re.search(r"#define\s+VR_OCCLUSION_TINT\s+0\b", header) and re.search(r"#define\s+VR_OCCLUSION_STORE\s+1\b", header)
    assert (capi.VR_OCCLUSION_TINT, capi.VR_OCCLUSION_STORE) == (om.TINT, om.STORE) == (0, 1)
    assert re.search(r"#define\s+VR_OCCLUSION_WHOLE_MAP\s+1u\b", header) and capi.VR_OCCLUSION_WHOLE_MAP == 1 == om.WHOLE_MAP
    assert C.sizeof(capi.OcclusionParams) == 64
    assert "vr_terrain_occlusion" in capi.EXPORTS and len(product_lib.vr_terrain_occlusion.argtypes) == 5
    # a call adds no kernel id: its kernel is untimed, like the brush's
    assert capi.VR_K_COUNT == 22 and product_lib.vr_timing_kernel_count() == 22
    hpp = open(os.path.join(ROOT, "include", "vrterrain.hpp")).read()
    assert "Occlusion(" in hpp and "vr_terrain_occlusion" in hpp
    # the ctypes size and offsets against the header's, and the declarations in C and in C++
    pf = [n for n, _ in capi.OcclusionParams._fields_]
    assert pf == ["radius", "max_height", "gain", "bias", "opacity", "color", "channel_mask", "directions", "mode", "flags", "reserved"]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include <vrterrain.h>\n'
                   'int (*occlusion_fn(void))(vr_terrain*, const vr_occlusion_params*, const vr_brush_dab*, uint32_t, int32_t*) { return vr_terrain_occlusion; }\n'
                   '#ifdef WITH_MAIN\nint main(void) { printf("%zu", sizeof(vr_occlusion_params));\n'
                   + "".join(f'printf(" %zu", offsetof(vr_occlusion_params, {n}));\n' for n in pf)
                   + 'printf(" %d %d %d %u\\n", (int)VR_OCCLUSION_MAX_REACH, (int)VR_OCCLUSION_TINT, (int)VR_OCCLUSION_STORE, VR_OCCLUSION_WHOLE_MAP); return 0; }\n#endif\n')
    inc = os.path.join(ROOT, "include")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", inc, "-c", str(src), "-o", str(tmp_path / "sizes.o")], check=True, capture_output=True, text=True)
    exe, lib_dir = str(tmp_path / "sizes"), os.path.join(ROOT, "vrenderer_amd", "lib")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-DWITH_MAIN", "-I", inc, str(src), "-o", exe, "-L", lib_dir, "-lvrterrain", f"-Wl,-rpath,{lib_dir}",
                    "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"], check=True, capture_output=True, text=True)
    got = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    want = ["64"] + [str(getattr(capi.OcclusionParams, n).offset) for n in pf] + ["64", "0", "1", "1"]
    assert got == want, got
    assert want[1:12] == ["0", "4", "8", "12", "16", "20", "36", "40", "44", "48", "52"]
    cpp = tmp_path / "occlusion.cpp"
    cpp.write_text('#include <cstddef>\n#include <vrterrain.hpp>\nbool occlusion(vRenderer::TerrainPass& tp, const vr_occlusion_params& p, const vr_brush_dab* d, int32_t r[4]) '
                   '{ return tp.Occlusion(p, d, 3, false, r) && tp.Occlusion(p, nullptr, 0, true); }\n'
                   'static_assert(sizeof(vr_occlusion_params) == 64 && offsetof(vr_occlusion_params, color) == 20 && offsetof(vr_occlusion_params, channel_mask) == 36 '
                   '&& offsetof(vr_occlusion_params, reserved) == 52, "vr_occlusion_params");\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", inc, "-c", str(cpp), "-o", str(tmp_path / "occlusion_cpp.o")], check=True, capture_output=True, text=True)


GOOD = dict(radius=8.0, max_height=12.5, gain=1.0, bias=0.0, opacity=1.0, color=(0.0, 0.0, 0.0, 255.0), channel_mask=7, directions=16, mode=0, flags=0,
            reserved=(0, 0, 0))


def test_refusals_answer_without_a_device(product_lib):
    """Every refusal of the header's list comes before any use of the device.  A handle that is no terrain is not written, and only the
    last refusal - the reach, which needs the maps' sizes - reads it: zeroed memory stands in for a terrain whose maps have no size, so
    a call good in everything else is refused there, as one with no step length at all."""
    lib = product_lib
    fake = C.create_string_buffer(1 << 20)                          # stands in for a terrain; a refused call does not write it
    nan, inf = float("nan"), float("inf")

    def call(t=True, p=True, dabs=True, n=1, d=(0.0, 0.0, 4.0, 0.5, 1.0), **kw):
        f = dict(GOOD, **kw)
        pp = capi.OcclusionParams(**{k: v for k, v in f.items() if k not in ("reserved", "color")})
        pp.color[:] = f["color"]
        pp.reserved[:] = f["reserved"]
        arr = (capi.BrushDab * max(n, 1))(*[capi.BrushDab(*d)] * max(n, 1))
        rect = (C.c_int32 * 4)(7, 7, 7, 7)
        rc = lib.vr_terrain_occlusion(C.cast(fake, C.c_void_p) if t else None, C.byref(pp) if p else None, arr if dabs else None, n, rect)
        assert tuple(rect) == (7, 7, 7, 7), kw
        return rc

    bad = [dict(t=False), dict(p=False), dict(dabs=False), dict(n=capi.VR_MAX_BRUSH_DABS + 1),
           dict(flags=2), dict(flags=3, dabs=False, n=0), dict(flags=0x80000000),
           dict(flags=1), dict(flags=1, n=0), dict(flags=1, dabs=False, n=1),                      # the flag together with dabs
           dict(reserved=(1, 0, 0)), dict(reserved=(0, 7, 0)), dict(reserved=(0, 0, 0x80000000)),
           dict(mode=2), dict(mode=0xFFFFFFFF),
           dict(directions=0), dict(directions=5), dict(directions=-4), dict(directions=12), dict(directions=32),
           dict(radius=0.0), dict(radius=-8.0), dict(max_height=0.0), dict(max_height=-12.5),
           dict(gain=-0.5), dict(gain=16.5), dict(bias=-0.125), dict(bias=8.0), dict(opacity=-0.01), dict(opacity=1.01),
           dict(color=(256.0, 0.0, 0.0, 0.0)), dict(color=(0.0, 0.0, 0.0, -1.0)),
           dict(channel_mask=0), dict(channel_mask=16),
           dict(d=(nan, 0.0, 4.0, 0.5, 1.0)), dict(d=(0.0, inf, 4.0, 0.5, 1.0)), dict(d=(0.0, 0.0, 0.0, 0.5, 1.0)), dict(d=(0.0, 0.0, -1.0, 0.5, 1.0)),
           dict(d=(0.0, 0.0, 4.0, 1.0, 1.0)), dict(d=(0.0, 0.0, 4.0, -0.1, 1.0)), dict(d=(0.0, 0.0, 4.0, 0.5, nan)),
           dict(d=(0.0, 0.0, 4.0, 0.5, 1.5)), dict(d=(0.0, 0.0, 4.0, 0.5, -0.1))]                  # strength is an opacity
    for field in ("radius", "max_height", "gain", "bias", "opacity"):
        bad += [{field: nan}, {field: inf}, {field: -inf}]
    for c in range(4):
        bad += [dict(color=tuple(v if k == c else 0.0 for k in range(4))) for v in (nan, inf)]
    dab_refusals = 0
    for kw in bad:
        assert call(**kw) == capi.VR_ERR_INVALID_ARGUMENT, kw
        msg = lib.vr_last_error().decode()
        if "d" in kw:
            dab_refusals += 1                                       # (the dab checks are the brush's own, and speak of the dab)
        else:
            assert "vr_terrain_occlusion" in msg and "MAX_REACH" not in msg, (kw, msg)
    assert dab_refusals == 9
    # the reach: the last refusal, behind every other
    for kw in (dict(), dict(flags=1, dabs=False, n=0), dict(n=0, dabs=False)):
        assert call(**kw) == capi.VR_ERR_INVALID_ARGUMENT, kw
        assert "vr_terrain_occlusion" in lib.vr_last_error().decode() and "VR_OCCLUSION_MAX_REACH" in lib.vr_last_error().decode()
    assert bytes(fake) == bytes(1 << 20)
