"""CPU tests of the stamps: the entry points are declared, mirrored and exported and refuse bad arguments without a device, and
vr_stamp.h's functions under g++ (tests/host/stamp_check.cpp) keep their invariants and give the constants, rectangles and bytes of
the numpy model (tests/stamp_model.py) on every case of tests/stamp_cases.py.  (The model's own properties and the preconditions of
the GPU cases are tests/test_stamp_model_cpu.py.)"""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from tests import stamp_cases as sc
from tests import stamp_model as sm
from tests.host_check import build_host_check, run_host_check
from vrenderer_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stamps_are_declared_mirrored_and_exported(product_lib, tmp_path):
    header = open(os.path.join(ROOT, "include", "vrterrain.h")).read()
    for pattern in (r"typedef struct vr_stamp vr_stamp;",
                    r"VR_API\s+int\s+vr_stamp_create\s*\(\s*vr_context\*\s*ctx,\s*int format,\s*int32_t w,\s*int32_t h,\s*const void\*\s*texels,\s*size_t row_pitch_bytes,"
                    r"\s*int device_pointer,\s*vr_stamp\*\*\s*out\)",
                    r"VR_API\s+int\s+vr_stamp_from_terrain\s*\(\s*vr_terrain\*\s*t,\s*int which,\s*int32_t x,\s*int32_t y,\s*int32_t w,\s*int32_t h,\s*vr_stamp\*\*\s*out\)",
                    r"VR_API\s+void\s+vr_stamp_destroy\s*\(\s*vr_stamp\*\s*stamp\)",
                    r"VR_API\s+int\s+vr_stamp_info\s*\(\s*const vr_stamp\*\s*stamp,\s*int32_t\*\s*format,\s*int32_t\*\s*w,\s*int32_t\*\s*h\)",
                    r"VR_API\s+int\s+vr_stamp_download\s*\(\s*vr_stamp\*\s*stamp,\s*void\*\s*host,\s*size_t bytes\)",
                    r"VR_API\s+int\s+vr_terrain_stamp\s*\(\s*vr_terrain\*\s*t,\s*int which,\s*vr_stamp\*\s*stamp,\s*const vr_stamp_params\*\s*params,\s*int32_t out_rect\[4\]\)",
                    r"VR_STAMP_R8 = 0, VR_STAMP_SRGBA8 = 1\b", r"VR_STAMP_BLEND = 0, VR_STAMP_ADD = 1, VR_STAMP_SUB = 2, VR_STAMP_MAX = 3, VR_STAMP_MIN = 4\b",
                    r"VR_STAMP_USE_ALPHA = 1\b"):
        assert re.search(pattern, header), pattern
    assert (capi.VR_STAMP_R8, capi.VR_STAMP_SRGBA8) == (0, 1) == (sm.R8, sm.SRGBA8)
    assert (capi.VR_STAMP_BLEND, capi.VR_STAMP_ADD, capi.VR_STAMP_SUB, capi.VR_STAMP_MAX, capi.VR_STAMP_MIN) == (0, 1, 2, 3, 4) == (sm.BLEND, sm.ADD, sm.SUB, sm.MAX, sm.MIN)
    assert capi.VR_STAMP_USE_ALPHA == 1 == sm.USE_ALPHA and C.sizeof(capi.StampParams) == 64
    for name, nargs in (("vr_stamp_create", 8), ("vr_stamp_from_terrain", 7), ("vr_stamp_destroy", 1), ("vr_stamp_info", 4), ("vr_stamp_download", 3),
                        ("vr_terrain_stamp", 5)):
        assert name in capi.EXPORTS and len(getattr(product_lib, name).argtypes) == nargs, name
    # the stamps add no kernel id: their kernels are untimed, like the brush's
    assert capi.VR_K_COUNT == 22 and product_lib.vr_timing_kernel_count() == 22
    assert re.search(r"vr_terrain_edit / _brush / _texture / _stamp / _erode", header)          # VR_OPT_GBUFFER_LAZY's list
    hpp = open(os.path.join(ROOT, "include", "vrterrain.hpp")).read()
    assert "class Stamp" in hpp and "vr_terrain_stamp" in hpp and "vr_stamp_from_terrain" in hpp
    # the ctypes sizes against the header's, and the declarations in C and in C++
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include <vrterrain.h>\n'
                   'int (*stamp_fn(void))(vr_terrain*, int, vr_stamp*, const vr_stamp_params*, int32_t*) { return vr_terrain_stamp; }\n'
                   'int (*create_fn(void))(vr_context*, int, int32_t, int32_t, const void*, size_t, int, vr_stamp**) { return vr_stamp_create; }\n'
                   '#ifdef WITH_MAIN\nint main(void) { '
                   'printf("%zu %zu %zu %zu %zu %d %d %d\\n", sizeof(vr_stamp_params), offsetof(vr_stamp_params, feather), offsetof(vr_stamp_params, op), '
                   'offsetof(vr_stamp_params, flags), offsetof(vr_stamp_params, reserved), (int)VR_STAMP_SRGBA8, (int)VR_STAMP_MIN, (int)VR_STAMP_USE_ALPHA); return 0; }\n#endif\n')
    inc = os.path.join(ROOT, "include")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", inc, "-c", str(src), "-o", str(tmp_path / "sizes.o")], check=True, capture_output=True, text=True)
    exe, lib_dir = str(tmp_path / "sizes"), os.path.join(ROOT, "vrenderer_amd", "lib")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-DWITH_MAIN", "-I", inc, str(src), "-o", exe, "-L", lib_dir, "-lvrterrain", f"-Wl,-rpath,{lib_dir}",
                    "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"], check=True, capture_output=True, text=True)
    got = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    P = capi.StampParams
    assert got == ["64", str(P.feather.offset), str(P.op.offset), str(P.flags.offset), str(P.reserved.offset), "1", "4", "1"], got
    cpp = tmp_path / "stamp.cpp"
    cpp.write_text('#include <vrterrain.hpp>\nbool stamp(vRenderer::Device& dev, vRenderer::TerrainPass& tp, const uint8_t* texels, int32_t r[4]) {\n'
                   '    vRenderer::Stamp a, b; vr_stamp_params p = {}; int32_t f, w, h;\n'
                   '    return a.Create(dev, VR_STAMP_R8, 5, 3, texels) && tp.CaptureStamp(0, 1, 2, 24, 16, b) && b.Info(f, w, h) && tp.Stamp(0, a, p, r) && tp.Stamp(0, b, p); }\n'
                   'static_assert(sizeof(vr_stamp_params) == 64, "vr_stamp_params");\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(cpp), "-o", str(tmp_path / "stamp_cpp.o")],
                   check=True, capture_output=True, text=True)


class FakeStamp(C.Structure):
    """What a refusal may look at of a vr_stamp (vr_stamp.hip: the context first, then format and size) - enough to stand in for one."""
    _fields_ = [("ctx", C.c_void_p), ("format", C.c_int32), ("w", C.c_int32), ("h", C.c_int32), ("rest", C.c_uint8 * 236)]


def test_refusals_answer_without_a_device(product_lib):
    """Every refusal of the header's list comes before any use of the device: handles that are no terrain, no stamp and no context -
    zeroed memory - are never used, and nothing is written but `out`."""
    lib = product_lib
    fake_t, fake_ctx = C.create_string_buffer(1 << 16), C.create_string_buffer(1 << 12)       # a zeroed terrain: no context, 0 x 0 maps
    texels = C.create_string_buffer(64 * 64 * 4)
    nan, inf = float("nan"), float("inf")
    tp, cp, xp = C.cast(fake_t, C.c_void_p), C.cast(fake_ctx, C.c_void_p), C.cast(texels, C.c_void_p)

    def create(ctx=cp, fmt=0, w=5, h=3, tex=xp, pitch=0, dev=0, out=True):
        o = C.c_void_p(0x1234)
        rc = lib.vr_stamp_create(ctx, fmt, w, h, tex, pitch, dev, C.byref(o) if out else None)
        assert not out or o.value is None
        return rc

    for kw in (dict(ctx=None), dict(out=False), dict(tex=None), dict(fmt=2), dict(fmt=-1), dict(w=0), dict(h=0), dict(w=4097), dict(h=4097), dict(w=-5),
               dict(pitch=4), dict(fmt=1, pitch=19), dict(fmt=1, dev=1, tex=C.c_void_p(xp.value + 2)), dict(fmt=1, dev=1, pitch=22)):
        assert create(**kw) == capi.VR_ERR_INVALID_ARGUMENT, kw

    def capture(t=tp, which=0, x=0, y=0, w=4, h=4, out=True):
        o = C.c_void_p(0x1234)
        rc = lib.vr_stamp_from_terrain(t, which, x, y, w, h, C.byref(o) if out else None)
        assert not out or o.value is None
        return rc

    # (the zeroed terrain's level 0 is 0 x 0: every rectangle lies outside it)
    for kw in (dict(t=None), dict(out=False), dict(which=2), dict(which=-1), dict(w=0), dict(h=0), dict(w=4097), dict(h=5000), dict(x=-1), dict(y=-1), dict(),
               dict(which=1), dict(x=2**31 - 1, w=4096)):
        assert capture(**kw) == capi.VR_ERR_INVALID_ARGUMENT, kw
    assert lib.vr_stamp_info(None, None, None, None) == capi.VR_ERR_INVALID_ARGUMENT
    assert lib.vr_stamp_download(None, xp, 64) == capi.VR_ERR_INVALID_ARGUMENT
    lib.vr_stamp_destroy(None)

    good = dict(x=1.0, z=2.0, size_x=8.0, size_z=6.0, rotation=0.5, opacity=0.5, feather=0.25, gain=1.0, offset=0.0, op=0, channel_mask=1, flags=0)

    def stamp(t=tp, which=0, st="r8", p=True, reserved=(0, 0, 0, 0), **kw):
        f = dict(good, **kw)
        sp = capi.StampParams(**f)
        sp.reserved[:] = reserved
        fs = FakeStamp(ctx=None, format={"r8": 0, "rgba": 1, "foreign": 0}.get(st, 0), w=5, h=3)
        if st == "foreign":
            fs.ctx = 0x1000                                          # another context than the zeroed terrain's (none); never followed
        before = bytes(fs)
        rect = (C.c_int32 * 4)(7, 7, 7, 7)
        rc = lib.vr_terrain_stamp(t, which, C.byref(fs) if st else None, C.byref(sp) if p else None, rect)
        assert bytes(fs) == before
        return rc

    bad = [dict(t=None), dict(st=None), dict(p=False), dict(which=2), dict(which=-1),
           dict(which=1, channel_mask=7), dict(which=0, st="rgba"),                   # a format that differs from `which`
           dict(st="foreign"),
           dict(size_x=0.0), dict(size_z=0.0), dict(size_x=-1.0), dict(size_z=-8.0),
           dict(opacity=-0.1), dict(opacity=1.1), dict(feather=-0.1), dict(feather=1.01),
           dict(gain=256.5), dict(gain=-257.0), dict(offset=255.5), dict(offset=-256.0),
           dict(op=5), dict(op=-1), dict(flags=2), dict(flags=3), dict(flags=0x80000000),
           dict(flags=1),                                                             # USE_ALPHA on R8
           dict(channel_mask=0), dict(channel_mask=16), dict(channel_mask=3),         # R8 requires 1
           dict(which=1, st="rgba", channel_mask=0), dict(which=1, st="rgba", channel_mask=16),
           dict(reserved=(0, 0, 0, 1)), dict(reserved=(-1, 0, 0, 0))]
    for field in ("x", "z", "size_x", "size_z", "rotation", "opacity", "feather", "gain", "offset"):
        bad += [{field: nan}, {field: inf}, {field: -inf}]
    for kw in bad:
        assert stamp(**kw) == capi.VR_ERR_INVALID_ARGUMENT, kw
    assert bytes(fake_t) == bytes(1 << 16) and bytes(fake_ctx) == bytes(1 << 12)


@pytest.fixture(scope="module")
def stamp_checks(tmp_path_factory):
    """The check program, and the same program under the address and undefined-behaviour sanitizers (stand-alone, nothing preloaded)."""
    d = tmp_path_factory.mktemp("stamp")
    flags = ["-ffp-contract=off"]
    return (build_host_check(d, "stamp_check", flags),
            build_host_check(d, "stamp_check", flags + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "stamp_check_san"))


def test_placements_keep_their_invariants(stamp_checks):
    """vr_stamp.h compiles without HIP.  200 seeded placements on maps of 1x1, 8x8, 17x33 and 48x40 with stamps of 1x1, 5x3, 33x17 and
    64x64, R8 and SRGBA8: no texel outside the rectangle changes, every covered texel lies inside it, every tap lies inside the
    stamp, no prepared constant is an infinity or a NaN."""
    for exe in stamp_checks:
        r = run_host_check(exe, timeout=300, expect=" cases, 0 failures", stderr_tail=4000)
        assert "6400 cases" in r.stdout, r.stdout[-400:]


def _host_stamp(exe, tmp_path, level0, calls, world):
    nc = 1 if level0.ndim == 2 else 4
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<4if", level0.shape[1], level0.shape[0], nc, len(calls), world))
        f.write(np.ascontiguousarray(level0).tobytes())
        for c in calls:
            p, st = c["params"], c["stamp"]
            f.write(struct.pack("<2i9fiII", st.shape[1], st.shape[0], p["x"], p["z"], p["size_x"], p["size_z"], p["rotation"], p["opacity"], p["feather"], p["gain"],
                                p["offset"], p["op"], p["channel_mask"], p["flags"]))
            f.write(np.ascontiguousarray(st).tobytes())
    subprocess.run([exe, "apply", fin, fout], check=True, timeout=300)
    raw, out, at = open(fout, "rb").read(), [], 0
    for _ in calls:
        consts = np.frombuffer(raw, np.float32, 8, at)
        rect = tuple(int(v) for v in np.frombuffer(raw, np.int32, 4, at + 32))
        out.append((consts, rect, np.frombuffer(raw, np.uint8, level0.size, at + 48).reshape(level0.shape)))
        at += 48 + level0.size
    assert at == len(raw)
    return out


@pytest.mark.parametrize("scene", sc.SCENES)
def test_header_on_the_host_gives_the_model_s_constants_rectangles_and_bytes(oracle, stamp_checks, tmp_path, scene):
    """Every case of tests/stamp_cases.py on the oracle's synthetic maps, each on the scene's original map: the header's preparation
    under g++ - plain and under the sanitizers - equals the model's in every constant (as bits) and rectangle, and the serial
    evaluator equals the model in every byte."""
    hm, al = sc.scene_maps(scene, oracle.synth_heightmap, oracle.synth_albedo)
    world = sc.WORLD[scene]
    miss = dict(name="miss", stamp=sc.stamp_texels(33, 17), params=sc.miss_params(scene, hm.shape))
    groups = ((hm, [c for k in range(len(sc.OPS)) for c in sc.op_sequence(scene, k, hm.shape)] + sc.variant_calls(scene, hm.shape) + [miss]),
              (al, sc.albedo_calls(scene, al.shape)))
    for level0, calls in groups:
        want = []
        for c in calls:
            k, rect = sm.prepare(c["params"], world, level0.shape, c["stamp"].shape)
            want.append((np.float32([k[n] for n in ("A00", "A01", "B0", "A10", "A11", "B1", "inv_u", "inv_v")]), rect, sm.stamp(level0, c["stamp"], c["params"], world)[0]))
        assert sum((w[2] != level0).any() for w in want) >= len(calls) - 1
        for exe in stamp_checks:
            got = _host_stamp(exe, tmp_path, level0, calls, world)
            for c, (gk, grect, gbytes), (wk, wrect, wbytes) in zip(calls, got, want):
                assert np.array_equal(gk.view(np.uint32), wk.view(np.uint32)), (scene, c["name"], gk.tolist(), wk.tolist())
                assert grect == tuple(wrect), (scene, c["name"], grect, wrect)
                assert np.array_equal(gbytes, wbytes), f"{scene}, {c['name']}: {(gbytes != wbytes).sum()} bytes differ, first {np.argwhere(gbytes != wbytes)[:4].tolist()}"
