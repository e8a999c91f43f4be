"""CPU tests of vr_terrain_texture: the entry point is declared, mirrored and exported and refuses bad arguments without a device,
vr_texture.h's functions under g++ (tests/host/texture_check.cpp) keep their invariants and give the bytes of the numpy model
(tests/texture_model.py).  Every test here needs the entry point or the header.  (The model's own properties and the preconditions of
the GPU cases, which need neither, are tests/test_texture_model_cpu.py.)"""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from tests import texture_model as tm
from tests.host_check import build_host_check, run_host_check
from vrenderer_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORLD, MAX_HEIGHT = 64.0, 12.5
MAPS = (((1, 1), (1, 1)), ((8, 8), (8, 8)), ((17, 33), (33, 17)), ((33, 17), (48, 40)), ((64, 64), (16, 16)))        # (w0, h0), (wa, ha)
SETS = 200


def test_texture_is_declared_mirrored_and_exported(product_lib, tmp_path):
    header = open(os.path.join(ROOT, "include", "vrterrain.h")).read()
    assert re.search(r"VR_API\s+int\s+vr_terrain_texture\s*\(\s*vr_terrain\*\s*t,\s*const vr_texture_params\*\s*p,\s*const vr_texture_layer\*\s*layers,"
                     r"\s*const vr_brush_dab\*\s*dabs,\s*uint32_t n,\s*int32_t out_rect\[4\]\)", header)
    assert re.search(r"#define\s+VR_TEXTURE_MAX_LAYERS\s+8\b", header) and capi.VR_TEXTURE_MAX_LAYERS == 8
    assert re.search(r"VR_TEXTURE_WHOLE_MAP = 1\b", header) and capi.VR_TEXTURE_WHOLE_MAP == 1 == tm.WHOLE_MAP
    assert C.sizeof(capi.TextureLayer) == 64 and C.sizeof(capi.TextureParams) == 32
    assert "vr_terrain_texture" in capi.EXPORTS and len(product_lib.vr_terrain_texture.argtypes) == 6
    # a call adds no kernel id: its kernel is untimed, like the brush's
    assert capi.VR_K_COUNT == 22 and product_lib.vr_timing_kernel_count() == 22
    hpp = open(os.path.join(ROOT, "include", "vrterrain.hpp")).read()
    assert "Texture(" in hpp and "vr_terrain_texture" in hpp
    # the ctypes sizes against the header's, and the declarations in C and in C++
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include <vrterrain.h>\n'
                   'int (*texture_fn(void))(vr_terrain*, const vr_texture_params*, const vr_texture_layer*, const vr_brush_dab*, uint32_t, int32_t*) { return vr_terrain_texture; }\n'
                   '#ifdef WITH_MAIN\nint main(void) { '
                   'printf("%zu %zu %zu %zu %d %d\\n", sizeof(vr_texture_layer), sizeof(vr_texture_params), offsetof(vr_texture_layer, channel_mask), '
                   'offsetof(vr_texture_params, max_height), (int)VR_TEXTURE_MAX_LAYERS, (int)VR_TEXTURE_WHOLE_MAP); return 0; }\n#endif\n')
    inc = os.path.join(ROOT, "include")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", inc, "-c", str(src), "-o", str(tmp_path / "sizes.o")], check=True, capture_output=True, text=True)
    exe, lib_dir = str(tmp_path / "sizes"), os.path.join(ROOT, "vrenderer_amd", "lib")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-DWITH_MAIN", "-I", inc, str(src), "-o", exe, "-L", lib_dir, "-lvrterrain", f"-Wl,-rpath,{lib_dir}",
                    "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"], check=True, capture_output=True, text=True)
    got = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    assert got == ["64", "32", str(capi.TextureLayer.channel_mask.offset), str(capi.TextureParams.max_height.offset), "8", "1"], got
    cpp = tmp_path / "texture.cpp"
    cpp.write_text('#include <vrterrain.hpp>\nbool texture(vRenderer::TerrainPass& tp, const vr_texture_layer* l, const vr_brush_dab* d, int32_t r[4]) '
                   '{ return tp.Texture(l, 2, 400.0f, d, 1, false, r) && tp.Texture(l, 2, 400.0f, nullptr, 0, true); }\n'
                   'static_assert(sizeof(vr_texture_layer) == 64 && sizeof(vr_texture_params) == 32, "vr_texture_layer / vr_texture_params");\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(cpp), "-o", str(tmp_path / "texture_cpp.o")],
                   check=True, capture_output=True, text=True)


GOOD_LAYER = dict(color=(10.0, 20.0, 30.0, 40.0), opacity=0.5, alt_lo=1.0, alt_hi=5.0, alt_fade=1.0, slope_lo=10.0, slope_hi=40.0, slope_fade=5.0,
                  channel_mask=7, reserved=(0, 0, 0, 0))


def c_layer(**kw):
    f = dict(GOOD_LAYER, **kw)
    l = capi.TextureLayer(opacity=f["opacity"], alt_lo=f["alt_lo"], alt_hi=f["alt_hi"], alt_fade=f["alt_fade"], slope_lo=f["slope_lo"],
                          slope_hi=f["slope_hi"], slope_fade=f["slope_fade"], channel_mask=f["channel_mask"])
    l.color[:] = f["color"]
    l.reserved[:] = f["reserved"]
    return l


def test_refusals_answer_without_a_device(product_lib):
    """Every refusal of the header's list comes before any use of the device: a handle that is no terrain is never looked into."""
    lib = product_lib
    fake = C.create_string_buffer(1 << 16)                          # stands in for a terrain; a refused call does not read it
    nan, inf = float("nan"), float("inf")

    def call(t=True, p=True, layers=True, dabs=True, n=1, num_layers=2, flags=0, max_height=400.0, reserved=(0, 0, 0, 0, 0), d=(0.0, 0.0, 4.0, 0.5, 1.0),
             second=None):
        tp = capi.TextureParams(num_layers=num_layers, flags=flags, max_height=max_height)
        tp.reserved[:] = reserved
        ls = (capi.TextureLayer * 9)(*([c_layer(), c_layer(**(second or {}))] + [c_layer()] * 7))
        arr = (capi.BrushDab * max(n, 1))(*[capi.BrushDab(*d)] * max(n, 1))
        rect = (C.c_int32 * 4)()
        return lib.vr_terrain_texture(C.cast(fake, C.c_void_p) if t else None, C.byref(tp) if p else None, ls if layers else None, arr if dabs else None, n, rect)

    bad = [dict(t=False), dict(p=False), dict(layers=False), dict(dabs=False), dict(n=capi.VR_MAX_BRUSH_DABS + 1),
           dict(num_layers=0), dict(num_layers=-1), dict(num_layers=9),
           dict(flags=2), dict(flags=3, dabs=False, n=0), dict(flags=0x80000000),
           dict(flags=1), dict(flags=1, n=0), dict(flags=1, dabs=False, n=1),                      # the flag together with dabs
           dict(reserved=(0, 0, 0, 0, 1)), dict(reserved=(7, 0, 0, 0, 0)),
           dict(max_height=nan), dict(max_height=inf), dict(max_height=0.0), dict(max_height=-400.0)]
    for field in ("opacity", "alt_lo", "alt_hi", "alt_fade", "slope_lo", "slope_hi", "slope_fade"):
        bad += [dict(second={field: nan}), dict(second={field: inf}), dict(second={field: -inf})]
    bad += [dict(second=dict(color=(nan, 0.0, 0.0, 0.0))), dict(second=dict(color=(0.0, 0.0, 0.0, inf))),
            dict(second=dict(color=(-0.5, 0.0, 0.0, 0.0))), dict(second=dict(color=(0.0, 255.5, 0.0, 0.0))),
            dict(second=dict(opacity=-0.1)), dict(second=dict(opacity=1.1)),
            dict(second=dict(alt_lo=5.5, alt_hi=5.0)),
            dict(second=dict(alt_fade=-1.0)), dict(second=dict(slope_fade=-0.5)),
            dict(second=dict(slope_lo=-1.0)), dict(second=dict(slope_lo=41.0, slope_hi=40.0)), dict(second=dict(slope_hi=89.5)), dict(second=dict(slope_lo=90.0, slope_hi=95.0)),
            dict(second=dict(channel_mask=0)), dict(second=dict(channel_mask=16)),
            dict(second=dict(reserved=(0, 0, 0, 1))), dict(second=dict(reserved=(-1, 0, 0, 0))),
            dict(d=(nan, 0.0, 4.0, 0.5, 1.0)), dict(d=(0.0, inf, 4.0, 0.5, 1.0)), dict(d=(0.0, 0.0, 0.0, 0.5, 1.0)), dict(d=(0.0, 0.0, -1.0, 0.5, 1.0)),
            dict(d=(0.0, 0.0, 4.0, 1.0, 1.0)), dict(d=(0.0, 0.0, 4.0, -0.1, 1.0)), dict(d=(0.0, 0.0, 4.0, 0.5, nan)),
            dict(d=(0.0, 0.0, 4.0, 0.5, 1.5)), dict(d=(0.0, 0.0, 4.0, 0.5, -0.1))]                  # strength is an opacity
    for kw in bad:
        assert call(**kw) == capi.VR_ERR_INVALID_ARGUMENT, kw
    assert bytes(fake) == bytes(1 << 16)


@pytest.fixture(scope="module")
def texture_checks(tmp_path_factory):
    """The check program, and the same program under the address and undefined-behaviour sanitizers (stand-alone, nothing preloaded)."""
    d = tmp_path_factory.mktemp("texture")
    flags = ["-ffp-contract=off"]
    return (build_host_check(d, "texture_check", flags),
            build_host_check(d, "texture_check", flags + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "texture_check_san"))


def test_prepared_layers_keep_their_invariants(texture_checks):
    """vr_texture.h compiles without HIP.  20000 seeded layers: no prepared edge or reciprocal is an infinity or a NaN, every weight
    lies in [0, opacity], and a layer of weight 0 moves no byte."""
    for exe in texture_checks:
        r = run_host_check(exe, timeout=300, expect=" layers, 0 failures", stderr_tail=4000)
        assert "20000 layers" in r.stdout, r.stdout[-400:]


def seeded_layers(rng, h, deg, mh):
    """1 .. 8 layers about the heights (steps) and slopes (degrees) the map holds: hard edges, zero-width bands, opacity 0 and 1, single channels."""
    out = []
    for _ in range(int(rng.integers(1, 9))):
        kind = int(rng.integers(0, 8))
        a = np.sort(rng.choice(h.ravel(), 2).astype(np.float64) + rng.uniform(-3.0, 3.0, 2)) * mh / 255.0
        s = np.clip(np.sort(rng.choice(deg.ravel(), 2) + rng.uniform(-5.0, 5.0, 2)), 0.0, 89.0)
        if kind == 1:
            a[1] = a[0] = float(np.float32(rng.choice(h.ravel()))) * mh / 255.0          # a zero-width altitude band
        if kind == 2:
            s[1] = s[0]                                              # a zero-width slope band
        if kind == 3:
            s[0], s[1] = 0.0, 89.0
        alt_fade = 0.0 if kind in (0, 4) else float(rng.uniform(0.0, 0.2 * mh))
        slope_fade = 0.0 if kind in (0, 5) else float(rng.uniform(0.0, 30.0))
        opacity = (0.0, 1.0, 1.0)[int(rng.integers(0, 3))] if kind in (6, 7) else float(rng.uniform(0.0, 1.0))
        mask = 1 << int(rng.integers(0, 4)) if kind in (2, 7) else int(rng.integers(1, 16))
        lo, hi = np.float32(a[0]), np.float32(a[1])
        slo, shi = np.float32(s[0]), np.float32(s[1])
        out.append(tm.layer(rng.uniform(0.0, 255.0, 4), opacity, min(lo, hi), max(lo, hi), alt_fade, min(slo, shi), max(slo, shi), slope_fade, mask))
    return out


def _host_texture(exe, tmp_path, hm, al, sets):
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<5i2f", hm.shape[1], hm.shape[0], al.shape[1], al.shape[0], len(sets), WORLD, MAX_HEIGHT))
        f.write(np.ascontiguousarray(hm).tobytes())
        f.write(np.ascontiguousarray(al).tobytes())
        for layers in sets:
            f.write(struct.pack("<i", len(layers)))
            for l in layers:
                f.write(struct.pack("<11fI", *l["color"], l["opacity"], l["alt_lo"], l["alt_hi"], l["alt_fade"], l["slope_lo"], l["slope_hi"], l["slope_fade"],
                                    l["channel_mask"]))
    subprocess.run([exe, "apply", fin, fout], check=True, timeout=300)
    return np.fromfile(fout, np.uint8).reshape((len(sets),) + al.shape)


@pytest.mark.parametrize("maps", MAPS)
def test_header_on_the_host_gives_the_model_s_bytes(texture_checks, tmp_path, maps):
    """200 seeded layer sets on a random pair of maps under a mask of 1: the header's functions under g++ - plain and under the
    sanitizers - and the numpy model agree in every byte."""
    (w0, h0), (wa, ha) = maps
    rng = np.random.default_rng(1000 * w0 + 10 * h0 + wa)
    # smooth enough for the slopes to spread over the bands, rough enough for every byte to matter
    base = rng.integers(0, 256, (h0, w0)).astype(np.float64)
    hm = np.clip(0.5 * base + 0.5 * (np.add.outer(np.arange(h0) * 3.0, np.arange(w0) * 5.0) % 256), 0, 255).astype(np.uint8)
    al = rng.integers(0, 256, (ha, wa, 4), dtype=np.uint8)
    h, s2, _ = tm.sample(hm, al.shape, MAX_HEIGHT, WORLD)
    deg = np.degrees(np.arctan(np.sqrt(s2.astype(np.float64))))
    sets = [seeded_layers(rng, h, deg, MAX_HEIGHT) for _ in range(SETS)]
    want = np.stack([tm.texture(hm, al, layers, MAX_HEIGHT, WORLD, whole_map=True)[0] for layers in sets])
    changed = (want != al[None]).any(-1).reshape(SETS, -1).sum(1)
    assert (changed > 0).sum() >= SETS // 2, (changed > 0).sum()      # most sets change the map - a model of nothing would not do
    for exe in texture_checks:
        got = _host_texture(exe, tmp_path, hm, al, sets)
        bad = [k for k in range(SETS) if not np.array_equal(got[k], want[k])]
        assert not bad, f"sets {bad[:5]} differ; set {bad[0]}: {(got[bad[0]] != want[bad[0]]).sum()} bytes, first {np.argwhere(got[bad[0]] != want[bad[0]])[:4].tolist()}"
