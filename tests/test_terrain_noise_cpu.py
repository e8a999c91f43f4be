"""CPU tests of vr_terrain_noise: the entry point is declared, mirrored and exported and refuses bad arguments without a device,
vr_noise.h's functions under g++ (tests/host/noise_check.cpp) keep the ranges the header states and give the constants and bytes of
the numpy model (tests/noise_model.py).  Every test here needs the entry point or the header.  (The model's own properties and the
preconditions of the GPU cases, which need neither, are tests/test_noise_model_cpu.py.)"""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from tests import noise_model as nm
from tests.host_check import build_host_check, run_host_check
from vrenderer_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORLD = 64.0
MAPS = ((1, 1), (8, 8), (17, 33), (33, 17), (64, 64))                 # (w, h)


def test_noise_is_declared_mirrored_and_exported(product_lib, tmp_path):
    header = open(os.path.join(ROOT, "include", "vrterrain.h")).read()
    assert re.search(r"VR_API\s+int\s+vr_terrain_noise\s*\(\s*vr_terrain\*\s*t,\s*int which,\s*const vr_noise_params\*\s*p,"
                     r"\s*const vr_brush_dab\*\s*dabs,\s*uint32_t n,\s*int32_t out_rect\[4\]\)", header)
    assert re.search(r"#define\s+VR_NOISE_MAX_OCTAVES\s+12\b", header) and capi.VR_NOISE_MAX_OCTAVES == 12 == nm.MAX_OCTAVES
    assert re.search(r"VR_NOISE_VALUE = 0, VR_NOISE_GRADIENT = 1\b", header) and (capi.VR_NOISE_VALUE, capi.VR_NOISE_GRADIENT) == (nm.VALUE, nm.GRADIENT) == (0, 1)
    assert re.search(r"VR_NOISE_FBM = 0, VR_NOISE_BILLOW = 1, VR_NOISE_RIDGED = 2\b", header)
    assert (capi.VR_NOISE_FBM, capi.VR_NOISE_BILLOW, capi.VR_NOISE_RIDGED) == (nm.FBM, nm.BILLOW, nm.RIDGED) == (0, 1, 2)
    assert re.search(r"VR_NOISE_ADD = 0, VR_NOISE_BLEND = 1\b", header) and (capi.VR_NOISE_ADD, capi.VR_NOISE_BLEND) == (nm.ADD, nm.BLEND) == (0, 1)
    assert re.search(r"VR_NOISE_WHOLE_MAP = 1\b", header) and capi.VR_NOISE_WHOLE_MAP == 1 == nm.WHOLE_MAP
    assert C.sizeof(capi.NoiseParams) == 64
    assert "vr_terrain_noise" in capi.EXPORTS and len(product_lib.vr_terrain_noise.argtypes) == 6
    # a call adds no kernel id: its kernel is untimed, like the brush's
    assert capi.VR_K_COUNT == 22 and product_lib.vr_timing_kernel_count() == 22
    hpp = open(os.path.join(ROOT, "include", "vrterrain.hpp")).read()
    assert "Noise(" in hpp and "vr_terrain_noise" in hpp
    for lists in re.findall(r"vr_terrain_edit[^\n]*_texture[^\n]*", header):          # the history paragraph's lists, and the stream's
        assert "_noise" in lists, lists
    # the ctypes size and offsets against the header's, and the declarations in C and in C++
    fields = [n for n, _ in capi.NoiseParams._fields_]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include <vrterrain.h>\n'
                   'int (*noise_fn(void))(vr_terrain*, int, const vr_noise_params*, const vr_brush_dab*, uint32_t, int32_t*) { return vr_terrain_noise; }\n'
                   '#ifdef WITH_MAIN\nint main(void) { printf("%zu", sizeof(vr_noise_params));\n'
                   + "".join(f'printf(" %zu", offsetof(vr_noise_params, {n}));\n' for n in fields)
                   + 'printf(" %d %d\\n", (int)VR_NOISE_MAX_OCTAVES, (int)VR_NOISE_WHOLE_MAP); return 0; }\n#endif\n')
    inc = os.path.join(ROOT, "include")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", inc, "-c", str(src), "-o", str(tmp_path / "sizes.o")], check=True, capture_output=True, text=True)
    exe, lib_dir = str(tmp_path / "sizes"), os.path.join(ROOT, "vrenderer_amd", "lib")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-DWITH_MAIN", "-I", inc, str(src), "-o", exe, "-L", lib_dir, "-lvrterrain", f"-Wl,-rpath,{lib_dir}",
                    "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"], check=True, capture_output=True, text=True)
    got = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    assert got == ["64"] + [str(getattr(capi.NoiseParams, n).offset) for n in fields] + ["12", "1"], got
    cpp = tmp_path / "noise.cpp"
    cpp.write_text('#include <vrterrain.hpp>\nbool noise(vRenderer::TerrainPass& tp, const vr_noise_params& p, const vr_brush_dab* d, int32_t r[4]) '
                   '{ return tp.Noise(0, p, d, 1, false, r) && tp.Noise(1, p, nullptr, 0, true); }\n'
                   'static_assert(sizeof(vr_noise_params) == 64, "vr_noise_params");\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(cpp), "-o", str(tmp_path / "noise_cpp.o")],
                   check=True, capture_output=True, text=True)


GOOD = dict(frequency=0.05, offset_x=1.0, offset_z=-2.0, lacunarity=2.0, gain=0.5, amplitude=40.0, base=100.0, seed=7, octaves=6, basis=1, fractal=0, op=0,
            channel_mask=1, flags=0, reserved=(0, 0))


def test_refusals_answer_without_a_device(product_lib):
    """Every refusal of the header's list but the one that needs the map's size comes before any use of the device: a handle that is
    no terrain is never looked into."""
    lib = product_lib
    fake = C.create_string_buffer(1 << 16)                          # stands in for a terrain; a refused call does not read it
    nan, inf = float("nan"), float("inf")

    def call(t=True, p=True, which=0, dabs=True, n=1, d=(0.0, 0.0, 4.0, 0.5, 1.0), **kw):
        f = dict(GOOD, **kw)
        np_ = capi.NoiseParams(**{k: v for k, v in f.items() if k != "reserved"})
        np_.reserved[:] = f["reserved"]
        arr = (capi.BrushDab * max(n, 1))(*[capi.BrushDab(*d)] * max(n, 1))
        rect = (C.c_int32 * 4)()
        return lib.vr_terrain_noise(C.cast(fake, C.c_void_p) if t else None, which, C.byref(np_) if p else None, arr if dabs else None, n, rect)

    bad = [dict(t=False), dict(p=False), dict(which=2), dict(which=-1), dict(dabs=False), dict(n=capi.VR_MAX_BRUSH_DABS + 1),
           dict(octaves=0), dict(octaves=-1), dict(octaves=13),
           dict(basis=2), dict(basis=-1), dict(fractal=3), dict(fractal=-1), dict(op=2), dict(op=-1),
           dict(flags=2), dict(flags=3, dabs=False, n=0), dict(flags=0x80000000),
           dict(flags=1), dict(flags=1, n=0), dict(flags=1, dabs=False, n=1),                      # the flag together with dabs
           dict(frequency=0.0), dict(frequency=-0.05),
           dict(lacunarity=0.99), dict(lacunarity=4.01), dict(gain=-0.01), dict(gain=1.01),
           dict(amplitude=255.5), dict(amplitude=-255.5), dict(base=-0.5), dict(base=255.5),
           dict(channel_mask=0), dict(channel_mask=16), dict(which=1, channel_mask=16), dict(which=1, channel_mask=0),
           dict(channel_mask=2), dict(channel_mask=15),                                            # the heightmap has the one channel
           dict(reserved=(1, 0)), dict(reserved=(0, -1)),
           dict(d=(nan, 0.0, 4.0, 0.5, 1.0)), dict(d=(0.0, inf, 4.0, 0.5, 1.0)), dict(d=(0.0, 0.0, 0.0, 0.5, 1.0)), dict(d=(0.0, 0.0, -1.0, 0.5, 1.0)),
           dict(d=(0.0, 0.0, 4.0, 1.0, 1.0)), dict(d=(0.0, 0.0, 4.0, -0.1, 1.0)), dict(d=(0.0, 0.0, 4.0, 0.5, nan)),
           dict(d=(0.0, 0.0, 4.0, 0.5, 1.5)), dict(d=(0.0, 0.0, 4.0, 0.5, -0.1))]                  # strength is an opacity
    for field in ("frequency", "offset_x", "offset_z", "lacunarity", "gain", "amplitude", "base"):
        bad += [{field: nan}, {field: inf}, {field: -inf}]
    for kw in bad:
        assert call(**kw) == capi.VR_ERR_INVALID_ARGUMENT, kw
    assert bytes(fake) == bytes(1 << 16)


@pytest.fixture(scope="module")
def noise_checks(tmp_path_factory):
    """The check program, and the same program under the address and undefined-behaviour sanitizers (stand-alone, nothing preloaded)."""
    d = tmp_path_factory.mktemp("noise")
    flags = ["-ffp-contract=off"]
    return (build_host_check(d, "noise_check", flags),
            build_host_check(d, "noise_check", flags + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "noise_check_san"))


def test_the_header_keeps_its_ranges(noise_checks):
    """vr_noise.h compiles without HIP.  400000 seeded points per basis: |n| <= 1, the fade in [0, 1], the gradient basis 0 at lattice
    points; 20000 seeded calls: finite constants, weights that sum to 1, |f| <= 1; the 2^22 refusal from both sides on four maps."""
    for exe in noise_checks:
        r = run_host_check(exe, timeout=600, expect=" points, 0 failures", stderr_tail=4000)
        assert "820016 points" in r.stdout, r.stdout[-400:]


def _sets():
    """Every basis x fractal x op at 1, 2 and 12 octaves, the lattice origin inside the map; then calls at the 2^22 bound."""
    out = []
    for _, basis in nm.BASES:
        for _, fractal in nm.FRACTALS:
            for _, op in nm.OPS:
                for octaves in (1, 2, 12):
                    out.append(nm.params(0.11, 140.0 if op == nm.ADD else -90.0, octaves=octaves, lacunarity=1.9, gain=0.55, offset=(4.7, -9.1),
                                         seed=1000 * basis + 100 * fractal + 10 * op + octaves, basis=basis, fractal=fractal, op=op, base=117.5, channel_mask=1))
    return out


def _boundary_sets(w, h):
    """Frequencies either side of the refusal on a w x h map (offset 100: the far corner's coordinate is (100 + 32 - 32 / w) * frequency)."""
    reach = 100.0 + 32.0 - 32.0 / w
    f0 = nm.COORD_LIMIT / reach
    return [nm.params(f0 * s, 10.0, octaves=1, offset=(100.0, 0.0), seed=5, basis=nm.VALUE) for s in (0.5, 0.999, 0.99999, 1.00001, 1.001, 2.0)]


def _host_noise(exe, tmp_path, texels, mask, sets):
    h, w = texels.shape[:2]
    ch = 1 if texels.ndim == 2 else 4
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<4if", w, h, ch, len(sets), WORLD))
        f.write(np.ascontiguousarray(texels).tobytes())
        f.write(np.ascontiguousarray(mask, np.float32).tobytes())
        for p in sets:
            f.write(struct.pack("<7fI4iI", p["frequency"], p["offset_x"], p["offset_z"], p["lacunarity"], p["gain"], p["amplitude"], p["base"], p["seed"],
                                p["octaves"], p["basis"], p["fractal"], p["op"], p["channel_mask"]))
    subprocess.run([exe, "apply", fin, fout], check=True, timeout=300)
    raw, at, res = open(fout, "rb").read(), 0, []
    for _ in sets:
        consts = np.frombuffer(raw, np.float32, 60, at).reshape(5, 12)
        ok = struct.unpack_from("<i", raw, at + 240)[0]
        at += 244
        if not ok:
            res.append((consts, False, None, None, None))
            continue
        out = np.frombuffer(raw, np.uint8, w * h * ch, at).reshape(texels.shape)
        at += w * h * ch
        f = np.frombuffer(raw, np.float32, w * h, at).reshape(h, w)
        at += 4 * w * h
        n = np.frombuffer(raw, np.float32, 12 * w * h, at).reshape(12, h, w)
        at += 48 * w * h
        res.append((consts, True, out, f, n))
    assert at == len(raw)
    return res


@pytest.mark.parametrize("channels", (1, 4), ids=("r8", "srgba8"))
@pytest.mark.parametrize("size", MAPS, ids=[f"{w}x{h}" for w, h in MAPS])
def test_header_on_the_host_gives_the_model_s_bytes(noise_checks, tmp_path, size, channels):
    """Every basis x fractal x op at 1, 2 and 12 octaves on a random map of either texel type under a random mask with zeros in it: the
    header's functions under g++ - plain and under the sanitizers - and the numpy model agree in every prepared constant, every n_o
    and f (as bits) and every byte; cells of both signs occur; the 2^22 refusal falls between the same two frequencies."""
    w, h = size
    rng = np.random.default_rng(100 * w + h + channels)
    texels = rng.integers(0, 256, (h, w) if channels == 1 else (h, w, 4), dtype=np.uint8)
    mask = np.where(rng.random((h, w)) < 0.25, 0.0, rng.random((h, w))).astype(np.float32)
    mask.flat[0] = 1.0
    sets = [dict(p, channel_mask=1 if channels == 1 else (5, 15, 8)[i % 3]) for i, p in enumerate(_sets())]
    edge = _boundary_sets(w, h)
    assert [nm.in_range(nm.prepare(p, WORLD, w, h), w, h) for p in edge] == [True, True, True, False, False, False]
    want = []
    for p in sets:
        d = {}
        out, _ = nm.noise(texels, p, WORLD, detail=d, mask=mask)
        want.append((d, d["f"], out))
        if min(w, h) >= 8:
            ix, iz = d["cells"][-1]
            assert ix.min() < 0 <= ix.max() and iz.min() < 0 <= iz.max(), (ix.min(), ix.max(), iz.min(), iz.max())
    changed = sum(int((o != texels).sum() > 0) for _, _, o in want)
    assert changed >= len(sets) * 3 // 4, changed                    # most sets change the map - a model of nothing would not do
    bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
    for exe in noise_checks:
        got = _host_noise(exe, tmp_path, texels, mask, sets + edge)
        for k, (p, (d, f, out)) in enumerate(zip(sets, want)):
            consts, ok, gout, gf, gn = got[k]
            assert ok, k
            for row, name in enumerate(("sx", "sz", "ox", "oz", "a")):
                full = np.zeros(12, np.float32)
                full[:p["octaves"]] = d["prepared"][name]
                assert np.array_equal(bits(consts[row]), bits(full)), (k, name, consts[row], full)
            assert np.array_equal(bits(gn[:p["octaves"]]), bits(d["n"])) and not gn[p["octaves"]:].any(), f"set {k}: n differs"
            assert np.array_equal(bits(gf), bits(f)), f"set {k}: f differs in {(bits(gf) != bits(f)).sum()} texels"
            assert np.array_equal(gout, out), f"set {k}: {(gout != out).sum()} bytes differ, first {np.argwhere(gout != out)[:4].tolist()}"
        assert [g[1] for g in got[len(sets):]] == [True, True, True, False, False, False]
