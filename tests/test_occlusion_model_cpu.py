"""CPU tests of the occlusion definition: vr_occlusion.h's functions under g++ (tests/host/occlusion_check.cpp), plain and under the
address and undefined-behaviour sanitizers, read every height byte through a tile's staged footprint without a clamp that binds and
give the prepared constants and the bytes of the numpy model (tests/occlusion_model.py); and the cases of tests/occlusion_cases.py
meet their preconditions on the model's output, on the oracle's synthetic maps - so that no GPU test can pass emptily."""
import struct
import subprocess

import numpy as np
import pytest

from tests import occlusion_cases as oc
from tests import occlusion_model as om
from tests import texture_cases as tc
from tests.erode_model import mask_of
from tests.host_check import build_host_check, run_host_check

F = np.float32
CONST_FLOATS = 65 + 65 + 4 * 16 + 8 + 6          # OcclusionConst, in 4-byte words


@pytest.fixture(scope="module")
def occlusion_checks(tmp_path_factory):
    """The check program, and the same program under the sanitizers (stand-alone, nothing preloaded)."""
    d = tmp_path_factory.mktemp("occlusion")
    flags = ["-ffp-contract=off"]
    return (build_host_check(d, "occlusion_check", flags),
            build_host_check(d, "occlusion_check", flags + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "occlusion_check_san"))


@pytest.fixture(scope="module")
def cases(oracle):
    return oc.all_cases(oracle.synth_heightmap, oracle.synth_albedo)


@pytest.fixture(scope="module")
def modelled(cases):
    """what -> the model's (albedo, rect, detail), computed once."""
    return {c[0]: oc.run_model(c[3], c[5], c[4]) for c in cases}


def test_the_staged_footprint_holds_every_sample(occlusion_checks):
    """vr_occlusion.h compiles without HIP.  300 seeded map sizes and radii: every tile's texels evaluated through the tile's staged
    footprint give the bytes of the direct loads, no clamp of the staged fetch binds, and a reach of 65 texels is refused."""
    for exe in occlusion_checks:
        r = run_host_check(exe, timeout=600, expect=" 0 binds, 0 failures", stderr_tail=4000)
        assert "300 maps" in r.stdout, r.stdout[-400:]


def test_the_figures_of_the_whole_map_on_the_synthetic_scenes(oracle):
    """What the definition gives on the oracle's maps at radius 8 and 16 directions, TINT towards black: the figures the cases were
    chosen by.  (Counts are exact - the march is integer arithmetic; the means hold to the two decimals stated.)"""
    want = {"fast64": (0.19, 0.50, 24680, 25668), "odd": (0.15, None, 8936, 7636)}
    for name, (mean, top, far, skips) in want.items():
        hm, al = oc.scene_maps(name, oracle.synth_heightmap, oracle.synth_albedo)
        out, rect, d = oc.run_model(al, oc.call(hm, oc.max_height(name), whole_map=True), oc.WORLD[name])
        o = d["o"]
        assert round(float(o.mean()), 2) == mean and (top is None or round(float(o.max()), 2) == top), (name, o.mean(), o.max())
        assert int(((d["den"] > 1) & (d["num"] > 0)).sum()) == far and int(d["skipped"].sum()) == skips, name
        if name == "fast64":
            changed = (out != al).any(-1)
            assert changed.sum() > 4000 and (out[..., :3] <= al[..., :3]).all() and np.array_equal(out[..., 3], al[..., 3])


def test_the_gpu_cases_meet_their_preconditions_on_the_model(cases, modelled):
    kinds, paths = set(), set()
    for what, name, hm, al, S, c, kind, st in cases:
        out, rect, d = modelled[what]
        assert oc.staged(hm.shape, al.shape, c[2], c[4], S) == st, what
        print(what, "staged" if st else "direct", oc.check_preconditions(al, out, c, rect, d, what, kind))
        kinds.add(kind); paths.add(st)
        if kind == "long":
            assert max(d["prepared"]["reach"]) == 64, (what, d["prepared"]["reach"])
    assert kinds == {"dabs", "whole", "gain", "long"} and paths == {True, False}
    by = {c[0]: c for c in cases}
    # the long cases' footprints: 161 x 137 bytes staged; above 32 KiB, so direct loads; every march of fast64 leaves the map
    _, _, hm, al, S, c, _, _ = by["multi, radius 64"]
    assert oc.footprint(hm.shape, al.shape, modelled["multi, radius 64"][2]["prepared"]["reach"]) == (161, 137)
    _, _, hm, al, S, c, _, _ = by["fine, radius 16"]
    fw, fh = oc.footprint(hm.shape, al.shape, modelled["fine, radius 16"][2]["prepared"]["reach"])
    assert fw * fh > oc.FOOT_BYTES
    d = modelled["fast64, radius 64"][2]
    axis = [i for i, (dx, dz, n, _) in enumerate(d["prepared"]["dirs"]) if (dx, dz) in ((1, 0), (-1, 0), (0, 1), (0, -1))]
    assert len(axis) == 4 and all(d["prepared"]["dirs"][i][2] == 64 for i in axis) and (d["skipped"][axis] > 0).all()


def test_a_reach_of_65_texels_is_refused_by_the_model_s_preparation():
    """The radius of tests/test_terrain_occlusion_gpu.py's refused call: 65 steps along the axes of fast64."""
    assert om.prepare(om.params(radius=65.0), 12.5, 64.0, 64, 64)["refused"]
    assert not om.prepare(om.params(radius=64.0), 12.5, 64.0, 64, 64)["refused"]


# ---- the header on the host -------------------------------------------------------------------------------------------------------
def _host_occlusion(exe, tmp_path, hm, al, world, mh, sets):
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<5i2f", hm.shape[1], hm.shape[0], al.shape[1], al.shape[0], len(sets), world, mh))
        f.write(np.ascontiguousarray(hm).tobytes())
        f.write(np.ascontiguousarray(al).tobytes())
        for p, mask in sets:
            f.write(struct.pack("<8fIiIi", p["radius"], p["gain"], p["bias"], p["opacity"], *p["color"], p["channel_mask"], p["directions"], p["mode"],
                                0 if mask is None else 1))
            if mask is not None:
                f.write(np.ascontiguousarray(mask, F).tobytes())
    subprocess.run([exe, "apply", fin, fout], check=True, timeout=600)
    raw, at, res = open(fout, "rb").read(), 0, []
    for _ in sets:
        accepted = struct.unpack_from("<i", raw, at)[0]
        words = np.frombuffer(raw, np.uint32, CONST_FLOATS, at + 4)
        at += 4 + 4 * CONST_FLOATS
        res.append((accepted, words, np.frombuffer(raw, np.uint8, al.size, at).reshape(al.shape)))
        at += al.size
    assert at == len(raw)
    return res


def _assert_constants(words, k, p, what):
    """The OcclusionConst the header prepared against the model's constants, bit for bit."""
    bits = lambda a: np.ascontiguousarray(a, F).view(np.uint32)
    assert np.array_equal(words[0:65], bits(k["V"])), f"{what}: V"
    assert np.array_equal(words[65:130], bits(k["rk"])), f"{what}: rk"
    D = p["directions"]
    ints = words[130:178].view(np.int32)
    assert ints[0:D].tolist() == [d[0] for d in k["dirs"]] and ints[16:16 + D].tolist() == [d[1] for d in k["dirs"]], f"{what}: directions"
    assert ints[32:32 + D].tolist() == [d[2] for d in k["dirs"]], f"{what}: steps {ints[32:32 + D].tolist()} {[d[2] for d in k['dirs']]}"
    assert np.array_equal(words[178:178 + D], bits([d[3] for d in k["dirs"]])), f"{what}: g"
    assert not words[130 + D:146].any() and not words[178 + D:194].any(), f"{what}: unused directions"
    assert np.array_equal(words[194:202], bits([p["bias"], p["gain"], p["opacity"], 1.0 / D] + list(p["color"]))), f"{what}: scalars"
    assert words[202:208].view(np.int32).tolist() == [p["channel_mask"], p["mode"], D, k["reach"][0], k["reach"][1], 0], f"{what}: integers"


@pytest.mark.parametrize("name", oc.SCENES)
def test_header_on_the_host_gives_the_model_s_bytes(occlusion_checks, tmp_path, oracle, name):
    """Every scene, 4, 8 and 16 directions, both modes, bias 0 and 0.25, the whole map and five dabs: the header's serial evaluator under
    g++ - plain and under the sanitizers - and the numpy model agree in every prepared constant and every byte."""
    hm, al = oc.scene_maps(name, oracle.synth_heightmap, oracle.synth_albedo)
    S, mh = oc.WORLD[name], oc.max_height(name)
    dabs = tc.five_dabs(al.shape, S, tc.DAB_SCALE[name])
    mask = mask_of(al.shape[:2], dabs, S)[0]
    calls = []
    for D in (4, 8, 16):
        for mode in (om.TINT, om.STORE):
            for bias in (0.0, 0.25):
                for whole in (True, False):
                    calls.append((om.params(directions=D, mode=mode, bias=bias, gain=1.0 if whole else 2.5, opacity=0.8 if bias else 1.0, color=(30.0, 12.5, 0.0, 200.0),
                                            channel_mask=(7, 8, 5, 15)[len(calls) % 4]), whole))
    assert len(calls) == 24
    want = [om.occlusion(hm, al, p, mh, S, dabs=None if whole else dabs, whole_map=whole) for p, whole in calls]
    assert sum((w[0] != al).any(-1).sum() >= 200 for w in want) == len(want)                       # a model of nothing would not do
    for exe in occlusion_checks:
        got = _host_occlusion(exe, tmp_path, hm, al, S, mh, [(p, None if whole else mask) for p, whole in calls])
        for (p, whole), (accepted, words, out), (wout, _, d) in zip(calls, got, want):
            what = f"{name}, {p['directions']} directions, mode {p['mode']}, bias {p['bias']}, {'whole map' if whole else 'five dabs'}"
            assert accepted == 1, what
            _assert_constants(words, d["prepared"], p, what)
            assert np.array_equal(out, wout), f"{what}: {(out != wout).sum()} bytes differ, first {np.argwhere(out != wout)[:4].tolist()}"
