"""CPU tests of the path definition: vr_path.h's functions under g++ (tests/host/path_check.cpp), plain and under the address and
undefined-behaviour sanitizers, keep every covered texel inside its segment's span, and
give the constants, segments, rectangle and bytes of the numpy model (tests/path_model.py) on every case of tests/path_cases.py; and
those cases meet their preconditions on the model's output, on the oracle's synthetic maps - so that no GPU test can pass emptily."""
import struct
import subprocess

import numpy as np
import pytest

from tests import path_cases as pc
from tests import path_model as pm
from tests.host_check import build_host_check, run_host_check

F = np.float32


@pytest.fixture(scope="module")
def path_checks(tmp_path_factory):
    """The check program, and the same program under the sanitizers (stand-alone, nothing preloaded)."""
    d = tmp_path_factory.mktemp("path")
    flags = ["-ffp-contract=off"]
    return (build_host_check(d, "path_check", flags),
            build_host_check(d, "path_check", flags + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "path_check_san"))


def test_covered_texels_lie_inside_the_span(path_checks):
    """vr_path.h compiles without HIP.  6002 seeded segments on six maps - non-square ones, zero-length segments, segments far outside
    the map: every texel with q < 1 lies inside its segment's span.  (The tile cull is the span alone: DESIGN.md 4ab.)"""
    for exe in path_checks:
        r = run_host_check(exe, timeout=600, expect=" points, 0 failures", stderr_tail=4000)
        assert "6002 points" in r.stdout, r.stdout[-400:]


def all_cases(oracle):
    """(what, texels, world, points, params, every_segment) of every call the GPU tests make against the model."""
    out = []
    for name in pc.SCENES:
        hm, al = pc.scene_maps(name, oracle.synth_heightmap, oracle.synth_albedo)
        S = pc.WORLD[name]
        for op in (pc.HEIGHT_OPS if name == "fast64" else (pc.scene_op(name),)):
            out.append((f"{name} {pc.OP_IDS[op]}", hm, S, *pc.height_case(name, hm, op), True))
        out.append((f"{name} paint", al, S, *pc.albedo_case(name, al), True))
    hm, _ = pc.scene_maps("fast64", oracle.synth_heightmap, oracle.synth_albedo)
    out.append(("zigzag", hm, 64.0, pc.zigzag(hm.shape, 64.0), pc.zigzag_params(), False))
    for what, (pts, p) in pc.degenerate_cases(hm.shape, 64.0).items():
        out.append((what, hm, 64.0, pts, p, False))
    return out


def test_the_gpu_cases_meet_their_preconditions_on_the_model(oracle):
    for what, texels, S, pts, p, every in all_cases(oracle):
        out, rect, detail = pc.run_model(texels, pts, p, S)
        if what in ("zigzag", "single", "closed", "repeated", "leaves"):
            assert (out != texels).sum() >= (100 if what == "zigzag" else 200), what
            continue
        print(what, pc.check_preconditions(texels, out, p, detail, what, every_segment=every))


def test_the_zigzag_has_winners_from_both_chunks_on_one_tile(oracle):
    """300 segments, all inside the tile [0, 32) x [8, 16): texels of that tile are won from below and from above index 256."""
    hm, _ = pc.scene_maps("fast64", oracle.synth_heightmap, oracle.synth_albedo)
    _, _, d = pc.run_model(hm, pc.zigzag(hm.shape, 64.0), pc.zigzag_params(), 64.0)
    assert len(d["segments"]) == 300
    win = d["winner"][8:16, 0:32]
    assert (win[win >= 0] < 256).sum() >= 20 and (win >= 256).sum() >= 20, ((win[win >= 0] < 256).sum(), (win >= 256).sum())
    assert all(s["x0"] < 32 and s["x1"] > 0 and s["y0"] < 16 and s["y1"] > 8 for s in d["segments"])


def test_the_degenerate_shapes_are_what_they_should_be(oracle):
    hm, _ = pc.scene_maps("fast64", oracle.synth_heightmap, oracle.synth_albedo)
    cases = pc.degenerate_cases(hm.shape, 64.0)
    det = {n: pc.run_model(hm, *cases[n], 64.0)[2] for n in cases}
    assert len(det["closed"]["segments"]) == 4 and set(det["closed"]["winner"][det["closed"]["covered"]].tolist()) == {0, 1, 2, 3}
    one = det["single"]
    assert len(one["segments"]) == 1 and float(one["segments"][0]["inv_len2"]) == 0.0 and not one["t"].any() and one["covered"].sum() >= 200
    rep = det["repeated"]
    assert len(rep["segments"]) == 3 and float(rep["segments"][1]["inv_len2"]) == 0.0
    # the zero-length segment ties with its predecessor's end wherever it is nearest: the lower index keeps those texels
    assert 1 not in set(rep["winner"][rep["covered"]].tolist())
    lv = det["leaves"]
    assert len(lv["segments"]) < 5 and lv["rect"][1] == 0 and lv["rect"][0] + lv["rect"][2] == hm.shape[1]


def test_a_texel_does_not_depend_on_segments_that_do_not_cover_it(oracle):
    """What lets the device cull: dropping every segment that covers no texel of a region leaves the region's bytes as they were."""
    hm, _ = pc.scene_maps("fast64", oracle.synth_heightmap, oracle.synth_albedo)
    pts, p = pc.height_case("fast64", hm, pm.LEVEL)
    full, _, d = pc.run_model(hm, pts, p, 64.0)
    head, _, _ = pc.run_model(hm, pts[:3], p, 64.0)
    only_head = d["covered"] & (d["winner"] <= 1)
    k = d["prepared"]
    q_rest = np.minimum(pm.texel_chain(d["segments"][2], k, 64, 64)[0], pm.texel_chain(d["segments"][3], k, 64, 64)[0])
    region = only_head & (q_rest >= 1)
    assert region.sum() >= 100 and np.array_equal(full[region], head[region])


def _host_paths(exe, tmp_path, texels, world, sets):
    h, w = texels.shape[:2]
    ch = 1 if texels.ndim == 2 else 4
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<4if", w, h, ch, len(sets), world))
        f.write(np.ascontiguousarray(texels).tobytes())
        for pts, p in sets:
            pts = np.ascontiguousarray(np.asarray(pts, F).reshape(-1, 3))
            f.write(struct.pack("<iI3f4fII", p["op"], p["channel_mask"], p["radius"], p["hardness"], p["opacity"], *p["color"], int(p["closed"]), len(pts)))
            f.write(pts.tobytes())
    subprocess.run([exe, "apply", fin, fout], check=True, timeout=300)
    raw, at, res = open(fout, "rb").read(), 0, []
    for _ in sets:
        consts = np.frombuffer(raw, F, 7, at)
        ns, x0, y0, x1, y1 = struct.unpack_from("<5i", raw, at + 28)
        at += 48
        segs = []
        for _ in range(ns):
            segs.append((np.frombuffer(raw, F, 7, at), struct.unpack_from("<4i", raw, at + 28)))
            at += 44
        out = np.frombuffer(raw, np.uint8, w * h * ch, at).reshape(texels.shape)
        at += w * h * ch
        planes = []
        for dt in (F, F, F, np.int32):
            planes.append(np.frombuffer(raw, dt, w * h, at).reshape(h, w))
            at += 4 * w * h
        res.append((consts, (x0, y0, x1, y1), segs, out, planes))
    assert at == len(raw)
    return res


def test_header_on_the_host_gives_the_model_s_bytes(path_checks, tmp_path, oracle):
    """Every case of tests/path_cases.py, and each with hardness 0 and a quarter of the radius: the header's functions under g++ - plain
    and under the sanitizers - and the numpy model agree in every prepared constant, every segment and span, the rectangle, q, t and f
    (as bits), the winning index and every byte."""
    bits = lambda a: np.ascontiguousarray(a, F).view(np.uint32)
    by_map = {}
    for what, texels, S, pts, p, _ in all_cases(oracle):
        by_map.setdefault((texels.tobytes(), texels.shape, S), (texels, S, []))[2].extend(
            [(what, pts, p), (what + ", thin", pts, dict(p, radius=float(F(p["radius"] * 0.25)), hardness=0.0))])
    assert len(by_map) >= 7
    for texels, S, sets in by_map.values():
        h, w = texels.shape[:2]
        want = [pc.run_model(texels, pts, p, S) for _, pts, p in sets]
        for exe in path_checks:
            got = _host_paths(exe, tmp_path, texels, S, [(pts, p) for _, pts, p in sets])
            for (what, _, p), (out, rect, d), (consts, grect, gsegs, gout, (gq, gt, gf, gwin)) in zip(sets, want, got):
                k = d["prepared"]
                assert np.array_equal(bits(consts), bits([k[n] for n in ("wx", "wz", "inv_r2", "h2", "k", "opacity", "R")])), what
                assert len(gsegs) == len(d["segments"]), what
                for (sf, si), s in zip(gsegs, d["segments"]):
                    assert np.array_equal(bits(sf), bits([s[n] for n in ("ax", "az", "dx", "dz", "inv_len2", "ha", "dh")])), what
                    assert si == (s["x0"], s["x1"], s["y0"], s["y1"]), (what, si, s)
                assert (grect[0], grect[1], grect[2] - grect[0], grect[3] - grect[1]) == rect, (what, grect, rect)
                assert np.array_equal(gwin, d["winner"]), what
                cov = d["covered"]
                assert np.array_equal(bits(gq), bits(d["q"])) and np.array_equal(bits(gt)[cov], bits(d["t"])[cov]) and np.array_equal(bits(gf), bits(d["f"])), what
                assert np.array_equal(gout, out), f"{what}: {(gout != out).sum()} bytes differ, first {np.argwhere(gout != out)[:4].tolist()}"
