"""CPU tests of the region definition: vr_region.h's functions under g++ (tests/host/region_check.cpp), plain and under the address and
undefined-behaviour sanitizers, keep every crossing and every near texel inside the edge's span and give the constants, edges,
rectangle, inside bits, q*, f and bytes of the numpy model (tests/region_model.py) on every case of tests/region_cases.py; the model
classifies as exact rational arithmetic does wherever a texel is farther than the rounding allowance from every edge; the tile cull
does not show on the model; and the cases meet their preconditions on the model's output, on the oracle's synthetic maps - so that
no GPU test can pass emptily."""
import math
import struct
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from tests import region_cases as rc
from tests import region_model as rm
from tests.host_check import build_host_check, run_host_check

F = np.float32


@pytest.fixture(scope="module")
def region_checks(tmp_path_factory):
    """The check program, and the same program under the sanitizers (stand-alone, nothing preloaded)."""
    d = tmp_path_factory.mktemp("region")
    flags = ["-ffp-contract=off"]
    return (build_host_check(d, "region_check", flags),
            build_host_check(d, "region_check", flags + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "region_check_san"))


@pytest.fixture(scope="module")
def cases(oracle):
    return rc.all_cases(oracle.synth_heightmap, oracle.synth_albedo)


@pytest.fixture(scope="module")
def modelled(cases):
    """what -> the model's (texels, rect, detail), computed once."""
    return {c[0]: rc.run_model(c[2], c[4], c[5], c[6], c[3]) for c in cases}


def test_nothing_of_an_edge_lies_outside_its_span(region_checks):
    """vr_region.h compiles without HIP.  3000 seeded polygons on six maps - non-square ones, vertices on texel centres and rows,
    horizontal and 45 degree edges through texel centres, zero-length edges, vertices out to 1e9 world sizes away: no edge crosses a
    row to the left of a texel outside its span or is nearer than the feather there, and the map classified tile by tile with the
    culled lists - and the distance chain skipped where the distance box misses the tile - has the parity and q* of no cull."""
    for exe in region_checks:
        r = run_host_check(exe, timeout=600, expect=" polygons, 0 failures", stderr_tail=4000)
        assert "3000 polygons" in r.stdout, r.stdout[-400:]


def test_the_gpu_cases_meet_their_preconditions_on_the_model(cases, modelled):
    kinds = set()
    for what, _, texels, S, pts, contours, p, kind in cases:
        out, rect, d = modelled[what]
        kinds.add(kind)
        if kind == "main":
            print(what, rc.check_preconditions(texels, out, p, d, what))
        elif kind == "sawtooth":
            n = rc.sawtooth_precondition(d, texels.shape)
            print(what, n)
            assert n >= 5 and (out != texels).sum() >= 200
        elif kind == "shadow":
            tiles = rc.shadow_precondition(d)
            print(what, tiles)
            left_edge = min(float(e["ax"]) for e in d["edges"])
            assert tiles and all(tx - left_edge >= 96 for tx, _ in tiles) and (out != texels).sum() >= 200
        else:
            assert (out != texels).sum() >= 200, what
    assert kinds == {"main", "sawtooth", "shadow", "shape", "aligned"}


def test_the_shapes_are_what_they_should_be(cases, modelled):
    by = {c[0]: c for c in cases}
    hm = by["island"][2]
    h, w = hm.shape
    isl = modelled["island"][2]
    assert isl["inside"][h // 5, w // 5] and not isl["inside"][h // 2, w // 2]                     # the second contour is a hole
    hh = modelled["hole in hole"][2]
    assert hh["inside"][h // 10, w // 2] and not hh["inside"][h * 3 // 10, w // 2] and hh["inside"][h // 2, w // 2]
    bt = modelled["bow-tie"][2]["inside"]
    assert bt[h // 2, w // 5] and bt[h // 2, w * 4 // 5] and not bt[h // 5, w // 2] and not bt[h * 4 // 5, w // 2]      # two lobes
    off = modelled["off all sides"]
    assert off[1] == (0, 0, w, h) and not off[2]["inside"].all() and all(off[2]["inside"][j, i] for j, i in ((0, w // 2), (h - 1, w // 2), (h // 2, 0), (h // 2, w - 1)))
    whole = modelled["contains the map"]
    assert whole[1] == (0, 0, w, h) and whole[2]["inside"].all() and len(whole[2]["edges"]) < 4
    assert all(float(e["ax"]) < 0 for e in whole[2]["edges"])                                      # what is left lies left of the map
    sq = modelled["on texel centres"][2]
    assert all(float(e[n]) == int(e[n]) for e in sq["edges"] for n in ("ax", "az", "bz"))
    al = modelled["aligned on texel centres"][2]
    assert all(float(e[n]) == int(e[n]) for e in al["edges"] for n in ("ax", "az", "bz"))
    want = np.zeros((h, w), bool)
    want[9:40, 13:51] = True                # half-open: the top vertices' row is in and the bottom ones' is out; a texel on the left edge is out, on the right one in
    assert np.array_equal(al["inside"], want)
    assert modelled["fast64 level skirt"][1][2] < w                                                # the rectangle is the polygon's, not the span's


def test_the_tile_cull_does_not_show_on_the_model(cases, modelled):
    """Every 32 x 8 tile evaluated with only the edges whose spans meet it: the inside bits, q* and the bytes of no cull."""
    for what, _, texels, S, pts, contours, p, _ in cases:
        out, rect, d = modelled[what]
        cout, crect, cd = rc.run_model(texels, pts, contours, p, S, cull=True)
        assert crect == rect and np.array_equal(cd["inside"], d["inside"]), what
        assert np.array_equal(cd["q"].view(np.uint32), d["q"].view(np.uint32)) and np.array_equal(cout, out), what


# ---- the exact classifier -------------------------------------------------------------------------------------------------------
def exact_classify(every, k, w, h):
    """(inside, near): inside by the even-odd rule in rational arithmetic, from the fp32 vertex numbers and the half-open rule, on every
    texel; near where a texel lies within an edge's allowance E of that edge, measured exactly (a float64 distance decides it where it
    is beyond 4 E or 1e-6 world units, whichever is more - far above a double's own error here)."""
    inside, near = np.zeros((h, w), bool), np.zeros((h, w), bool)
    wx, wz = Fraction(float(k["wx"])), Fraction(float(k["wz"]))
    ii, jj = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    for e in every:
        ax, az, bx, bz = (Fraction(float(e[n])) for n in ("ax", "az", "bx", "bz"))
        E = rm.allowance(e, k, w, h)
        for j in range(h):
            if (az <= j) == (bz <= j):
                continue
            cross = ax + (Fraction(j) - az) / (bz - az) * (bx - ax)          # texel i has the crossing to its left where i > cross
            inside[j, max(math.floor(cross) + 1, 0):] ^= True
        # distance: float64 first
        fax, faz, fdx, fdz = float(ax), float(az), float(bx - ax) * float(wx), float(bz - az) * float(wz)
        px, pz = (ii - fax) * float(wx), (jj - faz) * float(wz)
        l2 = fdx * fdx + fdz * fdz
        t = np.clip((px * fdx + pz * fdz) / l2, 0.0, 1.0) if l2 > 0 else np.zeros_like(px)
        d = np.hypot(px - t * fdx, pz - t * fdz)
        for j, i in np.argwhere(d < max(4.0 * E, 1e-6)):
            qx, qz = (Fraction(int(i)) - ax) * wx, (Fraction(int(j)) - az) * wz
            dx, dz = (bx - ax) * wx, (bz - az) * wz
            ll = dx * dx + dz * dz
            tt = min(max((qx * dx + qz * dz) / ll, Fraction(0)), Fraction(1)) if ll else Fraction(0)
            ex, ez = qx - tt * dx, qz - tt * dz
            if ex * ex + ez * ez <= Fraction(E) ** 2:
                near[j, i] = True
    return inside, near


def seeded_polygons():
    """(what, shape, world, points, contours): 240 polygons of 3 .. 7 vertices on three maps, the first vertex in the map's first
    quarter and the third in its last, so that the rectangle is a quarter of the map at least: random ones; ones with every vertex on a
    texel centre; ones with every vertex on a texel row and a short horizontal edge; ones with a short 45 degree edge through texel
    centres."""
    rng = np.random.default_rng(4242)
    out = []
    for n in range(240):
        h, w = ((120, 150), (97, 131), (128, 128))[n % 3]
        S = 64.0 if n % 2 else 150.0
        nv = int(rng.integers(3, 8))
        kind = (n // 3) % 4
        while True:
            t = np.stack([rng.uniform(-3, w + 3, nv), rng.uniform(-3, h + 3, nv)], 1)
            t[0] = rng.uniform(0, 0.25, 2) * (w, h)
            t[2] = rng.uniform(0.75, 1.0, 2) * (w, h)
            if kind != 1:
                break
            t = np.round(t)                   # (edges between texel centres that pass through at most one more: the cap on texels within E)
            d = (np.roll(t, -1, 0) - t).astype(int)
            if all(math.gcd(int(a), int(b)) <= 2 for a, b in d):
                break
        if kind == 2:
            t[:, 1] = np.round(t[:, 1]); t[1] = t[0] + (int(rng.integers(3, 9)), 0)
        if kind == 3:
            t[0] = np.round(t[0]); t[1] = t[0] + int(rng.integers(1, 6))
        out.append((f"seeded {n}", (h, w), S, np.float32([rc.vertex((h, w), S, x, y) for x, y in t]), None))
    return out


def test_the_model_classifies_as_exact_arithmetic_does(cases):
    """The named cases and 240 seeded polygons: every texel farther than E from every edge, measured exactly, has the exact
    classifier's inside bit.  The texels within E - left out - are at most 0.5 % of the call's rectangle in every case; that cap is
    asserted on the exact classifier's output alone."""
    named, seen = [], set()
    for what, _, texels, S, pts, contours, _, kind in cases:
        key = (texels.shape[:2], S, np.asarray(pts, F).tobytes(), contours)
        if kind != "aligned" and key not in seen:              # (the aligned square's whole outline runs through texel centres: its bits are written out above)
            seen.add(key)
            named.append((what, texels.shape[:2], S, pts, contours))
    assert len(named) >= 14
    total_near = total = 0
    for what, (h, w), S, pts, contours in named + seeded_polygons():
        p = rm.params(feather=0.0)
        k, every, edges, rect = rm.prepare(pts, contours, p, S, w, h)
        want, near = exact_classify(every, k, w, h)
        area = rect[2] * rect[3]
        assert near.sum() <= 0.005 * area, (what, int(near.sum()), area)
        got, _ = rm.classify(edges, k, w, h)
        far = ~near
        assert np.array_equal(got[far], want[far]), (what, np.argwhere((got != want) & far)[:4].tolist())
        total_near += int(near.sum()); total += area
        if area == 0:
            assert not want.any(), what
    print(f"{total_near} texels within E of an edge, of {total} in the rectangles")
    assert total > 50000


# ---- the header on the host -------------------------------------------------------------------------------------------------------
def _host_regions(exe, tmp_path, texels, world, sets):
    h, w = texels.shape[:2]
    ch = 1 if texels.ndim == 2 else 4
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<4if", w, h, ch, len(sets), world))
        f.write(np.ascontiguousarray(texels).tobytes())
        for pts, contours, p in sets:
            pts = np.ascontiguousarray(np.asarray(pts, F).reshape(-1, 2))
            counts = list(contours) if contours is not None else []
            f.write(struct.pack("<iI3f4fIII", p["op"], p["channel_mask"], p["target"], p["feather"], p["opacity"], *p["color"], int(p["feather_inside"]), len(counts), len(pts)))
            f.write(np.asarray(counts, np.uint32).tobytes())
            f.write(pts.tobytes())
    subprocess.run([exe, "apply", fin, fout], check=True, timeout=300)
    raw, at, res = open(fout, "rb").read(), 0, []
    for _ in sets:
        consts = np.frombuffer(raw, F, 6, at)
        flags, ne, x0, y0, x1, y1 = struct.unpack_from("<Ii4i", raw, at + 24)
        at += 48
        edges = []
        for _ in range(ne):
            edges.append((np.frombuffer(raw, F, 6, at), struct.unpack_from("<5i", raw, at + 24)))
            at += 44
        out = np.frombuffer(raw, np.uint8, w * h * ch, at).reshape(texels.shape)
        at += w * h * ch
        inside = np.frombuffer(raw, np.uint8, w * h, at).reshape(h, w)
        at += w * h
        q = np.frombuffer(raw, F, w * h, at).reshape(h, w)
        f = np.frombuffer(raw, F, w * h, at + 4 * w * h).reshape(h, w)
        at += 8 * w * h
        res.append((consts, flags, (x0, y0, x1, y1), edges, out, inside, q, f))
    assert at == len(raw)
    return res


def test_header_on_the_host_gives_the_model_s_bytes(region_checks, tmp_path, cases, modelled):
    """Every case of tests/region_cases.py: the header's functions under g++ - plain and under the sanitizers - and the numpy model
    agree in every prepared constant, every edge and span, the rectangle, the inside bit, q* and f (as bits) and every byte."""
    bits = lambda a: np.ascontiguousarray(a, F).view(np.uint32)
    by_map = {}
    for what, _, texels, S, pts, contours, p, _ in cases:
        by_map.setdefault((texels.tobytes(), texels.shape, S), (texels, S, []))[2].append((what, pts, contours, p))
    assert len(by_map) >= 7
    for texels, S, sets in by_map.values():
        for exe in region_checks:
            got = _host_regions(exe, tmp_path, texels, S, [(pts, contours, p) for _, pts, contours, p in sets])
            for (what, _, _, p), (consts, flags, grect, gedges, gout, gin, gq, gf) in zip(sets, got):
                out, rect, d = modelled[what]
                k = d["prepared"]
                assert np.array_equal(bits(consts), bits([k[n] for n in ("wx", "wz", "inv_r2", "opacity", "target", "R")])), what
                assert flags == (rm.FEATHER_INSIDE if p["feather_inside"] else 0) | (0x100 if k["soft"] else 0), what
                assert len(gedges) == len(d["edges"]), what
                for (ef, ei), e in zip(gedges, d["edges"]):
                    assert np.array_equal(bits(ef), bits([e[n] for n in ("ax", "az", "dx", "dz", "inv_len2", "bz")])), what
                    assert ei == (e["x0"], e["x1"], e["y0"], e["y1"], e["dist_x1"]), (what, ei, e)
                assert (grect[0], grect[1], grect[2] - grect[0], grect[3] - grect[1]) == rect, (what, grect, rect)
                assert np.array_equal(gin.astype(bool), d["inside"]), what
                assert np.array_equal(bits(gq), bits(d["q"])) and np.array_equal(bits(gf), bits(d["f"])), what
                assert np.array_equal(gout, out), f"{what}: {(gout != out).sum()} bytes differ, first {np.argwhere(gout != out)[:4].tolist()}"
