"""Views that send visible pixels through the near-plane / guard-band clipper, and the comparison of an implementation's
G-buffer planes with tests/f64_model.py on them (tests/test_raster_clip_cpu.py: the oracle; tests/test_raster_clip_f64.py:
the HIP tile pass).

The views were found on the CPU with the oracle as the implementation and are frozen here.  The 256 world's finest cells
are 1/16 of a unit wide, so a clipped triangle is visible only from an eye a fraction of a unit above the surface with the
near plane at 0.1: GROUND is the surface's height under the eye (the heightmap's texel there is 0.45 lower).  Conditions
per view, asserted by both test modules: at least `clipper` pixels won by clipper triangles, `clipped` > 0 triangles through
the clipper, and band + either + multi pixels at most 1 % of the covered ones."""
import numpy as np

import vrenderer_amd as vr
from tests import f64_model as F

SIZE = 256
EYE_X, EYE_Z, GROUND = 5.3, 3.2, 39.668
_LOW = (EYE_X, GROUND + 0.2, EYE_Z)
_GUARD_H = 50.19607843137255                                  # texel (128 - 2, 128 + 1) of the synthetic heightmap, as test_gpu_parity


def _v(eye, tgt, w, h, **kw):
    return dict(eye=eye, tgt=tgt, w=w, h=h, kw=kw)


# name -> view; `clipper`: the least number of pixels won by clipper triangles; `viewport`: (x, y, w, h) inside the target
VIEWS = {
    "near-45": dict(_v(_LOW, (10.957, 32.797, 7.443), 160, 90), clipper=500),
    "near-rolled": dict(_v(_LOW, (8.036, 30.471, 5.252), 160, 90, up=(0.6, 0.8, 0.0)), clipper=500),
    "near-150-degrees": dict(_v((EYE_X, GROUND + 0.5, EYE_Z), (10.957, 33.097, 7.443), 256, 144, vfov_deg=150.0, z_far=12.0), clipper=500),
    "guard-band": dict(_v((1.3, _GUARD_H + 0.5, -2.2), (1.32, _GUARD_H - 5.0, -2.18), 128, 72, vfov_deg=0.01), clipper=128 * 72),
    "near-and-guard": dict(_v((1.3, _GUARD_H + 0.5, -2.2), (1.32, _GUARD_H - 5.0, -2.18), 128, 72, vfov_deg=0.01, z_near=2.4807), clipper=500, both=1),
    "negative-viewport": dict(_v(_LOW, (10.957, 32.797, 7.443), 160, 90), clipper=200, viewport=(-37, -21, 200, 120)),
    "odd-131x75": dict(_v(_LOW, (12.55, 35.642, 8.638), 131, 75), clipper=100),
    "rank-1-of-2": dict(_v(_LOW, (8.036, 30.471, 5.252), 256, 144, up=(0.6, 0.8, 0.0)), clipper=500, part=(1, 2)),
    "eye-below": dict(_v((EYE_X, GROUND - 0.3, EYE_Z), (12.818, 42.788, 8.838), 160, 90), clipper=0),
}


def make_view(spec):
    vw, vh = (spec["viewport"][2:] if "viewport" in spec else (spec["w"], spec["h"]))
    v = vr.make_view(spec["eye"], spec["tgt"], vw, vh, **dict(dict(z_near=0.1), **spec["kw"]))
    if "viewport" in spec:
        v.viewport_x, v.viewport_y = spec["viewport"][:2]
    return v


def model_frame(ot, spec, view, lod):
    hml = [ot.height_mip(l) for l in range(ot.height_levels())]
    alb = [ot.albedo_mip(l) for l in range(ot.albedo_levels())]
    return F.render(ot, view, spec["w"], spec["h"], 400.0, float(SIZE), hml, alb, lod_for_sampling=lod, part=spec.get("part"))


def check_planes(name, spec, fr, planes, specular_code, dbg=None):
    """The planes (depth, diffuse, specular, normals, emissive) of one implementation against the model's frame `fr`:
    coverage by class, depth within the derived bound, world xz and LOD (dbg, if the implementation has the debug plane)
    within theirs, albedo within one SRGBA8 code on <= 0.1 % of the pixels, normals within one SNORM16 code on <= 2 % of the
    components, the rest exact.  Where the model allows either of two fragments, all of a pixel's values must agree with one
    of them.  Returns the worst error / bound ratios."""
    depth = planes["depth"]
    cov = depth < 1.0
    n_cov = int(cov.sum())
    clipper = int((fr.from_clipper & cov).sum())
    loose = int((fr.band | fr.either | fr.multi).sum())
    print(f"{name}: {fr.tri_count}, covered {n_cov}, clipper pixels {clipper}, band {int(fr.band.sum())}, either {int(fr.either.sum())}, "
          f"multi {int(fr.multi.sum())}, delta {fr.delta:.5f} px")
    assert fr.tri_count["degenerate"] == 0
    assert fr.tri_count["clipped"] > 0 and clipper >= spec["clipper"], (fr.tri_count, clipper)
    assert fr.tri_count["near_and_guard"] >= spec.get("both", 0), fr.tri_count
    assert loose <= 0.01 * n_cov, f"band share {loose} of {n_cov}: replace the view"
    missing, extra = (fr.cls == F.MUST) & ~cov, (fr.cls == F.EMPTY) & cov
    assert not missing.any() and not extra.any(), f"coverage: {missing.sum()} certain pixels empty at {np.argwhere(missing)[:4].tolist()}, " \
                                                  f"{extra.sum()} drawn outside every polygon at {np.argwhere(extra)[:4].tolist()}"
    m = cov & ~fr.multi
    rgb = np.stack([(planes["diffuse"] >> (8 * k)) & 255 for k in range(3)], -1).astype(np.int64)
    nn = planes["normals"][..., :3].view(np.int16).astype(np.int64)

    def against(o):
        r = {"depth": np.abs(depth.astype(np.float64) - o.depth) / np.maximum(o.depth_tol, 1e-300)}
        if dbg is not None:
            r["world x"] = np.abs(dbg[..., 1].astype(np.float64) - o.wx) / o.wx_tol
            r["world z"] = np.abs(dbg[..., 2].astype(np.float64) - o.wz) / o.wz_tol
            r["lod"] = np.abs(dbg[..., 0].astype(np.float64) - o.lod) / (F.lod_fn_tol(o.lod) + o.lod_term)
        ok = o.valid.copy()
        for a in r.values():
            ok &= np.nan_to_num(a, nan=np.inf) <= 1.0
        dc, dn = np.abs(rgb - o.albedo_codes), np.abs(nn - o.normal_codes)
        ok &= (dc.max(-1) <= 1) & (dn.max(-1) <= 1)
        return r, ok, dc, dn
    with np.errstate(divide="ignore", invalid="ignore"):
        r1, ok1, dc, dn = against(fr.first)
        use2 = np.zeros_like(ok1)
        if fr.second is not None:
            r2, ok2, dc2, dn2 = against(fr.second)
            use2 = fr.either & ~ok1 & ok2
            dc, dn = np.where(use2[..., None], dc2, dc), np.where(use2[..., None], dn2, dn)
            r1 = {k: np.where(use2, r2[k], a) for k, a in r1.items()}
    worst = {k: float(np.nan_to_num(a[m], nan=np.inf).max()) for k, a in r1.items()}
    for k in list(r1):
        worst[k + ", clipper pixels"] = float(np.nan_to_num(r1[k][m & fr.from_clipper], nan=np.inf).max(initial=0.0))
    print(f"{name}: worst error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    bad = m & ~(ok1 | use2)
    assert not bad.any(), f"{bad.sum()} pixels beyond their bounds, first {np.argwhere(bad)[:4].tolist()}: {worst}"
    assert (dc[m].max(-1) > 0).mean() <= 1e-3 and (dn[m] > 0).mean() <= 0.02, ((dc[m].max(-1) > 0).mean(), (dn[m] > 0).mean())
    assert np.all(planes["normals"][..., 3][cov] == 32767) and np.all(planes["emissive"][cov] == 0)
    assert np.all(planes["specular"][cov] == (specular_code | specular_code << 8 | specular_code << 16 | 0xff000000))
    untouched = fr.cls == F.EMPTY                 # (a fragment at depth 1.0 exactly passes LessOrEqual and is shaded)
    assert (planes["diffuse"][untouched] == 0).all() and (planes["normals"][untouched] == 0).all()
    return worst
