"""Input classes of the sky-pixel tests (tests/test_lighting_sky_cpu.py, tests/test_lighting_sky_gpu.py): views, light lists and
ambient colours at the extremes of the lighting model's domain (vrenderer_amd/csrc/vr_light_domain.h) and outside it.

kind "in":  inside sky_is_zero - every path may take its shortcut, and a cleared texel shades to +0.
kind "out": accepted, outside sky_is_zero - only the kernels that shade every texel run.
The expectation for a sky pixel comes from the float64 model (tests/f64_shading.py) through `table()`; where a case knows better
for single pixels it says so in `pixel_class` with the reason (the float64 model cannot hold an fp32 coincidence), and where the
float64 model's own answer is an artefact of how it is written the case says so in `frame_class`, with the derivation."""
import numpy as np

import vrenderer_amd as vr
from tests.common import AMBIENT_BOTTOM, AMBIENT_TOP

EYE, TARGET = (-37.5, 15.0, 10.0), (25.0, 7.5, -5.0)           # tests/common.py CAMERAS[5] at a 256-unit world
BIG = float(2.0 ** 40)                                          # kDomParamMax


class Case:
    def __init__(self, name, kind, view, lights, top=AMBIENT_TOP, bottom=AMBIENT_BOTTOM, pixel_class=None, why="", frame_class=None):
        self.name, self.kind, self.view, self.lights, self.top, self.bottom = name, kind, view, lights, tuple(top), tuple(bottom)
        self.pixel_class = pixel_class or {}                    # {(px, py): class} where the float64 model is not the reference
        self.why = why
        self.frame_class = frame_class                          # the class of every sky pixel where the float64 model's is set aside (why says why)

    def __repr__(self):
        return self.name


def infinite_far_view(w, h, z_near=0.1, eye=EYE, target=TARGET):
    """make_view's camera with perspProjD3DStyle's far plane at infinity: view_to_clip = [[xs,0,0,0],[0,ys,0,0],[0,0,1,1],[0,0,-zn,0]],
    whose inverse has the w column (0, 0, -1/zn, 1/zn) - and so has clip_to_world: w at depth 1 is exactly 0 in fp32."""
    v = vr.make_view(eye, target, w, h)
    p = np.array(v.view_to_clip[:], np.float64).reshape(4, 4)
    xs, ys = p[0, 0], p[1, 1]
    proj = np.array([[xs, 0, 0, 0], [0, ys, 0, 0], [0, 0, 1, 1], [0, 0, -z_near, 0]], np.float64)
    inv_proj = np.array([[1 / xs, 0, 0, 0], [0, 1 / ys, 0, 0], [0, 0, 0, -1 / z_near], [0, 0, 1, 1 / z_near]], np.float64)
    w2v = np.array(v.world_to_view[:], np.float64).reshape(4, 4)
    v2w = np.linalg.inv(w2v)
    v2w[:, 3] = (0.0, 0.0, 0.0, 1.0)
    v.view_to_clip[:] = [float(x) for x in proj.ravel()]
    v.world_to_clip[:] = [float(x) for x in (w2v @ proj).ravel()]
    v.clip_to_world[:] = [float(x) for x in (inv_proj @ v2w).ravel()]
    return v


def w_at_depth_one(view, w, h):
    """w of every pixel at depth 1 in the kernels' fp32 order, (h, w) float32."""
    return _reconstruct(view, w, h)[1]


def _reconstruct(view, w, h):
    f = np.float32
    m = np.array(view.clip_to_world[:], f).reshape(4, 4)
    ys, xs = np.mgrid[0:h, 0:w]
    cx = (xs.astype(f) + f(0.5)) * f(f(2.0) / f(w)) + f(-1.0)
    cy = (ys.astype(f) + f(0.5)) * f(f(-2.0) / f(h)) + f(1.0)
    e = [((cx * m[0, j] + cy * m[1, j]) + f(1.0) * m[2, j]) + m[3, j] for j in range(4)]
    with np.errstate(all="ignore"):
        rw = f(1.0) / e[3]
        return np.stack([e[0] * rw, e[1] * rw, e[2] * rw], -1), e[3]


def far_pixel_position(view, w, h, px, py):
    """The world position decode_surface reconstructs for pixel (px, py) at depth 1 with positional lights in the list: fp32, the
    checker's order, one correctly rounded reciprocal."""
    return tuple(float(x) for x in _reconstruct(view, w, h)[0][py, px])


def _axis(view):
    w2v = np.array(view.world_to_view[:], np.float64).reshape(4, 4)
    return w2v[:3, 2]                                           # the view direction in world space


def _nearest_admitted(view, w, h, make):
    """The light make(t) - t = distance from the eye along the view axis - as near the far plane as the predicate admits."""
    lo, hi = 100.0, 10000.0
    assert vr.light_domain(view, w, h, [make(lo)], AMBIENT_TOP, AMBIENT_BOTTOM)["sky_is_zero"]
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        if vr.light_domain(view, w, h, [make(mid)], AMBIENT_TOP, AMBIENT_BOTTOM)["sky_is_zero"]:
            lo = mid
        else:
            hi = mid
    return make(lo), lo


def cases(w, h, sky_pixel, eye=EYE, target=TARGET):
    """The finite classes for a w x h frame.  sky_pixel: a pixel whose texel is cleared in the frame the caller lights."""
    EYE, TARGET = eye, target
    v = vr.make_view(EYE, TARGET, w, h)
    axis = _axis(v)
    eye = np.array(EYE, np.float64)
    along = lambda t: tuple(eye + axis * t)                     # noqa: E731
    up = (0.05, 1.0, 0.02)

    def big(l):
        l.intensity = BIG
        l.color[:] = [BIG, BIG, BIG]
        return l

    out = []
    sun = big(vr.reference_sun())
    out.append(Case("in: sun, intensity and color at 2^40", "in", v, [sun]))
    shadowed = big(vr.reference_sun())
    shadowed.out_of_bounds_shadow = BIG
    out.append(Case("in: sun at 2^40 with out_of_bounds_shadow at 2^40", "in", v, [shadowed]))
    out.append(Case("in: unranged point light at 2^40", "in", v, [big(vr.point_light((5.0, 40.0, -3.0), 1.0, 0.0))]))
    out.append(Case("in: spot light at 2^40 looking at the sky", "in", v, [big(vr.spot_light((5.0, 10.0, -3.0), up, 1.0, 0.0, 20.0, 35.0))]))
    out.append(Case("in: spherical source at 2^40", "in", v, [big(vr.point_light((5.0, 40.0, -3.0), 1.0, 0.0, radius=4.0))]))
    near, t = _nearest_admitted(v, w, h, lambda t: vr.point_light(along(t), 800.0, 0.0))
    out.append(Case(f"in: unranged point light {t:.0f} along the axis, the nearest to the far plane the predicate admits", "in", v, [near, vr.reference_sun()]))
    out.append(Case("in: ranged light whose range ends on the far plane", "in", v, [vr.point_light(along(t - 1000.0), 5000.0, 10000.0 - (t - 1000.0))]))
    out.append(Case("in: ambient colours at 6e4", "in", v, [vr.reference_sun()], (6e4, 6e4, 6e4), (6e4, 5e4, 4e4)))
    far_eye = tuple(np.array(EYE) + np.array([2.0 ** 20, 0.0, 2.0 ** 20]))
    far_tgt = tuple(np.array(TARGET) + np.array([2.0 ** 20, 0.0, 2.0 ** 20]))
    v20 = vr.make_view(far_eye, far_tgt, w, h, z_near=10.0, z_far=100000.0)
    out.append(Case("in: world coordinates at 2^20", "in", v20, [vr.reference_sun(), vr.point_light(tuple(np.array(far_eye) + 30.0), 800.0, 0.0)]))

    hot = vr.reference_sun()
    hot.intensity = 3e38
    hot.color[:] = [10.0, 10.0, 10.0]
    out.append(Case("out: the 3e38 x 10 sun", "out", v, [hot],
                    why="intensity * color overflows fp32 where the two are multiplied first (the tiled pass stages that product); shade_pixel "
                        "and both references keep them apart"))
    oob = vr.reference_sun()
    oob.intensity, oob.out_of_bounds_shadow = 1e9, 1e30
    out.append(Case("out: sun at 1e9 with out_of_bounds_shadow at 1e30", "out", v, [oob],
                    why="under a shadow binding intensity * out_of_bounds_shadow overflows at a pixel outside the map; without one, zero"))
    vinf = infinite_far_view(w, h, eye=EYE, target=TARGET)
    w0 = ("w = 0 at depth 1: the reconstructed position is Inf or NaN and the float64 model carries the NaN to the result; an fp32 evaluation whose "
          "max / min / saturate return the operand that is a number (C's fmaxf and fminf, as the oracle uses them) drops it at a clamp")
    out.append(Case("out: infinite far plane, unranged point light", "out", vinf, [vr.point_light((5.0, 40.0, -3.0), 800.0, 0.0), vr.reference_sun()], why=w0))
    # Decided for this class: the float64 model is the side that is wrong.  Its NaN is numpy's: np.clip and np.maximum hand a NaN
    # on, while the shading language the model restates (HLSL: max, min and saturate return the operand that is a number, saturate(NaN)
    # is 0) and the instructions the kernels use for them (v_max_f32, v_min_f32, v_med3_f32) drop it.  Under those rules, with a
    # cleared texel and only a directional light: vi = NaN, NdotV = saturate(NaN) = 0, gv = 1/8; L and irr are finite, NdotLd =
    # max(0, 0) = 0, kd = 0; cosT = min(max(NaN, -1), 1) = -1, k1 and k2 finite, CL = Hv = NaN, hl2 > 0 is false so hs = 0; NdotH,
    # NdotL, VdotH = saturate(NaN) = 0; num = a2^2 * (0 * irr) * c = 0, den > 0, ks = 0; both terms add 0 * color = 0 and
    # finish_pixel adds products with occlusion = albedo = F0 = 0: +0.  (With a positional light irr = intensity * rd^2 is itself
    # NaN, and 0 * NaN stays: the class above is NaN under either rule.)
    out.append(Case("out: infinite far plane, sun only", "out", vinf, [vr.reference_sun()], why=w0 + "; decided: zero, by HLSL's NaN rules for max / min / saturate (tests/sky_classes.py)",
                    frame_class="zero"))
    on = vr.point_light(far_pixel_position(v, w, h, *sky_pixel), 800.0, 0.0)
    out.append(Case("out: point light on a far-plane pixel's reconstructed position", "out", v, [on], pixel_class={tuple(sky_pixel): "nan"},
                    why="at that pixel the fp32 light vector is exactly 0: rsq(0) = Inf, L = 0 * Inf = NaN and irr = intensity * Inf^2, so "
                        "kd = 0 * Inf is NaN whatever the saturates do; the float64 model reconstructs the position more exactly and misses the coincidence"))
    return out


def classify(rgb):
    """Per pixel of (..., 3) float values: 'nan', 'inf', 'zero' (+0 or -0 in all three) or 'finite'."""
    rgb = np.asarray(rgb, np.float64)
    c = np.full(rgb.shape[:-1], "finite", dtype=object)
    c[(rgb == 0).all(-1)] = "zero"
    c[np.isinf(rgb).any(-1)] = "inf"
    c[np.isnan(rgb).any(-1)] = "nan"
    return c


def cleared_planes(w, h):
    return dict(depth=np.ones((h, w), np.float32), diffuse=np.zeros((h, w), np.uint32), specular=np.zeros((h, w), np.uint32),
                normals=np.zeros((h, w, 4), np.uint16), emissive=np.zeros((h, w, 4), np.uint16))


def model_classes(case, w, h):
    """The float64 model's class of every pixel of a cleared w x h frame, (h, w), with the case's own per-pixel knowledge on top."""
    from tests import f64_shading
    pix = f64_shading.Pixels.from_planes(cleared_planes(w, h))
    with np.errstate(all="ignore"):
        ref = f64_shading.reference(pix, case.view, case.lights, case.top, case.bottom)["ref"]
    c = classify(ref.reshape(h, w, 3))
    if case.frame_class is not None:
        c[...] = case.frame_class
    for (px, py), cls in case.pixel_class.items():
        c[py, px] = cls
    return c
