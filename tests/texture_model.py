"""The definition of rule-based texturing (vr_terrain_texture) in numpy float32: vectorised over the albedo, a Python loop over the
layers, the preparation in Python floats (doubles).  Written from the text of vrenderer_amd/csrc/vr_texture.h's comment, not from
its functions or the kernel; the dab preparation, weight and mask are tests/brush_model.py's and tests/erode_model.py's.

  maps         heightmap w0 x h0 bytes, albedo wa x ha x 4 bytes, both over the world [-S/2, S/2]^2
  preparation  in double, each result rounded to fp32 once: rx = w0 / wa, rz = h0 / ha, kx = max_height / 255 * w0 / S,
               kz = max_height / 255 * h0 / S; per layer, with A(v) = v * 255 / max_height and T(d) = tan(d * pi / 180)^2, the ramps
                 altitude rise  A(alt_lo - alt_fade) .. A(alt_lo)         altitude fall  A(alt_hi) .. A(alt_hi + alt_fade)
                 slope rise     T(max(slope_lo - slope_fade, 0)) .. T(slope_lo)
                 slope fall     T(slope_hi) .. T(min(slope_hi + slope_fade, 89.5))
               a ramp from..to of width wd = to - from > 0 whose 1 / wd is a normal fp32 number is soft: edge = its outer end (`from`
               of a rise, `to` of a fall), inv = 1 / wd; every other ramp is hard: edge = the band's own end, inv = 0; an edge beyond
               fp32's range is +-FLT_MAX
  sample       fx = ((float)i + 0.5f) * rx - 0.5f, clamped to [0, w0 - 1]; i0 = floor(fx), tx = fx - i0, i1 = min(i0 + 1, w0 - 1); z
               likewise
  height texel h = byte; gx = (b[y][min(x + 1, w0 - 1)] - b[y][max(x - 1, 0)]) * 0.5f (integer difference first), gz likewise in y
  albedo texel h, gx, gz each bilinear over (i0, j0) (i1, j0) (i0, j1) (i1, j1): top = q00 + tx * (q10 - q00), bot = q01 + tx *
               (q11 - q01), q = top + tz * (bot - top); s2 = (gx * kx) * (gx * kx) + (gz * kz) * (gz * kz)
  band         soft: r = clamp(p, 0, 1), p = (v - edge) * inv rising, (edge - v) * inv falling, then (r * r) * (3 - 2 * r);
               hard: v >= edge rising, v <= edge falling, as 1 or 0; wl = ((ra_lo * ra_hi) * (rs_lo * rs_hi)) * opacity
  composite    val_c starts as the stored byte; per layer in order and per channel of its mask val_c = clamp(val_c + (m * wl) *
               (color[c] - val_c), 0, 255); the byte is floor(val_c + 0.5); m: the erosions' mask over the dabs prepared for the
               ALBEDO, or 1 everywhere; a texel with m == 0 is not written

Every array operation below is one IEEE fp32 operation per element, in the written order, so the result is the device's, bit for
bit."""
import math

import numpy as np

from tests.erode_model import mask_of

F = np.float32
FLT_MAX = float(np.finfo(np.float32).max)
FLT_MIN = float(np.finfo(np.float32).tiny)
WHOLE_MAP = 1
RAMPS = ("alt_lo", "alt_hi", "slope_lo", "slope_hi")
FIELDS = ("color", "opacity", "alt_lo", "alt_hi", "alt_fade", "slope_lo", "slope_hi", "slope_fade", "channel_mask")


def layer(color, opacity, alt_lo, alt_hi, alt_fade, slope_lo, slope_hi, slope_fade, channel_mask=0xF):
    """A layer as a dict with fp32-exact values (what the C struct carries)."""
    return dict(color=tuple(float(F(c)) for c in color), opacity=float(F(opacity)), alt_lo=float(F(alt_lo)), alt_hi=float(F(alt_hi)),
                alt_fade=float(F(alt_fade)), slope_lo=float(F(slope_lo)), slope_hi=float(F(slope_hi)), slope_fade=float(F(slope_fade)),
                channel_mask=int(channel_mask))


def _round(v):
    return F(min(max(v, -FLT_MAX), FLT_MAX))


def _ramp(lo, hi, rise):
    wd = hi - lo
    if wd > 0.0:
        r = 1.0 / wd
        if r <= FLT_MAX and float(F(r)) >= FLT_MIN:
            return _round(lo if rise else hi), F(r)
    return _round(hi if rise else lo), F(0)


def _tan2(deg):
    t = math.tan(deg * 3.14159265358979323846 / 180.0)
    return t * t


def prepare_layer(l, max_height):
    mh = float(F(max_height))
    A = 255.0 / mh
    below, above = max(l["slope_lo"] - l["slope_fade"], 0.0), min(l["slope_hi"] + l["slope_fade"], 89.5)
    return dict(color=[F(c) for c in l["color"]], opacity=F(l["opacity"]), channel_mask=l["channel_mask"],
                alt_lo=_ramp((l["alt_lo"] - l["alt_fade"]) * A, l["alt_lo"] * A, True),
                alt_hi=_ramp(l["alt_hi"] * A, (l["alt_hi"] + l["alt_fade"]) * A, False),
                slope_lo=_ramp(_tan2(below), _tan2(l["slope_lo"]), True),
                slope_hi=_ramp(_tan2(l["slope_hi"]), _tan2(above), False))


def _axis(n_albedo, r, n):
    f = (np.arange(n_albedo, dtype=F) + F(0.5)) * r - F(0.5)
    f = np.minimum(np.maximum(f, F(0)), F(n - 1)).astype(F)
    i0 = np.floor(f).astype(np.int64)
    return i0, np.minimum(i0 + 1, n - 1), (f - i0.astype(F)).astype(F)


def sample(hm, albedo_shape, max_height, world_size):
    """(h, s2, detail): float32 (ha, wa) each; detail: the sample points, for the tests' preconditions."""
    h0, w0 = hm.shape
    ha, wa = albedo_shape[:2]
    mh, S = float(F(max_height)), float(F(world_size))
    rx, rz = _round(w0 / wa), _round(h0 / ha)
    kx, kz = _round(mh / 255.0 * w0 / S), _round(mh / 255.0 * h0 / S)
    b = hm.astype(np.int32)
    xs, ys = np.arange(w0), np.arange(h0)
    hf = b.astype(F)
    gx = (b[:, np.minimum(xs + 1, w0 - 1)] - b[:, np.maximum(xs - 1, 0)]).astype(F) * F(0.5)
    gz = (b[np.minimum(ys + 1, h0 - 1), :] - b[np.maximum(ys - 1, 0), :]).astype(F) * F(0.5)
    i0, i1, tx = _axis(wa, rx, w0)
    j0, j1, tz = _axis(ha, rz, h0)
    tx, tz = tx[None, :], tz[:, None]

    def lerp2(q):
        q00, q10, q01, q11 = q[np.ix_(j0, i0)], q[np.ix_(j0, i1)], q[np.ix_(j1, i0)], q[np.ix_(j1, i1)]
        top = q00 + tx * (q10 - q00)
        bot = q01 + tx * (q11 - q01)
        return (top + tz * (bot - top)).astype(F)

    h, sx, sz = lerp2(hf), lerp2(gx), lerp2(gz)
    ax, az = sx * kx, sz * kz
    s2 = (ax * ax + az * az).astype(F)
    return h, s2, dict(i0=i0, i1=i1, j0=j0, j1=j1, tx=tx, tz=tz)


def _smooth(p):
    r = np.minimum(np.maximum(p, F(0)), F(1))
    return ((r * r) * (F(3) - F(2) * r)).astype(F)


def ramp_value(v, ramp, rise):
    edge, inv = ramp
    with np.errstate(over="ignore"):
        if inv == 0:
            return np.where(v >= edge if rise else v <= edge, F(1), F(0)).astype(F)
        return _smooth((v - edge) * inv if rise else (edge - v) * inv)


def ramps_of(p, h, s2):
    """The four ramp values of a prepared layer, in the order of RAMPS."""
    return [ramp_value(h, p["alt_lo"], True), ramp_value(h, p["alt_hi"], False), ramp_value(s2, p["slope_lo"], True), ramp_value(s2, p["slope_hi"], False)]


def layer_weight(p, h, s2):
    ra_lo, ra_hi, rs_lo, rs_hi = ramps_of(p, h, s2)
    return (((ra_lo * ra_hi) * (rs_lo * rs_hi)) * p["opacity"]).astype(F)


def texture(hm, al, layers, max_height, world_size, dabs=None, whole_map=False, detail=None):
    """One call on a copy of `al` ((ha, wa, 4) uint8) under the heightmap `hm` ((h0, w0) uint8) -> (new albedo, rect).  `detail`, a dict,
    receives what the tests' preconditions need: the mask, h, s2, the sample points, the prepared layers and their weights."""
    ha, wa = al.shape[:2]
    if whole_map:
        assert dabs is None or len(dabs) == 0
        m, rect = np.ones((ha, wa), F), (0, 0, wa, ha)
    else:
        m, rect = mask_of((ha, wa), dabs if dabs is not None else np.zeros((0, 5), F), world_size)
    h, s2, points = sample(hm, al.shape, max_height, world_size)
    prepared = [prepare_layer(l, max_height) for l in layers]
    val = al.astype(F)
    weights = []
    for p in prepared:
        wl = layer_weight(p, h, s2)
        weights.append(wl)
        a = m * wl
        for c in range(4):
            if p["channel_mask"] >> c & 1:
                new = val[..., c] + a * (p["color"][c] - val[..., c])
                val[..., c] = np.minimum(np.maximum(new, F(0)), F(255))
    out = np.where((m > F(0))[..., None], np.floor(val + F(0.5)).astype(np.uint8), al).astype(np.uint8)
    if detail is not None:
        detail.update(mask=m, h=h, s2=s2, points=points, prepared=prepared, weights=weights)
    return out, tuple(rect)
