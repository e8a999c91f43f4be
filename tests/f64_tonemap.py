"""The tone mapper (include/vrterrain.h) restated in float64, with derived error bounds.

Test infrastructure: written from the design's description of the three stages, not from the C oracle's code, so that it
can bound both fp32 implementations - the oracle (oracle/vr_oracle.c) and the HIP kernels - from outside.

Histogram.  Luminance L = 0.2126 r + 0.7152 g + 0.0722 b of the decoded halves; position
x = 255 * saturate((log2 L - min_log) / (max_log - min_log)); NaN, L <= 0 and denormal L (below 2^-126) go to x = 0,
L = +inf to x = 255.  A pixel adds Q - floor(Q frac(x)) to bin floor(x) and floor(Q frac(x)) to the next bin, where
Q = 64 >> s is the weight quantum (`quantum`: s the smallest shift with Q * pixels <= 2^32 - 1, pixels of the whole
frame).  Counts are exact integers.

  Bound.  The total is exact: sum(hist) == Q * pixels.  The fp32 position of a pixel lies in [x_lo, x_hi]:
  * delta (`position_delta`): the largest |kernel position - exact position| over EVERY fp32 luminance of the binades
    from 2^(floor(min_log) - 1) to 2^ceil(max_log) (the pinned log2 cubic, the fp32 rounding of scale and bias, the
    saturate and the product by 255, all emulated in fp32).  Outside those binades both positions saturate.  For the
    default range: 0.0190 bins (the cubic's error is 1.5e-3 in log2 units);
  * the fp32 luminance lies within E_LUM * 2^-24 * S of L, S = the same sum of magnitudes (three products, two sums and
    the constants' rounding: 4 roundings, one spare), so x_lo = X(L - e) - delta, x_hi = X(L + e) + delta with X the
    exact map (X of a value below 2^-126 is 0).
  A pixel's contribution to the cumulative count C_k = sum(h[0..k]) is ceil(Q * clamp(k + 1 - x, 0, 1)): the stated
  truncation of the split, which is non-increasing in x.  So the implementation's C_k lies between the model's C_k at
  x_hi (the "bright" envelope) and at x_lo (the "dark" envelope) for every k.  No widening for the truncation is
  needed: the model truncates as stated, and the truncation commutes with the monotone bound.
  Flag "cancel": the relative luminance error bound e / |L| exceeds TAU_CANCEL (negative channels).  Such a pixel is
  still inside the envelope, only with a wide interval.

Exposure.  Exact prefix sums P, T = P[256]; window [T low, T high]; bin i weighs the part of [P[i], P[i+1]] inside the
window; average log2 luminance over the window with bin i at min_log + i (max_log - min_log) / 255 (min_log when the
window is empty); target = clamp(2^avg, min_adapted, max_adapted); adaptation
old + (target - old)(1 - e^(-dt speed)), speed = speed_up when target > old, else speed_down.  Two rules written
down in the header: old <= 0 ("unset") jumps to the target, and so does a direction whose speed is <= 0.

  Bound (i) (`exposure_bound`), on one histogram: the fp32 evaluation rounds T, the two window ends (2 roundings, 2 u T)
  and every prefix sum (u T); the weights are differences of clamped prefix sums, so their errors telescope:
  |dA| <= 2 u T (|l_0| + |l_255| + 255 step) + sum w_i |dl_i| + 9 u sum w_i |l_i| (products and the depth-8 pairwise sum),
  |dW| <= 4 u T + 9 u W; |d avg| <= (|dA| + |avg| |dW|) / W + u |avg|, with dl_i the fp32 bin centres' actual error.
  The target's relative error is then E_EXP + ln2 |d avg| (E_EXP: the pinned exp2 cubic's relative error, over a
  2^-23 grid of the fraction plus its Lipschitz margin), and the adapted value lies in
  [adapt(target - d), adapt(target + d)] (adapt is monotone in the target) widened by u (3 k |diff| + |out|) for the
  step's own fp32 roundings.
  Bound (ii): the value must also lie between the model on the bright and on the dark envelope histograms, each widened
  by its bound (i): the windowed mean is monotone under first-order dominance of equal-total histograms.
  In a sequence, every step is evaluated from the implementation's previous value.

Operator.  With the implementation's adapted value A (min_adapted where A <= 0): s = 2^bias L / A,
mapped = s (1 + s / wp^2) / (1 + s) in the written order, v = c mapped / L per channel, byte = round(255 OETF(saturate v)).
The fp32 operator is within a relative eps of v (`operator`): eps = 2^-24 (E_OP + 2 E_LUM S / |L|), E_OP = 24 (the 21
roundings of exposure scale, 1 / wp^2, 1 / A, scaled, the two brackets, the division and the channel product, plus the
threshold table's own rounding, with margin) and twice the luminance's error (mapped / L has sensitivity below 1 to L,
and L enters twice).  A byte must equal the model's unless round(255 OETF(v (1 - eps))) != round(255 OETF(v (1 + eps))),
the flag "rounding", where either neighbour is accepted.  Where eps >= 1/2 (flag "cancel") any byte is accepted.
Exact classes (never flagged): NaN or L <= 0 -> 0; a negative channel -> 0; a channel with v (1 - eps) >= 1 -> 255, which
includes every pixel where the fp32 written order overflows to +inf; a channel of 0 -> 0; L = +inf -> s = inf,
inf / inf = NaN -> 0 (the IEEE result of the written order: a pixel with a +inf channel is black).

Measured worst ratios and flag counts are printed by the tests and stated in DESIGN.md 7b.
"""
import functools
import math

import numpy as np

U = 2.0 ** -24
BINS = 256
E_LUM = 5.0
E_OP = 24.0
TAU_CANCEL = 1e-3
LOG2_C = (1.4208646, -0.57725066, 0.1563861)
EXP2_C = (0.69583356, 0.22606716, 0.07809929)
LUM_C = (0.2126, 0.7152, 0.0722)


def quantum(pixels):
    """Q = 64 >> s, s the smallest shift with Q * pixels <= 2^32 - 1; 0 when no shift does (pixels >= 2^32)."""
    q = 64
    while q and q * int(pixels) > 2 ** 32 - 1:
        q >>= 1
    return q


def half(codes):
    return np.asarray(codes, np.uint16).view(np.float16).astype(np.float64)


def f32(v):
    return float(np.float32(v))


class PixelSet:
    """Distinct RGB half triplets with their counts (a frame, a sample or a closed-form banded frame)."""

    def __init__(self, codes, counts=None):
        self.codes = np.ascontiguousarray(np.asarray(codes, np.uint16).reshape(-1, 3))
        self.counts = np.ones(len(self.codes), np.int64) if counts is None else np.asarray(counts, np.int64)

    @classmethod
    def from_frame(cls, frame_u16, chunk=1 << 23):
        """Unique RGB triplets of an (h, w, 4) or (n, 4) / (n, 3) uint16 array, in chunks (an 8K frame included)."""
        a = np.asarray(frame_u16, np.uint16)
        a = a.reshape(-1, a.shape[-1])
        keys, counts = [], []
        for i in range(0, len(a), chunk):
            b = a[i:i + chunk, :3].astype(np.uint64)
            k, c = np.unique(b[:, 0] | (b[:, 1] << np.uint64(16)) | (b[:, 2] << np.uint64(32)), return_counts=True)
            keys.append(k); counts.append(c)
        k = np.concatenate(keys); c = np.concatenate(counts)
        k, inv = np.unique(k, return_inverse=True)
        c = np.bincount(inv, weights=c).astype(np.int64)
        codes = np.stack([k & np.uint64(0xffff), (k >> np.uint64(16)) & np.uint64(0xffff), k >> np.uint64(32)], -1).astype(np.uint16)
        return cls(codes, c)

    @property
    def pixels(self):
        return int(self.counts.sum())

    def rgb(self):
        return half(self.codes)


def luminance(rgb):
    """float64 luminance and the sum of magnitudes S of its terms."""
    with np.errstate(invalid="ignore"):
        L = LUM_C[0] * rgb[..., 0] + LUM_C[1] * rgb[..., 1] + LUM_C[2] * rgb[..., 2]
        S = LUM_C[0] * np.abs(rgb[..., 0]) + LUM_C[1] * np.abs(rgb[..., 1]) + LUM_C[2] * np.abs(rgb[..., 2])
    return L, S


def _exact_x(L, p):
    """Exact position of finite luminances; 0 below 2^-126 (denormal, zero, negative)."""
    lo, hi = f32(p.min_log_luminance), f32(p.max_log_luminance)
    L = np.asarray(L, np.float64)
    ok = L >= 2.0 ** -126
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (np.log2(np.where(ok, L, 1.0)) - lo) / (hi - lo)
    return np.where(ok, 255.0 * np.clip(t, 0.0, 1.0), 0.0)


@functools.lru_cache(maxsize=None)
def position_delta(min_log, max_log):
    """max |kernel position - exact position| over every fp32 value of the binades around [min_log, max_log]."""
    F = np.float32
    scale = F(1.0) / (F(max_log) - F(min_log))
    bias = (F(0.0) - F(min_log)) * scale
    c0, c1, c2 = (F(c) for c in LOG2_C)
    mant = (np.arange(1 << 23, dtype=np.uint32) | np.uint32(0x3f800000)).view(np.float32)
    tt = mant - F(1.0)
    p = tt * (c0 + tt * (c1 + tt * c2))
    log2m = np.log2(mant.astype(np.float64))
    worst = 0.0
    for e in range(math.floor(min_log) - 1, math.ceil(max_log) + 1):
        t = (F(e) + p) * scale + bias
        t = np.where(~(t > F(0.0)), F(0.0), np.where(t > F(1.0), F(1.0), t))
        hb = (t * F(255.0)).astype(np.float64)
        x = 255.0 * np.clip((e + log2m - float(min_log)) / (float(max_log) - float(min_log)), 0.0, 1.0)
        worst = max(worst, float(np.abs(hb - x).max()))
    return worst


@functools.lru_cache(maxsize=None)
def exp2_error():
    """Relative error of the pinned exp2 over a 2^-23 grid of the fraction, plus the Lipschitz margin between grid points."""
    F = np.float32
    f = (np.arange(1 << 23, dtype=np.float64) * 2.0 ** -23).astype(np.float32)
    c0, c1, c2 = (F(c) for c in EXP2_C)
    pv = F(1.0) + f * (c0 + f * (c1 + f * c2))
    err = np.abs(pv.astype(np.float64) / np.exp2(f.astype(np.float64)) - 1.0)
    return float(err.max()) + 2.0 ** -22


def positions(ps, p):
    """Model position x of each distinct pixel, its interval [x_lo, x_hi] and the 'cancel' flag."""
    rgb = ps.rgb()
    L, S = luminance(rgb)
    nan, inf = np.isnan(L), np.isposinf(L)
    fin = ~nan & ~inf & ~np.isneginf(L)
    Lf = np.where(fin, L, 0.0)
    e = E_LUM * U * np.where(fin, S, 0.0)
    d = position_delta(f32(p.min_log_luminance), f32(p.max_log_luminance))
    x = np.where(inf, 255.0, _exact_x(Lf, p))
    x_lo = np.where(fin, np.maximum(_exact_x(Lf - e, p) - d, 0.0), x)
    x_hi = np.where(fin, np.minimum(_exact_x(Lf + e, p) + d, 255.0), x)
    with np.errstate(divide="ignore", invalid="ignore"):
        cancel = fin & (e > TAU_CANCEL * np.abs(Lf)) & (Lf + e > 2.0 ** (f32(p.min_log_luminance) - 1))
    return x, x_lo, x_hi, cancel


def histogram_at(x, counts, q):
    """Exact integer histogram of pixels at positions x (counts each): Q - floor(Q frac) left, floor(Q frac) right."""
    x = np.clip(np.asarray(x, np.float64), 0.0, 255.0)
    left = np.floor(x).astype(np.int64)
    rw = np.floor((x - left) * q).astype(np.int64)
    rw = np.where(left >= BINS - 1, 0, rw)
    lw = q - rw
    h = np.bincount(left, weights=(lw * counts).astype(np.float64), minlength=BINS + 1)
    h += np.bincount(left + 1, weights=(rw * counts).astype(np.float64), minlength=BINS + 1)
    assert h.max() < 2.0 ** 53
    return h[:BINS].astype(np.int64)


def histogram_model(ps, p, frame_pixels=None):
    """Model, bright and dark envelope histograms of a pixel set; frame_pixels (default: the set's) fixes Q."""
    q = quantum(ps.pixels if frame_pixels is None else frame_pixels)
    assert q > 0
    x, x_lo, x_hi, cancel = positions(ps, p)
    return dict(q=q, pixels=ps.pixels, model=histogram_at(x, ps.counts, q), bright=histogram_at(x_hi, ps.counts, q),
                dark=histogram_at(x_lo, ps.counts, q), cancel=int(ps.counts[cancel].sum()),
                delta=position_delta(f32(p.min_log_luminance), f32(p.max_log_luminance)))


def check_histogram(got, hm, what=""):
    """Total exact, cumulative counts inside the envelope.  Returns the worst ratio to the envelope's half-width."""
    got = np.asarray(got, np.int64)
    assert got.sum() == hm["q"] * hm["pixels"], f"{what}: total {got.sum()} != Q * pixels = {hm['q'] * hm['pixels']}"
    c, lo, hi, mid = (np.cumsum(a) for a in (got, hm["bright"], hm["dark"], hm["model"]))
    bad = np.nonzero((c < lo) | (c > hi))[0]
    assert bad.size == 0, (f"{what}: cumulative count outside the float64 envelope at bins {bad[:8].tolist()}: "
                           f"got {c[bad[:4]].tolist()}, envelope {lo[bad[:4]].tolist()}..{hi[bad[:4]].tolist()}")
    up = np.where(c > mid, (c - mid) / np.maximum(hi - mid, 1), 0.0)
    dn = np.where(c < mid, (mid - c) / np.maximum(mid - lo, 1), 0.0)
    return float(max(up.max(), dn.max()))


# ---- exposure -----------------------------------------------------------------------------------
def _bin_centres(p):
    lo, hi = f32(p.min_log_luminance), f32(p.max_log_luminance)
    exact = lo + np.arange(BINS) * (hi - lo) / 255.0
    F = np.float32
    scale = F(1.0) / (F(hi) - F(lo))
    bias = (F(0.0) - F(lo)) * scale
    dev = ((np.arange(BINS).astype(np.float32) / F(255.0) - bias) / scale).astype(np.float64)
    return exact, np.abs(dev - exact)


def adapt(target, old, dt, p):
    if not old > 0.0:
        return target
    diff = target - old
    speed = f32(p.eye_adaptation_speed_up) if diff > 0.0 else f32(p.eye_adaptation_speed_down)
    if not speed > 0.0:
        return target
    return old + diff * (1.0 - math.exp(-f32(dt) * speed))


def exposure_model(hist, p, dt, old):
    """float64 exposure of an integer histogram; returns (adapted, target, avg, W)."""
    h = np.asarray(hist, np.int64)
    P = np.concatenate([[0], np.cumsum(h)])
    T = int(P[-1])
    lo, hi = T * f32(p.histogram_low_percentile), T * f32(p.histogram_high_percentile)
    w = np.clip(P[1:], lo, hi) - np.clip(P[:-1], lo, hi)
    l, _ = _bin_centres(p)
    W = float(w.sum())
    avg = float((w * l).sum() / W) if W > 0.0 else f32(p.min_log_luminance)
    target = min(max(2.0 ** avg, f32(p.min_adapted_luminance)), f32(p.max_adapted_luminance))
    return adapt(target, old, dt, p), target, avg, W, w


def exposure_bound(hist, p, dt, old):
    """Bound (i): the interval the fp32 exposure of `hist` must lie in, and the model value."""
    value, target, avg, W, w = exposure_model(hist, p, dt, old)
    T = float(np.asarray(hist, np.int64).sum())
    l, dl = _bin_centres(p)
    if W > 0.0:
        dA = 2 * U * T * (abs(l[0]) + abs(l[-1]) + abs(l[-1] - l[0])) + float((w * dl).sum()) + 9 * U * float((w * np.abs(l)).sum())
        dW = 4 * U * T + 9 * U * W
        davg = (dA + abs(avg) * dW) / W + U * abs(avg)
    else:
        davg = 0.0
    rel = exp2_error() + math.log(2.0) * davg * 1.01 + 2 * U
    dt_ = rel * target
    a, b = adapt(target - dt_, old, dt, p), adapt(target + dt_, old, dt, p)
    k = 1.0 - math.exp(-f32(dt) * max(f32(p.eye_adaptation_speed_up), f32(p.eye_adaptation_speed_down), 0.0))
    slack = U * (3 * k * abs(target - old) + abs(value)) * 1.01 + 1e-300
    return value, min(a, b) - slack, max(a, b) + slack


def check_exposure(got, hist, hm, p, dt, old, what=""):
    """Bounds (i) on the implementation's own histogram and (ii) on the envelopes.  Returns the worst ratios."""
    got = float(got)
    m, lo, hi = exposure_bound(hist, p, dt, old)
    assert lo <= got <= hi, f"{what}: adapted {got!r} outside bound (i) [{lo!r}, {hi!r}] around the model {m!r}"
    r1 = (got - m) / (hi - m) if got > m else ((m - got) / (m - lo) if got < m else 0.0)
    r2 = 0.0
    if hm is not None:
        _, lb, hb = exposure_bound(hm["bright"], p, dt, old)
        _, ld, hd = exposure_bound(hm["dark"], p, dt, old)
        e_lo, e_hi = min(lb, ld), max(hb, hd)
        assert e_lo <= got <= e_hi, f"{what}: adapted {got!r} outside bound (ii) [{e_lo!r}, {e_hi!r}]"
        mm = exposure_model(hm["model"], p, dt, old)[0]
        r2 = (got - mm) / (e_hi - mm) if got > mm else ((mm - got) / (mm - e_lo) if got < mm else 0.0)
    return r1, r2


# ---- operator ---------------------------------------------------------------------------------------
def _oetf255(v):
    v = np.clip(v, 0.0, 1.0)
    return 255.0 * np.where(v <= 0.0031308, 12.92 * v, 1.055 * np.power(v, 1.0 / 2.4) - 0.055)


def _round(y):
    return np.floor(y + 0.5)


def operator(codes, adapted, p):
    """Per channel: model byte (float64 written order), the accepted range [lo, hi] and the classes."""
    rgb = half(np.asarray(codes, np.uint16).reshape(-1, 3))
    L, S = luminance(rgb)
    A = float(np.float32(adapted))
    if not A > 0.0:
        A = f32(p.min_adapted_luminance)
    eb = 2.0 ** f32(p.exposure_bias)
    wp2 = f32(p.white_point) ** 2
    with np.errstate(all="ignore"):
        s = eb * L / A
        mapped = s * (1.0 + s / wp2) / (1.0 + s)
        v = rgb * mapped[:, None] / L[:, None]
        eps = U * (E_OP + 2 * E_LUM * S / np.abs(L))
        e_lum = E_LUM * U * S
    dark = ~(L > 0.0)                                               # NaN, zero, negative
    with np.errstate(invalid="ignore"):
        amb = np.isfinite(L) & ((dark & (L + e_lum > 0.0)) | (~dark & ~(eps < 0.5)))   # sign or size of L unresolved
    dark &= ~amb
    nanv = np.isnan(v) & ~dark[:, None] & ~amb[:, None]             # L = +inf: inf / inf
    v0 = np.where(np.isnan(v), 0.0, v)
    e = np.where(eps < 0.5, eps, 0.5)[:, None]
    with np.errstate(all="ignore"):
        model = _round(_oetf255(v0))
        lo = _round(_oetf255(v0 * (1.0 - e)))
        hi = _round(_oetf255(v0 * (1.0 + e)))
    zero = dark[:, None] | nanv
    cancel = amb[:, None] & (rgb != 0)
    model = np.where(zero, 0, model)
    lo = np.where(zero, 0, np.where(cancel, 0, lo))
    hi = np.where(zero, 0, np.where(cancel, 255, hi))
    cls = dict(dark=dark[:, None] & np.ones((1, 3), bool), inf_nan=nanv, negative=(rgb < 0) & ~zero & ~cancel,
               saturated=(lo == 255) & (hi == 255), rounding=(lo != hi) & ~cancel, cancel=cancel)
    return dict(model=model.astype(np.int64), lo=lo.astype(np.int64), hi=hi.astype(np.int64), eps=e, v=v0, cls=cls)


def check_ldr(got_rgb, codes, adapted, p, what="", counts=None):
    """got_rgb (n, 3) bytes of the pixels `codes` (n, 3).  Returns (worst ratio, flag counts, checked values)."""
    got = np.asarray(got_rgb, np.int64).reshape(-1, 3)
    r = operator(codes, adapted, p)
    bad = np.argwhere((got < r["lo"]) | (got > r["hi"]))
    if bad.size:
        i = bad[0][0]
        raise AssertionError(f"{what}: {len(bad)} LDR values outside the float64 model, first pixel {i}: hdr "
                             f"{np.asarray(codes).reshape(-1, 3)[i].tolist()} got {got[i].tolist()} model {r['model'][i].tolist()} "
                             f"accepted {r['lo'][i].tolist()}..{r['hi'][i].tolist()} (v {r['v'][i].tolist()})")
    # ratio: where the byte differs from the model's, how close 255 OETF(v) is to the rounding midpoint, in units of eps
    diff = (got != r["model"]) & ~r["cls"]["cancel"]
    worst = 0.0
    if diff.any():
        v = r["v"][diff]
        y = _oetf255(v)
        mid = np.floor(y) + 0.5
        dy = np.abs(_oetf255(v * (1.0 + r["eps"][np.nonzero(diff)[0], 0])) - y)
        worst = float((np.abs(y - mid) / np.maximum(dy, 1e-300)).max())
    counts = {k: int(v.sum()) for k, v in r["cls"].items()}
    checked = int(got.size - r["cls"]["cancel"].sum() - r["cls"]["rounding"].sum())
    return worst, counts, checked


# ---- inputs -----------------------------------------------------------------------------------------
def check_step(hist, adapted, ldr_rgb, ps_frame, p, dt, old, what, codes=None, frame_pixels=None):
    """One SimpleRender step of an implementation against the model: histogram envelope, exposure bounds (i) and (ii)
    from the implementation's previous value `old`, and the LDR bytes of `codes` (default: every pixel of ps_frame, in
    which case ldr_rgb holds one row per distinct pixel).  Returns a dict of worst ratios and flag counts."""
    hm = histogram_model(ps_frame, p, frame_pixels)
    rh = check_histogram(hist, hm, what)
    r1, r2 = check_exposure(adapted, hist, hm, p, dt, old, what)
    rl, counts, checked = check_ldr(ldr_rgb, ps_frame.codes if codes is None else codes, adapted, p, what)
    n = np.asarray(ldr_rgb).size
    assert checked > 0.9 * n, (what, checked, n, counts)
    return dict(hist=rh, exp_i=r1, exp_ii=r2, ldr=rl, flags=dict(counts, hist_cancel=hm["cancel"]), checked=checked)


SEQ_W, SEQ_H = 96, 64


def adaptation_cases():
    """(name, parameter overrides, [(frame kind, dt), ...]): bright / dark frames alternating, dt of 0, 1/60 and 1,
    speeds of 0, low == high, percentiles 0 and 1, min == max adapted."""
    alt = [("bright", 1 / 60), ("dark", 1 / 60), ("bright", 1 / 60), ("dark", 1 / 60)]
    dts = [("bright", 0.0), ("dark", 1 / 60), ("bright", 1.0), ("dark", 0.0), ("dark", 1.0), ("mid", 1 / 60)]
    return [("alternate", {}, alt), ("dt", {}, dts),
            ("speeds_0", dict(eye_adaptation_speed_up=0.0, eye_adaptation_speed_down=0.0), alt),
            ("speed_up_0", dict(eye_adaptation_speed_up=0.0), alt + [("mid", 1.0)]),
            ("low_eq_high", dict(histogram_low_percentile=0.9, histogram_high_percentile=0.9), alt),
            ("pct_0_1", dict(histogram_low_percentile=0.0, histogram_high_percentile=1.0), dts),
            ("pct_0_0", dict(histogram_low_percentile=0.0, histogram_high_percentile=0.0), alt[:2]),
            ("pct_1_1", dict(histogram_low_percentile=1.0, histogram_high_percentile=1.0), alt[:2]),
            ("min_eq_max", dict(min_adapted_luminance=0.1, max_adapted_luminance=0.1), alt[:3])]


def sequence_frame(kind, step):
    rng = np.random.default_rng(1000 + step)
    mean = dict(bright=-3.5, dark=-7.0, mid=-5.5)[kind]
    return lognormal_frame(rng, SEQ_W, SEQ_H, mean)


def _to_half(x):
    return np.asarray(x, np.float64).astype(np.float16).view(np.uint16)


def _decompose(L):
    """Half triplets whose luminance is close to L: g carries the bulk, r and b the remainder in finer units."""
    L = np.minimum(np.asarray(L, np.float64), 65504.0 * LUM_C[1])
    g = np.asarray(L / LUM_C[1], np.float64).astype(np.float16).astype(np.float64)
    g = np.where(LUM_C[1] * g > L, np.nextafter(g.astype(np.float16), np.float16(0)).astype(np.float64), g)
    r = ((L - LUM_C[1] * g) / LUM_C[0]).astype(np.float16).astype(np.float64)
    b = np.maximum((L - LUM_C[1] * g - LUM_C[0] * r) / LUM_C[2], 0.0)
    return np.stack([_to_half(r), _to_half(g), _to_half(b)], -1)


def edge_pixels(p, adapted=0.18, q=64):
    """Synthetic edge frame: (n, 3) RGB half codes.
    * every bin boundary and the fractional positions k + j/q (j = 0, 1, q/2, q-1), the blue channel stepped by +-1, +-2
      half ulps around each (fp32 luminances a few ulps apart);
    * the ends of the range (2^min_log, 2^max_log) and values beyond them;
    * every half code in each channel (the other two at 0.25): zeros, denormals, negatives (with positive luminance),
      the largest finite values, +-inf and NaN;
    * every positive finite half as grey (OETF rounding boundaries at any adapted value);
    * grey pixels at each OETF threshold and at the white point for `adapted`, +-2 half ulps."""
    lo, hi = f32(p.min_log_luminance), f32(p.max_log_luminance)
    out = []
    ks = np.arange(BINS)[:, None] + np.array([0.0, 1.0 / q, 0.5, (q - 1.0) / q])[None, :]
    x = ks.reshape(-1)
    x = x[x <= 255.0]
    Ls = 2.0 ** (lo + x * (hi - lo) / 255.0)
    Ls = np.concatenate([Ls, 2.0 ** np.array([lo, hi, lo - 0.5, lo - 1, lo - 20, hi + 0.5, hi + 1]), [65504.0, 2.0 ** -24]])
    base = _decompose(Ls)
    for db in (-2, -1, 0, 1, 2):
        t = base.copy()
        t[:, 2] = (t[:, 2].astype(np.int32) + db).clip(0, 0x7bff).astype(np.uint16)
        out.append(t)
    allh = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    quarter = _to_half(0.25)
    for c in range(3):
        t = np.full((65536, 3), quarter, np.uint16)
        t[:, c] = allh
        out.append(t)
    pos = np.arange(1, 0x7c00, dtype=np.uint16)
    out.append(np.repeat(pos[:, None], 3, 1))
    # grey pixels where v hits an OETF threshold or 1 (s = white point): solve mapped(s) = v for s
    eb = 2.0 ** f32(p.exposure_bias)
    wp = f32(p.white_point)
    kk = np.arange(1, 256) - 0.5
    c = kk / 255.0
    thr = np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)
    vt = np.concatenate([thr, [1.0]])
    s = (-(1.0 - vt) + np.sqrt((1.0 - vt) ** 2 + 4.0 * vt / wp ** 2)) * wp ** 2 / 2.0
    g = _to_half(s * adapted / eb).astype(np.int32)
    for d in (-2, -1, 0, 1, 2):
        gg = (g + d).clip(1, 0x7bff).astype(np.uint16)
        out.append(np.repeat(gg[:, None], 3, 1))
    return np.concatenate(out)


def as_frame(codes, w, fill=0):
    """(n, 3) codes -> (h, w, 4) RGBA16F frame, row-major, padded with `fill` (a half code), alpha 0."""
    n = len(codes)
    h = -(-n // w)
    f = np.full((h * w, 4), fill, np.uint16)
    f[:, 3] = 0
    f[:n, :3] = codes
    return f.reshape(h, w, 4)


def lognormal_frame(rng, w, h, mean_log2, sd=1.5, sky=0.2):
    """A plausible radiance frame: grey-ish lognormal pixels, a fraction `sky` of exact zeros."""
    L = np.exp2(rng.normal(mean_log2, sd, size=(h, w)))
    tint = rng.uniform(0.7, 1.3, size=(h, w, 3))
    rgb = L[..., None] * tint
    rgb[rng.random((h, w)) < sky] = 0.0
    f = np.zeros((h, w, 4), np.uint16)
    f[..., :3] = _to_half(np.minimum(rgb, 60000.0))
    return f


def banded(w, h, bright_rows, value):
    """Closed-form banded frame: the first h - bright_rows rows black, the rest grey `value`.  Returns the PixelSet."""
    g = _to_half(value)
    n_b = w * bright_rows
    return PixelSet(np.array([[0, 0, 0], [g, g, g]], np.uint16), np.array([w * h - n_b, n_b], np.int64))


def banded_share(w, h, bright_rows, value, rank, world, tile=128):
    """The same for the pixels rank `rank` of `world` owns (owner(tx, ty) = (tx + ty) mod world, 128-pixel tiles)."""
    g = _to_half(value)
    tx_n, ty_n = -(-w // tile), -(-h // tile)
    y0 = h - bright_rows
    black = bright = 0
    for ty in range(ty_n):
        rows = range(ty * tile, min(h, ty * tile + tile))
        nb = sum(1 for y in rows if y >= y0)
        for tx in range(tx_n):
            if (tx + ty) % world != rank:
                continue
            cols = min(w, tx * tile + tile) - tx * tile
            bright += nb * cols
            black += (len(rows) - nb) * cols
    return PixelSet(np.array([[0, 0, 0], [g, g, g]], np.uint16), np.array([black, bright], np.int64))
