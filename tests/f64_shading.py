"""The deferred lighting model (vr_deferred_dev.h) restated in float64, with a per-value error bound.

Test infrastructure: it is written from the model's formulas, not from the C oracle's code, so that it can bound both
fp32 implementations of the model - the oracle (oracle/vr_oracle.c) and the HIP kernels - from outside.

It works on pixel lists (x, y and the five texel words of each pixel), so that a seeded sample of a large frame can be
checked as well as a whole small one.  `reference()` returns, for every output value, the float64 result of the model and
a tolerance:

    tol = half rounding + B * 2^-24 * (sum of the magnitudes of the added terms) + A * spread

* half rounding: 2^-11 |ref|, at least 2^-25 (the subnormal half range);
* the B term bounds the rounding of the sums and products that make the value (per channel: every light's diffuse
  and specular term, the two ambient terms and the emissive value);
* `spread` is the largest change of the float64 result when its fp32 inputs are multiplied by independent factors
  1 +- K * 2^-24 (TRIALS random sign patterns): depth, the decoded N and roughness, the pixel-centre clip coordinates,
  clip_to_world, the camera, the light vectors and positions, cosH / sinH and the shadow light's world_to_clip.  A
  stable fp32 evaluation equals the exact one at slightly perturbed inputs (backward error), so the spread measures the
  conditioning that no fp32 evaluation can beat - clip -> world cancellation far from the camera, GGX highlights.

A value of a pixel in a named ill-conditioned class is excluded from that bound (flags, per pixel):

* AREA: sinT < TAU_AREA where the area-light correction rotates L towards R (R close to -L: the rotation direction
  is undefined);
* GRAZING: |N.L|, |N.CL| or |N.V| below TAU_GRAZING (the saturate kinks; with roughness -1, kk = 0 and 0/0);
* PCF: a shadow-map comparison or the in-map test of u, v, zc within rounding of flipping (a texel floor flip needs
  no flag: the tent's value is continuous across it);
* OVERFLOW: the value is within its tolerance of the half overflow threshold 65520.

Such a value must still lie in an envelope: between the pixel's result with the flagged light's contribution removed
and that result plus a bound of what the light can add (PCF: between the light fully shadowed and fully lit).  NaN in
the model (emissive NaN, or 0 * inf where kk = 0 and N.L or N.V saturate to 0) must be NaN in the implementation, an
infinity the same infinity.

Constants (ratio = error / tolerance over the unflagged values; measured on the edge-case frame, the terrain frames,
the 1024-light tiled frame, the 8K sample and the deferred fuzz test):

* K = 8: an fp32 input carries one rounding of its own; 8 covers the few roundings of the expression that produced it
  (window -> clip, decode, the dot products behind the saturated cosines, which are perturbed too).
* TRIALS = 6 sign patterns: with 4, one GGX highlight pixel (roughness 0.01) of the oracle reached ratio 1.02.
* A = 12, B = 32: the worst ratio is 0.9986 for the C oracle and 0.999 for the kernels (0.38 to 0.993 on the terrain
  frames, the 1024-light frame and the 8K sample).  It is dominated by the
  half rounding term (a value next to a rounding midpoint uses all of its 2^-11): the fp32 error proper is a small
  fraction of the budget, and a kernel change that moves a value by more than its half-rounding step fails.
  The all-light-type tiled kernels (test_tiled_ex_f64.py), kernel / oracle on the same input - equal to four digits
  everywhere, the worst value being one next to a rounding midpoint that both round alike: edge frame 512 `extra`
  0.9985 / 0.9985, 13 lights 0.9966 / 0.9966; edge frame 508 `extra` 0.9956 / 0.9956, 13 lights (row-major, packed) and
  suns + points 0.9947 / 0.9947; PCF frame, sun first (w = 1, 2, packed) and second 0.9986 / 0.9986, fourth of four and
  with every light type 0.9862 / 0.9862; 300 lights in one tile 0.9665 / 0.9665; terrain from the tile pass's ranges
  0.8142 / 0.8142.
* TAU_AREA = 1e-4 (sinT): the R = -L pixels; 1e-3 flags the same pixels on these frames.
* TAU_GRAZING = 1e-5: below it fp32 and float64 may disagree on whether a saturate clamps to 0 (exact zeros, as
  axis-aligned vectors give them, are not flagged).
* PCF_MARGIN = 4 x the spread of u, v, zc, plus 2^-22 relative.  The shadow tests use pcf_frame, whose geometry is
  exact in fp32 (asserted): there no comparison is ambiguous and the class is empty; the margin serves other frames.

Caps: check() defaults to 1e-4 of the checked values per class (real frames, the PCF frame).  The edge-case frame
exceeds that on purpose - EDGE_CAPS, up to 120 pixels of its 65,536 (5e-4 of the values): its bands concentrate the
classes (back-facing normals and a 20 degree sun give R = -L pixels, normals perpendicular to each sun, a block of
overflowing values under a light 1e-3 above the surface).  A flagged value whose envelope has no upper end (kk = 0:
the GGX peak 1 / (kk gv) is unbounded) keeps its lower end and is counted in the class "unbounded", capped as well.

Roughness codes <= -32767 decode to -1, where kk = 0.  The model is the design's formula there: G = 1 / (gl gv) with
gl = N.L, gv = N.V, so a light with N.L saturated to 0 gives 0 * inf = NaN and N.V = 0 gives inf.  The kernels and the
oracle produce the same, and these tests pin it: the tile pass never writes a negative roughness (it writes 32767), so
such texels only come from uploaded G-buffers, and the model defines their value rather than a clamp nobody specified.
A change that clamps kk must change this model with it.
"""
import numpy as np

U24 = 2.0 ** -24
K = 8.0
A = 12.0
B = 32.0
TRIALS = 6
TAU_AREA = 1e-4
TAU_GRAZING = 1e-5
PCF_MARGIN = 4.0
HALF_OVERFLOW = 65520.0

CLASSES = ("area", "grazing", "pcf", "overflow")         # (+ "unbounded": see check())

VR_LIGHT_DIRECTIONAL, VR_LIGHT_SPOT, VR_LIGHT_POINT = 1, 2, 3          # include/vrterrain.h


def srgb_eotf(codes):
    """sRGB8 -> linear from the EOTF formula (IEC 61966-2-1), float64."""
    c = np.asarray(codes, np.float64) / 255.0
    return np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)


def snorm16(codes):
    return np.maximum(np.asarray(codes).astype(np.int16).astype(np.float64) / 32767.0, -1.0)


def half(codes):
    return np.asarray(codes, np.uint16).view(np.float16).astype(np.float64)


class Pixels:
    """A list of pixels of a w x h frame: positions and texel words."""

    def __init__(self, w, h, px, py, depth, diffuse, specular, normals, emissive):
        self.w, self.h = w, h
        self.px, self.py = np.asarray(px, np.int64), np.asarray(py, np.int64)
        self.depth = np.asarray(depth, np.float32)
        self.diffuse, self.specular = np.asarray(diffuse, np.uint32), np.asarray(specular, np.uint32)
        self.normals, self.emissive = np.asarray(normals, np.uint16).reshape(-1, 4), np.asarray(emissive, np.uint16).reshape(-1, 4)

    @classmethod
    def from_planes(cls, planes, px=None, py=None):
        """planes: dict (or object with attributes) depth, diffuse, specular, normals, emissive of shape (h, w[, 4])."""
        get = (lambda k: planes[k]) if isinstance(planes, dict) else (lambda k: getattr(planes, k))
        h, w = get("depth").shape
        if px is None:
            py, px = np.divmod(np.arange(w * h), w)
        return cls(w, h, px, py, get("depth")[py, px], get("diffuse")[py, px], get("specular")[py, px],
                   get("normals")[py, px], get("emissive")[py, px])

    def __len__(self):
        return len(self.px)


def _light_params(l):
    half_ang = 0.5 * float(l.angular_size_or_inv_range) if l.type == VR_LIGHT_DIRECTIONAL else 0.0
    return dict(type=int(l.type), dir=np.array(l.direction[:], np.float64), pos=np.array(l.position[:], np.float64),
                color=np.array(l.color[:], np.float64), intensity=float(l.intensity), radius=float(l.radius),
                inv_range=float(l.angular_size_or_inv_range) if l.type != VR_LIGHT_DIRECTIONAL else 0.0,
                inner=float(l.inner_angle), outer=float(l.outer_angle), cosH=np.cos(half_ang), sinH=np.sin(half_ang),
                oob=float(l.out_of_bounds_shadow))


def _dot(a, b):
    return (a * b).sum(-1)


def _near0(x):
    """|x| < TAU_GRAZING, an exact 0 (axis vectors: fp32 gives it exactly too) excepted."""
    return (np.abs(x) < TAU_GRAZING) & (x != 0)


def _shadow_geometry(wp, w2c, res):
    c = np.concatenate([wp, np.ones_like(wp[:, :1])], -1)[:, :, None] * w2c.reshape(-1, 4, 4)
    c = c.sum(1)
    xc, yc, zc = c[:, 0] / c[:, 3], c[:, 1] / c[:, 3], c[:, 2] / c[:, 3]
    u, v = xc * 0.5 + 0.5, 0.5 - yc * 0.5
    return u, v, zc, u * res - 0.5, v * res - 0.5


def _pcf(u, v, zc, tx, ty, sh, lit=None, inside=None):
    """The 4x4 tent [1-f, 1, 1, f]^2 / 9 with LessEqual against receiver depth - bias, clamp addressing."""
    res = sh["res"]
    fxl, fyl = np.floor(tx), np.floor(ty)
    fx, fy = tx - fxl, ty - fyl
    ix, iy = fxl.astype(np.int64) - 1, fyl.astype(np.int64) - 1
    ins = (u >= 0) & (u <= 1) & (v >= 0) & (v <= 1) & (zc >= 0) & (zc <= 1) if inside is None else inside
    z = zc - sh["bias"]
    xs = np.clip(ix[:, None] + np.arange(4), 0, res - 1)
    ys = np.clip(iy[:, None] + np.arange(4), 0, res - 1)
    d = sh["depth"][ys[:, :, None], xs[:, None, :]]                      # (n, 4 rows, 4 texels)
    if lit is None:
        lit = z[:, None, None] <= d
    wx = np.stack([1 - fx, np.ones_like(fx), np.ones_like(fx), fx], -1)
    wy = np.stack([1 - fy, np.ones_like(fy), np.ones_like(fy), fy], -1)
    sf = (lit * wx[:, None, :] * wy[:, :, None]).sum((1, 2)) / 9.0
    return np.where(ins, sf, sh["oob"]), lit, ins, z[:, None, None] - d


def _evaluate(pix, view, lights, amb_top, amb_bot, shadow, rng=None, fixed=None):
    """One float64 evaluation; with rng, every fp32 input is multiplied by its own 1 +- K 2^-24.  Returns the output,
    the per-term magnitudes, per-light contributions and the quantities the flags and the PCF need."""
    n = len(pix)

    def pert(x):
        x = np.asarray(x, np.float64)
        if rng is None:
            return x
        shape = (n,) + x.shape if x.ndim == 0 or x.shape[0] != n else x.shape
        return x * (1.0 + K * U24 * rng.choice((-1.0, 1.0), size=shape))

    alb = np.stack([srgb_eotf((pix.diffuse >> s) & 255) for s in (0, 8, 16)], -1)
    f0 = np.stack([srgb_eotf((pix.specular >> s) & 255) for s in (0, 8, 16)], -1)
    occ = (pix.specular >> 24).astype(np.float64) / 255.0
    nn = snorm16(pix.normals)
    N, rough = pert(nn[:, :3]), pert(nn[:, 3])
    E = half(pix.emissive[:, :3])
    cx = pert((pix.px + 0.5) * 2.0 / pix.w - 1.0)
    cy = pert(1.0 - (pix.py + 0.5) * 2.0 / pix.h)
    depth = pert(pix.depth)
    c2w = pert(np.broadcast_to(np.array(view.clip_to_world[:], np.float64), (n, 16))).reshape(n, 4, 4)
    clip = np.stack([cx, cy, depth, np.ones(n)], -1)
    wp4 = (clip[:, :, None] * c2w).sum(1)
    wp = wp4[:, :3] / wp4[:, 3:]
    cam = pert(np.broadcast_to(np.array(view.camera_pos[:3], np.float64), (n, 3)))
    vi = wp - cam
    vi = vi / np.linalg.norm(vi, axis=-1, keepdims=True)
    V = -vi
    R = vi - 2.0 * _dot(vi, N)[:, None] * N
    ndv_raw = _dot(N, V)
    ndv = np.clip(pert(np.clip(ndv_raw, 0.0, 1.0)), 0.0, 1.0)
    alpha = np.maximum(0.01, rough * rough)
    kk = (rough + 1.0) ** 2 / 8.0
    gv = ndv * (1.0 - kk) + kk
    dterm, sterm, mag = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3))
    per_light, upper = [], []
    live = (nn[:, :3] != 0).any(-1)                     # a zero normal (clear values) makes every term an exact 0
    grazing = live & _near0(ndv_raw)
    area = np.zeros(n, bool)
    sinfo = None
    for i, l in enumerate(lights):
        p = _light_params(l)
        cosH, sinH = pert(p["cosH"]), pert(p["sinH"])
        if p["type"] == VR_LIGHT_DIRECTIONAL:
            L = -pert(np.broadcast_to(p["dir"], (n, 3)))
            irr = np.full(n, p["intensity"])
            reach = np.ones(n, bool)
        else:
            stl = pert(np.broadcast_to(p["pos"], (n, 3))) - wp
            d2 = _dot(stl, stl)
            dist = np.sqrt(d2)
            L = stl / dist[:, None]
            att = np.ones(n)
            if p["inv_range"] > 0:
                att = np.clip(1.0 - (d2 * p["inv_range"] ** 2) ** 2, 0.0, 1.0) ** 2
            spot = np.ones(n)
            if p["type"] == VR_LIGHT_SPOT:
                ang = np.arccos(np.clip(-_dot(L, p["dir"]), -1.0, 1.0))
                ts = np.clip((ang - p["inner"]) / (p["outer"] - p["inner"]), 0.0, 1.0)
                spot = 1.0 - ts * ts * (3.0 - 2.0 * ts)                   # 1 - smoothstep(inner, outer, angle)
            if p["radius"] > 0:
                ha = np.arctan(np.minimum(p["radius"] / dist, 1.0))
                irr = p["intensity"] / p["radius"] ** 2 * ha ** 2
                cosH, sinH = pert(np.cos(ha)), pert(np.sin(ha))
            else:
                irr = p["intensity"] / d2
            irr = irr * spot * att
            reach = (att > 0) & (spot > 0)
        if shadow is not None and i == shadow["light_index"]:
            w2c = pert(np.broadcast_to(shadow["w2c"], (n, 16)))
            geo = _shadow_geometry(wp, w2c, shadow["res"])
            if fixed is not None:
                sf, lit, ins, margin = _pcf(*geo, shadow, lit=fixed["lit"], inside=fixed["inside"])
            else:
                sf, lit, ins, margin = _pcf(*geo, shadow)
            sinfo = dict(geo=np.stack(geo, -1), wp=wp, lit=lit, inside=ins, margin=margin, sf=sf, irr=irr.copy())
            irr = irr * sf
            reach = reach & (sf != 0)
        ndl_raw = _dot(N, L)
        kd = np.maximum(ndl_raw, 0.0) / np.pi * irr
        # area-light correction: slerp(L, R, saturate(half / angle(L, R)))
        cosT = np.clip(_dot(R, L), -1.0, 1.0)
        ha = np.arctan2(sinH, cosH)
        theta = np.arccos(cosT)
        sinT = np.sqrt(1.0 - cosT * cosT)
        rot = theta > ha
        t = np.where(rot, ha / np.where(rot, theta, 1.0), 1.0)
        st = np.where(rot, np.sin(theta), 1.0)
        wa = np.where(rot, np.sin((1.0 - t) * theta) / st, 0.0)
        wb = np.where(rot, np.sin(t * theta) / st, 1.0)
        CL = wa[:, None] * L + wb[:, None] * R
        H = CL + V
        hn = np.linalg.norm(H, axis=-1)
        H = np.where(hn[:, None] > 0, H / np.where(hn > 0, hn, 1.0)[:, None], 0.0)
        ndcl_raw = _dot(N, CL)
        # the saturated cosines carry their own rounding: perturbed after the clamp, so that a clamped 1 (N.H of a
        # highlight) may also be 1 - K 2^-24, as an fp32 evaluation can give it
        ndh = np.clip(pert(np.clip(_dot(N, H), 0.0, 1.0)), 0.0, 1.0)
        ndl = np.clip(pert(np.clip(ndcl_raw, 0.0, 1.0)), 0.0, 1.0)
        vdh = np.clip(pert(np.clip(_dot(V, H), 0.0, 1.0)), 0.0, 1.0)
        tanH = sinH / cosH
        ca = np.clip(alpha + 0.5 * tanH, 0.0, 1.0)
        D = alpha ** 2 / (np.pi * (ndh ** 2 * (alpha ** 2 - 1.0) + 1.0) ** 2) * (alpha / ca) ** 2
        G = 1.0 / ((ndl * (1.0 - kk) + kk) * gv)
        F = f0 + (1.0 - f0) * ((1.0 - vdh) ** 5)[:, None]
        col = p["color"]
        dl = alb * kd[:, None] * col
        sl = F * (D * G * ndl / 4.0 * irr)[:, None] * col
        dl = np.where(reach[:, None], dl, 0.0)
        sl = np.where(reach[:, None], sl, 0.0)
        dterm, sterm = dterm + dl, sterm + sl
        mag = mag + np.abs(dl) + np.abs(sl)
        per_light.append(dl + sl)
        # what the light can add at most: Lambert + the GGX lobe's peak (F <= 1, NdotL <= 1, gl >= kk)
        full_irr = sinfo["irr"] if (sinfo is not None and i == shadow["light_index"]) else irr
        smax = (alpha / ca) ** 2 / (4.0 * np.pi * alpha ** 2 * np.minimum(kk, 1.0) * gv)
        upper.append(np.where(reach | (full_irr > 0), 1.0, 0.0)[:, None] * np.abs(full_irr)[:, None] * np.abs(col)
                     * (alb / np.pi + smax[:, None]))
        area_i = reach & rot & (sinT < TAU_AREA)
        graz_i = reach & (_near0(ndl_raw) | _near0(ndcl_raw))
        area |= live & area_i
        grazing |= live & graz_i
    tt = N[:, 1] * 0.5 + 0.5
    at, ab = np.array(amb_top, np.float64), np.array(amb_bot, np.float64)
    amb = (ab + (at - ab) * tt[:, None]) * occ[:, None]
    out = (dterm + amb * alb) + (sterm + amb * f0) + E
    mag = mag + np.abs(amb * alb) + np.abs(amb * f0) + np.abs(E)
    return dict(out=out, mag=mag, per_light=per_light, upper=upper, area=area, grazing=grazing, shadow=sinfo)


def _shadow_dict(shadow):
    if shadow is None:
        return None
    lv, depth, li, bias, oob = shadow
    depth = np.asarray(depth, np.float64)
    return dict(w2c=np.array(lv.world_to_clip[:], np.float64), depth=depth, res=depth.shape[0], light_index=li,
                bias=float(np.float32(bias)), oob=float(oob))


def _reaching(pix, view, lights, sh):
    """The lights without the ranged ones that reach none of the pixels by a wide margin (their term is an exact 0 in
    every evaluation; dropping them keeps long light lists cheap)."""
    if sh is not None or len(lights) <= 16:
        return lights
    wp = world_position(view, pix.w, pix.h, pix.px, pix.py, pix.depth)
    keep = []
    for l in lights:
        if l.type != VR_LIGHT_DIRECTIONAL and l.angular_size_or_inv_range > 0:
            d2 = ((wp - np.array(l.position[:], np.float64)) ** 2).sum(-1)
            if np.nanmin(d2) * float(l.angular_size_or_inv_range) ** 2 > 1.01:
                continue
        keep.append(l)
    return keep


def reference(pix, view, lights, amb_top, amb_bot, shadow=None, seed=0, exact_geometry=False):
    """shadow = (light view, res x res depth, light index, depth bias, out_of_bounds value) or None.
    Returns dict(ref (n, 3), tol (n, 3), flags {class: (n,) bool}, lo, hi (envelopes), and the model's inputs).
    exact_geometry: True - the frame's matrices make every step of window -> world -> light clip -> texel coordinates exact in
    fp32 (asserted: each value of the chain is an fp32 number, so a correctly rounded fp32 evaluation gives exactly it);
    then no shadow comparison or in-map test is ambiguous and none is flagged - a receiver exactly at a stored depth,
    u / v exactly 0 or 1 and zc exactly 0 or 1 are held to the tight bound.  "vz": the same for everything but the
    window -> clip x (a frame width that is not a power of two), so only the in-map test of u is flagged when ambiguous."""
    sh = _shadow_dict(shadow)
    lights = _reaching(pix, view, lights, sh)
    with np.errstate(all="ignore"):
        base = _evaluate(pix, view, lights, amb_top, amb_bot, sh)
        fixed = None if base["shadow"] is None else dict(lit=base["shadow"]["lit"], inside=base["shadow"]["inside"])
        rng = np.random.default_rng(seed)
        spread = np.zeros_like(base["out"])
        geo_spread = None
        for _ in range(TRIALS):
            p = _evaluate(pix, view, lights, amb_top, amb_bot, sh, rng=rng, fixed=fixed)
            dv = np.abs(p["out"] - base["out"])
            spread = np.maximum(spread, np.where(np.isfinite(dv), dv, 0.0))
            if fixed is not None:
                dg = np.abs(p["shadow"]["geo"] - base["shadow"]["geo"])
                geo_spread = dg if geo_spread is None else np.maximum(geo_spread, dg)
        ref = base["out"]
        halfr = np.maximum(2.0 ** -11 * np.abs(ref), 2.0 ** -25)
        tol = halfr + B * U24 * base["mag"] + A * spread
        flags = dict(area=base["area"], grazing=base["grazing"], pcf=np.zeros(len(pix), bool))
        lo, hi = ref.copy(), ref.copy()
        for i in range(len(lights)):
            sel = (base["area"] | base["grazing"])[:, None]
            off = ref - base["per_light"][i]
            lo = np.where(sel, np.minimum(lo, off), lo)
            hi = np.where(sel, np.maximum(hi, off + base["upper"][i]), hi)
        if fixed is not None and exact_geometry:
            s = base["shadow"]
            u, v, zc, tx, ty = s["geo"].T
            z = zc - sh["bias"]
            if exact_geometry == "vz":              # a width that is not a power of two: the window -> clip x is rounded
                chain = np.stack([s["wp"][:, 1], s["wp"][:, 2], v, zc, ty, z], -1)
            else:
                chain = np.concatenate([s["wp"], s["geo"], z[:, None]], -1)
            assert (chain.astype(np.float32).astype(np.float64) == chain).all(), "the shadow geometry is not exact in fp32"
            if exact_geometry == "vz":
                # the comparisons and v are exact; u carries the rounding of x (a texel floor flip is continuous): only
                # the in-map test of u can be ambiguous
                mu = PCF_MARGIN * geo_spread[:, 0] + 2.0 ** -22 * (np.abs(u) + 1.0)
                flags["pcf"] = (np.abs(u) <= mu) | (np.abs(u - 1) <= mu)
        elif fixed is not None:
            s = base["shadow"]
            u, v, zc = s["geo"].T[:3]
            m = PCF_MARGIN * geo_spread + 2.0 ** -22 * (np.abs(s["geo"]) + 1.0)
            mu, mv, mz = m.T[:3]
            near = lambda x, e, edge: np.abs(x - edge) <= e                                  # noqa: E731
            pcf = near(u, mu, 0) | near(u, mu, 1) | near(v, mv, 0) | near(v, mv, 1) | near(zc, mz, 0) | near(zc, mz, 1)
            mz_cmp = mz + 2.0 ** -22 * (np.abs(zc) + abs(sh["bias"]))
            pcf |= s["inside"] & (np.abs(s["margin"]) <= mz_cmp[:, None, None]).any((1, 2))
            flags["pcf"] = pcf
        if fixed is not None:
            s, pcf = base["shadow"], flags["pcf"]
            li = sh["light_index"]
            p_on = base["per_light"][li] / np.where(s["sf"] != 0, s["sf"], 1.0)[:, None]
            off = ref - base["per_light"][li]
            # fully shadowed .. fully lit: sf in [0, 1] scales the light's term (sf = 0 drops it)
            full = np.where((s["sf"] != 0)[:, None], off + p_on, off + base["upper"][li])
            lo = np.where(pcf[:, None], np.minimum(lo, np.minimum(off, full)), lo)
            hi = np.where(pcf[:, None], np.maximum(hi, np.maximum(off, full)), hi)
        ovf = np.isfinite(ref) & (np.abs(ref) + tol >= HALF_OVERFLOW) & (np.abs(ref) - tol < HALF_OVERFLOW)
        flags["overflow"] = ovf.any(-1)
    return dict(ref=ref, tol=tol, flags=flags, lo=lo, hi=hi, spread=spread,
                shadow_geo=None if base["shadow"] is None else base["shadow"]["geo"])


def check(got, r, pix, what, caps=None):
    """got: (n, 3) float64 (half values of the implementation).  Asserts the tight bound on unflagged values, the
    envelope on flagged ones, NaN / infinity agreement and the class caps (dict class -> maximum pixel count; default:
    1e-4 of the checked values, at least 0).  Returns dict(worst ratio, class counts)."""
    with np.errstate(all="ignore"):
        return _check(np.asarray(got, np.float64).reshape(-1, 3), r, pix, what, caps)


def _check(got, r, pix, what, caps):
    ref, tol = r["ref"], r["tol"]
    flagged = np.zeros(len(pix), bool)
    for c in CLASSES:
        flagged |= r["flags"][c]
    counts = {c: int(r["flags"][c].sum()) for c in CLASSES}

    def where(i):
        i = int(i)
        return (f"pixel ({pix.px[i]}, {pix.py[i]}) depth {pix.depth[i]!r} diffuse {pix.diffuse[i]:#010x} specular "
                f"{pix.specular[i]:#010x} normals {pix.normals[i].view(np.int16).tolist()} emissive "
                f"{half(pix.emissive[i]).tolist()}: got {got[i].tolist()} model {ref[i].tolist()} tol {tol[i].tolist()} "
                f"flags {[c for c in CLASSES if r['flags'][c][i]]}")

    nan_ref = np.isnan(ref)
    bad = nan_ref != np.isnan(got)
    if bad.any():
        i = np.argwhere(bad)[0][0]
        raise AssertionError(f"{what}: {int(bad.sum())} values NaN on one side only; {where(i)}")
    inf_ref = np.isinf(ref)
    bad = inf_ref & (got != ref)
    if bad.any():
        raise AssertionError(f"{what}: {int(bad.sum())} infinite model values differ; {where(np.argwhere(bad)[0][0])}")
    fin = ~nan_ref & ~inf_ref
    over = fin & (np.abs(ref) - tol >= HALF_OVERFLOW)
    bad = over & (got != np.sign(ref) * np.inf)
    if bad.any():
        raise AssertionError(f"{what}: {int(bad.sum())} values should overflow to inf; {where(np.argwhere(bad)[0][0])}")
    tight = fin & ~over & ~flagged[:, None]
    err = np.abs(got - ref)
    ratio = np.where(tight, err / tol, 0.0)
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    worst = float(ratio.max()) if ratio.size else 0.0
    if worst > 1.0:
        i = np.unravel_index(np.argmax(ratio), ratio.shape)[0]
        raise AssertionError(f"{what}: {int((ratio > 1).sum())} values outside the float64 bound, worst ratio "
                             f"error / tolerance {worst:.3g}; {where(i)}")
    env = fin & ~over & flagged[:, None] & np.isfinite(r["lo"])
    ovf_ok = r["flags"]["overflow"][:, None] & np.isinf(got)
    # an infinite upper end (kk = 0: the GGX peak bound 1 / (kk gv) is unbounded) keeps the lower end; such values are
    # counted against the cap of their own class, "unbounded"
    unbounded = env & ~np.isfinite(r["hi"])
    counts["unbounded"] = int(unbounded.any(-1).sum())
    slack = tol + B * U24 * np.where(np.isfinite(r["hi"]), np.abs(r["hi"]), np.abs(r["lo"]))
    bad = env & ~ovf_ok & ((got < r["lo"] - slack) | (np.isfinite(r["hi"]) & (got > r["hi"] + slack)))
    if bad.any():
        i = np.argwhere(bad)[0][0]
        raise AssertionError(f"{what}: {int(bad.sum())} flagged values outside their envelope "
                             f"[{r['lo'][i].tolist()}, {r['hi'][i].tolist()}]; {where(i)}")
    caps = caps or {}
    for c in CLASSES + ("unbounded",):
        cap = caps.get(c, int(1e-4 * got.size))
        assert counts[c] <= cap, f"{what}: {counts[c]} pixels in the ill-conditioned class {c!r}, cap {cap}"
    return dict(worst=worst, counts=counts, checked=int(tight.sum()))


def shade_frame(view, gb, lights, amb_top, amb_bot):
    """The model's value of every pixel of a frame (h, w, 3) - gb: planes as a dict or an object with attributes."""
    pix = Pixels.from_planes(gb)
    with np.errstate(all="ignore"):
        out = _evaluate(pix, view, lights, amb_top, amb_bot, None)["out"]
    return out.reshape(pix.h, pix.w, 3)


def compare(got_planes_rgb, pix, view, lights, amb_top, amb_bot, what, shadow=None, caps=None, seed=0):
    r = reference(pix, view, lights, amb_top, amb_bot, shadow=shadow, seed=seed)
    return check(got_planes_rgb, r, pix, what, caps=caps)


# Class caps on the edge-case frame (pixels; it concentrates the classes on purpose: the back-facing band and the 20
# degree sun give R = -L pixels, the light 1e-3 above a surface gives a block of values at the half overflow).  Frames
# of real scenes use check()'s default, 1e-4 of the checked values.
EDGE_CAPS = dict(area=100, grazing=100, pcf=0, overflow=120, unbounded=60)


# ---- the edge-case frame ---------------------------------------------------------------------------------------------
ROUGH_CODES = (0, 1, 327, 3277, 16384, 32767, -1, -327, -16384, -32767, -32768)
EDGE_EYE, EDGE_TARGET = (0.0, 60.0, 0.0), (0.0, 30.0, -100.0)


def world_position(view, w, h, px, py, depth):
    """Float64 window -> world (ReconstructWorldPosition)."""
    clip = np.stack([(np.asarray(px) + 0.5) * 2.0 / w - 1.0, 1.0 - (np.asarray(py) + 0.5) * 2.0 / h,
                     np.asarray(depth, np.float64), np.ones(np.shape(px))], -1)
    wp4 = clip @ np.array(view.clip_to_world[:], np.float64).reshape(4, 4)
    return wp4[..., :3] / wp4[..., 3:]


def _snorm(v):
    return np.round(np.clip(v, -1.0, 1.0) * 32767.0).astype(np.int16)


def edge_case_frame(vr, w, h, seed=1):
    """A synthetic G-buffer of labelled bands (rows) over a fixed camera: every sRGB code of albedo / F0 / occlusion,
    roughness codes at the edges (negative ones included), random, axis (-32768 included), back-facing and grazing
    normals, cleared texels (whole waves and single ones), depth 0, 1.0 with real planes, nextafter(1, 0) and >= 0.9999,
    emissive 0 / subnormal / 65504 / +inf / NaN.  Returns (view, planes dict, rows dict label -> row range)."""
    rng = np.random.default_rng(seed)
    view = vr.make_view(EDGE_EYE, EDGE_TARGET, w, h)
    n = w * h
    idx = np.arange(n)
    dist = np.exp(rng.uniform(np.log(2.0), np.log(3000.0), n))
    depth = (1.0 - 0.1 / dist).astype(np.float32)
    codes = lambda s: (idx * s + rng.integers(0, 256, n)) % 256                                     # noqa: E731
    diffuse = (codes(1) | codes(7) << 8 | codes(31) << 16 | 255 << 24).astype(np.uint32)
    specular = (codes(3) | codes(11) << 8 | codes(5) << 16 | (idx % 256) << 24).astype(np.uint32)
    nv = rng.normal(size=(n, 3))
    nv /= np.linalg.norm(nv, axis=-1, keepdims=True)
    rough = np.where(rng.random(n) < 0.5, np.array(ROUGH_CODES)[idx % len(ROUGH_CODES)],
                     rng.integers(0, 32768, n)).astype(np.int16)
    normals = np.concatenate([_snorm(nv), rough[:, None]], -1)
    emissive = np.zeros((n, 4), np.float16)
    emissive[:, :3] = np.abs(rng.normal(0, 0.05, (n, 3)))
    emissive[rng.random(n) < 0.5] = 0
    rows, y = {}, 0

    def band(label, k):
        nonlocal y
        rows[label] = (y, y + k)
        y += k
        return slice(rows[label][0] * w, rows[label][1] * w)

    s = band("cleared", 2)                                                  # whole waves of clear values
    depth[s], diffuse[s], specular[s], normals[s], emissive[s] = 1.0, 0, 0, 0, 0
    s = band("mixed_cleared", 2)
    m = np.zeros(n, bool); m[s] = (idx[s] % 7) == 3
    depth[m], diffuse[m], specular[m], normals[m], emissive[m] = 1.0, 0, 0, 0, 0
    s = band("far_plane", 2)                                                # depth 1.0 with real planes
    depth[s] = 1.0
    s = band("depth_edges", 2)
    depth[s] = np.array([0.0, np.nextafter(np.float32(1), np.float32(0)), 0.9999, 0.99995, 0.99999], np.float32)[idx[s] % 5]
    s = band("axis_normals", 2)
    ax = np.array([[32767, 0, 0], [-32767, 0, 0], [0, 32767, 0], [0, -32768, 0], [0, 0, 32767], [0, 0, -32768],
                   [-32768, -32768, -32768]], np.int16)
    normals[s, :3] = ax[idx[s] % len(ax)]
    s = band("back_facing", 2)
    wp = world_position(view, w, h, idx[s] % w, idx[s] // w, depth[s])
    vdir = np.array(EDGE_EYE) - wp
    vdir /= np.linalg.norm(vdir, axis=-1, keepdims=True)
    nb = nv[s] - (2.0 * (nv[s] * vdir).sum(-1, keepdims=True) + 0.3) * vdir
    normals[s, :3] = _snorm(nb / np.linalg.norm(nb, axis=-1, keepdims=True))
    rows["grazing"] = (y, y + 4)                                            # filled by edge_lights (it knows the lights)
    y += 4
    rows["near_light"] = (h - 13, h - 7)                                   # a light 1e-3 above a near, level surface
    for yy in range(h - 12, h - 7):
        for xx in range(w // 2 - 2, w // 2 + 3):
            depth[yy * w + xx] = np.float32(1.0 - 0.1 / 3.0)
            normals[yy * w + xx, :3] = (0, 32767, 0)
    s = band("emissive_edges", 1)
    e = np.array([0.0, 6e-8, 1e-5, 65504.0, np.inf, np.nan], np.float16)
    emissive[s, :3] = e[(idx[s] % len(e))][:, None]
    assert y <= h
    planes = dict(depth=depth.reshape(h, w), diffuse=diffuse.reshape(h, w), specular=specular.reshape(h, w),
                  normals=normals.view(np.uint16).reshape(h, w, 4), emissive=emissive.view(np.uint16).reshape(h, w, 4))
    return view, planes, rows


def edge_lights(vr, view, planes, rows):
    """Light lists at the model's edges for the edge-case frame; sets the 'grazing' rows' normals perpendicular to the
    suns.  Returns dict name -> list of lights ('tiled': the directional and punctual ones)."""
    h, w = planes["depth"].shape
    at = lambda x, y: world_position(view, w, h, x, y, planes["depth"][y, x])                       # noqa: E731
    suns = [vr.reference_sun(), vr.directional_light((0.3, -1.0, 0.2), 2.0, 0.0, (1.0, 0.9, 0.8)),
            vr.directional_light((-0.5, -0.4, -0.7), 1.5, 20.0, (0.6, 0.7, 1.0)), vr.directional_light((0.0, -1.0, 0.0), 1.0)]
    y0 = rows["grazing"][0]
    for i, l in enumerate(suns):                                            # N exactly perpendicular to each sun
        d = np.array(l.direction[:], np.float64)
        r = np.random.default_rng(i).normal(size=(w, 3))
        nrm = np.cross(d, r)
        nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
        planes["normals"][y0 + i, ::16, :3] = _snorm(nrm[::16]).view(np.uint16)
    pa = at(w // 3, h - 3)
    pb = at(2 * w // 3, h - 5)
    dist_edge = float(np.linalg.norm(pa - (pb + np.array([0.0, 15.0, 0.0]))))
    points = [vr.point_light(tuple(pb + [0.0, 15.0, 0.0]), 4000.0, dist_edge, (1.0, 0.5, 0.25)),          # range ends at pa
              vr.point_light(tuple(pb + [0.0, 15.0, 0.0]), 3000.0, dist_edge * (1 + 1e-6), (0.3, 1.0, 0.3)),  # pa just inside
              vr.point_light(tuple(at(w // 2, h - 10) + [0.0, 1e-3, 0.0]), 100.0, 0.0),                   # overflows the half range
              vr.point_light(tuple(pa + [5.0, 40.0, -5.0]), 20000.0, 0.0, (0.9, 0.9, 1.0))]
    pc = at(w // 4, h - 20)
    src = pc + np.array([0.0, 30.0, 10.0])
    axis = tuple(pc - src)
    extra = [vr.spot_light(tuple(src), axis, 9000.0, 0.0, 0.0, 25.0, (1.0, 0.2, 0.2)),
             vr.spot_light(tuple(src + [20.0, 0.0, 0.0]), axis, 9000.0, 300.0, 10.0, 10.01, (0.2, 0.2, 1.0)),
             vr.spot_light(tuple(src - [20.0, 0.0, 0.0]), axis, 9000.0, 300.0, 4.0, 40.0, (0.5, 1.0, 0.5)),
             vr.point_light(tuple(pc + [3.0, 8.0, 0.0]), 30000.0, 200.0, (1.0, 0.8, 0.6), radius=50.0),     # radius > distance
             vr.point_light(tuple(pa + [0.0, 20.0, 0.0]), 5000.0, 0.0, (0.7, 0.7, 0.7), radius=1e-3)]
    # inner / outer angle exactly at a pixel: the spots' cones pass through pixels around pc
    return dict(suns=suns, points=points, extra=extra, max=(suns + points + extra + suns[:3])[:16], tiled=suns + points)


def synthetic_shadow_map(res):
    """Quadrants: a ramp, a checkerboard, constant 0 and constant 1 (light-clip depths)."""
    y, x = np.mgrid[0:res, 0:res]
    ramp = (x + y) / (2.0 * res)
    checker = np.where((x // 3 + y // 3) % 2 == 0, 0.35, 0.65)
    d = np.where(y < res // 2, np.where(x < res // 2, ramp, checker), np.where(x < res // 2, 0.0, 1.0))
    return d.astype(np.float32)


# ---- the PCF frame ---------------------------------------------------------------------------------------------------
PCF_W, PCF_H, PCF_RES, PCF_BIAS = 2048, 64, 256, 2.0 ** -8


def _pcf_map(res):
    """Columns: a ramp, a checkerboard, a constant 0.5 (the step the receivers sit on), then 0 above 1."""
    y, x = np.mgrid[0:res, 0:res]
    q = res // 4
    d = np.where(x < q, (x + y) / (2.0 * res), np.where(x < 2 * q, np.where((x // 3 + y // 3) % 2 == 0, 0.375, 0.625),
                 np.where(x < 3 * q, 0.5, np.where(y < res // 2, 0.0, 1.0))))
    return d.astype(np.float32)


def pcf_frame(vr, w_scale=1.0, width=PCF_W, seed=3):
    """A frame whose camera and light matrices make the shadow lookup exact in fp32 (reference(exact_geometry=True)).

    Camera (orthographic, world = (64 cx, depth, 64 cy)) and light (xc = X / 32 - 2 / W, yc = Z / 32 + 2 / H, zc = Y, all
    times w_scale, w = w_scale) put u = 0 at column W/4 and u = 1 at 3W/4, v = 0 at row H/4 and v = 1 at 3H/4, and zc
    equal to the pixel's depth: the frame covers the whole map, its four edges and corners, and the outside.  Depths are
    on a 2^-12 grid with whole rows at 0 and 1; over the map's constant-0.5 columns the receivers sit exactly on the
    stored depth (0.5 + bias: LessEqual, lit) or one grid step above or below it.
    A width that is not a power of two rounds the window -> clip x (reference(exact_geometry="vz")).
    Returns (camera view, light view, shadow map, planes)."""
    W, H, res = width, PCF_H, PCF_RES
    rng = np.random.default_rng(seed)
    cam = vr.View()
    c2w = np.zeros(16)
    c2w[0 * 4 + 0], c2w[1 * 4 + 2], c2w[2 * 4 + 1], c2w[3 * 4 + 3] = 64.0, 64.0, 1.0, 1.0
    cam.clip_to_world[:] = [float(x) for x in c2w]
    cam.camera_pos[:] = [0.0, 200.0, 0.0, 1.0]
    cam.viewport_w, cam.viewport_h = W, H
    lv = vr.View()
    m = np.zeros(16)
    m[0 * 4 + 0], m[3 * 4 + 0] = 1.0 / 32.0, -2.0 / W
    m[2 * 4 + 1], m[3 * 4 + 1] = 1.0 / 32.0, 2.0 / H
    m[1 * 4 + 2], m[3 * 4 + 3] = 1.0, 1.0
    lv.world_to_clip[:] = [float(x) for x in m * w_scale]
    lv.viewport_w = lv.viewport_h = res
    smap = _pcf_map(res)
    py, px = np.mgrid[0:H, 0:W]
    n = W * H
    depth = rng.integers(0, 4097, (H, W)) / 4096.0
    depth[::8] = 0.0
    depth[4::8] = 1.0
    u = (px - W / 4) / (W / 2)
    tx = u * res - 0.5
    step = (np.floor(tx) - 1 >= res // 2 + 1) & (np.floor(tx) + 2 <= 3 * res // 4 - 2)
    depth = np.where(step, 0.5 + PCF_BIAS + rng.integers(-1, 2, (H, W)) / 4096.0, depth).astype(np.float32)
    nv = rng.normal(size=(n, 3))
    nv[:, 1] = np.abs(nv[:, 1]) + 0.3
    nv /= np.linalg.norm(nv, axis=-1, keepdims=True)
    normals = np.concatenate([_snorm(nv), rng.integers(3000, 32768, (n, 1)).astype(np.int16)], -1)
    planes = dict(depth=depth, diffuse=rng.integers(0, 2 ** 32, (H, W), dtype=np.uint32) | np.uint32(0xff000000),
                  specular=rng.integers(0, 2 ** 32, (H, W), dtype=np.uint32),
                  normals=normals.view(np.uint16).reshape(H, W, 4), emissive=np.zeros((H, W, 4), np.uint16))
    return cam, lv, smap, planes


def pcf_coverage(r_geo, res=PCF_RES, W=PCF_W):
    """How the checked in-map pixels of a full PCF frame (row-major pixel list) exercise the lookup: counts of u / v / zc
    exactly 0 and 1, of footprints over the map's edge, and of pixels on each load path of the quad kernels (a wave is
    256 consecutive pixels of a row; the 16-byte row loads run when no active lane's footprint hangs over the edge)."""
    u, v, zc, tx, ty = r_geo.T
    inside = (u >= 0) & (u <= 1) & (v >= 0) & (v <= 1) & (zc >= 0) & (zc <= 1)
    ix = np.floor(tx) - 1
    edge = inside & ((ix < 0) | (ix + 3 > res - 1))
    idx = np.arange(len(u))
    group = (idx // W) * 10 ** 6 + ((idx % W) // 256) * 10 + (idx % 4)
    g_edge = np.zeros(group.max() + 1, bool)
    np.logical_or.at(g_edge, group, edge)
    clamp = inside & g_edge[group]
    return dict(u0=int((inside & (u == 0)).sum()), u1=int((inside & (u == 1)).sum()), v0=int((inside & (v == 0)).sum()),
                v1=int((inside & (v == 1)).sum()), z0=int((inside & (zc == 0)).sum()), z1=int((inside & (zc == 1)).sum()),
                edge=int(edge.sum()), clamp_path=int(clamp.sum()), row_path=int((inside & ~clamp).sum()),
                outside=int((~inside).sum()))


# ---- inputs of the all-light-type tiled pass (tests/test_tiled_ex_f64.py and its CPU companion) ----------------------
def plan_facts(lights):
    """What vr_light_check gathers from a light list for light_plan() (vr_light_plan.h).  extra: a spot or a spherical
    (radius > 0) light is in the list.  cone: a spot light whose cone the culling stage tests - a positive outer_angle
    below pi / 2 and a unit axis (cone_cull_terms, vr_light_cull.h).  kinds: (type, spherical, ranged) of every light."""
    extra = cone = False
    kinds = set()
    for l in lights:
        directional = l.type == VR_LIGHT_DIRECTIONAL
        kinds.add((int(l.type), (not directional) and l.radius > 0, (not directional) and l.angular_size_or_inv_range > 0))
        if directional:
            continue
        extra = extra or l.type == VR_LIGHT_SPOT or l.radius > 0
        if l.type == VR_LIGHT_SPOT:
            # cone_cull_terms' constants (vr_light_cull.h): kConeAxisTolerance = 1e-6 on | |axis|^2 - 1 |, kConeAngleMargin
            # = 1e-5 added to outer_angle, and its bound 1.5707 on the sum - a change there must be followed here
            a2 = sum(float(x) ** 2 for x in l.direction[:3])
            cone = cone or (abs(a2 - 1.0) <= 1e-6 and l.outer_angle > 0 and float(l.outer_angle) + 1e-5 < 1.5707)
    return dict(extra=bool(extra), cone=bool(cone), kinds=kinds)


ALL_KINDS = {(VR_LIGHT_DIRECTIONAL, False, False), (VR_LIGHT_POINT, False, True), (VR_LIGHT_SPOT, False, True),
             (VR_LIGHT_SPOT, False, False), (VR_LIGHT_POINT, True, True), (VR_LIGHT_SPOT, True, False)}


def all_type_lights(vr, wp, covered, n, seed):
    """The sun, a point light, a spot light and a spherical point and spot source, extended to n lights by a fixed seed:
    point lights, spot lights with and without a range, spherical point and spot sources, each above a covered pixel of the
    frame (wp: (h, w, 3) world positions) and at least 5 units from every visible surface point (a light that all but
    touches the steep terrain would put single pixels at 10 and more, where one RGBA16F ulp is larger than the whole
    error budget)."""
    scale = 1.0
    surface = wp[covered]
    lights = [vr.reference_sun(), vr.point_light((10.0, 40.0, -5.0), 3000.0 * scale, 120.0, (1.0, 0.5, 0.25)),
              vr.spot_light((-20.0, 60.0, 10.0), (0.3, -1.0, -0.2), 6000.0 * scale, 200.0, 12.0, 25.0, (0.2, 1.0, 0.4)),
              vr.point_light((30.0, 35.0, -30.0), 2000.0 * scale, 150.0, (0.9, 0.9, 1.0), radius=6.0),
              vr.spot_light((0.0, 80.0, -40.0), (0.0, -1.0, 0.3), 9000.0 * scale, 0.0, 5.0, 40.0, (1.0, 0.2, 0.2), radius=3.0)]
    rng = np.random.default_rng(seed)
    ys, xs = np.nonzero(covered)
    while len(lights) < n:
        k = rng.integers(len(ys))
        pos = wp[ys[k], xs[k]] + np.array([rng.uniform(-3, 3), rng.uniform(6, 25), rng.uniform(-3, 3)])
        if np.sqrt(((surface - pos) ** 2).sum(axis=1)).min() < 5.0:
            continue
        col, inten, rad = rng.uniform(0.1, 1.0, 3), rng.uniform(5.0, 40.0) * scale, rng.uniform(15.0, 60.0)
        kind = len(lights) % 5
        axis = np.array([rng.uniform(-0.5, 0.5), -1.0, rng.uniform(-0.5, 0.5)])
        outer = rng.uniform(8.0, 70.0)
        if kind == 0:
            lights.append(vr.point_light(pos, inten, rad, col))
        elif kind == 1:
            lights.append(vr.spot_light(pos, axis, inten * 3, rad * 1.5, outer * 0.5, outer, col))
        elif kind == 2:
            lights.append(vr.spot_light(pos, axis, inten * 0.3, 0.0, outer * 0.6, outer, col))              # no range
        elif kind == 3:
            lights.append(vr.point_light(pos, inten, rad, col, radius=rng.uniform(0.5, 4.0)))
        else:
            lights.append(vr.spot_light(pos, axis, inten * 3, rad * 1.5, outer * 0.3, outer, col, radius=rng.uniform(0.5, 3.0)))
    return lights


def pcf_lights(vr):
    """(the shadowed sun, the unshadowed directional light) of the PCF tests."""
    return vr.reference_sun(), vr.directional_light((0.3, -1.0, 0.2), 0.5, 0.0)


def pcf_all_type_lights(vr):
    """The two directional lights of the PCF frame and one light of every other kind, 6 to 25 units above the receivers
    (which lie at heights 0 .. 1: every light is at least 5 units from every surface point).  The ranged point and spot
    lights stand in front of the sun in the list: in a tile that culls one of them the sun's staged slot differs from
    its list index.  Returns (lights, the sun's index)."""
    sun, fill = pcf_lights(vr)
    lights = [vr.point_light((-30.0, 12.0, 20.0), 250.0, 60.0, (1.0, 0.5, 0.25)),
              vr.spot_light((20.0, 15.0, -10.0), (0.2, -1.0, 0.1), 500.0, 80.0, 15.0, 35.0, (0.2, 1.0, 0.4)),
              fill, sun,
              vr.spot_light((-10.0, 20.0, -30.0), (0.0, -1.0, 0.2), 600.0, 0.0, 10.0, 30.0, (1.0, 0.2, 0.2)),         # no range
              vr.point_light((40.0, 10.0, 30.0), 150.0, 50.0, (0.9, 0.9, 1.0), radius=2.0),
              vr.spot_light((0.0, 25.0, 0.0), (-0.1, -1.0, 0.0), 900.0, 0.0, 20.0, 50.0, (0.6, 0.7, 1.0), radius=1.5)]
    return lights, 3


PCF_CROWD_W, PCF_CROWD_TILE, PCF_CROWD_N = 256, (3, 0), 300


def pcf_crowd_lights(vr, seed=6):
    """PCF_CROWD_N weak lights above the light tile PCF_CROWD_TILE of the PCF frame of width PCF_CROWD_W (spherical point
    lights, punctual and spherical spot lights pointing down, 6 to 7.5 units above the receivers' plane, short ranges and
    narrow cones: the tile's list holds them all, a pixel is reached by a few), the unshadowed directional light in front
    of them and the sun behind them.  Returns (lights, the sun's index)."""
    W, H = PCF_CROWD_W, PCF_H
    tx, ty = PCF_CROWD_TILE
    x0, x1 = 64.0 * (tx * 32 * 2.0 / W - 1.0), 64.0 * ((tx + 1) * 32 * 2.0 / W - 1.0)
    z1, z0 = 64.0 * (1.0 - ty * 32 * 2.0 / H), 64.0 * (1.0 - (ty + 1) * 32 * 2.0 / H)
    rng = np.random.default_rng(seed)
    sun, fill = pcf_lights(vr)
    lights = [fill]
    for i in range(PCF_CROWD_N):
        pos = (rng.uniform(x0 + 1.0, x1 - 1.0), rng.uniform(6.0, 7.5), rng.uniform(z0 + 1.0, z1 - 1.0))
        col = rng.uniform(0.1, 1.0, 3)
        axis = (rng.uniform(-0.2, 0.2), -1.0, rng.uniform(-0.2, 0.2))
        outer = rng.uniform(10.0, 25.0)
        if i % 3 == 0:
            lights.append(vr.point_light(pos, 4.0, 8.0, col, radius=rng.uniform(0.5, 2.0)))
        elif i % 3 == 1:
            lights.append(vr.spot_light(pos, axis, 12.0, 20.0, outer * 0.5, outer, col))
        else:
            lights.append(vr.spot_light(pos, axis, 12.0, 0.0, outer * 0.4, outer, col, radius=rng.uniform(0.5, 1.5)))
    return lights + [sun], len(lights)


def pcf_crowd_mask(seed=6):
    """4096 pixels of the PCF_CROWD_W frame: every pixel of PCF_CROWD_TILE and a seeded sample of its neighbours in the
    frame (the frame has two rows of light tiles: five of the eight exist)."""
    W, H = PCF_CROWD_W, PCF_H
    tx, ty = PCF_CROWD_TILE
    py, px = np.mgrid[0:H, 0:W]
    gx, gy = px // 32, py // 32
    hot = (gx == tx) & (gy == ty)
    near = (np.abs(gx - tx) <= 1) & (np.abs(gy - ty) <= 1) & ~hot
    idx = np.flatnonzero(near)
    pick = np.random.default_rng(seed).choice(idx, 4096 - int(hot.sum()), replace=False)
    mask = hot.copy()
    mask.flat[pick] = True
    assert mask.sum() == 4096
    return mask


def masked_pcf_coverage(r_geo, res=PCF_RES):
    """pcf_coverage's counts of u / v / zc exactly 0 and 1, of footprints over the map's edge and of pixels outside the map,
    for any list of pixels (a mask)."""
    u, v, zc, tx, ty = r_geo.T
    inside = (u >= 0) & (u <= 1) & (v >= 0) & (v <= 1) & (zc >= 0) & (zc <= 1)
    ix, iy = np.floor(tx) - 1, np.floor(ty) - 1
    edge = inside & ((ix < 0) | (ix + 3 > res - 1) | (iy < 0) | (iy + 3 > res - 1))
    return dict(u0=int((inside & (u == 0)).sum()), u1=int((inside & (u == 1)).sum()), v0=int((inside & (v == 0)).sum()),
                v1=int((inside & (v == 1)).sum()), z0=int((inside & (zc == 0)).sum()), z1=int((inside & (zc == 1)).sum()),
                edge=int(edge.sum()), outside=int((~inside).sum()))


class TiledCase:
    """One (frame, light list, shadow) input of the tiled pass with the conditions its check runs under, for the kernels
    and for the fp32 oracle alike: caps (None: check()'s default), mask (None: the whole frame), exact_geometry and the
    least share of values that must be held to the tight bound.  shadow: (light view, map, light index, bias) or None.
    The float64 reference is computed once per case and never changed."""

    def __init__(self, name, view, planes, lights, ambient, shadow=None, caps=None, mask=None, exact_geometry=False,
                 min_checked=0.9, rows=None):
        self.name, self.view, self.planes, self.lights, self.ambient = name, view, planes, list(lights), ambient
        self.shadow, self.caps, self.mask, self.exact_geometry, self.min_checked = shadow, caps, mask, exact_geometry, min_checked
        self.rows = rows
        self.h, self.w = planes["depth"].shape
        if mask is None:
            self.pix = Pixels.from_planes(planes)
        else:
            py, px = np.nonzero(mask)
            self.pix = Pixels.from_planes(planes, px, py)
        self._ref = None

    def reference(self):
        if self._ref is None:
            sh = None
            if self.shadow is not None:
                lv, smap, li, bias = self.shadow
                sh = (lv, smap, li, bias, self.lights[li].out_of_bounds_shadow)
            self._ref = reference(self.pix, self.view, self.lights, self.ambient[0], self.ambient[1], shadow=sh,
                                  exact_geometry=self.exact_geometry)
        return self._ref

    def check(self, frame, what, report=True):
        """frame: (h, w, 3) values of an implementation.  Returns check()'s result, with the shadow lookup's coverage of the
        checked pixels in it (a shadowed case)."""
        got = np.asarray(frame, np.float64)[self.pix.py, self.pix.px]
        r = self.reference()
        res = check(got, r, self.pix, f"{self.name}: {what}", caps=self.caps)
        assert res["checked"] > self.min_checked * got.size, res
        if self.shadow is not None:
            # a whole frame: pcf_coverage; a mask: the same keys from the geometry of the checked pixels (the two load-path
            # counts need a row-major list and are not asserted here)
            cov = pcf_coverage(r["shadow_geo"], W=self.w) if self.mask is None else masked_pcf_coverage(r["shadow_geo"])
            res["coverage"] = cov
            for k in ("v0", "v1", "z0", "z1", "edge", "outside"):
                assert cov[k] > 0, cov
            # u = 0 and u = 1 lie half a frame apart (W / 2 pixels: four light tiles at the narrowest width, 256): a whole
            # frame has both, a mask of three tile columns can hold one of them
            assert (cov["u0"] > 0 and cov["u1"] > 0) if self.mask is None else (cov["u0"] + cov["u1"] > 0), cov
        if report:
            print(f"{self.name}: {what}: worst ratio {res['worst']:.4f}, classes {res['counts']}"
                  + (f", coverage {res['coverage']}" if "coverage" in res else ""))
        return res

    def oracle_frame(self, oracle):
        """The fp32 oracle's half output for this input, (h, w, 3) float64."""
        gb = oracle.GBufferHost(self.w, self.h)
        for k, a in self.planes.items():
            getattr(gb, k)[...] = np.asarray(a).reshape(getattr(gb, k).shape)
        out = oracle.deferred(self.view, gb, self.lights, self.ambient[0], self.ambient[1], shadow=self.shadow)
        return oracle.half_to_float(out)[..., :3].astype(np.float64)


def tiled_edge_case(vr, ambient, width, lights_name):
    """The edge-case frame at width x 128 with 'extra', 'all' (suns + points + extra: 13 lights) or 'tiled' (suns +
    points) of edge_lights; EDGE_CAPS.  The caps are conditions on the input, and the frame's seed is part of it: at 508
    the seed 1 of the other widths puts 119 pixels into the class 'area' (cap 100) for the oracle as for any other
    implementation, and three R = -L texels with kk = 0 under a spot light (NaN or inf, as the undefined rotation falls);
    seed 2 gives 32 'area' pixels and none of those (test_tiled_ex_f64_cpu.py holds the oracle to it)."""
    view, planes, rows = edge_case_frame(vr, width, 128, seed={508: 2}.get(width, 1))
    L = edge_lights(vr, view, planes, rows)
    L["all"] = L["suns"] + L["points"] + L["extra"]
    return TiledCase(f"edge frame {width}, {lights_name}", view, planes, L[lights_name], ambient, caps=EDGE_CAPS, rows=rows)


def tiled_pcf_case(vr, ambient, lists, w_scale=1.0):
    """The PCF frame with one of the light lists 'sun_first' [sun, fill], 'sun_second' [fill, sun], 'twice' [fill, sun,
    fill, sun] (the second sun shadowed), 'all_types' (pcf_all_type_lights) or 'crowd' (pcf_crowd_lights at PCF_CROWD_W,
    checked on pcf_crowd_mask).  The shadow light's index goes to the model and to the oracle through the shadow tuple."""
    width = PCF_CROWD_W if lists == "crowd" else PCF_W
    cam, lv, smap, planes = pcf_frame(vr, w_scale, width)
    sun, fill = pcf_lights(vr)
    mask = None
    if lists == "all_types":
        lights, li = pcf_all_type_lights(vr)
    elif lists == "crowd":
        lights, li = pcf_crowd_lights(vr)
        mask = pcf_crowd_mask()
    else:
        lights, li = dict(sun_first=([sun, fill], 0), sun_second=([fill, sun], 1), twice=([fill, sun, fill, sun], 3))[lists]
    case = TiledCase(f"PCF frame {width}, w = {w_scale}, {lists}", cam, planes, lights, ambient, shadow=(lv, smap, li, PCF_BIAS),
                     mask=mask, exact_geometry=True, min_checked=0.99)
    case.light_view, case.shadow_map = lv, smap
    return case


def tiled_terrain_case(vr, ambient, view, planes, n=40, seed=20261019):
    """A terrain G-buffer (planes: as the tile pass left them) under all_type_lights; check()'s default caps."""
    h, w = planes["depth"].shape
    py, px = np.mgrid[0:h, 0:w]
    wp = world_position(view, w, h, px, py, planes["depth"])
    lights = all_type_lights(vr, wp, planes["depth"] < 1.0, n, seed)
    return TiledCase(f"terrain {w}x{h}, {n} lights", view, planes, lights, ambient)
