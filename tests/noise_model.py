"""The definition of procedural noise on a map (vr_terrain_noise) in numpy float32 / uint32: vectorised over the map, a Python loop
over the octaves, the preparation in Python floats (doubles).  Written from the text of vrenderer_amd/csrc/vr_noise.h's comment, not
from its functions or the kernel; the dab preparation, weight and mask are tests/brush_model.py's and tests/erode_model.py's.

  map          w x h texels over the world [-S/2, S/2]^2
  preparation  in double, each result rounded to fp32 once (beyond fp32's range: +-FLT_MAX): with the running products L_0 = 1,
               L_(o+1) = L_o * lacunarity, G_0 = 1, G_(o+1) = G_o * gain and F_o = frequency * L_o:
               sx[o] = S / w * F_o, sz[o] = S / h * F_o, ox[o] = (offset_x - S / 2) * F_o, oz[o] = (offset_z - S / 2) * F_o,
               a[o] = G_o / (G_0 + ... + G_(octaves-1))
  range        in double from the rounded constants: (0.5 | w - 0.5) * sx[o] + ox[o] and (0.5 | h - 0.5) * sz[o] + oz[o] below 2^22
               in magnitude for every octave, or the call is refused
  lattice      u = ((float)i + 0.5f) * sx[o] + ox[o]; cx = floor(u); tx = u - cx; the cell is int32(cx) as uint32 (wrapping); z likewise
  hash         h = (x * 0x9E3779B1) ^ (y * 0x85EBCA77) ^ (s * 0xC2B2AE3D); h ^= h >> 16; h *= 0x7FEB352D; h ^= h >> 15;
               h *= 0x846CA68B; h ^= h >> 16, in uint32; s = seed + o; the corners are (cx + 0|1, cz + 0|1)
  fade         min(((t * t) * t) * (t * (t * 6 - 15) + 10), 1)
  basis        VALUE: q = float(hash >> 8) * 2^-23 - 1; GRADIENT: k = hash >> 29 picks (1,0) (-1,0) (0,1) (0,-1) (r,r) (-r,r) (r,-r)
               (-r,-r), r = 0.70710678f, q = gx * dx + gz * dz with the offset to the corner; both: top = q00 + fx * (q10 - q00),
               bot = q01 + fx * (q11 - q01), e = top + fz * (bot - top); VALUE n = e, GRADIENT n = clamp(e * 1.41421354f, -1, 1)
  fractal      f = 0; f = f + a[o] * x_o ascending, x_o = n_o (FBM), 2 |n_o| - 1 (BILLOW), 1 - 2 |n_o| (RIDGED); f = clamp(f, -1, 1)
  apply        t = amplitude * f; ADD val = clamp(val + m * t, 0, 255); BLEND val = clamp(val + (m * 1) * ((base + t) - val), 0, 255);
               the byte is floor(val + 0.5), per channel of channel_mask; m: the erosions' mask over the dabs prepared for the map,
               or 1 everywhere; a texel with m == 0 is not written

Every array operation below is one IEEE fp32 (or uint32) operation per element, in the written order, so the result is the
device's, bit for bit."""
import numpy as np

from tests.erode_model import mask_of

F = np.float32
U = np.uint32
FLT_MAX = float(np.finfo(np.float32).max)
MAX_OCTAVES = 12
VALUE, GRADIENT = 0, 1
FBM, BILLOW, RIDGED = 0, 1, 2
ADD, BLEND = 0, 1
WHOLE_MAP = 1
COORD_LIMIT = 4194304.0
BASES = (("value", VALUE), ("gradient", GRADIENT))
FRACTALS = (("fbm", FBM), ("billow", BILLOW), ("ridged", RIDGED))
OPS = (("add", ADD), ("blend", BLEND))


def params(frequency, amplitude, octaves=6, lacunarity=2.0, gain=0.5, offset=(0.0, 0.0), seed=0, basis=GRADIENT, fractal=FBM, op=ADD, base=0.0,
           channel_mask=1):
    """A call's parameters as a dict with fp32-exact values (what the C struct carries)."""
    return dict(frequency=float(F(frequency)), offset_x=float(F(offset[0])), offset_z=float(F(offset[1])), lacunarity=float(F(lacunarity)),
                gain=float(F(gain)), amplitude=float(F(amplitude)), base=float(F(base)), seed=int(seed) & 0xFFFFFFFF, octaves=int(octaves),
                basis=int(basis), fractal=int(fractal), op=int(op), channel_mask=int(channel_mask))


def _round(v):
    return F(min(max(v, -FLT_MAX), FLT_MAX))


def prepare(p, world_size, w, h):
    """dict of float32 arrays sx, sz, ox, oz, a, one entry per octave of the call."""
    S = float(F(world_size))
    n = p["octaves"]
    total, G = 0.0, 1.0
    for _ in range(n):
        total += G
        G *= p["gain"]
    k = dict(sx=np.zeros(n, F), sz=np.zeros(n, F), ox=np.zeros(n, F), oz=np.zeros(n, F), a=np.zeros(n, F))
    L, G = 1.0, 1.0
    for o in range(n):
        Fo = p["frequency"] * L
        k["sx"][o] = _round(S / w * Fo)
        k["sz"][o] = _round(S / h * Fo)
        k["ox"][o] = _round((p["offset_x"] - S / 2) * Fo)
        k["oz"][o] = _round((p["offset_z"] - S / 2) * Fo)
        k["a"][o] = _round(G / total)
        L *= p["lacunarity"]
        G *= p["gain"]
    return k


def in_range(k, w, h):
    """The refusal that needs the map's size: every corner's lattice coordinate of every octave below 2^22 in magnitude."""
    for o in range(len(k["sx"])):
        sx, sz, ox, oz = (float(k[n][o]) for n in ("sx", "sz", "ox", "oz"))
        ends = (0.5 * sx + ox, (w - 0.5) * sx + ox, 0.5 * sz + oz, (h - 0.5) * sz + oz)
        if not all(abs(e) < COORD_LIMIT for e in ends):
            return False
    return True


def hash32(x, y, s):
    with np.errstate(over="ignore"):
        h = (x * U(0x9E3779B1)) ^ (y * U(0x85EBCA77)) ^ (U(s) * U(0xC2B2AE3D))
        h = h ^ (h >> U(16))
        h = h * U(0x7FEB352D)
        h = h ^ (h >> U(15))
        h = h * U(0x846CA68B)
        h = h ^ (h >> U(16))
    return h.astype(U)


def _axis(n, s, o):
    u = (np.arange(n, dtype=F) + F(0.5)) * s + o
    c = np.floor(u).astype(F)
    return c.astype(np.int32).astype(U), c.astype(np.int32), (u - c).astype(F)


def fade(t):
    a = t * F(6)
    b = a - F(15)
    c = t * b
    d = c + F(10)
    t3 = (t * t) * t
    return np.minimum(t3 * d, F(1)).astype(F)


def _lerp2(q00, q10, q01, q11, fx, fz):
    top = q00 + fx * (q10 - q00)
    bot = q01 + fx * (q11 - q01)
    return (top + fz * (bot - top)).astype(F)


_R = F(0.70710678)
_GX = np.array([1, -1, 0, 0, _R, -_R, _R, -_R], F)
_GZ = np.array([0, 0, 1, -1, _R, _R, -_R, -_R], F)


def basis_at(basis, cx, cz, tx, tz, s):
    """n of one octave: cx, cz uint32 arrays and tx, tz float32 arrays that broadcast against each other; s: the octave's hash seed."""
    one = U(1)
    with np.errstate(over="ignore"):
        x1, z1 = (cx + one).astype(U), (cz + one).astype(U)
    h00, h10, h01, h11 = hash32(cx, cz, s), hash32(x1, cz, s), hash32(cx, z1, s), hash32(x1, z1, s)
    fx, fz = fade(tx), fade(tz)
    if basis == VALUE:
        q = [(h >> U(8)).astype(np.int32).astype(F) * F(2.0 ** -23) - F(1) for h in (h00, h10, h01, h11)]
        return _lerp2(*q, fx, fz)
    dx1, dz1 = tx - F(1), tz - F(1)
    q = []
    for h, dx, dz in ((h00, tx, tz), (h10, dx1, tz), (h01, tx, dz1), (h11, dx1, dz1)):
        k = (h >> U(29)).astype(np.int64)
        q.append((_GX[k] * dx + _GZ[k] * dz).astype(F))
    e = _lerp2(*q, fx, fz)
    return np.minimum(np.maximum(e * F(1.41421354), F(-1)), F(1)).astype(F)


def term(fractal, n):
    if fractal == FBM:
        return n
    two = F(2) * np.abs(n)
    return (two - F(1)) if fractal == BILLOW else (F(1) - two)


def fractal_of(p, world_size, w, h, detail=None):
    """f, float32 (h, w), of every texel of a w x h map.  `detail` receives n (octaves, h, w), the int32 cells per octave and axis and the
    prepared constants."""
    k = prepare(p, world_size, w, h)
    assert in_range(k, w, h), "the model's caller asks for what the library refuses"
    f = np.zeros((h, w), F)
    ns, cells = [], []
    for o in range(p["octaves"]):
        cx, ix, tx = _axis(w, k["sx"][o], k["ox"][o])
        cz, iz, tz = _axis(h, k["sz"][o], k["oz"][o])
        n = basis_at(p["basis"], cx[None, :], cz[:, None], tx[None, :], tz[:, None], (p["seed"] + o) & 0xFFFFFFFF)
        f = (f + k["a"][o] * term(p["fractal"], n)).astype(F)
        ns.append(n)
        cells.append((ix, iz))
    f = np.minimum(np.maximum(f, F(-1)), F(1)).astype(F)
    if detail is not None:
        detail.update(n=np.stack(ns), cells=cells, prepared=k)
    return f


def noise(texels, p, world_size, dabs=None, whole_map=False, detail=None, mask=None):
    """One call on a copy of `texels` ((h, w) uint8 for the heightmap, (h, w, 4) uint8 for the albedo) -> (new texels, rect).  `detail`,
    a dict, receives what the tests' preconditions need: mask, f, n per octave, the cells, the prepared constants.  `mask` (the host
    check's): a float32 (h, w) mask in place of the dabs'; the rectangle is then the whole map."""
    h, w = texels.shape[:2]
    if mask is not None:
        assert dabs is None and not whole_map
        m, rect = np.ascontiguousarray(mask, F), (0, 0, w, h)
    elif whole_map:
        assert dabs is None or len(dabs) == 0
        m, rect = np.ones((h, w), F), (0, 0, w, h)
    else:
        m, rect = mask_of((h, w), dabs if dabs is not None else np.zeros((0, 5), F), world_size)
    d = {} if detail is None else detail
    f = fractal_of(p, world_size, w, h, d)
    d.update(mask=m, f=f)
    t = F(p["amplitude"]) * f
    val = texels.astype(F).reshape(h, w, -1)
    out = val.copy()
    for c in range(val.shape[2]):
        if not p["channel_mask"] >> c & 1:
            continue
        v = val[..., c]
        if p["op"] == ADD:
            new = v + m * t
        else:
            to = F(p["base"]) + t
            new = v + (m * F(1)) * (to - v)
        out[..., c] = np.minimum(np.maximum(new, F(0)), F(255))
    res = np.where((m > F(0))[..., None], np.floor(out + F(0.5)).astype(np.uint8), texels.reshape(h, w, -1)).astype(np.uint8)
    return res.reshape(texels.shape), tuple(rect)
