"""Model of the albedo's packed footprint table (vrenderer_amd/csrc/vr_packed.h), in numpy, written from that header's text: what the
fused tile pass reads instead of the float table 'fast' of tests/tables_model.py.  Input: one level of an albedo chain as uint8
(h, w, 4); output: that level's table.

    pack   (h + 3, w + 3, 4) uint32     entry (ix, iy): a dword per texel of the clamp-addressed footprint (ix-1, iy-1) (ix, iy-1)
                                        (ix-1, iy) (ix, iy), each r << 2 | g << 12 | b << 22 (alpha is not kept)

A 10-bit field is its code times four: the byte offset of the code's float in a 256-float table.  decode() takes the twelve floats of
every entry out of such a table; with the sRGB table of tables_model they are the four 'fast' entries (ix, iy) (ix+1, iy) (ix, iy+1)
(ix+1, iy+1), bit for bit.  Integers throughout: nothing to round."""
import numpy as np

from tests import tables_model as tm


def pack_texels(level):
    """(h, w) uint32: r << 2 | g << 12 | b << 22 of every texel of an (h, w, 4) uint8 level."""
    t = np.asarray(level, np.uint8).astype(np.uint32)
    return (t[..., 0] << np.uint32(2)) | (t[..., 1] << np.uint32(12)) | (t[..., 2] << np.uint32(22))


def pack_table(level):
    level = np.asarray(level, np.uint8)
    assert level.ndim == 3 and level.shape[2] == 4
    return np.stack(tm._footprint(pack_texels(level), 3), -1)


def decode(table, lut):
    """(h + 3, w + 3, 4 texels, 3 channels) float32: every field of every entry through `lut` by its byte offset."""
    table = np.asarray(table, np.uint32)
    off = np.stack([(table >> np.uint32(10 * c)) & np.uint32(0x3ff) for c in range(3)], -1)
    assert not (off & 3).any() and not (table >> np.uint32(30)).any()
    return np.asarray(lut, np.float32)[off >> 2]


def dirty_span(lo, hi, w):
    """The entries of one axis that texels [lo, hi) of a w-texel level dirty: entry ix reads texels clamp(ix - 1) and clamp(ix)."""
    return tm.dirty_entries(lo, hi, w, w + 3, 0, 1)


def mismatches(got, level):
    """[] or [(what, (iy, ix), device entry, model entry, count)] of one level's read-back against the model of `level`."""
    want = pack_table(level)
    if got.shape != want.shape or got.dtype != want.dtype:
        return [("shape", None, (got.shape, str(got.dtype)), (want.shape, str(want.dtype)), 0)]
    at = np.argwhere((got != want).any(-1))
    if len(at) == 0:
        return []
    iy, ix = (int(v) for v in at[0])
    return [("pack", (iy, ix), [hex(v) for v in got[iy, ix]], [hex(v) for v in want[iy, ix]], len(at))]


def assert_packed_is_the_model(tp, what):
    """Every level and every entry, the clamped rim included, of a TerrainPass's packed table against the model of the device's own
    level.  Returns what was read."""
    got = tp.PackedTables()
    assert len(got) == tp.mip_levels("albedo"), what
    for l, g in enumerate(got):
        for bad in mismatches(g, tp.download_mip("albedo", l)):
            raise AssertionError(f"{what}: level {l}, {bad[0]}: first wrong entry (iy, ix) = {bad[1]}, device {bad[2]}, model {bad[3]} ({bad[4]} entries differ)")
    return got
