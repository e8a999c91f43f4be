"""CPU tests of vrenderer_amd.passes._rows, which lays dab rows (5 columns, padded to vr_brush_dab's 8) and path points (2 or 3
columns, padded to vr_path_point's 4) out as the C arrays the level-0 entry points take.  No device, no library."""
import numpy as np
import pytest

from vrenderer_amd.passes import _rows

DABS, POINTS = ((5,), 8), ((2, 3), 4)


def _check(out, n, full):
    assert out.dtype == np.float32 and out.shape == (n, full) and out.flags["C_CONTIGUOUS"]


@pytest.mark.parametrize("n", (1, 7))
def test_dab_rows(n):
    """(n, 5), flat 5n and (n, 8) input give a C-contiguous float32 (n, 8); columns 5 to 7 are zero when padded; an (n, 8) input keeps
    its values, whatever its strides and type."""
    rows = np.arange(5 * n, dtype=np.float64).reshape(n, 5) + 0.5
    for given in (rows, rows.reshape(-1), rows.tolist(), np.asfortranarray(rows)):
        out = _rows(given, *DABS)
        _check(out, n, 8)
        assert np.array_equal(out[:, :5], rows.astype(np.float32)) and not out[:, 5:].any()
    wide = np.arange(8 * n, dtype=np.float32).reshape(n, 8) + 1.0
    for given in (wide, np.asfortranarray(wide), wide.astype(np.float64), np.repeat(wide, 2, axis=1)[:, ::2]):
        out = _rows(given, *DABS)
        _check(out, n, 8)
        assert np.array_equal(out, wide)


def test_no_rows():
    out = _rows(np.zeros((0, 5), np.float32), *DABS)
    _check(out, 0, 8)
    _check(_rows(np.zeros((0, 3), np.float32), *POINTS), 0, 4)


def test_a_wrong_width_is_refused():
    for given, layout in ((np.zeros((3, 6)), DABS), (np.zeros((3, 4)), DABS), (np.zeros((3, 5)), POINTS), (np.zeros((3, 1)), POINTS), (np.zeros((2, 3, 5)), DABS)):
        with pytest.raises(AssertionError):
            _rows(given, *layout)


@pytest.mark.parametrize("cols", (2, 3, 4))
def test_path_points(cols):
    """(n, 2) and (n, 3) give (n, 4) with zeros behind; (n, 4) keeps its values; a flat array is rows of (x, z, height)."""
    pts = np.arange(6 * cols, dtype=np.float64).reshape(6, cols) - 3.25
    out = _rows(pts, *POINTS)
    _check(out, 6, 4)
    assert np.array_equal(out[:, :cols], pts.astype(np.float32)) and not out[:, cols:].any()
    flat = _rows(np.arange(12.0), *POINTS)
    _check(flat, 4, 4)
    assert np.array_equal(flat[:, :3], np.arange(12, dtype=np.float32).reshape(4, 3)) and not flat[:, 3].any()
