"""The host side of the orientations (csrc/orientation.h through m355_orientation_compose and m355_orientation_from_exif; no device): the composition
against the numpy definition for all 64 pairs, the EXIF table against the eight stored images of one asymmetric pattern written out literally, the
rejections, and the header's formula evaluated point by point against the numpy form."""
import ctypes

import numpy as np
import pytest

from test_emu_picture import emu_lib  # noqa: F401  (fixture)
import export_oriented_util as ou
from export_oriented_util import M355_ERR_INVALID, ORIENTATIONS, orient
from libde265_amd import capi

A = np.arange(15, dtype=np.int32).reshape(3, 5) * 7 + 1      # 3 x 5, distinct values


def test_constants():
    assert (capi.ORIENT_MIRROR, capi.ORIENT_FLIP, capi.ORIENT_TRANSPOSE) == (1, 2, 4)
    assert (capi.ORIENT_ROTATE_0, capi.ORIENT_ROTATE_180, capi.ORIENT_ROTATE_90_CW, capi.ORIENT_ROTATE_90_CCW) == (0, 3, 5, 6)


def test_the_eight_orientations_are_what_the_header_names():
    assert np.array_equal(orient(A, 0), A)
    assert np.array_equal(orient(A, 1), A[:, ::-1]) and np.array_equal(orient(A, 2), A[::-1])
    assert np.array_equal(orient(A, capi.ORIENT_ROTATE_180), np.rot90(A, 2))
    assert np.array_equal(orient(A, 4), A.T)
    assert np.array_equal(orient(A, capi.ORIENT_ROTATE_90_CW), np.rot90(A, -1))
    assert np.array_equal(orient(A, capi.ORIENT_ROTATE_90_CCW), np.rot90(A, 1))
    assert np.array_equal(orient(A, 7), np.rot90(A, 2).T)
    assert len({orient(A, o).tobytes() + bytes(orient(A, o).shape) for o in ORIENTATIONS}) == 8


@pytest.mark.parametrize("o", ORIENTATIONS)
def test_formula_point_by_point_is_the_numpy_form(o):
    assert np.array_equal(ou.orient_pointwise(A, o), orient(A, o))
    pairs = np.stack([A, -A], axis=-1)                      # an element of two values moves as a unit
    assert np.array_equal(ou.orient_pointwise(pairs, o), orient(pairs, o))


def test_compose_all_pairs(emu_lib):  # noqa: F811
    for f in ORIENTATIONS:
        for t in ORIENTATIONS:
            c = emu_lib.orientation_compose(f, t)
            assert c in ORIENTATIONS
            assert np.array_equal(orient(orient(A, f), t), orient(A, c)), (f, t, c)
    # an irot (90 degrees anticlockwise) followed by an imir about the vertical axis
    assert emu_lib.orientation_compose(capi.ORIENT_ROTATE_90_CCW, capi.ORIENT_MIRROR) == 7


# the upright picture and how a file with each EXIF Orientation stores it: the value names the visual side that the stored row 0 and column 0 lie on
UPRIGHT = [[1, 2, 3],
           [4, 5, 6]]
STORED = {
    1: [[1, 2, 3], [4, 5, 6]],          # top, left
    2: [[3, 2, 1], [6, 5, 4]],          # top, right
    3: [[6, 5, 4], [3, 2, 1]],          # bottom, right
    4: [[4, 5, 6], [1, 2, 3]],          # bottom, left
    5: [[1, 4], [2, 5], [3, 6]],        # left, top
    6: [[3, 6], [2, 5], [1, 4]],        # right, top
    7: [[6, 3], [5, 2], [4, 1]],        # right, bottom
    8: [[4, 1], [5, 2], [6, 3]],        # left, bottom
}
EXIF_TABLE = {1: 0, 2: 1, 3: 3, 4: 2, 5: 4, 6: 5, 7: 7, 8: 6}


def test_exif_table(emu_lib):  # noqa: F811
    for exif, stored in STORED.items():
        o = emu_lib.orientation_from_exif(exif)
        assert o == EXIF_TABLE[exif]
        assert np.array_equal(orient(np.array(stored), o), np.array(UPRIGHT)), exif


def test_rejections(emu_lib):  # noqa: F811
    lib = emu_lib.lib
    out = ctypes.c_int(-77)
    for f, t in ((-1, 0), (0, -1), (8, 0), (0, 8), (3, 1 << 20)):
        assert lib.m355_orientation_compose(f, t, ctypes.byref(out)) == M355_ERR_INVALID, (f, t)
    assert lib.m355_orientation_compose(1, 2, None) == M355_ERR_INVALID
    for exif in (0, 9, -1, 100):
        assert lib.m355_orientation_from_exif(exif, ctypes.byref(out)) == M355_ERR_INVALID, exif
    assert lib.m355_orientation_from_exif(1, None) == M355_ERR_INVALID
    assert out.value == -77, "a rejected call wrote its result"
