"""m355_maps_unit, the host-only statement of the side maps (csrc/map_element.h through a linear search over host lists), against the numpy
restatement of tests/maps_util.py: the synthetic pictures of the device scenarios, the hand-built sampling picture, a picture with one CU removed,
lists with a record that does not count, and one picture of each list fixture under tests/golden/.  No device: the helper is host code, reached
through the interpreter build of the library."""
import numpy as np
import pytest

import maps_util as mu
from golden_io import load_gold
from test_emu_picture import emu_lib  # noqa: F401  (fixture)


@pytest.fixture(scope="module")
def lib(emu_lib):  # noqa: F811
    return emu_lib


@pytest.mark.parametrize("name", list(mu.GEOMETRIES))
def test_synthetic_geometries(lib, name):
    pic, painted = mu.synthetic(name)
    big = name.startswith("416")
    for lu in mu.UNITS:
        # (a linear search per unit: the largest picture at 4x4 units is sampled every third unit, every map and every other size in full)
        mu.check_host_unit(lib, pic, lu, painted=painted, step=3 if big and lu == 2 else 1)


def test_sampling_picture(lib):
    pic = mu.sampling_picture()
    for lu in (2, 3, 4):
        mu.check_host_unit(lib, pic, lu)


def test_one_cu_removed(lib):
    pic, _ = mu.synthetic("200x120_ctb16")
    cut, _ = mu.without_one_cu(pic, len(pic.cus) // 2)
    for lu in (2, 3):
        mu.check_host_unit(lib, cut, lu)


def test_records_that_do_not_count(lib):
    for what, pic, _ in mu.skipped_pictures():
        mu.check_host_unit(lib, pic, 2)


@pytest.mark.parametrize("fixture,index", [("girlshy_full.m355gold.gz", 1), ("encintra_ctb16_lq.m355gold.gz", 0), ("encintra_ctb32_hq.m355gold.gz", 0),
                                           ("encintra_ctb64.m355gold.gz", 0)])
def test_golden_lists(lib, fixture, index):
    pic = load_gold(fixture)[1][index]
    painted = mu.paint(pic)
    c = painted["count"]
    assert c["cu"].max() <= 1 and c["tu"].max() <= 1 and c["pred"].max() <= 1, "recorded lists do not overlap"
    assert (c["cu"] == 1).all(), "the coding units of a recorded picture cover it"
    for lu in (3, 5):
        mu.check_host_unit(lib, pic, lu, painted=painted)
    mu.check_host_unit(lib, pic, 2, painted=painted, step=5)


def test_refused_arguments(lib):
    pic, _ = mu.synthetic("72x40_ctb64")
    c, keep = pic.to_c()
    import ctypes
    buf = (ctypes.c_uint8 * 8)()
    L = lib.lib
    a = ctypes.addressof(c)
    assert L.m355_maps_unit(a, 0, 2, 0, 0, buf) == 0
    for args in ((None, 0, 2, 0, 0, buf), (a, 0, 2, 0, 0, None), (a, -1, 2, 0, 0, buf), (a, 7, 2, 0, 0, buf), (a, 0, 1, 0, 0, buf), (a, 0, 7, 0, 0, buf),
                 (a, 0, 2, 18, 0, buf), (a, 0, 2, 0, 10, buf), (a, 0, 2, -1, 0, buf), (a, 0, 6, 2, 0, buf)):
        assert L.m355_maps_unit(*args) == mu.INVALID, args[1:5]
    assert L.m355_maps_unit(a, 0, 6, 1, 0, buf) == 0, "the last unit hangs over the edge and exists"
    del keep
    assert np.frombuffer(bytes(buf)[:4], "<u4")[0] != mu.NONE_CU
