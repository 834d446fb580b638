"""The host-only helpers that go with the statistics requests (include/de265_mi355x.h): m355_stats_quantile against a numpy cumulative sum,
m355_colour_linear against step 1 of the colour transform stated here, and m355_colour_pixel — which now runs that same step-1 code — against the
values the commit before the helper was factored out delivered (tests/golden/colour_pixel_parent.npy).  No device."""
import os

import numpy as np
import pytest

from test_emu_picture import emu_lib  # noqa: F401  (fixture)
from libde265_amd import capi

INVALID = 3
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "colour_pixel_parent.npy")


def quantile(hist, num, den):
    """the definition in Python integers: the smallest b with den * cumsum[b] >= num * total"""
    run, total = 0, int(sum(int(v) for v in hist))
    for b, v in enumerate(hist):
        run += int(v)
        if den * run >= num * total:
            return b
    raise AssertionError("not reached")


def test_quantile_against_cumulative_sum(emu_lib):  # noqa: F811
    rng = np.random.default_rng(4100)
    for k in range(60):
        hist = rng.integers(0, [3, 1000, 1 << 32][k % 3], 256, dtype=np.uint64)
        if k % 4 == 0:
            hist[rng.integers(0, 256, 200)] = 0                     # runs of empty bins
        cum = np.cumsum(hist.astype(object))
        for num, den in ((1, 2), (999, 1000), (1, 1000), (1, 1 << 20), ((1 << 20) - 1, 1 << 20), (1 << 20, 1 << 20), (7, 7), (1, 1)):
            want = int(np.argmax([den * int(c) >= num * int(cum[-1]) for c in cum]))
            assert want == quantile(hist, num, den)
            assert emu_lib.stats_quantile(hist, num, den) == want, "histogram %d at %d / %d" % (k, num, den)


def test_quantile_edges(emu_lib):  # noqa: F811
    one = [0] * 256
    one[97] = 12345
    for num, den in ((1, 1000), (1, 2), (1000, 1000)):
        assert emu_lib.stats_quantile(one, num, den) == 97          # a single non-empty bin
    two = [0] * 256
    two[3], two[200] = 999, 1
    assert emu_lib.stats_quantile(two, 999, 1000) == 3 and emu_lib.stats_quantile(two, 1000, 1000) == 200   # num == den: the last non-empty bin
    full = [(1 << 32) - 1] * 256                                    # the largest total: 64-bit products
    assert emu_lib.stats_quantile(full, 1 << 20, 1 << 20) == 255 and emu_lib.stats_quantile(full, 1, 1 << 20) == 0
    for hist, num, den in (([0] * 256, 1, 2), (one, 0, 2), (one, 3, 2), (one, 1, (1 << 20) + 1), (None, 1, 2)):
        with pytest.raises(capi.M355Error) as e:
            emu_lib.stats_quantile(hist, num, den)
        assert e.value.code == INVALID
    import ctypes
    assert emu_lib.lib.m355_stats_quantile((ctypes.c_uint32 * 256)(*one), 1, 2, None) == INVALID, "null result"


def linear(lut_in, v):
    """step 1 as the header states it"""
    k, f = v >> 6, v & 63
    return (lut_in[k].astype(np.int64) * (64 - f) + lut_in[k + 1].astype(np.int64) * f + 32) >> 6


def test_colour_linear_is_step_one(emu_lib):  # noqa: F811
    v = np.arange(65536)
    pq = emu_lib.colour_preset(16, 9, 1, 1, tone=capi.TONE_REINHARD, peak_nits=1000)
    identity = capi.colour_tables([min(64 * k, 65535) * 256 + (min(64 * k, 65535) >> 8) for k in range(capi.COLOUR_IN_KNOTS)], [1 << 14, 0, 0, 0, 1 << 14, 0, 0, 0, 1 << 14],
                                  [0] * capi.COLOUR_OUT_KNOTS)
    for name, t in (("PQ", pq), ("identity", identity)):
        want = linear(np.array(list(t.lut_in), np.int64), v)
        got = np.array([emu_lib.colour_linear(t, int(x)) for x in v], np.int64)
        assert np.array_equal(got, want), name
        assert int(got.max()) <= capi.COLOUR_ONE
    with pytest.raises(capi.M355Error) as e:
        emu_lib.colour_linear(pq, 65536)
    assert e.value.code == INVALID
    import ctypes
    assert emu_lib.lib.m355_colour_linear(None, 0, ctypes.byref(ctypes.c_uint32())) == INVALID
    assert emu_lib.lib.m355_colour_linear(ctypes.byref(pq), 0, None) == INVALID


def test_colour_pixel_is_unchanged(emu_lib):  # noqa: F811
    """1000 seeded pixels through a PQ / BT.2020 -> BT.709 preset with the Reinhard curve: columns 0..2 the pixel, 3..5 what the parent commit
    delivered for M355_RGB_U16, 6..8 for M355_RGB_U8"""
    rec = np.load(GOLDEN)
    assert rec.shape == (1000, 9)
    t = emu_lib.colour_preset(16, 9, 1, 1, tone=capi.TONE_REINHARD, peak_nits=1000)
    for row in rec:
        px = [int(x) for x in row[:3]]
        assert emu_lib.colour_pixel(t, px, capi.RGB_U16) == tuple(int(x) for x in row[3:6]), px
        assert emu_lib.colour_pixel(t, px, capi.RGB_U8) == tuple(int(x) for x in row[6:9]), px
