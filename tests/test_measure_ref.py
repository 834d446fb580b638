"""The numpy restatement the comparison-request tests take their expected values from (tests/measure_util.py: int64 differences, the MSE
summed row by row in double) against the reference's own functions — SSD, SAD and MSE of libde265/quality.cc in the reference build:
SSD / SAD exactly, MSE bit for bit.  8-bit planes (all quality.cc knows) with strides above the width; SSD and SAD return uint32_t, so the
sizes keep width * height below 66051 (65025 * 66051 < 2^32): they cannot wrap."""
import ctypes
import struct

import numpy as np
import pytest

from measure_util import measure_plane

SIZES = [(50, 22), (1032, 16), (516, 8), (7, 3), (2, 2)]


def bind(ref):
    u8p, i = ctypes.c_void_p, ctypes.c_int
    fns = {}
    for name, sym, res in (("SSD", "_Z3SSDPKhiS0_iii", ctypes.c_uint32), ("SAD", "_Z3SADPKhiS0_iii", ctypes.c_uint32), ("MSE", "_Z3MSEPKhiS0_iii", ctypes.c_double)):
        f = getattr(ref, sym)
        f.argtypes, f.restype = [u8p, i, u8p, i, i, i], res
        fns[name] = f
    return fns


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("kind", ["random", "extreme"])
def test_restatement_equals_quality_cc(ref, w, h, kind):
    assert w * h < 66051
    fns = bind(ref)
    rng = np.random.default_rng(1000 * w + h)
    sa, sb = w + 5, w + 11
    a, b = rng.integers(0, 256, (h, sa), dtype=np.uint8), rng.integers(0, 256, (h, sb), dtype=np.uint8)
    if kind == "extreme":
        a[:, :w] = 255
        b[:, :w] = 0
    want = measure_plane(a[:, :w], b[:, :w])
    args = (a.ctypes.data, sa, b.ctypes.data, sb, w, h)
    assert fns["SSD"](*args) == want["ssd"]
    assert fns["SAD"](*args) == want["sad"]
    assert struct.pack("<d", fns["MSE"](*args)) == struct.pack("<d", want["mse"])
