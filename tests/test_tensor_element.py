"""m355_tensor_element (host only, no device): the float stage of m355_frames_export_tensor, the function the kernel compiles too
(libde265_amd/csrc/tensor_element.h), for EVERY integer 0..65535 under every dtype against the numpy restatement of the header's definition
(export_tensor_util.element_bits): two separate float32 operations — a contracted multiply-add differs on these inputs, which the test checks of its
own reference —, then binary16 by numpy's conversion (round to nearest even, subnormals, infinity) or bfloat16 by the integer expression, which is
cross-checked against torch.bfloat16 where torch imports.  No (scale, bias) pair makes a nonzero binary32 subnormal.  And the descriptor's layout."""
import ctypes
import os
import re

import numpy as np
import pytest

from test_emu_picture import emu_lib  # noqa: F401  (fixture)
from export_tensor_util import DTYPES, ELEMENT_PAIRS as PAIRS, bf16_bits, element_bits
from libde265_amd import capi

M355_ERR_INVALID = 3
V = np.arange(65536, dtype=np.uint32)


@pytest.fixture(params=["product", "interpreter"])
def lib(request):
    """both builds of the header's host side: the product library (the host pass of the HIP compiler; loading it needs no device) and the
    SIMT-interpreter build (the plain C++ fallbacks the CPU tier's kernels run)"""
    return capi.Library() if request.param == "product" else request.getfixturevalue("emu_lib")


def library_bits(lib, scale, bias, dtype):
    out, bits = np.zeros(len(V), np.uint32), ctypes.c_uint32()
    fn = lib.lib.m355_tensor_element
    for v in range(len(V)):
        assert fn(v, scale, bias, dtype, ctypes.byref(bits)) == 0
        out[v] = bits.value
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "%.6g_%.6g" % p)
def test_every_integer(lib, pair, dtype):
    scale, bias = pair
    want = element_bits(V, scale, bias, dtype)
    got = library_bits(lib, scale, bias, dtype)
    bad = np.flatnonzero(got != want.astype(np.uint32))
    assert not len(bad), "%d values differ, first v = %d: 0x%x, expected 0x%x" % (len(bad), bad[0], got[bad[0]], int(want[bad[0]]))


def test_the_inputs_see_what_they_should():
    """of the reference alone: the pairs hold values at which a fused multiply-add differs from two roundings, at which truncation differs from round
    to nearest even in both 16-bit formats, binary16 subnormals and binary16 infinities; and no product or sum is a nonzero binary32 subnormal"""
    fused = truncated16 = truncated_bf = subnormal = infinite = 0
    tiny = np.finfo(np.float32).tiny
    for scale, bias in PAIRS:
        t = V.astype(np.float32) * np.float32(scale)
        r = t + np.float32(bias)
        for x in (t, r):
            assert not np.any((x != 0) & (np.abs(x) < tiny)), "a binary32 subnormal: outside the contract"
        exact = (V.astype(np.float64) * np.float64(np.float32(scale)) + np.float64(np.float32(bias))).astype(np.float32)   # one rounding: what an FMA gives
        fused += int(np.count_nonzero(exact != r))
        with np.errstate(over="ignore"):
            h = r.astype(np.float16)
        bits16 = h.view(np.uint16)
        subnormal += int(np.count_nonzero(((bits16 & 0x7C00) == 0) & ((bits16 & 0x3FF) != 0)))
        infinite += int(np.count_nonzero(np.isinf(h)))
        with np.errstate(over="ignore"):
            toward_zero = np.where(np.abs(h.astype(np.float32)) > np.abs(r), np.nextafter(h, np.float16(0)), h)
        truncated16 += int(np.count_nonzero(toward_zero.view(np.uint16) != bits16))
        truncated_bf += int(np.count_nonzero((r.view(np.uint32) >> 16).astype(np.uint16) != bf16_bits(r)))
    assert fused and truncated16 and truncated_bf and subnormal and infinite, (fused, truncated16, truncated_bf, subnormal, infinite)


def test_bf16_restatement_is_torch_bfloat16():
    torch = pytest.importorskip("torch")
    for scale, bias in PAIRS:
        r = V.astype(np.float32) * np.float32(scale) + np.float32(bias)
        want = torch.from_numpy(r).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
        assert np.array_equal(bf16_bits(r), want), (scale, bias)


def test_tensor_element_rejects_bad_arguments(lib):
    fn, bits = lib.lib.m355_tensor_element, ctypes.c_uint32(0x12345678)
    for dtype in (-1, 3):
        assert fn(1, 1.0, 0.0, dtype, ctypes.byref(bits)) == M355_ERR_INVALID
    for scale, bias in ((float("inf"), 0.0), (float("nan"), 0.0), (1.0, float("-inf")), (1.0, float("nan"))):
        assert fn(1, scale, bias, capi.TENSOR_F32, ctypes.byref(bits)) == M355_ERR_INVALID
    assert fn(1, 1.0, 0.0, capi.TENSOR_F32, None) == M355_ERR_INVALID
    assert bits.value == 0x12345678
    assert lib.tensor_element(255, 1.0, 0.0, capi.TENSOR_F32) == 0x437F0000 and lib.tensor_element(255, 1.0, 0.0, capi.TENSOR_BF16) == 0x437F
    assert lib.tensor_element(1, 1.0, 0.0, capi.TENSOR_F16) == 0x3C00


def test_tensor_desc_abi():
    """sizeof and the field offsets of m355_tensor_desc as the header declares it (LP64), against the ctypes structure; the header's field order is
    read from the header itself"""
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "de265_mi355x.h")).read()
    body = re.search(r"typedef struct m355_tensor_desc \{(.*?)\} m355_tensor_desc;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names, offsets, ofs = [], {}, 0
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, rest = re.match(r"(int32_t|int64_t|float|void\*)\s*(.*)", decl).groups()
        size = 4 if ctype in ("int32_t", "float") else 8
        for item in rest.split(","):
            name, count = re.match(r"\s*(\w+)(?:\[(\d+)\])?", item).groups()
            ofs = (ofs + size - 1) // size * size
            names.append(name); offsets[name] = ofs
            ofs += size * int(count or 1)
    assert names == [n for n, _ in capi.TensorDesc._fields_]
    for n in names:
        assert getattr(capi.TensorDesc, n).offset == offsets[n], n
    assert ctypes.sizeof(capi.TensorDesc) == (ofs + 7) // 8 * 8 == 104
    assert (capi.TENSOR_MAX_FRAMES, capi.TENSOR_NCHW, capi.TENSOR_NHWC, capi.TENSOR_F32, capi.TENSOR_F16, capi.TENSOR_BF16) == \
        tuple(int(re.search(r"#define M355_TENSOR_%s\s+(\d+)" % n, header).group(1)) for n in ("MAX_FRAMES", "NCHW", "NHWC", "F32", "F16", "BF16"))
