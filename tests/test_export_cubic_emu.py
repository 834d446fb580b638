"""M355_FILTER_CUBIC on the SIMT-interpreter build: the filter rows (m355_resize_taps_filtered against the Python-integer restatement, the sizes at
which the row's sums leave 63 bits included), their properties and rejections, the restatement against an independent float64 Catmull-Rom resize,
and every cubic instantiation of k_export_resized and k_export_resized_rgb (RR_FRAME, RR_BATCH, RR_ROIS) against the restatement: the format matrix
at 64x32, 16-bit samples, impulses and checkerboards of 0 and the maximum, the identity, rectangle against cropped frame, the smallest sizes, several
tiles per row, a batch, regions of different ratios with a mirrored one, the argument checks, the gate and the reader bookkeeping.  Expected values
come from export_cubic_util.py; every comparison of an export is exact."""
import ctypes
import random

import numpy as np
import pytest

from test_emu_picture import emu_lib  # noqa: F401  (fixture)
from oracle_py import Oracle
import export_resized_util as tri
import export_resized_rgb_util as tri_rgb
import export_tensor_util as tri_tensor
import export_tensor_rois_util as tri_rois
from export_util import FORMATS, M355_ERR_INVALID, format_id
from export_cubic_util import (ABS_SUM_BOUND, CUBIC, MATRIX_SIZES, MAX_N, check_16_bit_formats, check_minimum_sizes, check_rect_equals_cropped_frame,
                               check_several_tiles, check_tensor_batch, check_tensor_rois, check_value_cases, convert, cubic, float_resize, max_taps,
                               ratio_ok, resize_plane, taps, upload_random)
from test_export_resized_emu import TAP_PAIRS
from libde265_amd import capi


@pytest.fixture()
def ctx(emu_lib):  # noqa: F811
    c = capi.Context(emu_lib, 0)
    yield c
    c.close()


def check_row(lib, sn, dn, cosited, i):
    want = taps(sn, dn, cosited, i)
    assert lib.resize_taps(sn, dn, cosited, i, filter=CUBIC) == want, "cubic taps %d -> %d, cosited %d, row %d" % (sn, dn, cosited, i)
    first, q = want
    assert 0 <= first and first + len(q) <= sn and 1 <= len(q) <= max_taps(sn, dn) <= 16
    assert sum(q) == 1 << 14 and sum(abs(x) for x in q) <= ABS_SUM_BOUND
    return q


def check_axis(lib, sn, dn, rows=None):
    for cosited in (0, 1):
        for i in (range(dn) if rows is None else rows):
            check_row(lib, sn, dn, cosited, i)


CUBIC_PAIRS = [p for p in TAP_PAIRS if ratio_ok(*p)] + [(64, 16), (16, 64), (13, 12)]


@pytest.mark.parametrize("sn,dn", CUBIC_PAIRS)
def test_cubic_taps_equal_the_restatement(emu_lib, sn, dn):  # noqa: F811
    assert ratio_ok(sn, dn)
    check_axis(emu_lib, sn, dn)


@pytest.mark.parametrize("sn,dn", [(16384, 16383), (16383, 4096), (12289, 16384)])
def test_cubic_taps_where_the_sums_leave_63_bits(emu_lib, sn, dn):  # noqa: F811
    """N has up to 48 bits there, so 2 (P << 14) + N does not fit 63: the first and last rows, the middle, and 40 random ones"""
    rng = random.Random(8500 + sn)
    rows = sorted(set([0, 1, 2, dn // 2 - 1, dn // 2, dn - 3, dn - 2, dn - 1] + [rng.randrange(dn) for _ in range(40)]))
    check_axis(emu_lib, sn, dn, rows)


def test_cubic_taps_of_random_pairs(emu_lib):  # noqa: F811
    rng = random.Random(8501)
    for _ in range(200):
        sn = rng.randint(1, 400)
        dn = rng.randint((sn + 3) // 4, min(8 * sn, 400))
        assert ratio_ok(sn, dn)
        check_axis(emu_lib, sn, dn)


def test_cubic_row_properties(emu_lib):  # noqa: F811
    """the identity row is {0, 1 << 14, 0} (folded at the ends), 13 -> 12 co-sited holds the largest sum of |q| the definition's sweep found, some
    coefficient is negative, and ratio 4 reaches 16 coefficients"""
    for n in (1, 2, 7, 64):
        for i in range(n):
            first, q = emu_lib.resize_taps(n, n, 0, i, filter=CUBIC)
            full = {first + j: x for j, x in enumerate(q)}
            assert full.get(i) == 1 << 14 and all(x == 0 for k, x in full.items() if k != i), (n, i, first, q)
            if 0 < i < n - 1:
                assert (first, q) == (i - 1, [0, 1 << 14, 0])
    sums = [sum(abs(x) for x in check_row(emu_lib, 13, 12, 1, i)) for i in range(12)]
    assert max(sums) == 20788
    assert any(x < 0 for i in range(12) for x in taps(13, 12, 1, i)[1])
    assert max(len(emu_lib.resize_taps(64, 16, 0, i, filter=CUBIC)[1]) for i in range(16)) == 16


def test_cubic_taps_reject_bad_arguments(emu_lib):  # noqa: F811
    assert emu_lib.resize_taps(65, 16, 0, 0) is not None, "the triangle takes 65 -> 16"
    bad = [(65, 16, 0, 0), (16, 129, 0, 0), (MAX_N + 1, MAX_N, 0, 0), (MAX_N, MAX_N + 1, 0, 0), (0, 4, 0, 0), (4, 0, 0, 0), (-3, 4, 0, 0), (8, 4, 2, 0),
           (8, 4, -1, 0), (8, 4, 0, -1), (8, 4, 0, 4)]
    for args in bad:
        assert emu_lib.resize_taps(*args, filter=CUBIC) is None, args
    for f in (-1, 2, 77):
        assert emu_lib.resize_taps(8, 4, 0, 0, filter=f) is None, "filter %d" % f
    first, coeff = ctypes.c_int32(), (ctypes.c_int32 * 16)()
    assert emu_lib.lib.m355_resize_taps_filtered(CUBIC, 8, 4, 0, 0, None, coeff) < 0
    assert emu_lib.lib.m355_resize_taps_filtered(CUBIC, 8, 4, 0, 0, ctypes.byref(first), None) < 0
    assert emu_lib.resize_taps(64, 16, 0, 15, filter=CUBIC) is not None and emu_lib.resize_taps(8, 64, 1, 63, filter=CUBIC) is not None
    assert emu_lib.resize_taps(MAX_N, MAX_N, 0, MAX_N - 1, filter=CUBIC) is not None


def test_filter_0_is_the_triangle_row_for_row(emu_lib):  # noqa: F811
    for sn, dn in TAP_PAIRS[:9] + [(65, 16)]:
        for cosited in (0, 1):
            for i in range(dn):
                row = emu_lib.resize_taps(sn, dn, cosited, i, filter=capi.FILTER_TRIANGLE, filtered_entry=True)
                assert row is not None and row == emu_lib.resize_taps(sn, dn, cosited, i) == tri.taps(sn, dn, cosited, i)
    for args in [(65, 8, 0, 0), (8, 65, 0, 0), (8, 4, 2, 0)]:
        assert emu_lib.resize_taps(*args, filter=capi.FILTER_TRIANGLE, filtered_entry=True) is None


@pytest.mark.parametrize("pattern", ["noise", "checkerboard"])
def test_the_restatement_is_an_antialiased_bicubic_resize(pattern):
    """no library: the integer restatement at U8 against a float64 Catmull-Rom resize written independently, rounded and clipped: at most 1 apart.
    The prefix rounding puts each coefficient within one unit of 2^-14 of the real weight; with at most 16 coefficients and an overshoot of at most
    1.27 that is below 0.32 LSB per pass, the intermediate rounding (2^-8 LSB) is negligible: below 0.7 LSB before the final rounding"""
    rng = np.random.default_rng(8510)
    for (sw, sh), (ow, oh) in [((64, 48), (16, 12)), ((64, 48), (48, 20)), ((40, 24), (64, 64)), ((17, 9), (5, 3)), ((12, 8), (96, 64)), ((96, 80), (25, 21))]:
        if pattern == "noise":
            S = rng.integers(0, 256, (sh, sw))
        else:
            S = ((np.arange(sw)[None, :] + np.arange(sh)[:, None]) % 2 * 255).astype(np.int64)
        for cosited in (0, 1):
            a = convert(resize_plane(S.astype(np.uint8), ow, oh, cosited, 8), 8, capi.EXPORT_U8, np.uint8).astype(np.int64)
            f = float_resize(S, ow, oh, cosited)
            assert float(np.abs(a - f)[(f >= 0) & (f <= 255)].max()) < 1.2
            diff = int(np.abs(a - np.clip(np.rint(f), 0, 255).astype(np.int64)).max())
            print("%s %dx%d -> %dx%d cosited %d: largest difference %d" % (pattern, sw, sh, ow, oh, cosited, diff))
            assert diff <= 1, "%s %dx%d -> %dx%d, cosited %d: %d apart" % (pattern, sw, sh, ow, oh, cosited, diff)


@pytest.mark.parametrize("fmt", FORMATS, ids=format_id)
def test_cubic_resized_format_matrix(ctx, oracle, fmt):
    with cubic(ctx) as c:
        tri.check_format_matrix_resized(c, Oracle(oracle), dict(fmt, width=64, height=32, log2_ctb=5), MATRIX_SIZES)


@pytest.mark.parametrize("fmt", FORMATS, ids=format_id)
def test_cubic_resized_rgb_format_matrix(ctx, oracle, fmt):
    with cubic(ctx) as c:
        tri_rgb.check_format_matrix(c, Oracle(oracle), dict(fmt, width=64, height=32, log2_ctb=5), MATRIX_SIZES)


@pytest.mark.parametrize("fmt", FORMATS[:4], ids=format_id)
def test_cubic_tensor_format_matrix(ctx, oracle, fmt):
    """NCHW / NHWC x F32 / F16 / BF16 at the sizes of the cubic matrix"""
    with cubic(ctx) as c:
        tri_tensor.check_format_matrix(c, Oracle(oracle), dict(fmt, width=64, height=32, log2_ctb=5))


@pytest.mark.parametrize("rgb", [False, True], ids=["yuv", "rgb"])
def test_cubic_16_bit_samples(ctx, rgb):
    check_16_bit_formats(ctx, rgb)


@pytest.mark.parametrize("bit_depth", [8, 12, 16])
def test_cubic_values_and_clips(ctx, bit_depth):
    check_value_cases(ctx, bit_depth)


@pytest.mark.parametrize("bit_depth", [8, 12, 16])
def test_cubic_rgb_values_and_clips(ctx, bit_depth):
    check_value_cases(ctx, bit_depth, rgb=True)


@pytest.mark.parametrize("bit_depth", [8, 12, 16])
def test_cubic_constants_ramps_and_alternations(ctx, bit_depth):
    """export_resized_util.value_cases: a constant plane stays constant at 0 and at the maximum, in the restatement and in the export"""
    with cubic(ctx) as c:
        tri.check_values(c, bit_depth)


@pytest.mark.parametrize("bit_depth,layout", [(8, capi.EXPORT_PLANAR), (10, capi.EXPORT_SEMIPLANAR)])
def test_cubic_same_size_is_the_plain_export(ctx, oracle, bit_depth, layout):
    with cubic(ctx) as c:
        tri.check_identity(c, Oracle(oracle), bit_depth, layout)


@pytest.mark.parametrize("bit_depth,layout", [(8, capi.RGB_PACKED), (10, capi.RGB_PLANAR)])
def test_cubic_whole_frame_at_its_own_size_is_the_rgb_export(ctx, oracle, bit_depth, layout):
    with cubic(ctx) as c:
        tri_rgb.check_identity(c, Oracle(oracle), bit_depth, layout)


@pytest.mark.parametrize("rgb", [False, True], ids=["yuv", "rgb"])
def test_cubic_rectangle_equals_cropped_frame(ctx, rgb):
    check_rect_equals_cropped_frame(ctx, rgb)


@pytest.mark.parametrize("rgb", [False, True], ids=["yuv", "rgb"])
def test_cubic_minimum_sizes(ctx, rgb):
    check_minimum_sizes(ctx, rgb)


@pytest.mark.parametrize("rgb", [False, True], ids=["yuv", "rgb"])
def test_cubic_several_tiles(ctx, rgb):
    check_several_tiles(ctx, rgb)


def test_cubic_tensor_batch(ctx):
    check_tensor_batch(ctx)


def test_cubic_tensor_regions_of_different_ratios(ctx):
    check_tensor_rois(ctx)


def test_filter_0_entry_points_are_the_plain_ones(ctx):
    """every _filtered entry point with M355_FILTER_TRIANGLE delivers what the plain one delivers, byte for byte, at a ratio the cubic filter rejects"""
    frame, planes = upload_random(ctx, (64, 32), 1, 10, 8570)
    try:
        out = (8, 4)
        a = ctx.frame_export_finish(ctx.frame_export_resized(frame, capi.EXPORT_SEMIPLANAR, capi.EXPORT_MSB16, out), raw=True)[1]
        b = ctx.frame_export_finish(ctx.frame_export_resized(frame, capi.EXPORT_SEMIPLANAR, capi.EXPORT_MSB16, out, filtered_entry=True), raw=True)[1]
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
        a = ctx.frame_export_finish(ctx.frame_export_resized_rgb(frame, capi.RGB_PACKED, capi.RGB_U8, capi.MATRIX_BT709, 0, out), raw=True)[1]
        b = ctx.frame_export_finish(ctx.frame_export_resized_rgb(frame, capi.RGB_PACKED, capi.RGB_U8, capi.MATRIX_BT709, 0, out, filtered_entry=True), raw=True)[1]
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
        scale, bias = tri_tensor.imagenet(capi.RGB_U8)
        args = (capi.TENSOR_NCHW, capi.TENSOR_F16, capi.RGB_U8, capi.MATRIX_BT709, 0, out, scale, bias)
        a = ctx.tensor_export_finish(ctx.frames_export_tensor([frame, frame], *args))
        b = ctx.tensor_export_finish(ctx.frames_export_tensor([frame, frame], *args, filtered_entry=True))
        assert np.array_equal(a[1], b[1])
        rois = [(0, 0, 64, 32, 0), (2, 2, 40, 20, capi.ROI_MIRROR)]
        a = ctx.tensor_export_finish(ctx.frames_export_tensor_rois([frame, frame], rois, *args))
        b = ctx.tensor_export_finish(ctx.frames_export_tensor_rois([frame, frame], rois, *args, filtered_entry=True))
        assert np.array_equal(a[1], b[1])
    finally:
        ctx.frame_destroy(frame)


def test_cubic_exports_reject_bad_arguments(ctx):
    """through one cubic call of each entry point: an unknown filter, more than 4x down on either axis (which the triangle takes), an ROI entry beyond
    4x down beside good ones, and what the plain calls reject; every rejected call returns M355_ERR_INVALID, and the destination they all name
    still holds the bytes it was allocated with"""
    lib = ctx.L.lib
    frame = ctx.frame_create(64, 32, 1, 10, 10)
    nbytes = 3 * 3 * 64 * 256          # three slices of the tensor descriptor below; the planes of the other descriptors need less
    buf = ctx.device_alloc(nbytes)
    one = (ctypes.c_int * 1)(frame)

    def resize_desc(out=(32, 16), pitch=300, dst=True):
        d = capi.ResizeDesc(layout=capi.EXPORT_PLANAR, samples=capi.EXPORT_NATIVE, out_width=out[0], out_height=out[1])
        for j in range(3):
            d.dst[j] = buf + j * 64 * 300 if dst else None
            d.pitch[j] = pitch
        return d

    def rgb_desc(out=(32, 16), pitch=300):
        d = capi.ResizeRgbDesc(layout=capi.RGB_PACKED, samples=capi.RGB_U8, matrix=capi.MATRIX_BT709, full_range=0, out_width=out[0], out_height=out[1])
        d.dst[0] = buf
        d.pitch[0] = pitch
        return d

    def tensor_desc(out=(32, 16), stride_h=256):
        d = capi.TensorDesc(layout=capi.TENSOR_NCHW, dtype=capi.TENSOR_F32, samples=capi.RGB_U8, matrix=capi.MATRIX_BT709, full_range=0, out_width=out[0],
                            out_height=out[1], stride_n=3 * 64 * 256, stride_c=64 * 256, stride_h=stride_h)
        d.scale = (ctypes.c_float * 3)(1.0, 1.0, 1.0)
        d.dst = buf
        return d

    def rois(*r):
        return (capi.TensorRoi * len(r))(*[capi.TensorRoi(*x) for x in r])

    whole = rois((0, 0, 0, 0, 0))
    calls = {
        "resized": lambda d, f: lib.m355_frame_export_resized_filtered(ctx.h, frame, ctypes.byref(d), f),
        "rgb": lambda d, f: lib.m355_frame_export_resized_rgb_filtered(ctx.h, frame, ctypes.byref(d), f),
        "tensor": lambda d, f: lib.m355_frames_export_tensor_filtered(ctx.h, one, 1, ctypes.byref(d), f),
        "rois": lambda d, f: lib.m355_frames_export_tensor_rois_filtered(ctx.h, one, whole, 1, ctypes.byref(d), f),
    }
    descs = {"resized": resize_desc, "rgb": rgb_desc, "tensor": tensor_desc, "rois": tensor_desc}
    for name, call in calls.items():
        mk = descs[name]
        for f in (-1, 2, 1 << 20):
            assert call(mk(), f) == M355_ERR_INVALID, "%s: filter %d" % (name, f)
        assert call(mk(out=(14, 16)), CUBIC) == M355_ERR_INVALID, "%s: more than 4x down, width" % name
        assert call(mk(out=(32, 6)), CUBIC) == M355_ERR_INVALID, "%s: more than 4x down, height" % name
        assert "cubic" in ctx.L.error()
        assert call(mk(out=(33, 16)), CUBIC) == M355_ERR_INVALID, "%s: odd width" % name
        assert call(mk(out=(0, 16)), CUBIC) == M355_ERR_INVALID, "%s: no width" % name
    assert calls["resized"](resize_desc(pitch=63), CUBIC) == M355_ERR_INVALID
    assert calls["resized"](resize_desc(dst=False), CUBIC) == M355_ERR_INVALID
    assert calls["rgb"](rgb_desc(pitch=95), CUBIC) == M355_ERR_INVALID
    assert calls["tensor"](tensor_desc(stride_h=124), CUBIC) == M355_ERR_INVALID
    three = (ctypes.c_int * 3)(frame, frame, frame)
    # the limit is checked per entry: to 12x6, 48x24 goes from two places, 50x24 does not (50 > 4 * 12), and the message names the entry
    d = tensor_desc(out=(12, 6))
    assert lib.m355_frames_export_tensor_rois_filtered(ctx.h, three, rois((0, 0, 48, 24, 0), (2, 2, 48, 24, 1), (14, 8, 50, 24, 0)), 3, ctypes.byref(d), CUBIC) == M355_ERR_INVALID
    assert "entry 2" in ctx.L.error()
    ctx.wait()
    assert np.all(ctx.device_read(buf, nbytes) == capi.DEVICE_FILL), "a rejected export wrote to its destination"
    assert lib.m355_frames_export_tensor_rois_filtered(ctx.h, three, rois((0, 0, 48, 24, 0), (2, 2, 48, 24, 1), (14, 8, 50, 24, 0)), 3, ctypes.byref(d), capi.FILTER_TRIANGLE) == 0, ctx.L.error()
    assert lib.m355_frames_export_tensor_rois_filtered(ctx.h, three, rois((0, 0, 48, 24, 0), (2, 2, 48, 24, 1), (14, 8, 46, 24, 0)), 3, ctypes.byref(d), CUBIC) == 0, ctx.L.error()
    ctx.wait()
    # the limit itself is fine: exactly 4x down on both axes
    assert calls["resized"](resize_desc(out=(16, 8)), CUBIC) == 0, ctx.L.error()
    assert calls["rgb"](rgb_desc(out=(16, 8)), CUBIC) == 0, ctx.L.error()
    assert calls["tensor"](tensor_desc(out=(16, 8)), CUBIC) == 0, ctx.L.error()
    ctx.wait()
    ctx.device_free(buf)
    ctx.frame_destroy(frame)


def test_cubic_exports_behind_a_rejected_decode_write_nothing(ctx):
    with cubic(ctx) as c:
        tri.check_gate_resized(c)
        tri_rgb.check_gate(c)
        tri_tensor.check_gate(c)
        tri_rois.check_gate(c)


@pytest.mark.parametrize("depth", [1, 3])
def test_cubic_exports_behind_recycled_frames(ctx, depth):
    """(the interpreter runs every launch to its end at once: this walks the reader bookkeeping, the GPU tier is what can see a missing wait)"""
    with cubic(ctx) as c:
        tri.check_hazard_resized(c, depth)
        tri_rgb.check_hazard(c, depth)
        tri_tensor.check_hazard(c, depth)
        tri_rois.check_hazard(c, depth)
