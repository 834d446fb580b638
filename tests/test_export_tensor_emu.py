"""m355_frames_export_tensor on the SIMT-interpreter build: the format matrix at 64x32, the composition through the public calls, batches of distinct
frames with different pitches, the same frame twice, one and several workgroups per slice, the smallest outputs, padded strides, the argument checks
with the overlap rules at their exact boundary, the gate per slice, the reader bookkeeping and a pinned-host destination.  Expected values: the planes
m355_frame_download returns through export_tensor_util.py (the integer restatement of the resized R'G'B' export, held against that call's own output,
then the float stage in numpy); every comparison is bit-exact, and every byte of the destination outside the tensor's elements must be untouched —
every export here has padded stride_h, stride_c and stride_n (capi.Context.frames_export_tensor), apart from the boundary cases of the argument test.

The build holds four instantiations, k_export_resized_rgb<source bytes, element bytes, RR_BATCH>; layout, F16 / BF16, chroma format and U8 / U16 of the integer stage
are run-time switches.  Which test reaches which (every test of the matrix runs NCHW and NHWC, U8 and U16, with F32, F16 and BF16):
  <1, 2>, <1, 4>  test_tensor_format_matrix[bd8_8_cf1], [bd8_8_cf4] (monochrome), test_tensor_minimum_sizes[8], test_tensor_gate_is_per_slice
  <2, 2>, <2, 4>  test_tensor_format_matrix[bd10_10_cf1], [bd12_12_cf2] (4:2:2), [bd10_10_cf3] (4:4:4), [bd10_9_cf1], test_tensor_minimum_sizes[10],
                  test_single_frame_is_the_resized_rgb_export_as_float (<2, 4>), test_batch_of_distinct_frames, test_same_frame_twice,
                  test_tensor_export_behind_recycled_frames (<2, 2>), test_tensor_export_into_pinned_host_memory"""
import ctypes

import numpy as np
import pytest

from test_emu_picture import emu_lib  # noqa: F401  (fixture)
from oracle_py import Oracle
from export_tensor_util import (FORMATS, M355_ERR_INVALID, check_batch, check_every_integer, check_composition, check_format_matrix, check_gate, check_hazard, check_minimum_sizes,
                                check_pinned_host, check_same_frame_twice, format_id)
from libde265_amd import capi


@pytest.fixture()
def ctx(emu_lib):  # noqa: F811
    c = capi.Context(emu_lib, 0)
    yield c
    c.close()


@pytest.mark.parametrize("fmt", FORMATS, ids=format_id)
def test_tensor_format_matrix(ctx, oracle, fmt):
    check_format_matrix(ctx, Oracle(oracle), dict(fmt, width=64, height=32, log2_ctb=5))


def test_single_frame_is_the_resized_rgb_export_as_float(ctx, oracle):
    check_composition(ctx, Oracle(oracle), dict(width=64, height=32, bit_depth=10, seed=8001, log2_ctb=5))


def test_every_integer_through_the_kernel(ctx):
    """(here the interpreter build's plain C++ float stage inside the kernel; the GPU tier runs the device's)"""
    check_every_integer(ctx)


def test_batch_of_distinct_frames(ctx, oracle):
    check_batch(ctx, Oracle(oracle))


def test_same_frame_twice(ctx, oracle):
    check_same_frame_twice(ctx, Oracle(oracle))


@pytest.mark.parametrize("bit_depth", [8, 10])
def test_tensor_minimum_sizes(ctx, oracle, bit_depth):
    check_minimum_sizes(ctx, Oracle(oracle), bit_depth)


def test_tensor_export_rejects_bad_arguments(ctx):
    """every rejected case returns M355_ERR_INVALID and leaves the destination as it was allocated; the limits themselves are accepted"""
    lib = ctx.L.lib
    frame = ctx.frame_create(64, 32, 1, 10, 10)
    same = ctx.frame_create(64, 32, 1, 10, 10)
    large = ctx.frame_create(128, 64, 1, 10, 10)
    small = ctx.frame_create(32, 16, 1, 10, 10)
    f422 = ctx.frame_create(64, 32, 2, 10, 10)
    depth8 = ctx.frame_create(64, 32, 1, 8, 8)
    depth12 = ctx.frame_create(64, 32, 1, 12, 12)      # (the element size of frame, another bit depth)
    depth9c = ctx.frame_create(64, 32, 1, 10, 9)
    mono = ctx.frame_create(64, 40, 0, 8, 8)
    nbytes = 1 << 16
    buf = ctx.device_alloc(nbytes)
    inf, nan = float("inf"), float("nan")

    def desc(out=(32, 16), layout=capi.TENSOR_NCHW, dtype=capi.TENSOR_F16, samples=capi.RGB_U8, matrix=capi.MATRIX_BT709, full=0, rect=(0, 0, 0, 0),
             scale=(1, 1, 1), bias=(0, 0, 0), dst=0, sn=4096, sc=1200, sh=72):
        d = capi.TensorDesc(layout=layout, dtype=dtype, samples=samples, matrix=matrix, full_range=full, out_width=out[0], out_height=out[1],
                            stride_n=sn, stride_c=sc, stride_h=sh)
        d.x0, d.y0, d.width, d.height = rect
        d.scale = (ctypes.c_float * 3)(*scale)
        d.bias = (ctypes.c_float * 3)(*bias)
        d.dst = None if dst is None else buf + dst
        return d

    def call(frames, d, n=None):
        arr = (ctypes.c_int * max(1, len(frames)))(*frames)
        return lib.m355_frames_export_tensor(ctx.h, arr, len(frames) if n is None else n, ctypes.byref(d) if d is not None else None)

    two = [frame, same]
    # 32x16 F16: NCHW row 64 bytes, E = 15 * sh + 64; NHWC row 192 bytes
    E = 15 * 72 + 64
    En = 15 * 200 + 192
    bad = [
        ("n 0", [frame], desc(), 0),
        ("n negative", [frame], desc(), -1),
        ("n above the limit", [frame] * 33, desc(), None),
        ("a bad handle", [frame, frame + 100], desc(), None),
        ("a negative handle", [-1], desc(), None),
        ("another chroma format", [frame, f422], desc(), None),
        ("another element size", [frame, depth8], desc(), None),
        ("another luma bit depth", [frame, depth12], desc(), None),
        ("another chroma bit depth", [frame, depth9c], desc(), None),
        ("whole frames of different sizes", [frame, large], desc(), None),
        ("a frame that does not contain the rectangle", [frame, small], desc(rect=(0, 0, 64, 32)), None),
        ("a frame that does not contain the rectangle, first", [small, frame], desc(rect=(0, 0, 64, 32)), None),
        ("rectangle leaves the frame", two, desc(rect=(32, 0, 48, 16)), None),
        ("rectangle off the chroma grid", two, desc(rect=(1, 0, 16, 16)), None),
        ("rectangle of no width", two, desc(rect=(0, 0, -4, 16)), None),
        ("out_width 0", two, desc(out=(0, 16)), None),
        ("out_height negative", two, desc(out=(32, -16)), None),
        ("out_width odd, 4:2:0", two, desc(out=(33, 16), sh=80), None),
        ("out_height odd, 4:2:0", two, desc(out=(32, 17), sc=1300), None),
        ("more than 8x down", two, desc(out=(6, 16)), None),
        ("one sample beyond 8x down", [mono], desc(out=(7, 40), rect=(0, 0, 57, 40), sc=4000), None),
        ("one sample beyond 8x up", [mono], desc(out=(65, 20), rect=(0, 0, 8, 20), sh=136, sc=4000), None),
        ("unknown samples", two, desc(samples=2), None),
        ("unknown matrix", two, desc(matrix=3), None),
        ("negative matrix", two, desc(matrix=-1), None),
        ("full_range 2", two, desc(full=2), None),
        ("unknown layout", two, desc(layout=2), None),
        ("negative layout", two, desc(layout=-1), None),
        ("unknown dtype", two, desc(dtype=3), None),
        ("negative dtype", two, desc(dtype=-1), None),
        ("scale infinite", two, desc(scale=(1, inf, 1)), None),
        ("scale NaN", two, desc(scale=(nan, 1, 1)), None),
        ("bias infinite", two, desc(bias=(0, 0, -inf)), None),
        ("bias NaN", two, desc(bias=(0, nan, 0)), None),
        ("no destination", two, desc(dst=None), None),
        ("F16 destination at an odd address", two, desc(dst=1), None),
        ("F32 destination off a multiple of 4", two, desc(dtype=capi.TENSOR_F32, dst=2, sh=128, sc=2048, sn=8192), None),
        ("F16 stride_h odd", two, desc(sh=73), None),
        ("F32 stride_h off a multiple of 4", two, desc(dtype=capi.TENSOR_F32, sh=130, sc=2400, sn=8192), None),
        ("F16 stride_c odd", two, desc(sc=1201), None),
        ("F32 stride_c off a multiple of 4", two, desc(dtype=capi.TENSOR_F32, sh=128, sc=2050, sn=8192), None),
        ("F16 stride_n odd", two, desc(sn=4097), None),
        ("F32 stride_n off a multiple of 4", two, desc(dtype=capi.TENSOR_F32, sh=128, sc=2048, sn=8194), None),
        ("NCHW stride_h one element below the row", two, desc(sh=62), None),
        ("NHWC stride_h one element below the row", two, desc(layout=capi.TENSOR_NHWC, sh=190), None),
        ("F32 stride_h one element below the row", two, desc(dtype=capi.TENSOR_F32, sh=124, sc=2048, sn=8192), None),
        ("stride_h negative", two, desc(sh=-72), None),
        ("NCHW stride_c one element below E", two, desc(sc=E - 2, sn=8192), None),
        ("NCHW stride_c one element below E, one frame", [frame], desc(sc=E - 2), None),
        ("NCHW stride_n one element below 2 stride_c + E", two, desc(sc=E, sn=3 * E - 2), None),
        ("NHWC stride_n one element below E", two, desc(layout=capi.TENSOR_NHWC, sh=200, sn=En - 2), None),
        ("stride_n negative", two, desc(sn=-4096), None),
    ]
    for what, frames, d, n in bad:
        assert call(frames, d, n) == M355_ERR_INVALID, what
    assert lib.m355_frames_export_tensor(ctx.h, None, 1, ctypes.byref(desc())) == M355_ERR_INVALID
    assert call([frame], None) == M355_ERR_INVALID
    assert lib.m355_frames_export_tensor(None, (ctypes.c_int * 1)(frame), 1, ctypes.byref(desc())) == M355_ERR_INVALID
    ctx.wait()
    assert np.all(ctx.device_read(buf, nbytes) == capi.DEVICE_FILL), "a rejected export wrote to its destination"
    # the limits themselves: strides exactly at the row, at E and at 2 stride_c + E (a dense tensor); 32 frames; the ratio limits; strides that one
    # frame or NHWC does not use may hold anything
    good = [
        ("dense NCHW", two, desc(sh=64, sc=16 * 64, sn=3 * 16 * 64)),
        ("NCHW at E", two, desc(sc=E, sn=3 * E)),
        ("dense NHWC", two, desc(layout=capi.TENSOR_NHWC, sh=192, sc=1, sn=16 * 192)),
        ("NHWC at E", two, desc(layout=capi.TENSOR_NHWC, sh=200, sc=-7, sn=En)),
        ("one frame, stride_n unused", [frame], desc(sn=-3)),
        ("32 times the same frame", [frame] * 32, desc(out=(8, 4), sh=16, sc=64, sn=192)),
        ("exactly 8x down", [mono], desc(out=(7, 40), rect=(0, 0, 56, 40), sc=4000)),
        ("exactly 8x up", [mono], desc(out=(64, 32), rect=(0, 0, 8, 4), sh=128, sc=4096)),
        ("the rectangle inside frames of different sizes", [frame, large], desc(rect=(0, 0, 64, 32))),
    ]
    for what, frames, d in good:
        assert call(frames, d) == 0, "%s: %s" % (what, ctx.L.error())
    ctx.wait()
    ctx.device_free(buf)
    for f in (frame, same, large, small, f422, depth8, depth12, depth9c, mono):
        ctx.frame_destroy(f)


def test_dense_tensor_has_no_gaps(ctx):
    """strides exactly at their lower bounds: every byte of the buffer is an element, the bytes in front of and behind the tensor are untouched"""
    rng = np.random.default_rng(8300)
    frame = ctx.frame_create(64, 32, 3, 10, 10)
    planes = [rng.integers(0, 1024, (32, 64)).astype(np.uint16) for _ in range(3)]
    ctx.frame_upload(frame, planes)
    from export_tensor_util import expected_ints, expected_tensor, imagenet
    scale, bias = imagenet(capi.RGB_U8)
    w, h, n, guard = 33, 9, 2, 64
    ints = [expected_ints(planes, (3, 10, 10), capi.RGB_U8, capi.MATRIX_BT709, 0, (w, h))] * n
    for layout, dtype, eb in ((capi.TENSOR_NCHW, capi.TENSOR_F16, 2), (capi.TENSOR_NHWC, capi.TENSOR_BF16, 2), (capi.TENSOR_NCHW, capi.TENSOR_F32, 4)):
        row = w * eb * (3 if layout == capi.TENSOR_NHWC else 1)
        sc = h * row if layout == capi.TENSOR_NCHW else 0
        sn = 3 * h * w * eb
        buf = ctx.device_alloc(2 * guard + n * sn)
        d = capi.TensorDesc(layout=layout, dtype=dtype, samples=capi.RGB_U8, matrix=capi.MATRIX_BT709, full_range=0, out_width=w, out_height=h,
                            stride_n=sn, stride_c=sc, stride_h=row)
        d.scale = (ctypes.c_float * 3)(*scale)
        d.bias = (ctypes.c_float * 3)(*bias)
        d.dst = buf + guard
        assert ctx.L.lib.m355_frames_export_tensor(ctx.h, (ctypes.c_int * n)(frame, frame), n, ctypes.byref(d)) == 0, ctx.L.error()
        raw = ctx.device_read(buf, 2 * guard + n * sn)
        ctx.device_free(buf)
        assert np.all(raw[:guard] == capi.DEVICE_FILL) and np.all(raw[-guard:] == capi.DEVICE_FILL)
        got = raw[guard:-guard].view(np.uint32 if eb == 4 else np.uint16)
        assert np.array_equal(got, expected_tensor(ints, layout, dtype, scale, bias).ravel()), (layout, dtype)
    ctx.frame_destroy(frame)


def test_tensor_gate_is_per_slice(ctx):
    check_gate(ctx)


@pytest.mark.parametrize("depth", [1, 3])
def test_tensor_export_behind_recycled_frames(ctx, depth):
    """(the interpreter runs every launch to its end at once: this walks the reader bookkeeping, the GPU tier is what can see a missing wait)"""
    check_hazard(ctx, depth)


def test_tensor_export_into_pinned_host_memory(ctx, oracle):
    check_pinned_host(ctx, Oracle(oracle))
