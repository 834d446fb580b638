"""The four _filtered exports of the glue (glue/_build/libde265.so) with M355_FILTER_CUBIC: m355_glue_export_image_resized_filtered,
m355_glue_export_image_resized_rgb_filtered, m355_glue_export_images_tensor_filtered and m355_glue_export_images_tensor_rois_filtered.  CPU tier: the
backend is the SIMT-interpreter build (M355_LIB), as in test_glue_export_resized.py.  The pictures of a generated stream with a non-empty conformance
window (tests/test_streams.py G_CONFWIN, 4:2:0, 8 bits) are exported through the NULL rectangle (the window) and through an explicit rectangle; all
must equal the cubic restatement (export_cubic_util.py) of the planes de265_get_image_plane returns (the rectangle: of its samples as
m355_glue_export_image delivers them).  With M355_FILTER_TRIANGLE each _filtered call delivers what the plain call delivers; an unknown filter and a
ratio beyond 4x down are rejected and write nothing; the decoder's CPU pixel table is never called."""
import ctypes

import numpy as np

from export_cubic_util import CUBIC, expected_export_resized, expected_ints, expected_resized_rgb
from export_tensor_util import assert_tensor, expected_tensor, imagenet
from export_tensor_rois_util import MIRROR, reverse_columns
from export_util import M355_ERR_INVALID, assert_export
from libde265_amd import capi
from test_emu_picture import emu_lib, EMU_SO  # noqa: F401  (fixture)
from test_glue_export import Exporter, bind, decode, host_planes
from test_glue_export_resized import ResizedExporter, bind_resized
from test_glue_export_resized_rgb import ResizedRgbExporter, bind_resized_rgb
from test_glue_export_rgb import shapes_of
from test_glue_export_tensor import Tensor, bind_tensor, export_batch
from test_glue_export_tensor_rois import bind_rois, export_rois
from test_glue_live import glue_lib
from test_streams import G_CONFWIN, make_stream

RECT = (6, 2, 50, 22)
SIZES = [(96, 40), (320, 176), (64, 32)]      # of the window: down by a non-integer ratio, up, down by almost 4
TOO_SMALL = (32, 16)                           # more than 4x down, which the triangle takes
OUT = (96, 40)                                 # of the window: inside 4x down


def bind_filtered(glue):
    vp, i, f3, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_float), ctypes.c_int64
    pi = ctypes.POINTER(i)
    glue.m355_glue_export_image_resized_filtered.argtypes = [vp, i, i, pi, pi, ctypes.POINTER(vp), ctypes.POINTER(i64), i, vp]
    glue.m355_glue_export_image_resized_rgb_filtered.argtypes = [vp, i, i, i, i, pi, pi, ctypes.POINTER(vp), ctypes.POINTER(i64), i, vp]
    glue.m355_glue_export_images_tensor_filtered.argtypes = [ctypes.POINTER(vp), i, i, i, i, i, i, pi, pi, f3, f3, vp, i64, i64, i64, i, vp]
    glue.m355_glue_export_images_tensor_rois_filtered.argtypes = [ctypes.POINTER(vp), ctypes.POINTER(i * 5), i, i, i, i, i, i, pi, f3, f3, vp, i64, i64, i64, i, vp]
    bind_resized(glue)
    bind_resized_rgb(glue)
    bind_tensor(glue)
    return bind_rois(glue)


class _Filtered:
    """the glue library with m355_glue_export_image standing for one of the two single-picture _filtered calls (what Exporter.export calls)"""

    def __init__(self, glue, out_size, filter, rgb=None):
        self._glue, self._out, self._filter, self._rgb = glue, (ctypes.c_int * 2)(*out_size), filter, rgb

    def m355_glue_export_image(self, img, layout, samples, r, dst, pitch, stream):
        if self._rgb is None:
            return self._glue.m355_glue_export_image_resized_filtered(img, layout, samples, r, self._out, dst, pitch, self._filter, stream)
        return self._glue.m355_glue_export_image_resized_rgb_filtered(img, layout, samples, self._rgb[0], self._rgb[1], r, self._out, dst, pitch, self._filter, stream)


class FilteredExporter(Exporter):
    def __init__(self, ex, out_size, filter, rgb=None):
        self.glue, self.L, self.mctx = _Filtered(ex.glue, out_size, filter, rgb), ex.L, ex.mctx


def stream(tmp_path):
    return make_stream(tmp_path, 256, 128, 8, 1, 1, 3, 118, 10, 1, 1, 0, 1, 1, G_CONFWIN)


def rect_planes(ex, img, rect):
    """an explicit rectangle counts from the coded picture's corner, not the window's: its samples come from the plain export of the same rectangle"""
    shapes = [(rect[3], rect[2], np.uint8)] + [(rect[3] // 2, rect[2] // 2, np.uint8)] * 2
    return ex.export(img, capi.EXPORT_PLANAR, capi.EXPORT_NATIVE, rect, shapes)[0]


def rejected(ex, call, nbytes):
    """call(dst pointer) must return M355_ERR_INVALID and leave the buffer as it was filled"""
    p = ex.L.m355_device_alloc(ex.mctx, nbytes)
    fill = np.full(nbytes, capi.DEVICE_FILL, np.uint8)
    assert p and ex.L.m355_device_write(ex.mctx, p, fill.ctypes.data, nbytes) == 0
    for c in call if isinstance(call, (list, tuple)) else [call]:
        assert c(p) == M355_ERR_INVALID
    back = np.zeros(nbytes, np.uint8)
    assert ex.L.m355_device_read(ex.mctx, p, back.ctypes.data, nbytes) == 0
    ex.L.m355_device_free(ex.mctx, p)
    assert np.all(back == capi.DEVICE_FILL), "a rejected export wrote to its destination"


def test_cubic_resized_images_equal_the_resized_host_planes(emu_lib, tmp_path, monkeypatch):  # noqa: F811
    monkeypatch.setenv("M355_LIB", EMU_SO)
    glue = bind_filtered(glue_lib())

    def check(ex, img, j):
        assert glue.de265_get_chroma_format(img) == 1 and glue.de265_get_bits_per_pixel(img, 0) == 8
        assert (glue.de265_get_image_width(img, 0), glue.de265_get_image_height(img, 0)) != (256, 128), "the stream has no conformance window"
        host = host_planes(glue, img)
        want = expected_export_resized(host, 1, 8, 8, capi.EXPORT_PLANAR, capi.EXPORT_NATIVE, SIZES[j])
        shapes = [(p.shape[0], p.shape[1], p.dtype) for p in want]
        got, raws = FilteredExporter(ex, SIZES[j], CUBIC).export(img, capi.EXPORT_PLANAR, capi.EXPORT_NATIVE, None, shapes)
        assert_export(got, raws, want, "picture %d" % j)
        # filter 0 is the plain call
        a = FilteredExporter(ex, SIZES[j], capi.FILTER_TRIANGLE).export(img, capi.EXPORT_PLANAR, capi.EXPORT_NATIVE, None, shapes)[1]
        b = ResizedExporter(ex, SIZES[j]).export(img, capi.EXPORT_PLANAR, capi.EXPORT_NATIVE, None, shapes)[1]
        assert all(np.array_equal(x, y) for x, y in zip(a, b)) and not all(np.array_equal(x, y) for x, y in zip(a, raws))
        if j == 1:
            want = expected_export_resized(rect_planes(ex, img, RECT), 1, 8, 8, capi.EXPORT_SEMIPLANAR, capi.EXPORT_U8, (36, 14))
            got, raws = FilteredExporter(ex, (36, 14), CUBIC).export(img, capi.EXPORT_SEMIPLANAR, capi.EXPORT_U8, RECT, [(p.shape[0], p.shape[1], p.dtype) for p in want])
            assert_export(got, raws, want, "picture %d, rectangle" % j)
        if j == 0:
            ow, oh = TOO_SMALL
            out, pitch = (ctypes.c_int * 2)(ow, oh), (ctypes.c_int64 * 3)(ow, ow // 2, ow // 2)

            def call(filter, size=out):
                def go(p):
                    dst = (ctypes.c_void_p * 3)(p, p + ow * oh, p + 2 * ow * oh)
                    return glue.m355_glue_export_image_resized_filtered(img, capi.EXPORT_PLANAR, capi.EXPORT_NATIVE, None, size, dst, pitch, filter, None)
                return go
            rejected(ex, [call(CUBIC), call(2), call(-1), call(CUBIC, None)], 3 * ow * oh)

    n, _ = decode(glue, emu_lib, check, data=stream(tmp_path))
    assert n == 3
    assert glue.m355_glue_cpu_pixel_calls() == 0, "the decoder called into its CPU pixel table"


def test_cubic_resized_rgb_images_equal_the_composed_host_planes(emu_lib, tmp_path, monkeypatch):  # noqa: F811
    monkeypatch.setenv("M355_LIB", EMU_SO)
    glue = bind_filtered(glue_lib())

    def check(ex, img, j):
        host = host_planes(glue, img)
        for layout, samples, matrix, full in ((capi.RGB_PACKED, capi.RGB_U8, capi.MATRIX_BT601, 1), (capi.RGB_PLANAR, capi.RGB_U16, capi.MATRIX_BT709, 0)):
            want = expected_resized_rgb(host, 1, 8, 8, layout, samples, matrix, full, SIZES[j])
            got, raws = FilteredExporter(ex, SIZES[j], CUBIC, (matrix, full)).export(img, layout, samples, None, shapes_of(want))
            assert_export(got, raws, want, "picture %d, layout %d" % (j, layout))
        a = FilteredExporter(ex, SIZES[j], capi.FILTER_TRIANGLE, (capi.MATRIX_BT709, 0)).export(img, capi.RGB_PLANAR, capi.RGB_U16, None, shapes_of(want))[1]
        b = ResizedRgbExporter(ex, capi.MATRIX_BT709, 0, SIZES[j]).export(img, capi.RGB_PLANAR, capi.RGB_U16, None, shapes_of(want))[1]
        assert all(np.array_equal(x, y) for x, y in zip(a, b)) and not all(np.array_equal(x, y) for x, y in zip(a, raws))
        if j == 1:
            want = expected_resized_rgb(rect_planes(ex, img, RECT), 1, 8, 8, capi.RGB_PACKED, capi.RGB_U16, capi.MATRIX_BT2020, 0, (64, 30))
            got, raws = FilteredExporter(ex, (64, 30), CUBIC, (capi.MATRIX_BT2020, 0)).export(img, capi.RGB_PACKED, capi.RGB_U16, RECT, shapes_of(want))
            assert_export(got, raws, want, "picture %d, rectangle, up" % j)
        if j == 0:
            ow, oh = TOO_SMALL
            out, pitch = (ctypes.c_int * 2)(ow, oh), (ctypes.c_int64 * 3)(3 * ow, 0, 0)

            def call(filter):
                def go(p):
                    dst = (ctypes.c_void_p * 3)(p, None, None)
                    return glue.m355_glue_export_image_resized_rgb_filtered(img, capi.RGB_PACKED, capi.RGB_U8, capi.MATRIX_BT709, 0, None, out, dst, pitch, filter, None)
                return go
            rejected(ex, [call(CUBIC), call(2)], 3 * ow * oh)

    n, _ = decode(glue, emu_lib, check, data=stream(tmp_path))
    assert n == 3
    assert glue.m355_glue_cpu_pixel_calls() == 0, "the decoder called into its CPU pixel table"


def filtered_batch(glue, t, imgs, dtype, samples, matrix, full, rect, scale, bias, filter):
    arr = (ctypes.c_void_p * len(imgs))(*imgs)
    r = (ctypes.c_int * 4)(*rect) if rect is not None else None
    return glue.m355_glue_export_images_tensor_filtered(arr, len(imgs), t.layout, dtype, samples, matrix, full, r, (ctypes.c_int * 2)(t.w, t.h),
                                                        (ctypes.c_float * 3)(*scale), (ctypes.c_float * 3)(*bias), t.p, t.sn, t.sc, t.sh, filter, None)


def filtered_rois(glue, t, imgs, rois, dtype, samples, matrix, full, scale, bias, filter):
    arr = (ctypes.c_void_p * len(imgs))(*imgs)
    ra = ((ctypes.c_int * 5) * len(rois))(*[(ctypes.c_int * 5)(*r) for r in rois])
    return glue.m355_glue_export_images_tensor_rois_filtered(arr, ra, len(imgs), t.layout, dtype, samples, matrix, full, (ctypes.c_int * 2)(t.w, t.h),
                                                             (ctypes.c_float * 3)(*scale), (ctypes.c_float * 3)(*bias), t.p, t.sn, t.sc, t.sh, filter, None)


def held_pictures(glue, emu, tmp_path, check):
    """the stream's three pictures, held until the last one has come out (as in test_glue_export_tensor.py), then check(ex, imgs)"""
    imgs = []

    def take(ex, img, j):
        imgs.append(img)
        if j == 2:
            check(ex, imgs)

    n, _ = decode(glue, emu, take, data=stream(tmp_path))
    assert n == 3
    assert glue.m355_glue_cpu_pixel_calls() == 0, "the decoder called into its CPU pixel table"


def test_cubic_images_of_a_stream_as_one_batch(emu_lib, tmp_path, monkeypatch):  # noqa: F811
    monkeypatch.setenv("M355_LIB", EMU_SO)
    glue = bind_filtered(glue_lib())

    def check(ex, imgs):
        scale, bias = imagenet(capi.RGB_U8)
        args = (capi.RGB_U8, capi.MATRIX_BT709, 0)
        for layout, dtype, rect in ((capi.TENSOR_NCHW, capi.TENSOR_F32, None), (capi.TENSOR_NHWC, capi.TENSOR_F16, RECT)):
            t = Tensor(ex, 3, layout, dtype, OUT)
            assert filtered_batch(glue, t, imgs, dtype, *args, rect, scale, bias, CUBIC) == 0
            planes = [host_planes(glue, img) if rect is None else rect_planes(ex, img, rect) for img in imgs]
            ints = [expected_ints(p, (1, 8, 8), *args, OUT) for p in planes]
            assert_tensor(t.finish(), expected_tensor(ints, layout, dtype, scale, bias), "cubic batch, layout %d" % layout)
        a, b = Tensor(ex, 3, capi.TENSOR_NCHW, capi.TENSOR_F32, OUT), Tensor(ex, 3, capi.TENSOR_NCHW, capi.TENSOR_F32, OUT)
        assert filtered_batch(glue, a, imgs, capi.TENSOR_F32, *args, None, scale, bias, capi.FILTER_TRIANGLE) == 0
        assert export_batch(glue, b, imgs, capi.TENSOR_F32, *args, None, scale, bias) == 0
        assert np.array_equal(a.finish()[1], b.finish()[1]), "filter 0 is not the plain call"
        bad = Tensor(ex, 3, capi.TENSOR_NCHW, capi.TENSOR_F32, TOO_SMALL)
        assert filtered_batch(glue, bad, imgs, capi.TENSOR_F32, *args, None, scale, bias, CUBIC) == M355_ERR_INVALID
        assert filtered_batch(glue, bad, imgs, capi.TENSOR_F32, *args, None, scale, bias, 2) == M355_ERR_INVALID
        assert np.all(bad.finish()[1] == capi.DEVICE_FILL), "a rejected export wrote to its destination"

    held_pictures(glue, emu_lib, tmp_path, check)


def test_cubic_regions_of_the_images_of_a_stream_as_one_batch(emu_lib, tmp_path, monkeypatch):  # noqa: F811
    monkeypatch.setenv("M355_LIB", EMU_SO)
    glue = bind_filtered(glue_lib())

    def check(ex, imgs):
        scale, bias = imagenet(capi.RGB_U16)
        args = (capi.RGB_U16, capi.MATRIX_BT601, 1)
        order = [imgs[2], imgs[1], imgs[1], imgs[0]]
        rois = [(100, 60, 40, 30, 0), (0, 0, 96, 40, 0), (0, 0, 96, 40, MIRROR), (0, 0, 0, 0, 0)]      # (the last: that picture's window)
        layout, dtype = capi.TENSOR_NHWC, capi.TENSOR_F32
        t = Tensor(ex, 4, layout, dtype, OUT)
        assert filtered_rois(glue, t, order, rois, dtype, *args, scale, bias, CUBIC) == 0
        want = []
        for img, r in zip(order, rois):
            planes = rect_planes(ex, img, r[:4]) if any(r[:4]) else host_planes(glue, img)
            w = expected_tensor([expected_ints(planes, (1, 8, 8), *args, OUT)], layout, dtype, scale, bias)[0]
            want.append(reverse_columns(w, layout) if r[4] else w)
        got = t.finish()
        assert_tensor(got, np.stack(want), "four cubic regions of three pictures")
        assert not np.array_equal(got[0][1], got[0][2])
        a, b = Tensor(ex, 4, layout, dtype, OUT), Tensor(ex, 4, layout, dtype, OUT)
        assert filtered_rois(glue, a, order, rois, dtype, *args, scale, bias, capi.FILTER_TRIANGLE) == 0
        assert export_rois(glue, b, order, rois, dtype, *args, scale, bias) == 0
        assert np.array_equal(a.finish()[1], b.finish()[1]), "filter 0 is not the plain call"
        # the cubic limit per entry: 40 rows do not go to 8 (the triangle takes them); an unknown filter
        bad = Tensor(ex, 4, layout, dtype, (24, 8))
        assert filtered_rois(glue, bad, order, rois[:1] + [(0, 0, 96, 32, 0), (0, 0, 96, 40, 0), (0, 0, 96, 32, 0)], dtype, *args, scale, bias, CUBIC) == M355_ERR_INVALID
        assert filtered_rois(glue, bad, order, rois, dtype, *args, scale, bias, 7) == M355_ERR_INVALID
        assert np.all(bad.finish()[1] == capi.DEVICE_FILL), "a rejected export wrote to its destination"

    held_pictures(glue, emu_lib, tmp_path, check)
