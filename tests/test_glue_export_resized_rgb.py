"""m355_glue_export_image_resized_rgb: decoded pictures leave the reference-API decoder (glue/_build/libde265.so) resized and as R'G'B' in DEVICE
memory, without a download.  CPU tier: the backend is the SIMT-interpreter build (M355_LIB), as in test_glue_export.py.  The pictures of a generated
stream with a non-empty conformance window (tests/test_streams.py G_CONFWIN, 4:2:0, 8 bits) are exported through the NULL rectangle (the window) to a
size of their own — down by a non-integer ratio, up, down by almost 8 —, with an explicit matrix and range and with -1 / -1 (what the stream signals,
through the mapping of m355_glue_export_image_rgb); one of them in addition through an explicit rectangle.  All must equal the composed restatement
(export_resized_rgb_util.py) of the planes de265_get_image_plane returns (the rectangle: of its samples as m355_glue_export_image delivers them).
A matrix outside M355_MATRIX_* is rejected and writes nothing, the decoder's CPU pixel table is never called, and a run that only takes such pictures
downloads nothing."""
import ctypes

import numpy as np

from export_resized_rgb_util import M355_ERR_INVALID, assert_export, expected_resized_rgb
from libde265_amd import capi
from test_emu_picture import emu_lib, EMU_SO  # noqa: F401  (fixture)
from test_glue_export import Exporter, bind, decode, host_planes
from test_glue_export_rgb import MATRIX_OF, shapes_of
from test_glue_live import glue_lib
from test_streams import G_CONFWIN, make_stream

RECT = (6, 2, 50, 22)
SIZES = [(96, 40), (320, 176), (32, 16)]


def bind_resized_rgb(glue):
    vp, i = ctypes.c_void_p, ctypes.c_int
    glue.m355_glue_export_image_resized_rgb.argtypes = [vp, i, i, i, i, ctypes.POINTER(i), ctypes.POINTER(i), ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_int64), vp]
    for f in (glue.de265_get_image_matrix_coefficients, glue.de265_get_image_full_range_flag):
        f.argtypes, f.restype = [vp], i
    return bind(glue)


class _ResizedRgb:
    """the glue library with m355_glue_export_image standing for the new call with one matrix, range and output size (what Exporter.export calls)"""

    def __init__(self, glue, matrix, full, out_size):
        self._glue, self._matrix, self._full, self._out = glue, matrix, full, (ctypes.c_int * 2)(*out_size)

    def m355_glue_export_image(self, img, layout, samples, r, dst, pitch, stream):
        return self._glue.m355_glue_export_image_resized_rgb(img, layout, samples, self._matrix, self._full, r, self._out, dst, pitch, stream)


class ResizedRgbExporter(Exporter):
    """Exporter.export through m355_glue_export_image_resized_rgb"""

    def __init__(self, ex, matrix, full, out_size):
        self.glue, self.L, self.mctx = _ResizedRgb(ex.glue, matrix, full, out_size), ex.L, ex.mctx


def export_resized_rgb(ex, glue, img, planes, layout, samples, matrix, full, out_size, rect, what):
    """one picture through the glue with (matrix, full) as given — -1 included — against the composed restatement of `planes` (the samples of the
    rectangle) with what they stand for"""
    m = MATRIX_OF[glue.de265_get_image_matrix_coefficients(img)] if matrix == -1 else matrix
    r = (1 if glue.de265_get_image_full_range_flag(img) else 0) if full == -1 else full
    want = expected_resized_rgb(planes, 1, 8, 8, layout, samples, m, r, out_size)
    got, raws = ResizedRgbExporter(ex, matrix, full, out_size).export(img, layout, samples, rect, shapes_of(want))
    assert_export(got, raws, want, what)
    return got


def stream(tmp_path):
    return make_stream(tmp_path, 256, 128, 8, 1, 1, 3, 117, 10, 1, 1, 0, 1, 1, G_CONFWIN)


def test_resized_rgb_images_equal_the_composed_host_planes(emu_lib, tmp_path, monkeypatch):  # noqa: F811
    monkeypatch.setenv("M355_LIB", EMU_SO)
    glue = bind_resized_rgb(glue_lib())

    def check(ex, img, j):
        assert glue.de265_get_chroma_format(img) == 1 and glue.de265_get_bits_per_pixel(img, 0) == 8
        assert (glue.de265_get_image_width(img, 0), glue.de265_get_image_height(img, 0)) != (256, 128), "the stream has no conformance window"
        host = host_planes(glue, img)               # (the window's samples: what the NULL rectangle resizes)
        export_resized_rgb(ex, glue, img, host, capi.RGB_PACKED, capi.RGB_U8, capi.MATRIX_BT601, 1, SIZES[j], None, "picture %d, BT.601 full" % j)
        export_resized_rgb(ex, glue, img, host, capi.RGB_PLANAR, capi.RGB_U16, -1, -1, SIZES[j], None, "picture %d, as signalled" % j)
        if j == 1:
            # an explicit rectangle counts from the coded picture's corner, not the window's: its samples come from the plain export of the same rectangle
            shapes = [(RECT[3], RECT[2], np.uint8)] + [(RECT[3] // 2, RECT[2] // 2, np.uint8)] * 2
            inside, _ = ex.export(img, capi.EXPORT_PLANAR, capi.EXPORT_NATIVE, RECT, shapes)
            export_resized_rgb(ex, glue, img, inside, capi.RGB_PACKED, capi.RGB_U16, -1, 0, (36, 14), RECT, "picture %d, rectangle" % j)
            export_resized_rgb(ex, glue, img, inside, capi.RGB_PLANAR, capi.RGB_U8, capi.MATRIX_BT2020, -1, (64, 30), RECT, "picture %d, rectangle, up" % j)
        if j == 0:
            # a value outside M355_MATRIX_* passed explicitly is rejected, and so is full_range 2; nothing is written
            ow, oh = SIZES[0]
            dst, pitch, out = (ctypes.c_void_p * 3)(), (ctypes.c_int64 * 3)(), (ctypes.c_int * 2)(ow, oh)
            nbytes = oh * 3 * ow
            dst[0] = ex.L.m355_device_alloc(ex.mctx, nbytes)
            fill = np.full(nbytes, capi.DEVICE_FILL, np.uint8)
            assert dst[0] and ex.L.m355_device_write(ex.mctx, dst[0], fill.ctypes.data, nbytes) == 0
            pitch[0] = 3 * ow
            for bad in (3, 9, -2):
                assert glue.m355_glue_export_image_resized_rgb(img, capi.RGB_PACKED, capi.RGB_U8, bad, 0, None, out, dst, pitch, None) == M355_ERR_INVALID, bad
            assert glue.m355_glue_export_image_resized_rgb(img, capi.RGB_PACKED, capi.RGB_U8, capi.MATRIX_BT709, 2, None, out, dst, pitch, None) == M355_ERR_INVALID
            assert glue.m355_glue_export_image_resized_rgb(img, capi.RGB_PACKED, capi.RGB_U8, capi.MATRIX_BT709, 0, None, None, dst, pitch, None) == M355_ERR_INVALID
            back = np.zeros(nbytes, np.uint8)
            assert ex.L.m355_device_read(ex.mctx, dst[0], back.ctypes.data, nbytes) == 0
            ex.L.m355_device_free(ex.mctx, dst[0])
            assert np.all(back == capi.DEVICE_FILL), "a rejected export wrote to its destination"

    n, _ = decode(glue, emu_lib, check, data=stream(tmp_path))
    assert n == 3
    assert glue.m355_glue_cpu_pixel_calls() == 0, "the decoder called into its CPU pixel table"


def test_resized_rgb_export_alone_downloads_nothing(emu_lib, tmp_path, monkeypatch):  # noqa: F811
    monkeypatch.setenv("M355_LIB", EMU_SO)
    glue = bind_resized_rgb(glue_lib())
    sums = []

    def take(ex, img, j):
        ow, oh = SIZES[j]
        layout = capi.RGB_PACKED if j % 2 else capi.RGB_PLANAR
        shapes = [(oh, 3 * ow, np.uint8)] if j % 2 else [(oh, ow, np.uint8)] * 3
        got, _ = ResizedRgbExporter(ex, -1, -1, SIZES[j]).export(img, layout, capi.RGB_U8, None, shapes)
        sums.append(int(got[0].sum()))

    n, downloads = decode(glue, emu_lib, take, data=stream(tmp_path))
    assert n == 3 and downloads == 0, "a picture that was only exported was brought back to the host"
    assert len(set(sums)) > 1
    assert glue.m355_glue_cpu_pixel_calls() == 0
