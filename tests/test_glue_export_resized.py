"""m355_glue_export_image_resized: decoded pictures leave the reference-API decoder (glue/_build/libde265.so) resized into DEVICE memory, without a
download.  CPU tier: the backend is the SIMT-interpreter build (M355_LIB), as in test_glue_export.py.  The pictures of a generated stream with a
non-empty conformance window (tests/test_streams.py G_CONFWIN, 4:2:0) are exported planar, samples as they are, through the NULL rectangle (the
window) to a size of their own — down by a non-integer ratio, up, down by almost 8 —, one of them in addition through an explicit rectangle as
semi-planar 8-bit; all must equal the restatement (export_resized_util.py) applied to the planes de265_get_image_plane returns (the rectangle: to
its samples as m355_glue_export_image delivers them).  The decoder's CPU pixel table is never called, and a run that only exports resized pictures
downloads nothing."""
import ctypes

import numpy as np

from export_resized_util import assert_export, expected_export_resized
from libde265_amd import capi
from test_emu_picture import emu_lib, EMU_SO  # noqa: F401  (fixture)
from test_glue_export import Exporter, bind, decode, host_planes
from test_glue_live import glue_lib
from test_streams import G_CONFWIN, make_stream

RECT = (6, 2, 50, 22)
SIZES = [(96, 40), (320, 176), (32, 16)]


def bind_resized(glue):
    vp, i = ctypes.c_void_p, ctypes.c_int
    glue.m355_glue_export_image_resized.argtypes = [vp, i, i, ctypes.POINTER(i), ctypes.POINTER(i), ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_int64), vp]
    return bind(glue)


class _Resized:
    """the glue library with m355_glue_export_image standing for the resized call at one output size (what Exporter.export calls)"""

    def __init__(self, glue, out_size):
        self._glue, self._out = glue, (ctypes.c_int * 2)(*out_size)

    def m355_glue_export_image(self, img, layout, samples, r, dst, pitch, stream):
        return self._glue.m355_glue_export_image_resized(img, layout, samples, r, self._out, dst, pitch, stream)


class ResizedExporter(Exporter):
    """Exporter.export through m355_glue_export_image_resized to out_size"""

    def __init__(self, ex, out_size):
        self.glue, self.L, self.mctx = _Resized(ex.glue, out_size), ex.L, ex.mctx


def export_resized(ex, img, host, layout, samples, out_size, rect, what):
    want = expected_export_resized(host, 1, 8, 8, layout, samples, out_size, rect)
    got, raws = ResizedExporter(ex, out_size).export(img, layout, samples, rect, [(p.shape[0], p.shape[1], p.dtype) for p in want])
    assert_export(got, raws, want, what)
    return got


def stream(tmp_path):
    return make_stream(tmp_path, 256, 128, 8, 1, 1, 3, 116, 10, 1, 1, 0, 1, 1, G_CONFWIN)


def test_resized_images_equal_the_resized_host_planes(emu_lib, tmp_path, monkeypatch):  # noqa: F811
    monkeypatch.setenv("M355_LIB", EMU_SO)
    glue = bind_resized(glue_lib())

    def check(ex, img, j):
        assert glue.de265_get_chroma_format(img) == 1 and glue.de265_get_bits_per_pixel(img, 0) == 8
        assert (glue.de265_get_image_width(img, 0), glue.de265_get_image_height(img, 0)) != (256, 128), "the stream has no conformance window"
        host = host_planes(glue, img)
        export_resized(ex, img, host, capi.EXPORT_PLANAR, capi.EXPORT_NATIVE, SIZES[j], None, "picture %d" % j)
        if j == 1:
            # an explicit rectangle counts from the coded picture's corner, not the window's: its samples come from the plain export of the same rectangle
            shapes = [(RECT[3], RECT[2], np.uint8)] + [(RECT[3] // 2, RECT[2] // 2, np.uint8)] * 2
            inside, _ = ex.export(img, capi.EXPORT_PLANAR, capi.EXPORT_NATIVE, RECT, shapes)
            want = expected_export_resized(inside, 1, 8, 8, capi.EXPORT_SEMIPLANAR, capi.EXPORT_U8, (36, 14))
            got, raws = ResizedExporter(ex, (36, 14)).export(img, capi.EXPORT_SEMIPLANAR, capi.EXPORT_U8, RECT, [(p.shape[0], p.shape[1], p.dtype) for p in want])
            assert_export(got, raws, want, "picture %d, rectangle" % j)

    n, _ = decode(glue, emu_lib, check, data=stream(tmp_path))
    assert n == 3
    assert glue.m355_glue_cpu_pixel_calls() == 0, "the decoder called into its CPU pixel table"


def test_resized_export_alone_downloads_nothing(emu_lib, tmp_path, monkeypatch):  # noqa: F811
    monkeypatch.setenv("M355_LIB", EMU_SO)
    glue = bind_resized(glue_lib())
    sums = []

    def take(ex, img, j):
        ow, oh = SIZES[j]
        shapes = [(oh, ow, np.uint8), (oh // 2, ow // 2, np.uint8), (oh // 2, ow // 2, np.uint8)]
        got, _ = ResizedExporter(ex, SIZES[j]).export(img, capi.EXPORT_PLANAR, capi.EXPORT_NATIVE, None, shapes)
        sums.append(int(got[0].sum()))

    n, downloads = decode(glue, emu_lib, take, data=stream(tmp_path))
    assert n == 3 and downloads == 0, "a picture that was only exported was brought back to the host"
    assert len(set(sums)) > 1
    assert glue.m355_glue_cpu_pixel_calls() == 0
