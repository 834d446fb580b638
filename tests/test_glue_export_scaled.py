"""m355_glue_export_image_scaled: decoded pictures leave the reference-API decoder (glue/_build/libde265.so) downscaled into DEVICE memory,
without a download.  CPU tier: the backend is the SIMT-interpreter build (M355_LIB), as in test_glue_export.py.  The first 8 output pictures of
girlshy.h265 are exported planar, samples as they are, picture k at the scale 1 << (k mod 3 + 1) — through the NULL rectangle (the conformance
window) where the window is a multiple of the scale on the chroma grid, through an explicit rectangle that is one where it is not —, picture 3
in addition semi-planar 8-bit; all must equal the numpy restatement (export_scaled_util.py) applied to the planes de265_get_image_plane returns.
The decoder's CPU pixel table is never called, and a run that only exports scaled pictures downloads nothing."""
import ctypes

import numpy as np

from export_scaled_util import assert_export, expected_export_scaled
from libde265_amd import capi
from test_emu_picture import emu_lib, EMU_SO  # noqa: F401  (fixture)
from test_glue_export import Exporter, bind, decode, host_planes
from test_glue_live import glue_lib


def bind_scaled(glue):
    vp, i = ctypes.c_void_p, ctypes.c_int
    glue.m355_glue_export_image_scaled.argtypes = [vp, i, i, ctypes.POINTER(i), i, ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_int64), vp]
    return bind(glue)


class ScaledExporter(Exporter):
    """Exporter.export through m355_glue_export_image_scaled at self.k"""

    def __init__(self, ex, k):
        self.glue, self.L, self.mctx, self.k = _Scaled(ex.glue, k), ex.L, ex.mctx, k


class _Scaled:
    """the glue library with m355_glue_export_image standing for the scaled call at one scale (what Exporter.export calls)"""

    def __init__(self, glue, k):
        self._glue, self._k = glue, k

    def m355_glue_export_image(self, img, layout, samples, r, dst, pitch, stream):
        return self._glue.m355_glue_export_image_scaled(img, layout, samples, r, self._k, dst, pitch, stream)


def scaled_rect(glue, img, k):
    """None where the image's window is a multiple of the scale on the 4:2:0 grid, else the largest such rectangle, off the origin where it fits"""
    w, h, m = glue.de265_get_image_width(img, 0), glue.de265_get_image_height(img, 0), 2 << k
    if w % m == 0 and h % m == 0:
        return None
    rw, rh = w // m * m, h // m * m
    return (2 if rw + 2 <= w else 0, 2 if rh + 2 <= h else 0, rw, rh)


def shapes_of(want):
    return [(p.shape[0], p.shape[1], p.dtype) for p in want]


def export_scaled(ex, img, host, layout, samples, k, what):
    rect = scaled_rect(ex.glue, img, k)
    want = expected_export_scaled(host, 1, 8, 8, layout, samples, k, rect)
    got, raws = ScaledExporter(ex, k).export(img, layout, samples, rect, shapes_of(want))
    assert_export(got, raws, want, what)
    return got, rect


def test_scaled_images_equal_the_scaled_host_planes(emu_lib, monkeypatch):  # noqa: F811
    monkeypatch.setenv("M355_LIB", EMU_SO)
    glue = bind_scaled(glue_lib())
    rects = []

    def check(ex, img, j):
        assert glue.de265_get_chroma_format(img) == 1 and glue.de265_get_bits_per_pixel(img, 0) == 8
        host = host_planes(glue, img)
        rects.append(export_scaled(ex, img, host, capi.EXPORT_PLANAR, capi.EXPORT_NATIVE, j % 3 + 1, "picture %d" % j)[1])
        if j == 3:
            export_scaled(ex, img, host, capi.EXPORT_SEMIPLANAR, capi.EXPORT_U8, j % 3 + 1, "picture %d, semi-planar" % j)

    n, _ = decode(glue, emu_lib, check, max_pictures=8)
    assert n == 8
    assert any(r is None for r in rects), "no picture went through the NULL rectangle"
    assert glue.m355_glue_cpu_pixel_calls() == 0, "the decoder called into its CPU pixel table"


def test_scaled_export_alone_downloads_nothing(emu_lib, monkeypatch):  # noqa: F811
    monkeypatch.setenv("M355_LIB", EMU_SO)
    glue = bind_scaled(glue_lib())
    sums = []

    def take(ex, img, j):
        k = j % 3 + 1
        rect = scaled_rect(glue, img, k)
        w, h = (glue.de265_get_image_width(img, 0), glue.de265_get_image_height(img, 0)) if rect is None else rect[2:]
        shapes = [(h >> k, w >> k, np.uint8), (h >> (k + 1), w >> (k + 1), np.uint8), (h >> (k + 1), w >> (k + 1), np.uint8)]
        got, _ = ScaledExporter(ex, k).export(img, capi.EXPORT_PLANAR, capi.EXPORT_NATIVE, rect, shapes)
        sums.append(int(got[0].sum()))

    n, downloads = decode(glue, emu_lib, take, max_pictures=8)
    assert n == 8 and downloads == 0, "a picture that was only exported was brought back to the host"
    assert len(set(sums)) > 1
    assert glue.m355_glue_cpu_pixel_calls() == 0
