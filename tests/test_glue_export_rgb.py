"""m355_glue_export_image_rgb: decoded pictures leave the reference-API decoder (glue/_build/libde265.so) as R'G'B' in DEVICE memory, without a
download.  CPU tier: the backend is the SIMT-interpreter build (M355_LIB), as in test_glue_export.py.  Generated streams (8-bit 4:2:0, 10-bit 4:4:4;
no conformance window, so the planes de265_get_image_plane returns are the frame the chroma filter clamps to) are decoded through the glue and every
picture is taken with an explicit matrix and range and with -1 / -1 — what the stream signals, through the documented mapping —, whole and as a
rectangle; all must equal the Python-integer restatement (export_rgb_util.py) applied to the host planes.  A matrix value outside M355_MATRIX_* is
rejected and writes nothing, the decoder's CPU pixel table is never called, and a run that only takes RGB pictures downloads nothing."""
import ctypes

import numpy as np
import pytest

from export_rgb_util import M355_ERR_INVALID, assert_export, expected_rgb
from libde265_amd import capi
from test_emu_picture import emu_lib, EMU_SO  # noqa: F401  (fixture)
from test_glue_export import Exporter, bind, decode, host_planes
from test_glue_live import glue_lib
from test_streams import make_stream

RECT = (6, 2, 50, 22)
# matrix_coeffs of the VUI (de265_get_image_matrix_coefficients) -> M355_MATRIX_*; 2 = unspecified
MATRIX_OF = {1: capi.MATRIX_BT709, 2: capi.MATRIX_BT709, 5: capi.MATRIX_BT601, 6: capi.MATRIX_BT601, 9: capi.MATRIX_BT2020}


def bind_rgb(glue):
    vp, i = ctypes.c_void_p, ctypes.c_int
    glue.m355_glue_export_image_rgb.argtypes = [vp, i, i, i, i, ctypes.POINTER(i), ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_int64), vp]
    for f in (glue.de265_get_image_matrix_coefficients, glue.de265_get_image_full_range_flag):
        f.argtypes, f.restype = [vp], i
    return bind(glue)


class _Rgb:
    """the glue library with m355_glue_export_image standing for the RGB call with one matrix and range (what Exporter.export calls)"""

    def __init__(self, glue, matrix, full):
        self._glue, self._matrix, self._full = glue, matrix, full

    def m355_glue_export_image(self, img, layout, samples, r, dst, pitch, stream):
        return self._glue.m355_glue_export_image_rgb(img, layout, samples, self._matrix, self._full, r, dst, pitch, stream)


class RgbExporter(Exporter):
    """Exporter.export through m355_glue_export_image_rgb"""

    def __init__(self, ex, matrix, full):
        self.glue, self.L, self.mctx = _Rgb(ex.glue, matrix, full), ex.L, ex.mctx


def shapes_of(want):
    return [(p.shape[0], p.shape[1], p.dtype) for p in want]


def export_rgb(ex, glue, img, host, layout, samples, matrix, full, rect, what):
    """one picture through the glue with (matrix, full) as given — -1 included — against the restatement with what they stand for"""
    cf, bdl = glue.de265_get_chroma_format(img), glue.de265_get_bits_per_pixel(img, 0)
    bdc = glue.de265_get_bits_per_pixel(img, 1) if cf else bdl
    m = MATRIX_OF[glue.de265_get_image_matrix_coefficients(img)] if matrix == -1 else matrix
    r = (1 if glue.de265_get_image_full_range_flag(img) else 0) if full == -1 else full
    want = expected_rgb(host, cf, bdl, bdc, layout, samples, m, r, rect)
    got, raws = RgbExporter(ex, matrix, full).export(img, layout, samples, rect, shapes_of(want))
    assert_export(got, raws, want, what)
    return got


# (coded width, height, bit depth, seed, chroma format of oracle/ref_streamgen.cc)
@pytest.mark.parametrize("w,h,bd,seed,chroma", [(256, 128, 8, 131, 1), (192, 128, 10, 132, 3)])
def test_rgb_images_equal_the_converted_host_planes(emu_lib, tmp_path, monkeypatch, w, h, bd, seed, chroma):  # noqa: F811
    monkeypatch.setenv("M355_LIB", EMU_SO)
    glue = bind_rgb(glue_lib())
    frames = 3
    data = make_stream(tmp_path, w, h, bd, 1, 1, frames, seed, 10, 1, 1, 0, chroma)

    def check(ex, img, j):
        # exported first: at this point nothing has asked for the picture's samples
        shape = [(h, 3 * w, np.uint8)]
        first, raws = RgbExporter(ex, capi.MATRIX_BT601, 1).export(img, capi.RGB_PACKED, capi.RGB_U8, None, shape)
        host = host_planes(glue, img)
        assert host[0].shape == (h, w), "the stream has a conformance window: the host planes are not the frame"
        assert_export(first, raws, expected_rgb(host, chroma, bd, bd, capi.RGB_PACKED, capi.RGB_U8, capi.MATRIX_BT601, 1), "picture %d, BT.601 full" % j)
        export_rgb(ex, glue, img, host, capi.RGB_PLANAR, capi.RGB_U16, -1, -1, None, "picture %d, as signalled" % j)
        export_rgb(ex, glue, img, host, capi.RGB_PACKED, capi.RGB_U16, -1, 1, RECT, "picture %d, signalled matrix, rectangle" % j)
        export_rgb(ex, glue, img, host, capi.RGB_PLANAR, capi.RGB_U8, capi.MATRIX_BT2020, -1, RECT, "picture %d, BT.2020, rectangle" % j)
        if j == 0:
            # a value outside M355_MATRIX_* passed explicitly is rejected; nothing is written
            dst, pitch = (ctypes.c_void_p * 3)(), (ctypes.c_int64 * 3)()
            nbytes = h * 3 * w
            dst[0] = ex.L.m355_device_alloc(ex.mctx, nbytes)
            fill = np.full(nbytes, capi.DEVICE_FILL, np.uint8)
            assert dst[0] and ex.L.m355_device_write(ex.mctx, dst[0], fill.ctypes.data, nbytes) == 0
            pitch[0] = 3 * w
            for bad in (3, 9, -2):
                assert glue.m355_glue_export_image_rgb(img, capi.RGB_PACKED, capi.RGB_U8, bad, 0, None, dst, pitch, None) == M355_ERR_INVALID, bad
            assert glue.m355_glue_export_image_rgb(img, capi.RGB_PACKED, capi.RGB_U8, capi.MATRIX_BT709, 2, None, dst, pitch, None) == M355_ERR_INVALID
            back = np.zeros(nbytes, np.uint8)
            assert ex.L.m355_device_read(ex.mctx, dst[0], back.ctypes.data, nbytes) == 0
            ex.L.m355_device_free(ex.mctx, dst[0])
            assert np.all(back == capi.DEVICE_FILL), "a rejected RGB export wrote to its destination"

    n, _ = decode(glue, emu_lib, check, data=data)
    assert n == frames
    assert glue.m355_glue_cpu_pixel_calls() == 0, "the decoder called into its CPU pixel table"


def test_rgb_export_alone_downloads_nothing(emu_lib, monkeypatch):  # noqa: F811
    monkeypatch.setenv("M355_LIB", EMU_SO)
    glue = bind_rgb(glue_lib())
    sums = []

    def take(ex, img, j):
        w, h = glue.de265_get_image_width(img, 0), glue.de265_get_image_height(img, 0)
        layout = capi.RGB_PACKED if j % 2 else capi.RGB_PLANAR
        shapes = [(h, 3 * w, np.uint8)] if j % 2 else [(h, w, np.uint8)] * 3
        got, _ = RgbExporter(ex, -1, -1).export(img, layout, capi.RGB_U8, None, shapes)
        sums.append(int(got[0].sum()))

    n, downloads = decode(glue, emu_lib, take, max_pictures=8)
    assert n == 8 and downloads == 0, "a picture that was only exported as RGB was brought back to the host"
    assert len(set(sums)) > 1
    assert glue.m355_glue_cpu_pixel_calls() == 0
