"""m355_glue_export_image_pixels: decoded pictures leave the reference-API decoder (glue/_build/libde265.so) as the pixels a compositor takes, in DEVICE
memory, without a download.  CPU tier: the backend is the SIMT-interpreter build (M355_LIB), as in test_glue_export.py.  The first output picture of
girlshy.h265 is exported as BGRA8 at its own size (out_size NULL: m355_frame_export_pixels) and as A2R10G10B10 at half its size
(m355_frame_export_resized_pixels), with -1 / -1 / -1 for matrix, range and chroma sample location type (what the stream signals).  Both must equal
the restatement (export_pixels_util.py) of the planes de265_get_image_plane returns afterwards; a format outside M355_PIXEL_* is rejected and writes
nothing, and the decoder's CPU pixel table is never called."""
import ctypes

import numpy as np

import export_pixels_util as pu
from export_pixels_util import M355_ERR_INVALID
from export_util import assert_export
from libde265_amd import capi
from test_emu_picture import emu_lib, EMU_SO  # noqa: F401  (fixture)
from test_glue_export import bind, decode, host_planes
from test_glue_export_rgb import MATRIX_OF
from test_glue_live import glue_lib


def bind_pixels(glue):
    vp, i = ctypes.c_void_p, ctypes.c_int
    glue.m355_glue_export_image_pixels.argtypes = [vp, i, i, i, i, ctypes.POINTER(i), ctypes.POINTER(i), vp, ctypes.c_int64, i, i, i, vp]
    glue.m355_glue_image_chroma_loc.argtypes = [vp]
    for f in (glue.de265_get_image_matrix_coefficients, glue.de265_get_image_full_range_flag):
        f.argtypes, f.restype = [vp], i
    return bind(glue)


def export_pixels(ex, img, format, alpha, out_size, size, pad=12, expect=0):
    """one picture through the glue into a buffer of size[1] rows with DEVICE_FILL in every byte -> (rows, the whole buffer as (rows, pitch) bytes)"""
    w, h = size
    n = w * capi.pixel_bytes(format)
    pitch = n + pad
    buf = ex.L.m355_device_alloc(ex.mctx, h * pitch)
    assert buf
    fill = np.full(h * pitch, capi.DEVICE_FILL, np.uint8)
    assert ex.L.m355_device_write(ex.mctx, buf, fill.ctypes.data, fill.size) == 0
    out = (ctypes.c_int * 2)(*out_size) if out_size is not None else None
    assert ex.glue.m355_glue_export_image_pixels(img, format, alpha, -1, -1, None, out, buf, pitch, 0, -1, 0, None) == expect
    raw = np.zeros(h * pitch, np.uint8)
    assert ex.L.m355_device_read(ex.mctx, buf, raw.ctypes.data, raw.size) == 0
    ex.L.m355_device_free(ex.mctx, buf)
    raw = raw.reshape(h, pitch)
    return np.ascontiguousarray(raw[:, :n]), raw


def test_pixel_images_equal_the_packed_host_planes(emu_lib, monkeypatch):  # noqa: F811
    monkeypatch.setenv("M355_LIB", EMU_SO)
    glue = bind_pixels(glue_lib())

    def check(ex, img, j):
        assert glue.de265_get_chroma_format(img) == 1 and glue.de265_get_bits_per_pixel(img, 0) == 8
        w, h = glue.de265_get_image_width(img, 0), glue.de265_get_image_height(img, 0)
        half = (w // 2 & ~1, h // 2 & ~1)
        # exported first: at this point nothing has asked for the picture's samples
        own = export_pixels(ex, img, capi.PIXEL_BGRA8, 200, None, (w, h))
        small = export_pixels(ex, img, capi.PIXEL_A2R10G10B10, 3, half, half)
        bad = export_pixels(ex, img, 5, 0, None, (w, h), expect=M355_ERR_INVALID)
        assert np.all(bad[1] == capi.DEVICE_FILL), "a rejected export wrote to its destination"
        m = MATRIX_OF[glue.de265_get_image_matrix_coefficients(img)]
        full = 1 if glue.de265_get_image_full_range_flag(img) else 0
        loc = glue.m355_glue_image_chroma_loc(img)
        planes = host_planes(glue, img)
        assert_export([own[0]], [own[1]], [pu.expected_pixels(planes, 1, 8, 8, capi.PIXEL_BGRA8, 200, m, full, None, loc)], "BGRA8 at its own size")
        assert_export([small[0]], [small[1]], [pu.expected_resized_pixels(planes, 1, 8, capi.PIXEL_A2R10G10B10, 3, m, full, half, None, loc)],
                      "A2R10G10B10 at half size")
        assert len(np.unique(own[0])) > 64

    n, _ = decode(glue, emu_lib, check, max_pictures=1)
    assert n == 1
    assert glue.m355_glue_cpu_pixel_calls() == 0, "the decoder called into its CPU pixel table"
