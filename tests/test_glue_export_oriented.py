"""m355_glue_export_image_oriented and m355_glue_export_image_pixels_oriented: decoded pictures leave the reference-API decoder (glue/_build/libde265.so)
turned, in DEVICE memory, without a download.  CPU tier: the backend is the SIMT-interpreter build (M355_LIB), as in test_glue_export_pixels.py.  The first
output picture of girlshy.h265 is exported with orientation 5 (90 degrees clockwise) and a NULL rectangle (the conformance window) through both calls; each
must equal export_oriented_util.orient of what the un-oriented glue call delivers, and of the restatement of the planes de265_get_image_plane returns
afterwards.  A null image and a decoder that shards its pictures are rejected."""
import ctypes

import numpy as np

import export_oriented_util as ou
import export_pixels_util as pu
from export_oriented_util import M355_ERR_INVALID
from export_util import assert_export
from synth_util import assert_planes_equal
from libde265_amd import capi
from test_emu_picture import emu_lib, EMU_SO  # noqa: F401  (fixture)
from test_glue_export import decode, host_planes, planar_shapes
from test_glue_export_pixels import bind_pixels, export_pixels
from test_glue_export_rgb import MATRIX_OF
from test_glue_live import glue_lib

CW = capi.ORIENT_ROTATE_90_CW


def bind_oriented(glue):
    vp, i = ctypes.c_void_p, ctypes.c_int
    glue.m355_glue_export_image_oriented.argtypes = [vp, i, i, ctypes.POINTER(i), i, ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_int64), vp]
    glue.m355_glue_export_image_pixels_oriented.argtypes = [vp, i, i, i, i, ctypes.POINTER(i), i, vp, ctypes.c_int64, i, vp]
    return bind_pixels(glue)


def buffers(ex, shapes, pad=12):
    """destination buffers with DEVICE_FILL in every byte for [(rows, elements, dtype)] -> (dst array, pitch array, pointers)"""
    dst, pitch, bufs = (ctypes.c_void_p * 3)(), (ctypes.c_int64 * 3)(), []
    for k, (rows, n, dt) in enumerate(shapes):
        pitch[k] = n * np.dtype(dt).itemsize + pad
        bufs.append(ex.L.m355_device_alloc(ex.mctx, rows * pitch[k]))
        assert bufs[-1]
        fill = np.full(rows * pitch[k], capi.DEVICE_FILL, np.uint8)
        assert ex.L.m355_device_write(ex.mctx, bufs[-1], fill.ctypes.data, fill.size) == 0
        dst[k] = bufs[-1]
    return dst, pitch, bufs


def read_back(ex, shapes, pitch, bufs):
    planes, raws = [], []
    for k, (rows, n, dt) in enumerate(shapes):
        raw = np.zeros(rows * pitch[k], np.uint8)
        assert ex.L.m355_device_read(ex.mctx, bufs[k], raw.ctypes.data, raw.size) == 0
        ex.L.m355_device_free(ex.mctx, bufs[k])
        raw = raw.reshape(rows, pitch[k])
        raws.append(raw)
        planes.append(np.ascontiguousarray(raw[:, :n * np.dtype(dt).itemsize]).view(dt))
    return planes, raws


def test_oriented_images_equal_the_oriented_plain_exports(emu_lib, monkeypatch):  # noqa: F811
    monkeypatch.setenv("M355_LIB", EMU_SO)
    glue = bind_oriented(glue_lib())

    def check(ex, img, j):
        assert glue.de265_get_chroma_format(img) == 1 and glue.de265_get_bits_per_pixel(img, 0) == 8
        w, h = glue.de265_get_image_width(img, 0), glue.de265_get_image_height(img, 0)
        shapes = planar_shapes(glue, img)
        # exported first: at this point nothing has asked for the picture's samples
        plain, _ = ex.export(img, capi.EXPORT_PLANAR, capi.EXPORT_NATIVE, None, shapes)
        turned_shapes = [(n, rows, dt) for rows, n, dt in shapes]
        dst, pitch, bufs = buffers(ex, turned_shapes)
        assert glue.m355_glue_export_image_oriented(img, capi.EXPORT_PLANAR, capi.EXPORT_NATIVE, None, CW, dst, pitch, None) == 0
        got, raws = read_back(ex, turned_shapes, pitch, bufs)
        assert_export(got, raws, [ou.orient(p, CW) for p in plain], "planes, 90 degrees clockwise")
        px_plain = export_pixels(ex, img, capi.PIXEL_BGRA8, 200, None, (w, h))[0]
        (pdst,), (ppitch,), pbufs = [a[:1] for a in buffers(ex, [(w, 4 * h, np.uint8)])]
        assert glue.m355_glue_export_image_pixels_oriented(img, capi.PIXEL_BGRA8, 200, -1, -1, None, CW, pdst, ppitch, -1, None) == 0
        (px,), (px_raw,) = read_back(ex, [(w, 4 * h, np.uint8)], [ppitch], pbufs)
        assert_export([px], [px_raw], [ou.orient_rows(px_plain, CW, 4)], "pixels, 90 degrees clockwise")
        # a null image
        dst, pitch, bufs = buffers(ex, turned_shapes)
        assert glue.m355_glue_export_image_oriented(None, capi.EXPORT_PLANAR, capi.EXPORT_NATIVE, None, CW, dst, pitch, None) == M355_ERR_INVALID
        assert glue.m355_glue_export_image_pixels_oriented(None, capi.PIXEL_BGRA8, 200, -1, -1, None, CW, dst[0], pitch[0], -1, None) == M355_ERR_INVALID
        assert glue.m355_glue_export_image_oriented(img, capi.EXPORT_PLANAR, capi.EXPORT_NATIVE, None, 8, dst, pitch, None) == M355_ERR_INVALID
        for raw in read_back(ex, turned_shapes, pitch, bufs)[1]:
            assert np.all(raw == capi.DEVICE_FILL), "a rejected export wrote to its destination"
        # against the restatements of the planes the application reads
        m = MATRIX_OF[glue.de265_get_image_matrix_coefficients(img)]
        full = 1 if glue.de265_get_image_full_range_flag(img) else 0
        loc = glue.m355_glue_image_chroma_loc(img)
        planes = host_planes(glue, img)
        assert_planes_equal(got, [ou.orient(p, CW) for p in planes], "planes against the host planes")
        assert_planes_equal([px], [ou.orient_rows(pu.expected_pixels(planes, 1, 8, 8, capi.PIXEL_BGRA8, 200, m, full, None, loc), CW, 4)], "pixels against the host planes")
        assert got[0].shape == (w, h) and len(np.unique(px)) > 64

    n, _ = decode(glue, emu_lib, check, max_pictures=1)
    assert n == 1
    assert glue.m355_glue_cpu_pixel_calls() == 0, "the decoder called into its CPU pixel table"


def test_a_sharded_decoder_is_rejected(emu_lib, monkeypatch):  # noqa: F811
    """a decoder that shards its pictures over several ranks holds complete frames only behind the gather: both calls are M355_ERR_INVALID, as
    m355_glue_export_image is, and write nothing"""
    monkeypatch.setenv("M355_LIB", EMU_SO)
    monkeypatch.setenv("M355_GLUE_RANKS", "2")
    glue = bind_oriented(glue_lib())
    seen = []

    def check(ex, img, j):
        w, h = glue.de265_get_image_width(img, 0), glue.de265_get_image_height(img, 0)
        shapes = [(n, rows, dt) for rows, n, dt in planar_shapes(glue, img)]
        dst, pitch, bufs = buffers(ex, shapes)
        assert glue.m355_glue_export_image(img, capi.EXPORT_PLANAR, capi.EXPORT_NATIVE, None, dst, pitch, None) == M355_ERR_INVALID
        assert glue.m355_glue_export_image_oriented(img, capi.EXPORT_PLANAR, capi.EXPORT_NATIVE, None, CW, dst, pitch, None) == M355_ERR_INVALID
        assert glue.m355_glue_export_image_pixels_oriented(img, capi.PIXEL_BGRA8, 200, -1, -1, None, CW, dst[0], pitch[0], -1, None) == M355_ERR_INVALID
        for raw in read_back(ex, shapes, pitch, bufs)[1]:
            assert np.all(raw == capi.DEVICE_FILL)
        seen.append((w, h))

    n, _ = decode(glue, emu_lib, check, max_pictures=1)
    assert n == 1 and seen
