"""m355_glue_export_image: decoded pictures leave the reference-API decoder (glue/_build/libde265.so) into DEVICE memory, without a download.
CPU tier: the backend is the SIMT-interpreter build (M355_LIB), as in test_glue_live.py.  Every output picture of girlshy.h265 is exported
(planar, samples as they are, the image's conformance window) and must equal the planes de265_get_image_plane returns; one picture also goes out
through an explicit rectangle as semi-planar 8-bit and must equal the numpy restatement; the decoder's CPU pixel table is never called; and a run
that only exports downloads nothing.  Two generated streams with a NON-EMPTY conformance window (tests/test_streams.py G_CONFWIN; 4:2:0 and 4:4:4)
pin the window arithmetic of the NULL-rectangle case: offsets, SubWidthC / SubHeightC, cropped size."""
import ctypes

import numpy as np
import pytest

import de265_py
from export_util import assert_export, expected_export
from libde265_amd import capi
from test_emu_picture import emu_lib, EMU_SO  # noqa: F401  (fixture)
from test_glue_live import STREAM, glue_lib
from test_streams import G_CONFWIN, G_CTB16, G_TB16, make_stream

RECT = (6, 2, 50, 22)


def bind(glue):
    vp, i = ctypes.c_void_p, ctypes.c_int
    glue.m355_glue_export_image.argtypes = [vp, i, i, ctypes.POINTER(i), ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_int64), vp]
    glue.m355_glue_backend_context.argtypes = [vp]
    glue.m355_glue_backend_context.restype = vp
    glue.m355_glue_stats.argtypes = [vp] + [ctypes.POINTER(ctypes.c_longlong)] * 3
    return de265_py.bind(glue)


class Exporter:
    """device buffers from the backend the glue has loaded (m355_device_*), one export of an image per call"""

    def __init__(self, glue, backend, dec):
        self.glue, self.L, self.mctx = glue, backend.lib, glue.m355_glue_backend_context(dec)
        assert self.mctx

    def export(self, img, layout, samples, rect, shapes, pad=12):
        """shapes: [(rows, elements, dtype)] of the destination planes -> (planes, whole buffers as (rows, pitch) bytes)"""
        dst, pitch, bufs = (ctypes.c_void_p * 3)(), (ctypes.c_int64 * 3)(), []
        for k, (rows, n, dt) in enumerate(shapes):
            pitch[k] = n * np.dtype(dt).itemsize + pad
            bufs.append(self.L.m355_device_alloc(self.mctx, rows * pitch[k]))
            assert bufs[-1]
            fill = np.full(rows * pitch[k], capi.DEVICE_FILL, np.uint8)
            assert self.L.m355_device_write(self.mctx, bufs[-1], fill.ctypes.data, fill.size) == 0
            dst[k] = bufs[-1]
        r = (ctypes.c_int * 4)(*rect) if rect is not None else None
        assert self.glue.m355_glue_export_image(img, layout, samples, r, dst, pitch, None) == 0
        planes, raws = [], []
        for k, (rows, n, dt) in enumerate(shapes):
            raw = np.zeros(rows * pitch[k], np.uint8)
            assert self.L.m355_device_read(self.mctx, bufs[k], raw.ctypes.data, raw.size) == 0
            self.L.m355_device_free(self.mctx, bufs[k])
            raw = raw.reshape(rows, pitch[k])
            raws.append(raw)
            planes.append(np.ascontiguousarray(raw[:, :n * np.dtype(dt).itemsize]).view(dt))
        return planes, raws


def host_planes(glue, img):
    out = []
    for c in range(1 if glue.de265_get_chroma_format(img) == 0 else 3):
        stride = ctypes.c_int()
        p = glue.de265_get_image_plane(img, c, ctypes.byref(stride))
        w, h = glue.de265_get_image_width(img, c), glue.de265_get_image_height(img, c)
        dt = np.uint8 if glue.de265_get_bits_per_pixel(img, c) <= 8 else np.uint16
        a = np.empty((h, w), dt)
        for y in range(h):
            a[y] = np.frombuffer((ctypes.c_char * (w * a.itemsize)).from_address(p + y * stride.value), dt, w)
        out.append(a)
    return out


def planar_shapes(glue, img):
    """the planes de265.h describes for the image (its conformance window): [(rows, elements, dtype)]"""
    return [(glue.de265_get_image_height(img, c), glue.de265_get_image_width(img, c), np.uint8 if glue.de265_get_bits_per_pixel(img, c) <= 8 else np.uint16)
            for c in range(1 if glue.de265_get_chroma_format(img) == 0 else 3)]


def decode(glue, backend, per_picture, threads=2, max_pictures=None, data=None):
    """a stream (girlshy) through the decoder; per_picture(exporter, img, index) for every output picture (the first max_pictures) -> (pictures, downloads)"""
    data = data if data is not None else open(STREAM, "rb").read()
    dec = glue.de265_new_decoder()
    assert dec
    try:
        assert glue.de265_start_worker_threads(dec, threads) == 0
        buf = ctypes.create_string_buffer(data, len(data))
        assert glue.de265_push_data(dec, buf, len(data), 0, None) == 0 and glue.de265_flush_data(dec) == 0
        ex = Exporter(glue, backend, dec)
        n, more = 0, ctypes.c_int(1)
        while more.value:
            more.value = 0
            assert glue.de265_decode(dec, ctypes.byref(more)) == 0
            while True:
                img = glue.de265_get_next_picture(dec)
                if not img:
                    break
                per_picture(ex, img, n)
                n += 1
                if max_pictures and n >= max_pictures:
                    more.value = 0
                    break
        stats = [ctypes.c_longlong() for _ in range(3)]
        assert glue.m355_glue_stats(dec, *[ctypes.byref(s) for s in stats]) == 0
        return n, stats[2].value
    finally:
        glue.de265_free_decoder(dec)


def test_exported_images_equal_the_host_planes(emu_lib, monkeypatch):  # noqa: F811
    monkeypatch.setenv("M355_LIB", EMU_SO)
    glue = bind(glue_lib())

    def check(ex, img, k):
        # exported first: at this point nothing has asked for the picture's samples
        got, raws = ex.export(img, capi.EXPORT_PLANAR, capi.EXPORT_NATIVE, None, planar_shapes(glue, img))
        want = host_planes(glue, img)
        assert_export(got, raws, want, "picture %d" % k)
        if k == 3:
            rows = [(RECT[3], RECT[2], np.uint8), (RECT[3] // 2, RECT[2], np.uint8)]
            got, raws = ex.export(img, capi.EXPORT_SEMIPLANAR, capi.EXPORT_U8, RECT, rows)
            assert_export(got, raws, expected_export(want, 1, 8, 8, capi.EXPORT_SEMIPLANAR, capi.EXPORT_U8, RECT), "picture %d, rectangle" % k)

    n, downloads = decode(glue, emu_lib, check)
    assert n == 75 and downloads == 75
    assert glue.m355_glue_cpu_pixel_calls() == 0, "the decoder called into its CPU pixel table"


# (coded width, height, seed, chroma format, geometry bits of oracle/ref_streamgen.cc): the application sees a cropped picture
@pytest.mark.parametrize("w,h,seed,chroma,geom", [(192, 128, 110, 3, G_CTB16 | G_TB16 | G_CONFWIN), (256, 128, 116, 1, G_CONFWIN)])
def test_null_rectangle_is_the_conformance_window(emu_lib, tmp_path, monkeypatch, w, h, seed, chroma, geom):  # noqa: F811
    monkeypatch.setenv("M355_LIB", EMU_SO)
    glue = bind(glue_lib())
    frames = 3
    data = make_stream(tmp_path, w, h, 8, 1, 1, frames, seed, 10, 1, 1, 0, chroma, 1, geom)

    def check(ex, img, k):
        shapes = planar_shapes(glue, img)
        assert (shapes[0][1], shapes[0][0]) != (w, h), "the stream has no conformance window"
        got, raws = ex.export(img, capi.EXPORT_PLANAR, capi.EXPORT_NATIVE, None, shapes)
        want = host_planes(glue, img)
        assert_export(got, raws, want, "picture %d" % k)
        semi = [shapes[0], (shapes[1][0], 2 * shapes[1][1], shapes[1][2])]
        got, raws = ex.export(img, capi.EXPORT_SEMIPLANAR, capi.EXPORT_MSB16, None, [(r, n, np.uint16) for r, n, _ in semi])
        assert_export(got, raws, expected_export(want, chroma, 8, 8, capi.EXPORT_SEMIPLANAR, capi.EXPORT_MSB16), "picture %d, semi-planar" % k)

    n, _ = decode(glue, emu_lib, check, data=data)
    assert n == frames
    assert glue.m355_glue_cpu_pixel_calls() == 0


def test_export_alone_downloads_nothing(emu_lib, monkeypatch):  # noqa: F811
    monkeypatch.setenv("M355_LIB", EMU_SO)
    glue = bind(glue_lib())
    sums = []

    def take(ex, img, k):
        got, _ = ex.export(img, capi.EXPORT_PLANAR, capi.EXPORT_NATIVE, None, planar_shapes(glue, img))
        sums.append(int(got[0].sum()))

    n, downloads = decode(glue, emu_lib, take, max_pictures=8)
    assert n == 8 and downloads == 0, "a picture that was only exported was brought back to the host"
    assert len(set(sums)) > 1
    assert glue.m355_glue_cpu_pixel_calls() == 0
