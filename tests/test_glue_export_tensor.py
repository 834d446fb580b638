"""m355_glue_export_images_tensor: decoded pictures leave the reference-API decoder (glue/_build/libde265.so) as ONE normalised float tensor in DEVICE
memory, a batch per launch, without a download.  CPU tier: the backend is the SIMT-interpreter build (M355_LIB), as in test_glue_export_resized_rgb.py.
The three pictures of a generated stream with a non-empty conformance window (tests/test_streams.py G_CONFWIN, 4:2:0, 8 bits) are held until the
last one has come out of the decoder and exported as batches: two of them through the NULL rectangle (the window of the first) with -1 / -1 (the
matrix and range the stream signals), all three — in another order, one twice — through an explicit rectangle with an explicit matrix.  Each slice must equal the restatement
(export_tensor_util.py) of the planes de265_get_image_plane returns for ITS picture (the rectangle: of its samples as m355_glue_export_image delivers
them), bit for bit, and the bytes outside the tensor's elements must be untouched.  Bad arguments are rejected and write nothing; the decoder's CPU
pixel table is never called."""
import ctypes

import numpy as np

from export_tensor_util import M355_ERR_INVALID, assert_tensor, expected_ints, expected_tensor, imagenet
from libde265_amd import capi
from test_emu_picture import emu_lib, EMU_SO  # noqa: F401  (fixture)
from test_glue_export import bind, decode, host_planes
from test_glue_export_rgb import MATRIX_OF
from test_glue_live import glue_lib
from test_streams import G_CONFWIN, make_stream

RECT = (6, 2, 50, 22)


def bind_tensor(glue):
    vp, i, f3, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_float), ctypes.c_int64
    glue.m355_glue_export_images_tensor.argtypes = [ctypes.POINTER(vp), i, i, i, i, i, i, ctypes.POINTER(i), ctypes.POINTER(i), f3, f3, vp, i64, i64, i64, vp]
    for f in (glue.de265_get_image_matrix_coefficients, glue.de265_get_image_full_range_flag):
        f.argtypes, f.restype = [vp], i
    return bind(glue)


class Tensor:
    """one destination buffer from the backend the glue has loaded, made as capi.Context.frames_export_tensor makes it: filled with DEVICE_FILL, every
    stride `pad` bytes above the smallest the call accepts"""

    def __init__(self, ex, n, layout, dtype, out_size, pad=12):
        self.ex, self.n, self.layout, (self.w, self.h) = ex, n, layout, out_size
        self.eb = 4 if dtype == capi.TENSOR_F32 else 2
        row = self.w * self.eb * (3 if layout == capi.TENSOR_NHWC else 1)
        self.sh = row + pad
        extent = (self.h - 1) * self.sh + row
        self.sc = extent + pad if layout == capi.TENSOR_NCHW else 0
        self.sn = (2 * self.sc + extent) + pad
        self.nbytes = (n - 1) * self.sn + 2 * self.sc + extent
        self.p = ex.L.m355_device_alloc(ex.mctx, self.nbytes)
        assert self.p
        fill = np.full(self.nbytes, capi.DEVICE_FILL, np.uint8)
        assert ex.L.m355_device_write(ex.mctx, self.p, fill.ctypes.data, self.nbytes) == 0

    def finish(self):
        """-> (elements, raw, outside) as capi.Context.tensor_export_finish; frees the buffer"""
        raw = np.zeros(self.nbytes, np.uint8)
        assert self.ex.L.m355_device_read(self.ex.mctx, self.p, raw.ctypes.data, self.nbytes) == 0
        self.ex.L.m355_device_free(self.ex.mctx, self.p)
        n, h, w, eb = self.n, self.h, self.w, self.eb
        if self.layout == capi.TENSOR_NCHW:
            shape, strides = (n, 3, h, w, eb), (self.sn, self.sc, self.sh, eb, 1)
        else:
            shape, strides = (n, h, w, 3, eb), (self.sn, self.sh, 3 * eb, eb, 1)
        elements = np.ascontiguousarray(np.lib.stride_tricks.as_strided(raw, shape, strides)).view(np.uint32 if eb == 4 else np.uint16).reshape(shape[:-1])
        inside = np.zeros(self.nbytes, np.uint8)
        np.lib.stride_tricks.as_strided(inside, shape, strides)[...] = 1
        return elements, raw, raw[inside == 0]


def export_batch(glue, t, imgs, dtype, samples, matrix, full, rect, scale, bias, n=None):
    arr = (ctypes.c_void_p * len(imgs))(*imgs)
    r = (ctypes.c_int * 4)(*rect) if rect is not None else None
    return glue.m355_glue_export_images_tensor(arr, len(imgs) if n is None else n, t.layout, dtype, samples, matrix, full, r, (ctypes.c_int * 2)(t.w, t.h),
                                               (ctypes.c_float * 3)(*scale), (ctypes.c_float * 3)(*bias), t.p, t.sn, t.sc, t.sh, None)


def test_images_of_a_stream_as_one_batch(emu_lib, tmp_path, monkeypatch):  # noqa: F811
    monkeypatch.setenv("M355_LIB", EMU_SO)
    glue = bind_tensor(glue_lib())
    data = make_stream(tmp_path, 256, 128, 8, 1, 1, 3, 117, 10, 1, 1, 0, 1, 1, G_CONFWIN)
    imgs = []

    def take(ex, img, j):
        # the pictures are held until the stream's last one has come out: the decoder keeps a picture's frame until it decodes into it again, and a
        # picture whose frame has gone is rejected by the glue, not exported
        imgs.append(img)
        if j == 2:
            check(ex)

    def check(ex):
        for img in imgs:
            assert glue.de265_get_chroma_format(img) == 1 and glue.de265_get_bits_per_pixel(img, 0) == 8
            assert (glue.de265_get_image_width(img, 0), glue.de265_get_image_height(img, 0)) != (256, 128), "the stream has no conformance window"
        # exported first: at this point nothing has asked for the pictures' samples
        scale, bias = imagenet(capi.RGB_U8)
        window = Tensor(ex, 2, capi.TENSOR_NCHW, capi.TENSOR_F16, (96, 40))
        assert export_batch(glue, window, imgs[:2], capi.TENSOR_F16, capi.RGB_U8, -1, -1, None, scale, bias) == 0
        got_window = window.finish()
        order = [imgs[2], imgs[0], imgs[1], imgs[2]]
        scale16, bias16 = imagenet(capi.RGB_U16)
        inside = Tensor(ex, 4, capi.TENSOR_NHWC, capi.TENSOR_F32, (36, 14))
        assert export_batch(glue, inside, order, capi.TENSOR_F32, capi.RGB_U16, capi.MATRIX_BT601, 1, RECT, scale16, bias16) == 0
        got_inside = inside.finish()
        # rejected, nothing written: no pictures, too many, a null picture, an unknown matrix, an unknown dtype
        bad = Tensor(ex, 2, capi.TENSOR_NCHW, capi.TENSOR_F16, (96, 40))
        assert export_batch(glue, bad, imgs[:2], capi.TENSOR_F16, capi.RGB_U8, -1, -1, None, scale, bias, n=0) == M355_ERR_INVALID
        assert export_batch(glue, bad, imgs[:2], capi.TENSOR_F16, capi.RGB_U8, -1, -1, None, scale, bias, n=33) == M355_ERR_INVALID
        assert export_batch(glue, bad, [imgs[0], None], capi.TENSOR_F16, capi.RGB_U8, -1, -1, None, scale, bias) == M355_ERR_INVALID
        assert export_batch(glue, bad, imgs[:2], capi.TENSOR_F16, capi.RGB_U8, 9, 0, None, scale, bias) == M355_ERR_INVALID
        assert export_batch(glue, bad, imgs[:2], 3, capi.RGB_U8, -1, -1, None, scale, bias) == M355_ERR_INVALID
        assert np.all(bad.finish()[1] == capi.DEVICE_FILL), "a rejected export wrote to its destination"

        host = {img: host_planes(glue, img) for img in imgs}            # (the window's samples: what the NULL rectangle resizes)
        assert not np.array_equal(host[imgs[0]][0], host[imgs[1]][0])
        m = MATRIX_OF[glue.de265_get_image_matrix_coefficients(imgs[0])]
        r = 1 if glue.de265_get_image_full_range_flag(imgs[0]) else 0
        ints = [expected_ints(host[img], (1, 8, 8), capi.RGB_U8, m, r, (96, 40)) for img in imgs[:2]]
        assert_tensor(got_window, expected_tensor(ints, capi.TENSOR_NCHW, capi.TENSOR_F16, scale, bias), "the window of two pictures")
        # an explicit rectangle counts from the coded picture's corner, not the window's: its samples come from the plain export of the same rectangle
        shapes = [(RECT[3], RECT[2], np.uint8)] + [(RECT[3] // 2, RECT[2] // 2, np.uint8)] * 2
        cut = {img: ex.export(img, capi.EXPORT_PLANAR, capi.EXPORT_NATIVE, RECT, shapes)[0] for img in imgs}
        ints = [expected_ints(cut[img], (1, 8, 8), capi.RGB_U16, capi.MATRIX_BT601, 1, (36, 14)) for img in order]
        assert_tensor(got_inside, expected_tensor(ints, capi.TENSOR_NHWC, capi.TENSOR_F32, scale16, bias16), "the rectangle of four slices")
        assert np.array_equal(got_inside[0][0], got_inside[0][3]) and not np.array_equal(got_inside[0][0], got_inside[0][1])

    n, _ = decode(glue, emu_lib, take, data=data)
    assert n == 3
    assert glue.m355_glue_cpu_pixel_calls() == 0, "the decoder called into its CPU pixel table"
