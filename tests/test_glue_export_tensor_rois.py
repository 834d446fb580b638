"""m355_glue_export_images_tensor_rois: REGIONS of decoded pictures leave the reference-API decoder (glue/_build/libde265.so) as one normalised float
tensor in device memory, one rectangle per slice, in one launch and without a download.  CPU tier: the backend is the SIMT-interpreter build
(M355_LIB), as in test_glue_export_tensor.py.  The three pictures of the generated stream with a non-empty conformance window (tests/test_streams.py
G_CONFWIN, 4:2:0, 8 bits) are held until the last one has come out, then exported as one batch of five slices: a different rectangle per picture,
one picture twice (its rectangle plain and mirrored), and one entry with all-zero rectangle fields, which must resolve to THAT picture's own
conformance window.  Each slice must equal the restatement (export_tensor_util.py) of the samples of its picture — an explicit rectangle counts
from the coded picture's corner: its samples come from m355_glue_export_image of the same rectangle; the window's from de265_get_image_plane —, bit
for bit, mirrored slices with their columns reversed, and equal the slice m355_glue_export_images_tensor delivers for that picture and rectangle
alone.  Bad arguments are rejected and write nothing; the decoder's CPU pixel table is never called."""
import ctypes

import numpy as np

from export_tensor_util import M355_ERR_INVALID, assert_tensor, expected_ints, expected_tensor, imagenet
from export_tensor_rois_util import MIRROR, reverse_columns
from libde265_amd import capi
from test_emu_picture import emu_lib, EMU_SO  # noqa: F401  (fixture)
from test_glue_export import decode, host_planes
from test_glue_export_tensor import Tensor, bind_tensor, export_batch
from test_glue_live import glue_lib
from test_streams import G_CONFWIN, make_stream

RECTS = [(6, 2, 50, 22), (0, 0, 96, 40), (100, 60, 40, 30)]
OUT = (48, 20)


def bind_rois(glue):
    vp, i, f3, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_float), ctypes.c_int64
    glue.m355_glue_export_images_tensor_rois.argtypes = [ctypes.POINTER(vp), ctypes.POINTER(i * 5), i, i, i, i, i, i, ctypes.POINTER(i), f3, f3, vp, i64, i64, i64, vp]
    return bind_tensor(glue)


def export_rois(glue, t, imgs, rois, dtype, samples, matrix, full, scale, bias, n=None, null_rois=False):
    arr = (ctypes.c_void_p * len(imgs))(*imgs)
    ra = None if null_rois else ((ctypes.c_int * 5) * len(rois))(*[(ctypes.c_int * 5)(*r) for r in rois])
    return glue.m355_glue_export_images_tensor_rois(arr, ra, len(imgs) if n is None else n, t.layout, dtype, samples, matrix, full, (ctypes.c_int * 2)(t.w, t.h),
                                                    (ctypes.c_float * 3)(*scale), (ctypes.c_float * 3)(*bias), t.p, t.sn, t.sc, t.sh, None)


def test_regions_of_the_images_of_a_stream_as_one_batch(emu_lib, tmp_path, monkeypatch):  # noqa: F811
    monkeypatch.setenv("M355_LIB", EMU_SO)
    glue = bind_rois(glue_lib())
    data = make_stream(tmp_path, 256, 128, 8, 1, 1, 3, 117, 10, 1, 1, 0, 1, 1, G_CONFWIN)
    imgs = []

    def take(ex, img, j):
        imgs.append(img)                       # (held until the stream's last picture has come out, as in test_glue_export_tensor.py)
        if j == 2:
            check(ex)

    def check(ex):
        for img in imgs:
            assert (glue.de265_get_image_width(img, 0), glue.de265_get_image_height(img, 0)) != (256, 128), "the stream has no conformance window"
        scale, bias = imagenet(capi.RGB_U16)
        # picture 2 with its rectangle, picture 0 with another, picture 1 twice (plain and mirrored), picture 0 through the all-zero entry
        order = [imgs[2], imgs[0], imgs[1], imgs[1], imgs[0]]
        rois = [RECTS[2] + (0,), RECTS[0] + (0,), RECTS[1] + (0,), RECTS[1] + (MIRROR,), (0, 0, 0, 0, MIRROR)]
        layout, dtype = capi.TENSOR_NHWC, capi.TENSOR_F32
        t = Tensor(ex, 5, layout, dtype, OUT)
        assert export_rois(glue, t, order, rois, dtype, capi.RGB_U16, capi.MATRIX_BT601, 1, scale, bias) == 0
        got = t.finish()
        # the same slices through the existing entry, one picture and one rectangle per call (NULL: the window of that picture)
        singles = []
        for img, r in zip(order, rois):
            s = Tensor(ex, 1, layout, dtype, OUT)
            assert export_batch(glue, s, [img], dtype, capi.RGB_U16, capi.MATRIX_BT601, 1, r[:4] if any(r[:4]) else None, scale, bias) == 0
            one = s.finish()[0][0]
            singles.append(reverse_columns(one, layout) if r[4] else one)
        # rejected, nothing written: null rois, no entries, too many, a null picture, an unknown flag, a rectangle outside its picture, an unknown dtype
        bad = Tensor(ex, 2, layout, dtype, OUT)
        two, r2 = imgs[:2], [RECTS[0] + (0,), RECTS[1] + (0,)]
        args = (dtype, capi.RGB_U16, capi.MATRIX_BT601, 1, scale, bias)
        assert export_rois(glue, bad, two, r2, *args, null_rois=True) == M355_ERR_INVALID
        assert export_rois(glue, bad, two, r2, *args, n=0) == M355_ERR_INVALID
        assert export_rois(glue, bad, two, r2, *args, n=33) == M355_ERR_INVALID
        assert export_rois(glue, bad, [imgs[0], None], r2, *args) == M355_ERR_INVALID
        assert export_rois(glue, bad, two, [RECTS[0] + (0,), RECTS[1] + (2,)], *args) == M355_ERR_INVALID
        assert export_rois(glue, bad, two, [RECTS[0] + (0,), (200, 100, 100, 60, 0)], *args) == M355_ERR_INVALID
        assert export_rois(glue, bad, two, r2, 3, capi.RGB_U16, capi.MATRIX_BT601, 1, scale, bias) == M355_ERR_INVALID
        assert np.all(bad.finish()[1] == capi.DEVICE_FILL), "a rejected export wrote to its destination"

        # the restatement: an explicit rectangle's samples from the plain export of the same rectangle, the window's from the host planes
        want = []
        for img, r in zip(order, rois):
            if any(r[:4]):
                shapes = [(r[3], r[2], np.uint8)] + [(r[3] // 2, r[2] // 2, np.uint8)] * 2
                planes = ex.export(img, capi.EXPORT_PLANAR, capi.EXPORT_NATIVE, r[:4], shapes)[0]
            else:
                planes = host_planes(glue, img)
            w = expected_tensor([expected_ints(planes, (1, 8, 8), capi.RGB_U16, capi.MATRIX_BT601, 1, OUT)], layout, dtype, scale, bias)[0]
            want.append(reverse_columns(w, layout) if r[4] else w)
        assert_tensor(got, np.stack(want), "five regions of three pictures")
        for i, one in enumerate(singles):
            assert np.array_equal(got[0][i], one), "slice %d differs from m355_glue_export_images_tensor of that picture and rectangle" % i
        assert np.array_equal(got[0][3], reverse_columns(got[0][2], layout)) and not np.array_equal(got[0][3], got[0][2])
        assert not np.array_equal(got[0][1], got[0][4])

    n, _ = decode(glue, emu_lib, take, data=data)
    assert n == 3
    assert glue.m355_glue_cpu_pixel_calls() == 0, "the decoder called into its CPU pixel table"
