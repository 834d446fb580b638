"""m355_glue_measure_image: decoded pictures of the reference-API decoder (glue/_build/libde265.so) compared with another picture on the DEVICE,
without a download — what `dec265 -m` does with MSE() of quality.cc on host planes.  CPU tier: the backend is the SIMT-interpreter build
(M355_LIB), as in test_glue_export.py.  Every output picture of girlshy.h265 is measured against device copies of the planes
de265_get_image_plane returned in an earlier run (no difference), in a run that only measures and therefore downloads nothing; one picture is
measured against a perturbed copy, and its mse must equal the reference's own MSE() on the same host planes bit for bit; the decoder's CPU
pixel table is never called.  One generated stream with a non-empty conformance window pins the NULL-rectangle case."""
import ctypes
import struct

import numpy as np

from measure_util import assert_result, expected
from libde265_amd import capi
from test_emu_picture import emu_lib, EMU_SO  # noqa: F401  (fixture)
from test_glue_export import bind as bind_export, decode, host_planes
from test_glue_live import glue_lib
from test_streams import G_CONFWIN, make_stream


def bind(glue):
    vp, i = ctypes.c_void_p, ctypes.c_int
    glue.m355_glue_measure_image.argtypes = [vp, ctypes.POINTER(i), ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(capi.Measure)]
    return bind_export(glue)


def measure(ex, img, planes, rect=None):
    """the image against `planes` (the rectangle's, numpy) copied into device memory of the backend the glue has loaded -> the list capi returns"""
    ref, pitch, bufs = (ctypes.c_void_p * 3)(), (ctypes.c_int64 * 3)(), []
    for k, a in enumerate(planes):
        pitch[k] = a.shape[1] * a.itemsize + 6
        raw = np.full((a.shape[0], pitch[k]), capi.DEVICE_FILL, np.uint8)
        raw[:, :a.shape[1] * a.itemsize] = np.ascontiguousarray(a).view(np.uint8).reshape(a.shape[0], -1)
        bufs.append(ex.L.m355_device_alloc(ex.mctx, raw.size))
        assert bufs[-1] and ex.L.m355_device_write(ex.mctx, bufs[-1], raw.ctypes.data, raw.size) == 0
        ref[k] = bufs[-1]
    out = capi.Measure()
    r = (ctypes.c_int * 4)(*rect) if rect is not None else None
    rc = ex.glue.m355_glue_measure_image(img, r, ref, pitch, ctypes.byref(out))
    for p in bufs:
        ex.L.m355_device_free(ex.mctx, p)
    assert rc == 0
    return [dict(ssd=int(out.ssd[c]), sad=int(out.sad[c]), n_diff=int(out.n_diff[c]), max_abs=int(out.max_abs[c]),
                 first=None if out.first_x[c] < 0 else (int(out.first_x[c]), int(out.first_y[c])), mse=float(out.mse[c])) for c in range(len(planes))]


def test_measured_images_equal_an_earlier_runs_planes(emu_lib, ref, monkeypatch):  # noqa: F811
    monkeypatch.setenv("M355_LIB", EMU_SO)
    glue = bind(glue_lib())
    earlier = []
    n, downloads = decode(glue, emu_lib, lambda ex, img, k: earlier.append(host_planes(glue, img)))
    assert n == 75 and downloads == 75
    mse = ref._Z3MSEPKhiS0_iii
    mse.argtypes, mse.restype = [ctypes.c_void_p, ctypes.c_int] * 2 + [ctypes.c_int] * 2, ctypes.c_double

    def check(ex, img, k):
        planes = earlier[k]
        assert_result(measure(ex, img, planes), expected(planes, planes, None, 1), "picture %d" % k)
        if k == 3:
            other = [p.copy() for p in planes]
            other[0][::7, ::5] ^= 0x1B
            other[1][4, 9] += 1
            other[2][:, -1] ^= 0xFF
            got = measure(ex, img, other)
            assert_result(got, expected(planes, other, None, 1), "picture %d against a perturbed copy" % k)
            for c, (a, b) in enumerate(zip(planes, other)):
                want = mse(a.ctypes.data, a.shape[1], b.ctypes.data, b.shape[1], a.shape[1], a.shape[0])
                assert want > 0 and struct.pack("<d", got[c]["mse"]) == struct.pack("<d", want), "plane %d: mse against the reference's MSE()" % c
            rect = (6, 2, 50, 22)
            part = [p[1:12, 3:28] if c else p[2:24, 6:56] for c, p in enumerate(other)]
            assert_result(measure(ex, img, part, rect), expected(planes, part, rect, 1), "picture %d, rectangle" % k)

    n, downloads = decode(glue, emu_lib, check)
    assert n == 75 and downloads == 0, "a picture that was only measured was brought back to the host"
    assert glue.m355_glue_cpu_pixel_calls() == 0, "the decoder called into its CPU pixel table"


def test_null_rectangle_is_the_conformance_window(emu_lib, tmp_path, monkeypatch):  # noqa: F811
    monkeypatch.setenv("M355_LIB", EMU_SO)
    glue = bind(glue_lib())
    w, h, frames = 256, 128, 3
    data = make_stream(tmp_path, w, h, 8, 1, 1, frames, 116, 10, 1, 1, 0, 1, 1, G_CONFWIN)

    def check(ex, img, k):
        first = measure(ex, img, [np.zeros((glue.de265_get_image_height(img, c), glue.de265_get_image_width(img, c)), np.uint8) for c in range(3)])
        want = host_planes(glue, img)                               # (the window: what de265.h describes for the image)
        assert (want[0].shape[1], want[0].shape[0]) != (w, h), "the stream has no conformance window"
        other = [p.copy() for p in want]
        other[0][0, 0] ^= 1
        other[1][-1, -1] ^= 2
        got = measure(ex, img, other)
        assert_result([dict(g, first=None) for g in got], [dict(x, first=None) for x in expected(want, other, None, 1)], "picture %d" % k)
        # first_x / first_y are coordinates in the coded frame: the window's corner samples
        x0, y0 = got[0]["first"]
        assert (x0, y0) != (0, 0) and got[1]["first"] == (x0 // 2 + want[1].shape[1] - 1, y0 // 2 + want[1].shape[0] - 1)
        assert_result([dict(g, first=None) for g in first], [dict(x, first=None) for x in expected(want, [np.zeros_like(p) for p in want], None, 1)], "picture %d against zero" % k)

    n, _ = decode(glue, emu_lib, check, data=data)
    assert n == frames
    assert glue.m355_glue_cpu_pixel_calls() == 0
