"""m355_glue_ssim_image: decoded pictures of the reference-API decoder (glue/_build/libde265.so) measured against another picture on the DEVICE,
without a download — the SSIM half of `dec265 -m`, as m355_frame_ssim_async defines it.  CPU tier: the backend is the SIMT-interpreter build
(M355_LIB), as in test_glue_measure.py.  The first pictures of girlshy.h265 are measured against device copies of the planes
de265_get_image_plane returned in an earlier run (every window 2^30, ssim 1.0), in a run that only measures and therefore downloads nothing; one
picture is measured against a perturbed copy with maps, with a rectangle and with a plane selection, against the numpy restatement
(tests/ssim_util.py) on the downloaded planes."""
import ctypes

import numpy as np

import ssim_util as su
from libde265_amd import capi
from test_emu_picture import emu_lib, EMU_SO  # noqa: F401  (fixture)
from test_glue_export import bind as bind_export, decode, host_planes
from test_glue_live import glue_lib

PICTURES = 5


def bind(glue):
    vp, i, p64 = ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int64)
    glue.m355_glue_ssim_image.argtypes = [vp, ctypes.POINTER(i), ctypes.POINTER(vp), p64, i, ctypes.POINTER(vp), p64, ctypes.POINTER(capi.Ssim)]
    return bind_export(glue)


def ssim(ex, img, planes, rect=None, select=0, want_maps=None):
    """the image against `planes` (the rectangle's, numpy) copied into device memory of the backend the glue has loaded -> (the list capi returns, maps)"""
    ref, pitch, bufs = (ctypes.c_void_p * 3)(), (ctypes.c_int64 * 3)(), []
    for k, a in enumerate(planes):
        pitch[k] = a.shape[1] * a.itemsize + 6
        raw = np.full((a.shape[0], pitch[k]), capi.DEVICE_FILL, np.uint8)
        raw[:, :a.shape[1] * a.itemsize] = np.ascontiguousarray(a).view(np.uint8).reshape(a.shape[0], -1)
        bufs.append(ex.L.m355_device_alloc(ex.mctx, raw.size))
        assert bufs[-1] and ex.L.m355_device_write(ex.mctx, bufs[-1], raw.ctypes.data, raw.size) == 0
        ref[k] = bufs[-1]
    maps, map_pitch, got_maps = None, None, [None] * 3
    if want_maps is not None:
        maps, map_pitch = (ctypes.c_void_p * 3)(), (ctypes.c_int64 * 3)()
        for k, m in enumerate(want_maps):
            if m is not None:
                map_pitch[k] = 4 * m.shape[1] + 8
                maps[k] = ex.L.m355_device_alloc(ex.mctx, m.shape[0] * map_pitch[k])
                assert maps[k]
                bufs.append(maps[k])
    out = capi.Ssim()
    r = (ctypes.c_int * 4)(*rect) if rect is not None else None
    rc = ex.glue.m355_glue_ssim_image(img, r, ref, pitch, select, maps, map_pitch, ctypes.byref(out))
    if rc == 0 and want_maps is not None:
        for k, m in enumerate(want_maps):
            if m is not None:
                raw = np.zeros(m.shape[0] * map_pitch[k], np.uint8)
                assert ex.L.m355_device_read(ex.mctx, maps[k], raw.ctypes.data, raw.size) == 0
                got_maps[k] = raw.reshape(m.shape[0], map_pitch[k])[:, :4 * m.shape[1]].copy().view(np.int32)
    for p in bufs:
        ex.L.m355_device_free(ex.mctx, p)
    assert rc == 0
    return [dict(sum_q=int(out.sum_q[c]), n=int(out.n[c]), min_q=int(out.min_q[c]), ssim=float(out.ssim[c])) for c in range(3)], got_maps


def test_ssim_of_images_equals_the_restatement_on_their_planes(emu_lib, monkeypatch):  # noqa: F811
    monkeypatch.setenv("M355_LIB", EMU_SO)
    glue = bind(glue_lib())
    earlier = []
    n, downloads = decode(glue, emu_lib, lambda ex, img, k: earlier.append(host_planes(glue, img)), max_pictures=PICTURES)
    assert n == PICTURES and downloads == PICTURES

    def check(ex, img, k):
        planes = earlier[k]
        geom = (planes[0].shape[1], planes[0].shape[0], 1, 8, 8)
        want, _ = su.expected(planes, planes, None, geom)
        assert all(w["min_q"] == su.ONE and w["ssim"] == 1.0 for w in want)
        su.assert_result(ssim(ex, img, planes)[0], want, "picture %d against its own planes" % k)
        if k == 3:
            other = su.perturbed(planes, (8, 8, 8), seed=9)
            want, want_maps = su.expected(planes, other, None, geom)
            assert all(0 < w["ssim"] < 1 for w in want)
            got, got_maps = ssim(ex, img, other, want_maps=want_maps)
            su.assert_result(got, want, "picture %d against a perturbed copy" % k)
            assert all((g == m).all() for g, m in zip(got_maps, want_maps)), "the maps"
            rect = (6, 2, 50, 40)
            part = [p[1:21, 3:28] if c else p[2:42, 6:56] for c, p in enumerate(other)]
            su.assert_result(ssim(ex, img, part, rect)[0], su.expected(planes, part, rect, geom)[0], "picture %d, rectangle" % k)
            su.assert_result(ssim(ex, img, other, select=1)[0], su.expected(planes, other, None, geom, planes=1)[0], "picture %d, luma only" % k)

    n, downloads = decode(glue, emu_lib, check, max_pictures=PICTURES)
    assert n == PICTURES and downloads == 0, "a picture that was only measured was brought back to the host"
    assert glue.m355_glue_cpu_pixel_calls() == 0, "the decoder called into its CPU pixel table"
