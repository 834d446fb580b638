"""m355_glue_msssim_image: decoded pictures of the reference-API decoder (glue/_build/libde265.so) measured against another picture on the DEVICE on
several scales, without a download, as m355_frame_msssim_async defines it.  CPU tier: the backend is the SIMT-interpreter build (M355_LIB), as in
test_glue_ssim.py.  The first pictures of girlshy.h265 are measured against device copies of the planes de265_get_image_plane returned in an earlier
run (luma on five levels: msssim 1.0; all planes on as many levels as chroma has), in a run that only measures and therefore downloads nothing; one
picture is measured against a perturbed copy, whole and with a rectangle and a plane selection, against the numpy restatement
(tests/msssim_util.py) on the downloaded planes."""
import ctypes

import msssim_util as mu
import numpy as np
import ssim_util as su
from libde265_amd import capi
from test_emu_picture import emu_lib, EMU_SO  # noqa: F401  (fixture)
from test_glue_export import bind as bind_export, decode, host_planes
from test_glue_live import glue_lib

PICTURES = 5


def bind(glue):
    vp, i, p64 = ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int64)
    glue.m355_glue_msssim_image.argtypes = [vp, ctypes.POINTER(i), ctypes.POINTER(vp), p64, i, i, ctypes.POINTER(capi.Msssim)]
    return bind_export(glue)


def msssim(ex, img, planes, levels, rect=None, select=0):
    """the image against `planes` (the rectangle's, numpy) copied into device memory of the backend the glue has loaded -> the list capi returns"""
    ref, pitch, bufs = (ctypes.c_void_p * 3)(), (ctypes.c_int64 * 3)(), []
    for k, a in enumerate(planes):
        pitch[k] = a.shape[1] * a.itemsize + 6
        raw = np.full((a.shape[0], pitch[k]), capi.DEVICE_FILL, np.uint8)
        raw[:, :a.shape[1] * a.itemsize] = np.ascontiguousarray(a).view(np.uint8).reshape(a.shape[0], -1)
        bufs.append(ex.L.m355_device_alloc(ex.mctx, raw.size))
        assert bufs[-1] and ex.L.m355_device_write(ex.mctx, bufs[-1], raw.ctypes.data, raw.size) == 0
        ref[k] = bufs[-1]
    out = capi.Msssim()
    r = (ctypes.c_int * 4)(*rect) if rect is not None else None
    rc = ex.glue.m355_glue_msssim_image(img, r, ref, pitch, select, levels, ctypes.byref(out))
    for p in bufs:
        ex.L.m355_device_free(ex.mctx, p)
    assert rc == 0
    return capi.msssim_list(out)


def test_msssim_of_images_equals_the_restatement_on_their_planes(emu_lib, monkeypatch):  # noqa: F811
    monkeypatch.setenv("M355_LIB", EMU_SO)
    glue = bind(glue_lib())
    earlier = []
    n, downloads = decode(glue, emu_lib, lambda ex, img, k: earlier.append(host_planes(glue, img)), max_pictures=PICTURES)
    assert n == PICTURES and downloads == PICTURES

    def check(ex, img, k):
        planes = earlier[k]
        geom = (planes[0].shape[1], planes[0].shape[0], 1, 8, 8)
        luma_levels, all_levels = mu.most_levels(geom[0], geom[1], 0), mu.most_levels(geom[0], geom[1], 1)
        assert luma_levels == mu.LEVELS and all_levels >= 3
        want = mu.expected(planes, planes, None, geom, planes=1, levels=luma_levels)
        assert want[0]["msssim"] == 1.0 and want[0]["sum_cs"] == [mu.ONE * v for v in want[0]["n"]]
        mu.assert_result(msssim(ex, img, planes, luma_levels, select=1), want, "picture %d: luma against itself" % k)
        mu.assert_result(msssim(ex, img, planes, all_levels), mu.expected(planes, planes, None, geom, levels=all_levels), "picture %d against its own planes" % k)
        if k == 3:
            other = su.perturbed(planes, (8, 8, 8), seed=9)
            want = mu.expected(planes, other, None, geom, levels=all_levels)
            assert all(0 < w["sum_cs"][j] < mu.ONE * w["n"][j] for w in want for j in range(all_levels))
            mu.assert_result(msssim(ex, img, other, all_levels), want, "picture %d against a perturbed copy" % k)
            want = mu.expected(planes, other, None, geom, planes=1, levels=luma_levels)
            assert 0 < want[0]["msssim"] < 1
            mu.assert_result(msssim(ex, img, other, luma_levels, select=1), want, "picture %d, luma on five levels" % k)
            rect = (6, 2, 50, 40)
            part = [p[1:21, 3:28] if c else p[2:42, 6:56] for c, p in enumerate(other)]
            mu.assert_result(msssim(ex, img, part, 2, rect, select=1), mu.expected(planes, part, rect, geom, planes=1, levels=2), "picture %d, rectangle, luma" % k)

    n, downloads = decode(glue, emu_lib, check, max_pictures=PICTURES)
    assert n == PICTURES and downloads == 0, "a picture that was only measured was brought back to the host"
    assert glue.m355_glue_cpu_pixel_calls() == 0, "the decoder called into its CPU pixel table"
