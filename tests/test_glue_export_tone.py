"""Tone objects through the glue: m355_glue_colour_create_tone and m355_glue_colour_preset_tone_for_image on a generated stream whose SPS is rewritten
to signal BT.2020 / PQ (test_glue_export_colour.py's helpers, imported).  The preset for the image is the backend's m355_colour_preset_tone of the
signalled values, byte for byte; the handle goes through the existing _colour export calls as it is and delivers the restatement of
export_tone_util.py; m355_glue_colour_destroy destroys it.  CPU tier: the backend is the SIMT-interpreter build (M355_LIB); one case runs the product
on the GPU."""
import ctypes

import numpy as np
import pytest

import export_tone_util as tu
from export_rgb_util import assert_export
from export_siting_util import expected_ints_sited
from export_tensor_util import assert_tensor, expected_tensor
from libde265_amd import capi
from test_emu_picture import emu_lib, EMU_SO  # noqa: F401  (fixture)
from test_glue_export_colour import BIAS, FRAMES, H, OUT, RECT, SCALE, W, bind_colour, decode, rr_through, signalled, with_colour_description
from test_glue_export_tensor import Tensor
from test_glue_live import glue_lib
from test_streams import make_stream

OUT_ARGS = (1, 1, capi.TONE_BT2390, capi.NORM_MAXRGB, 203, 1000)      # out_transfer, out_primaries, tone, norm, white, peak


def bind_tone(glue):
    vp, i = ctypes.c_void_p, ctypes.c_int
    pt, pq = ctypes.POINTER(capi.ColourTables), ctypes.POINTER(capi.ColourTone)
    glue.m355_glue_colour_create_tone.argtypes = [vp, pt, pq, ctypes.POINTER(i)]
    glue.m355_glue_colour_preset_tone_for_image.argtypes = [vp, i, i, i, i, i, i, pt, pq]
    return bind_colour(glue)


def run_streams(glue, backend, tmp_path):
    data = with_colour_description(make_stream(tmp_path, W, H, 8, 1, 1, FRAMES, 143, 10, 1, 1, 0, 1), 9, 16, 9)
    held = []

    def per_picture(ex, dec, img, j):
        assert signalled(glue, img) == (9, 16)
        t, q, h = capi.ColourTables(), capi.ColourTone(), ctypes.c_int(0)
        ref = ctypes.byref
        assert glue.m355_glue_colour_preset_tone_for_image(img, *OUT_ARGS, ref(t), ref(q)) == 0
        bt, bq = backend.colour_preset_tone(16, 9, 1, 1, tone=capi.TONE_BT2390, norm=capi.NORM_MAXRGB, white_nits=203, peak_nits=1000)
        assert bytes(t) == bytes(bt) and bytes(q) == bytes(bq), "the preset for the image is not the backend's"
        for norm in (capi.NORM_LUMA, 2):
            args = OUT_ARGS[:3] + (norm,) + OUT_ARGS[4:]
            tl, ql = capi.ColourTables(), capi.ColourTone()
            rc = glue.m355_glue_colour_preset_tone_for_image(img, *args, ref(tl), ref(ql))
            assert rc == (0 if norm == capi.NORM_LUMA else tu.M355_ERR_INVALID)
            if rc == 0:
                assert bytes(ql) == bytes(backend.colour_preset_tone(16, 9, 1, 1, tone=capi.TONE_BT2390, norm=norm, white_nits=203, peak_nits=1000)[1])
        assert glue.m355_glue_colour_preset_tone_for_image(None, *OUT_ARGS, ref(t), ref(q)) == tu.M355_ERR_INVALID
        S = tu.from_ctypes(t, q)
        assert glue.m355_glue_colour_create_tone(dec, ref(t), ref(q), ref(h)) == 0 and h.value >= 0x100
        from test_glue_export import host_planes
        host = None
        for rect in (None, RECT):
            for samples in (capi.RGB_U8, capi.RGB_U16):
                got = rr_through(ex, glue, img, rect, h.value, samples=samples)
                host = host if host is not None else host_planes(glue, img)
                ints = [c.astype(np.int64) for c in expected_ints_sited(host, 8, capi.RGB_U16, capi.MATRIX_BT2020, 0, OUT, 0, rect)]     # matrix_coeffs 9
                assert_export(*got, tu.shape_rgb(tu.pixels(S, ints, samples), capi.RGB_PACKED, samples), "picture %d rect %s samples %d" % (j, rect, samples))
        held.append((img, host))
        if j == FRAMES - 1:
            imgs = [i for i, _ in held]
            ints = [tu.pixels(S, [c.astype(np.int64) for c in expected_ints_sited(hp, 8, capi.RGB_U16, capi.MATRIX_BT2020, 0, (64, 32), 0)], capi.RGB_U8) for _, hp in held]
            want = expected_tensor(ints, capi.TENSOR_NCHW, capi.TENSOR_F16, SCALE, BIAS)
            t16 = Tensor(ex, len(imgs), capi.TENSOR_NCHW, capi.TENSOR_F16, (64, 32))
            assert glue.m355_glue_export_images_tensor_colour((ctypes.c_void_p * len(imgs))(*imgs), len(imgs), t16.layout, capi.TENSOR_F16, capi.RGB_U8, -1, -1, None,
                                                              (ctypes.c_int * 2)(64, 32), (ctypes.c_float * 3)(*SCALE), (ctypes.c_float * 3)(*BIAS), t16.p, t16.sn, t16.sc,
                                                              t16.sh, capi.FILTER_TRIANGLE, 0, h.value, None) == 0
            assert_tensor(t16.finish(), want, "tensor")
            rois = ((ctypes.c_int * 5) * 2)((ctypes.c_int * 5)(0, 0, 0, 0, 0), (ctypes.c_int * 5)(*RECT, capi.ROI_MIRROR))
            tr = Tensor(ex, 2, capi.TENSOR_NCHW, capi.TENSOR_F16, (64, 32))
            assert glue.m355_glue_export_images_tensor_rois_colour((ctypes.c_void_p * 2)(imgs[0], imgs[0]), rois, 2, tr.layout, capi.TENSOR_F16, capi.RGB_U8, -1, -1,
                                                                   (ctypes.c_int * 2)(64, 32), (ctypes.c_float * 3)(*SCALE), (ctypes.c_float * 3)(*BIAS), tr.p, tr.sn,
                                                                   tr.sc, tr.sh, capi.FILTER_TRIANGLE, 0, h.value, None) == 0
            mirrored = tu.pixels(S, [c.astype(np.int64) for c in expected_ints_sited(held[0][1], 8, capi.RGB_U16, capi.MATRIX_BT2020, 0, (64, 32), 0, RECT)], capi.RGB_U8)
            want_rois = np.stack([want[0], expected_tensor([mirrored], capi.TENSOR_NCHW, capi.TENSOR_F16, SCALE, BIAS)[0][:, :, ::-1]])
            assert_tensor(tr.finish(), want_rois, "rois")
        q.gain[3] = capi.TONE_GAIN_ONE + 1
        assert glue.m355_glue_colour_create_tone(dec, ref(t), ref(q), ref(h)) == tu.M355_ERR_INVALID and h.value >= 0x100
        assert glue.m355_glue_colour_create_tone(dec, ref(t), None, ref(h)) == tu.M355_ERR_INVALID
        assert glue.m355_glue_colour_create_tone(None, ref(t), ref(q), ref(h)) == tu.M355_ERR_INVALID
        assert glue.m355_glue_colour_destroy(dec, h.value) == 0
        assert glue.m355_glue_colour_destroy(dec, h.value) == tu.M355_ERR_INVALID

    assert decode(glue, backend, per_picture, data) == FRAMES
    assert glue.m355_glue_cpu_pixel_calls() == 0, "the decoder called into its CPU pixel table"


def test_tone_objects_through_the_glue(emu_lib, tmp_path, monkeypatch):  # noqa: F811
    monkeypatch.setenv("M355_LIB", EMU_SO)
    run_streams(bind_tone(glue_lib()), emu_lib, tmp_path)


@pytest.mark.gpu
def test_tone_objects_through_the_glue_gpu(tmp_path, monkeypatch):
    monkeypatch.delenv("M355_LIB", raising=False)
    run_streams(bind_tone(glue_lib()), capi.Library(), tmp_path)
