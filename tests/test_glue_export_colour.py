"""The colour transform through the glue: m355_glue_image_colour, m355_glue_colour_create / _destroy, m355_glue_colour_preset_for_image and the _colour
forms of the composed exports.  CPU tier: the backend is the SIMT-interpreter build (M355_LIB), as in test_glue_export_siting.py, whose NAL helpers are
imported; one case runs the product on the GPU.  A generated 8-bit stream signals nothing: the accessor gives 2 / 2 and the preset treats that as
BT.709.  The stream generator cannot write a VUI, so the SPS is rewritten to carry one with colour_description 9 / 16 / 9 and nothing else: the
decoder's own parser reads it, the planes do not change, the accessor reports 9 / 16, the preset for the image is m355_colour_preset of those values,
the _colour export is the restatement of export_colour_util.py, and the _sited call is the _colour call with 0."""
import ctypes

import numpy as np
import pytest

import export_colour_util as cu
from export_rgb_util import assert_export
from export_siting_util import expected_ints_sited
from export_tensor_util import assert_tensor, expected_tensor
from libde265_amd import capi
from test_emu_picture import emu_lib, EMU_SO  # noqa: F401  (fixture)
from test_glue_export import Exporter, host_planes
from test_glue_export_siting import SPS_NUT, _Call, bind_sited, escape, split_nals, unescape
from test_glue_export_tensor import Tensor
from test_glue_live import glue_lib
from test_streams import make_stream

W, H, FRAMES = 128, 64, 2
OUT = (96, 48)
RECT = (6, 2, 50, 22)
SCALE, BIAS = [1.0 / 255, 0.5 / 255, 2.0 / 255], [0.0, -1.0, 0.25]
OUT_ARGS = (1, 1, capi.TONE_REINHARD, 203, 1000)      # out_transfer, out_primaries, tone, white, peak


def with_colour_description(data, primaries, transfer, matrix):
    """the stream with its SPS signalling colour_description in a VUI that holds nothing else"""
    out, seen = bytearray(), 0
    for lead, nal in split_nals(data):
        if (nal[0] >> 1) & 0x3F == SPS_NUT:
            seen += 1
            bits = "".join(format(x, "08b") for x in unescape(nal[2:]))
            stop = bits.rindex("1")
            assert len(bits) - stop <= 8 and bits[stop - 2:stop] == "00", "the SPS has a VUI or an extension already"
            # aspect, overscan: absent; video signal: present — video_format 5, limited range, colour description; chroma loc, neutral chroma, field
            # seq, frame field, default window, timing, restriction: absent
            vui = "00" + "1" + "101" + "0" + "1" + format(primaries, "08b") + format(transfer, "08b") + format(matrix, "08b") + "0" + "000000"
            bits = bits[:stop - 2] + "1" + vui + "0" + "1"
            bits += "0" * (-len(bits) % 8)
            nal = nal[:2] + escape(bytes(int(bits[k:k + 8], 2) for k in range(0, len(bits), 8)))
        out += lead + nal
    assert seen >= 1, "no SPS in the stream"
    return bytes(out)


def bind_colour(glue):
    vp, i, f3, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_float), ctypes.c_int64
    pi, pv, p64, pt = ctypes.POINTER(i), ctypes.POINTER(vp), ctypes.POINTER(i64), ctypes.POINTER(capi.ColourTables)
    glue.m355_glue_image_colour.argtypes = [vp, pi, pi]
    glue.m355_glue_colour_create.argtypes = [vp, pt, pi]
    glue.m355_glue_colour_destroy.argtypes = [vp, i]
    glue.m355_glue_colour_preset_for_image.argtypes = [vp, i, i, i, i, i, pt]
    glue.m355_glue_export_image_resized_rgb_colour.argtypes = [vp, i, i, i, i, pi, pi, pv, p64, i, i, i, vp]
    glue.m355_glue_export_images_tensor_colour.argtypes = [pv, i, i, i, i, i, i, pi, pi, f3, f3, vp, i64, i64, i64, i, i, i, vp]
    glue.m355_glue_export_images_tensor_rois_colour.argtypes = [pv, ctypes.POINTER(i * 5), i, i, i, i, i, i, pi, f3, f3, vp, i64, i64, i64, i, i, i, vp]
    return bind_sited(glue)


def decode(glue, backend, per_picture, data):
    """test_glue_export.decode with the decoder handed to per_picture(exporter, decoder, img, index), which the colour objects belong to"""
    dec = glue.de265_new_decoder()
    assert dec
    try:
        assert glue.de265_start_worker_threads(dec, 2) == 0
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
                per_picture(ex, dec, img, n)
                n += 1
        return n
    finally:
        glue.de265_free_decoder(dec)


def signalled(glue, img):
    p, t = ctypes.c_int(-1), ctypes.c_int(-1)
    assert glue.m355_glue_image_colour(img, ctypes.byref(p), ctypes.byref(t)) == 0
    return p.value, t.value


def preset_for(glue, img):
    t = capi.ColourTables()
    assert glue.m355_glue_colour_preset_for_image(img, *OUT_ARGS, ctypes.byref(t)) == 0
    return t


def rr_through(ex, glue, img, rect, colour, sited=False, samples=capi.RGB_U8):
    """the picture resized to OUT as packed R'G'B' (matrix and range as signalled, chroma_loc 0) through the _colour call, or through the _sited call"""
    out_size = (ctypes.c_int * 2)(*OUT)

    def call(i, layout, smp, r, dst, pitch, stream):
        if sited:
            return glue.m355_glue_export_image_resized_rgb_sited(i, layout, smp, -1, -1, r, out_size, dst, pitch, 0, 0, stream)
        return glue.m355_glue_export_image_resized_rgb_colour(i, layout, smp, -1, -1, r, out_size, dst, pitch, 0, 0, colour, stream)

    sub = Exporter.__new__(Exporter)
    sub.glue, sub.L, sub.mctx = _Call(call), ex.L, ex.mctx
    return sub.export(img, capi.RGB_PACKED, samples, rect, [(OUT[1], 3 * OUT[0], np.uint16 if samples == capi.RGB_U16 else np.uint8)])


def run_streams(glue, backend, tmp_path):
    data = make_stream(tmp_path, W, H, 8, 1, 1, FRAMES, 143, 10, 1, 1, 0, 1)
    planes = {}

    def plain_stream(ex, dec, img, j):
        assert signalled(glue, img) == (2, 2)
        assert bytes(preset_for(glue, img)) == bytes(backend.colour_preset(2, 2, *OUT_ARGS)) == bytes(backend.colour_preset(1, 1, *OUT_ARGS))
        planes[j] = host_planes(glue, img)

    assert decode(glue, backend, plain_stream, data) == FRAMES
    held = []

    def hdr_stream(ex, dec, img, j):
        assert signalled(glue, img) == (9, 16), "the decoder's parser did not read the rewritten VUI"
        t = preset_for(glue, img)
        assert bytes(t) == bytes(backend.colour_preset(16, 9, *OUT_ARGS))
        T = cu.from_ctypes(t)
        h = ctypes.c_int(0)
        assert glue.m355_glue_colour_create(dec, ctypes.byref(t), ctypes.byref(h)) == 0 and h.value >= 0x100
        first = rr_through(ex, glue, img, None, h.value)            # exported first: nothing has asked for the picture's samples
        host = host_planes(glue, img)
        for a, b in zip(host, planes[j]):
            assert np.array_equal(a, b), "the rewritten stream decodes to other planes"
        for rect in (None, RECT):
            for samples in (capi.RGB_U8, capi.RGB_U16):
                ints = [c.astype(np.int64) for c in expected_ints_sited(host, 8, capi.RGB_U16, capi.MATRIX_BT2020, 0, OUT, 0, rect)]     # matrix_coeffs 9
                want = cu.shape_rgb(cu.colour_pixels(T, ints, samples), capi.RGB_PACKED, samples)
                got = first if rect is None and samples == capi.RGB_U8 else rr_through(ex, glue, img, rect, h.value, samples=samples)
                assert_export(*got, want, "picture %d rect %s samples %d" % (j, rect, samples))
            a, b = rr_through(ex, glue, img, rect, 0), rr_through(ex, glue, img, rect, 0, sited=True)
            assert np.array_equal(a[1][0], b[1][0]), "the _sited call is not the _colour call with 0"
            plain = cu.shape_rgb(expected_ints_sited(host, 8, capi.RGB_U8, capi.MATRIX_BT2020, 0, OUT, 0, rect), capi.RGB_PACKED, capi.RGB_U8)
            assert_export(*a, plain, "picture %d rect %s, colour 0" % (j, rect))
        held.append((img, host))
        if j == FRAMES - 1:
            imgs = [i for i, _ in held]
            ints = [cu.colour_pixels(T, [c.astype(np.int64) for c in expected_ints_sited(hp, 8, capi.RGB_U16, capi.MATRIX_BT2020, 0, (64, 32), 0)], capi.RGB_U8)
                    for _, hp in held]
            want = expected_tensor(ints, capi.TENSOR_NCHW, capi.TENSOR_F16, SCALE, BIAS)
            for sited in (False, True):
                t16 = Tensor(ex, len(imgs), capi.TENSOR_NCHW, capi.TENSOR_F16, (64, 32))
                args = ((ctypes.c_void_p * len(imgs))(*imgs), len(imgs), t16.layout, capi.TENSOR_F16, capi.RGB_U8, -1, -1, None, (ctypes.c_int * 2)(64, 32),
                        (ctypes.c_float * 3)(*SCALE), (ctypes.c_float * 3)(*BIAS), t16.p, t16.sn, t16.sc, t16.sh, capi.FILTER_TRIANGLE, 0)
                if sited:
                    assert glue.m355_glue_export_images_tensor_sited(*args, None) == 0
                    assert not np.array_equal(t16.finish()[0], want)
                else:
                    assert glue.m355_glue_export_images_tensor_colour(*args, h.value, None) == 0
                    assert_tensor(t16.finish(), want, "tensor")
            rois = ((ctypes.c_int * 5) * 2)((ctypes.c_int * 5)(0, 0, 0, 0, 0), (ctypes.c_int * 5)(*RECT, capi.ROI_MIRROR))
            tr = Tensor(ex, 2, capi.TENSOR_NCHW, capi.TENSOR_F16, (64, 32))
            assert glue.m355_glue_export_images_tensor_rois_colour((ctypes.c_void_p * 2)(imgs[0], imgs[0]), rois, 2, tr.layout, capi.TENSOR_F16, capi.RGB_U8, -1, -1,
                                                                   (ctypes.c_int * 2)(64, 32), (ctypes.c_float * 3)(*SCALE), (ctypes.c_float * 3)(*BIAS), tr.p, tr.sn,
                                                                   tr.sc, tr.sh, capi.FILTER_TRIANGLE, 0, h.value, None) == 0
            host0 = held[0][1]
            mirrored = cu.colour_pixels(T, [c.astype(np.int64) for c in expected_ints_sited(host0, 8, capi.RGB_U16, capi.MATRIX_BT2020, 0, (64, 32), 0, RECT)], capi.RGB_U8)
            want_rois = np.stack([want[0], expected_tensor([mirrored], capi.TENSOR_NCHW, capi.TENSOR_F16, SCALE, BIAS)[0][:, :, ::-1]])
            assert_tensor(tr.finish(), want_rois, "rois")
        assert glue.m355_glue_colour_destroy(dec, h.value) == 0
        assert glue.m355_glue_colour_destroy(dec, h.value) == cu.M355_ERR_INVALID
        assert glue.m355_glue_colour_create(None, ctypes.byref(t), ctypes.byref(h)) == cu.M355_ERR_INVALID

    assert decode(glue, backend, hdr_stream, with_colour_description(data, 9, 16, 9)) == FRAMES
    assert glue.m355_glue_cpu_pixel_calls() == 0, "the decoder called into its CPU pixel table"


def test_signalled_colour_through_the_glue(emu_lib, tmp_path, monkeypatch):  # noqa: F811
    monkeypatch.setenv("M355_LIB", EMU_SO)
    run_streams(bind_colour(glue_lib()), emu_lib, tmp_path)


@pytest.mark.gpu
def test_signalled_colour_through_the_glue_gpu(tmp_path, monkeypatch):
    monkeypatch.delenv("M355_LIB", raising=False)
    run_streams(bind_colour(glue_lib()), capi.Library(), tmp_path)
