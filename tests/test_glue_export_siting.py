"""The chroma sample location type through the glue: m355_glue_image_chroma_loc and the _sited forms of the export calls.  CPU tier: the backend is
the SIMT-interpreter build (M355_LIB), as in test_glue_export_rgb.py; one case runs the product on the GPU.  A generated 8-bit 4:2:0 stream signals
nothing: the accessor gives 0, and chroma_loc = -1 equals an explicit 0 equals the plain call.  The stream generator cannot write a VUI, so the test
rewrites the stream's SPS to carry one whose only content is chroma_sample_loc_type_top_field = bottom_field = 2 (or 4): the decoder's own parser
reads it, the planes do not change, the accessor reports it, -1 exports what an explicit 2 exports and what the restatement of
export_siting_util.py gives, and a signalled 4 is rejected with nothing written."""
import ctypes

import numpy as np
import pytest

from export_rgb_util import M355_ERR_INVALID, assert_export, expected_rgb
from export_siting_util import expected_ints_sited, expected_rgb_sited
from export_tensor_util import assert_tensor, expected_tensor
from libde265_amd import capi
from test_emu_picture import emu_lib, EMU_SO  # noqa: F401  (fixture)
from test_glue_export import Exporter, bind, decode, host_planes
from test_glue_export_tensor import Tensor
from test_glue_live import glue_lib
from test_streams import make_stream

RECT = (6, 2, 50, 22)
W, H, FRAMES = 128, 64, 2
SPS_NUT = 33


# ---- the SPS rewrite ------------------------------------------------------------------------------------------------------------------------------

def split_nals(data):
    """an Annex B stream -> [(start code, NAL bytes)]"""
    marks, k = [], 0
    while True:
        k = data.find(b"\x00\x00\x01", k)
        if k < 0:
            break
        marks.append(k)
        k += 3
    out = []
    for n, k in enumerate(marks):
        end = len(data) if n + 1 == len(marks) else marks[n + 1]
        nal = data[k + 3:end]
        lead = b"\x00\x00\x01"
        if n + 1 < len(marks) and nal.endswith(b"\x00"):      # the zero_byte of the next four-byte start code
            nal = nal[:-1]
        if k > 0 and data[k - 1] == 0:
            lead = b"\x00\x00\x00\x01"
        out.append((lead, nal))
    return out


def unescape(b):
    out, zeros = bytearray(), 0
    for x in b:
        if zeros >= 2 and x == 3:
            zeros = 0
            continue
        out.append(x)
        zeros = zeros + 1 if x == 0 else 0
    return bytes(out)


def escape(b):
    out, zeros = bytearray(), 0
    for x in b:
        if zeros >= 2 and x <= 3:
            out.append(3)
            zeros = 0
        out.append(x)
        zeros = zeros + 1 if x == 0 else 0
    return bytes(out)


def ue(v):
    n = (v + 1).bit_length()
    return "0" * (n - 1) + format(v + 1, "b")


def with_chroma_loc(data, loc):
    """the stream with its SPS signalling chroma_sample_loc_type_top_field = bottom_field = loc in a VUI that holds nothing else"""
    out, seen = bytearray(), 0
    for lead, nal in split_nals(data):
        if (nal[0] >> 1) & 0x3F == SPS_NUT:
            seen += 1
            payload = unescape(nal[2:])
            bits = "".join(format(x, "08b") for x in payload)
            stop = bits.rindex("1")
            assert len(bits) - stop <= 8, "more than the alignment bits behind the stop bit"
            assert bits[stop - 2:stop] == "00", "the SPS has a VUI or an extension already"     # vui_parameters_present_flag, sps_extension_present_flag
            # aspect, overscan, video signal: absent; chroma loc: present, both fields; neutral chroma, field seq, frame field, default window, timing,
            # restriction: absent
            vui = "000" + "1" + ue(loc) + ue(loc) + "000000"
            bits = bits[:stop - 2] + "1" + vui + "0" + "1"
            bits += "0" * (-len(bits) % 8)
            payload = bytes(int(bits[k:k + 8], 2) for k in range(0, len(bits), 8))
            nal = nal[:2] + escape(payload)
        out += lead + nal
    assert seen >= 1, "no SPS in the stream"
    return bytes(out)


def test_the_rewrite_round_trips():
    """escape / unescape and the NAL split are inverse on bytes that need emulation prevention"""
    raw = bytes([0x42, 0x01, 0, 0, 0, 0, 1, 0, 0, 3, 0, 0, 2, 7, 0, 0])
    assert unescape(escape(raw)) == raw and b"\x00\x00\x01" not in escape(raw) and b"\x00\x00\x00" not in escape(raw)[:-2]
    stream = b"\x00\x00\x00\x01" + escape(raw)[:-2] + b"\x80" + b"\x00\x00\x01" + b"\x26\x01\x99"
    assert b"".join(a + b for a, b in split_nals(stream)) == stream
    assert [ue(v) for v in (0, 1, 2, 4)] == ["1", "010", "011", "00101"]


# ---- the glue calls -----------------------------------------------------------------------------------------------------------------------------

def bind_sited(glue):
    vp, i, f3, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_float), ctypes.c_int64
    pi, pv, p64 = ctypes.POINTER(i), ctypes.POINTER(vp), ctypes.POINTER(i64)
    glue.m355_glue_image_chroma_loc.argtypes, glue.m355_glue_image_chroma_loc.restype = [vp], i
    glue.m355_glue_export_image_rgb.argtypes = [vp, i, i, i, i, pi, pv, p64, vp]
    glue.m355_glue_export_image_rgb_sited.argtypes = [vp, i, i, i, i, pi, pv, p64, i, i, vp]
    glue.m355_glue_export_image_resized_sited.argtypes = [vp, i, i, pi, pi, pv, p64, i, i, vp]
    glue.m355_glue_export_image_resized_rgb_sited.argtypes = [vp, i, i, i, i, pi, pi, pv, p64, i, i, vp]
    glue.m355_glue_export_images_tensor_sited.argtypes = [pv, i, i, i, i, i, i, pi, pi, f3, f3, vp, i64, i64, i64, i, i, vp]
    glue.m355_glue_export_images_tensor_rois_sited.argtypes = [pv, ctypes.POINTER(i * 5), i, i, i, i, i, i, pi, f3, f3, vp, i64, i64, i64, i, i, vp]
    return bind(glue)


class _Call:
    """the glue library with m355_glue_export_image standing for one RGB call (what Exporter.export calls)"""

    def __init__(self, fn):
        self.m355_glue_export_image = fn


def rgb_through(ex, glue, img, rect, loc, plain=False):
    """the picture as packed 8-bit BT.709 limited R'G'B' through the _sited call with chroma_loc = loc, or through the plain call"""
    w, h = (W, H) if rect is None else rect[2:]

    def call(img, layout, samples, r, dst, pitch, stream):
        if plain:
            return glue.m355_glue_export_image_rgb(img, layout, samples, capi.MATRIX_BT709, 0, r, dst, pitch, stream)
        return glue.m355_glue_export_image_rgb_sited(img, layout, samples, capi.MATRIX_BT709, 0, r, dst, pitch, 0, loc, stream)

    sub = Exporter.__new__(Exporter)
    sub.glue, sub.L, sub.mctx = _Call(call), ex.L, ex.mctx
    return sub.export(img, capi.RGB_PACKED, capi.RGB_U8, rect, [(h, 3 * w, np.uint8)])


SCALE, BIAS = [1.0 / 255, 0.5 / 255, 2.0 / 255], [0.0, -1.0, 0.25]


def tensor_through(ex, glue, imgs, rect, loc, out_size=(64, 32)):
    t = Tensor(ex, len(imgs), capi.TENSOR_NCHW, capi.TENSOR_F16, out_size)
    r = (ctypes.c_int * 4)(*rect) if rect is not None else None
    rc = glue.m355_glue_export_images_tensor_sited((ctypes.c_void_p * len(imgs))(*imgs), len(imgs), t.layout, capi.TENSOR_F16, capi.RGB_U8, capi.MATRIX_BT709, 0, r,
                                                   (ctypes.c_int * 2)(*out_size), (ctypes.c_float * 3)(*SCALE), (ctypes.c_float * 3)(*BIAS), t.p, t.sn, t.sc, t.sh,
                                                   capi.FILTER_TRIANGLE, loc, None)
    return rc, t.finish()


def run_streams(glue, backend, tmp_path):
    """the generated stream, its rewrite signalling 2 and its rewrite signalling 4 through the glue"""
    data = make_stream(tmp_path, W, H, 8, 1, 1, FRAMES, 141, 10, 1, 1, 0, 1)
    planes = {}

    def plain_stream(ex, img, j):
        assert glue.m355_glue_image_chroma_loc(img) == 0
        first = rgb_through(ex, glue, img, None, -1)               # exported first: nothing has asked for the picture's samples
        host = planes[j] = host_planes(glue, img)
        assert host[0].shape == (H, W)
        want = expected_rgb(host, 1, 8, 8, capi.RGB_PACKED, capi.RGB_U8, capi.MATRIX_BT709, 0)
        assert_export(*first, want, "picture %d, as signalled (nothing)" % j)
        assert_export(*rgb_through(ex, glue, img, None, 0), want, "picture %d, explicit 0" % j)
        assert_export(*rgb_through(ex, glue, img, None, 0, plain=True), want, "picture %d, the plain call" % j)

    assert decode(glue, backend, plain_stream, data=data)[0] == FRAMES

    held = []

    def sited_stream(ex, img, j):
        assert glue.m355_glue_image_chroma_loc(img) == 2, "the decoder's parser did not read the rewritten VUI"
        signalled = rgb_through(ex, glue, img, None, -1)
        host = host_planes(glue, img)
        for a, b in zip(host, planes[j]):
            assert np.array_equal(a, b), "the rewritten stream decodes to other planes"
        for rect in (None, RECT):
            want = expected_rgb_sited(host, 8, 8, capi.RGB_PACKED, capi.RGB_U8, capi.MATRIX_BT709, 0, 2, rect)
            zero = expected_rgb(host, 1, 8, 8, capi.RGB_PACKED, capi.RGB_U8, capi.MATRIX_BT709, 0, rect)
            assert not np.array_equal(want[0], zero[0])
            assert_export(*(signalled if rect is None else rgb_through(ex, glue, img, rect, -1)), want, "picture %d rect %s, as signalled" % (j, rect))
            assert_export(*rgb_through(ex, glue, img, rect, 2), want, "picture %d rect %s, explicit 2" % (j, rect))
        held.append((img, host))
        if j == FRAMES - 1:
            imgs = [i for i, _ in held]
            for rect in (None, RECT):
                ints = []
                for _, hp in held:
                    ints.append(expected_ints_sited(hp, 8, capi.RGB_U8, capi.MATRIX_BT709, 0, (64, 32), 2, rect))
                want = expected_tensor(ints, capi.TENSOR_NCHW, capi.TENSOR_F16, SCALE, BIAS)
                for loc in (-1, 2):
                    rc, got = tensor_through(ex, glue, imgs, rect, loc)
                    assert rc == 0
                    assert_tensor(got, want, "tensor rect %s chroma_loc %d" % (rect, loc))

    assert decode(glue, backend, sited_stream, data=with_chroma_loc(data, 2))[0] == FRAMES

    def bottom_sited_stream(ex, img, j):
        assert glue.m355_glue_image_chroma_loc(img) == 4
        dst, pitch = (ctypes.c_void_p * 3)(), (ctypes.c_int64 * 3)()
        nbytes = H * 3 * W
        dst[0] = ex.L.m355_device_alloc(ex.mctx, nbytes)
        fill = np.full(nbytes, capi.DEVICE_FILL, np.uint8)
        assert dst[0] and ex.L.m355_device_write(ex.mctx, dst[0], fill.ctypes.data, nbytes) == 0
        pitch[0] = 3 * W
        args = (img, capi.RGB_PACKED, capi.RGB_U8, capi.MATRIX_BT709, 0, None, dst, pitch, 0)
        assert glue.m355_glue_export_image_rgb_sited(*args, -1, None) == M355_ERR_INVALID
        assert glue.m355_glue_export_image_rgb_sited(*args, 4, None) == M355_ERR_INVALID
        t = Tensor(ex, 1, capi.TENSOR_NCHW, capi.TENSOR_F16, (64, 32))
        rc = glue.m355_glue_export_images_tensor_sited((ctypes.c_void_p * 1)(img), 1, t.layout, capi.TENSOR_F16, capi.RGB_U8, capi.MATRIX_BT709, 0, None,
                                                       (ctypes.c_int * 2)(64, 32), (ctypes.c_float * 3)(*SCALE), (ctypes.c_float * 3)(*BIAS), t.p, t.sn, t.sc, t.sh,
                                                       capi.FILTER_TRIANGLE, -1, None)
        assert rc == M355_ERR_INVALID and np.all(t.finish()[1] == capi.DEVICE_FILL)
        back = np.zeros(nbytes, np.uint8)
        assert ex.L.m355_device_read(ex.mctx, dst[0], back.ctypes.data, nbytes) == 0
        ex.L.m355_device_free(ex.mctx, dst[0])
        assert np.all(back == capi.DEVICE_FILL), "a rejected export wrote to its destination"
        # the picture itself is fine: an explicit type leaves the stream's aside
        assert_export(*rgb_through(ex, glue, img, None, 0), expected_rgb(host_planes(glue, img), 1, 8, 8, capi.RGB_PACKED, capi.RGB_U8, capi.MATRIX_BT709, 0), "explicit 0")

    assert decode(glue, backend, bottom_sited_stream, data=with_chroma_loc(data, 4))[0] == FRAMES
    assert glue.m355_glue_cpu_pixel_calls() == 0, "the decoder called into its CPU pixel table"


def test_signalled_chroma_loc_through_the_glue(emu_lib, tmp_path, monkeypatch):  # noqa: F811
    monkeypatch.setenv("M355_LIB", EMU_SO)
    run_streams(bind_sited(glue_lib()), emu_lib, tmp_path)


def test_the_other_sited_glue_calls(emu_lib, tmp_path, monkeypatch):  # noqa: F811
    """m355_glue_export_image_resized_sited, _resized_rgb_sited and m355_glue_export_images_tensor_rois_sited with -1 on the stream that signals 2:
    what the backend delivers for the same frame with an explicit 2 through its own interface is pinned by the export tests; here -1 must equal 2
    and differ from 0"""
    monkeypatch.setenv("M355_LIB", EMU_SO)
    glue = bind_sited(glue_lib())
    data = with_chroma_loc(make_stream(tmp_path, W, H, 8, 1, 1, 1, 142, 10, 1, 1, 0, 1), 2)
    out_size = (ctypes.c_int * 2)(64, 32)

    def through(ex, fn, shapes):
        sub = Exporter.__new__(Exporter)
        sub.glue, sub.L, sub.mctx = _Call(fn), ex.L, ex.mctx
        return sub.export

    def check(ex, img, j):
        got = {}
        for loc in (-1, 2, 0):
            resized = lambda i, layout, samples, r, dst, pitch, s: glue.m355_glue_export_image_resized_sited(i, layout, samples, r, out_size, dst, pitch, 0, loc, s)  # noqa: E731
            rr = lambda i, layout, samples, r, dst, pitch, s: glue.m355_glue_export_image_resized_rgb_sited(i, layout, samples, -1, -1, r, out_size, dst, pitch, 0, loc, s)  # noqa: E731
            a = through(ex, resized, None)(img, capi.EXPORT_PLANAR, capi.EXPORT_NATIVE, None, [(32, 64, np.uint8), (16, 32, np.uint8), (16, 32, np.uint8)])
            b = through(ex, rr, None)(img, capi.RGB_PACKED, capi.RGB_U8, None, [(32, 3 * 64, np.uint8)])
            t = Tensor(ex, 2, capi.TENSOR_NHWC, capi.TENSOR_F32, (64, 32))
            rois = ((ctypes.c_int * 5) * 2)((ctypes.c_int * 5)(0, 0, 0, 0, 0), (ctypes.c_int * 5)(*RECT, capi.ROI_MIRROR))
            assert glue.m355_glue_export_images_tensor_rois_sited((ctypes.c_void_p * 2)(img, img), rois, 2, t.layout, capi.TENSOR_F32, capi.RGB_U8, -1, -1, out_size,
                                                                  (ctypes.c_float * 3)(*SCALE), (ctypes.c_float * 3)(*BIAS), t.p, t.sn, t.sc, t.sh, 0, loc, None) == 0
            got[loc] = (a, b, t.finish())
        host = host_planes(glue, img)
        want = expected_ints_sited(host, 8, capi.RGB_U8, capi.MATRIX_BT709, 0, (64, 32), 2)
        assert np.array_equal(got[2][1][0][0], np.stack(want, axis=-1).reshape(32, -1).astype(np.uint8)), "resized R'G'B', explicit 2, against the restatement"
        for k in range(2):
            for x, y in zip(got[-1][k][1], got[2][k][1]):
                assert np.array_equal(x, y), "call %d: -1 differs from the signalled 2" % k
            assert any(not np.array_equal(x, y) for x, y in zip(got[0][k][1], got[2][k][1])), "call %d: type 2 equals type 0" % k
        assert np.array_equal(got[-1][2][1], got[2][2][1]) and not np.array_equal(got[0][2][1], got[2][2][1])

    assert decode(glue, emu_lib, check, data=data)[0] == 1
    assert glue.m355_glue_cpu_pixel_calls() == 0


@pytest.mark.gpu
def test_signalled_chroma_loc_through_the_glue_gpu(tmp_path, monkeypatch):
    monkeypatch.delenv("M355_LIB", raising=False)
    run_streams(bind_sited(glue_lib()), capi.Library(), tmp_path)
