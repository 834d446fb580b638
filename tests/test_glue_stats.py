"""m355_glue_stats_image and m355_glue_image_content_peak: what is in a decoded picture of the reference-API decoder (glue/_build/libde265.so), measured
on the DEVICE without a download.  CPU tier: the backend is the SIMT-interpreter build (M355_LIB), as in test_glue_measure.py.  Every output picture
of girlshy.h265: the statistics equal the numpy statistics (tests/stats_util.py) of the planes de265_get_image_plane returned in an earlier run, in a
run that only measures and therefore downloads nothing; the decoder's CPU pixel table is never called.  One generated stream with a non-empty
conformance window pins the NULL rectangle.  One generated stream rewritten to signal PQ / BT.2020 (test_glue_export_colour.py) pins that -1 resolves
to what is signalled, the content peak against its restatement from the numpy light histogram, and the preset built with that peak."""
import ctypes

import numpy as np

import stats_util as su
from libde265_amd import capi
from test_emu_picture import emu_lib, EMU_SO  # noqa: F401  (fixture)
from test_glue_export import bind as bind_export, decode, host_planes
from test_glue_export_colour import bind_colour, with_colour_description
from test_glue_live import glue_lib
from test_streams import G_CONFWIN, make_stream

INVALID = 3


def bind(glue):
    vp, i, u = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32
    glue.m355_glue_stats_image.argtypes = [vp, ctypes.POINTER(i), i, i, i, i, i, ctypes.POINTER(capi.Stats)]
    glue.m355_glue_image_content_peak.argtypes = [vp, ctypes.POINTER(capi.Stats), u, u, i, ctypes.POINTER(i)]
    bind_colour(glue)
    return bind_export(glue)


def stats(glue, img, rect=None, black=0, light=0, matrix=0, full_range=0, chroma_loc=0, raw=False):
    out = capi.Stats()
    r = (ctypes.c_int * 4)(*rect) if rect is not None else None
    assert glue.m355_glue_stats_image(img, r, black, light, matrix, full_range, chroma_loc, ctypes.byref(out)) == 0
    d = capi.stats_dict(out, 1 if glue.de265_get_chroma_format(img) == 0 else 3, bool(light))
    return (d, out) if raw else d


def test_statistics_equal_an_earlier_runs_planes(emu_lib, monkeypatch):  # noqa: F811
    monkeypatch.setenv("M355_LIB", EMU_SO)
    glue = bind(glue_lib())
    earlier = []
    n, downloads = decode(glue, emu_lib, lambda ex, img, k: earlier.append(host_planes(glue, img)))
    assert n == 75 and downloads == 75

    def check(ex, img, k):
        planes = earlier[k]
        geom = (planes[0].shape[1], planes[0].shape[0], 1, 8, 8)
        su.assert_stats(stats(glue, img, black=16 + k), su.expected(planes, geom, black=16 + k), "picture %d" % k)
        if k == 3:
            light = (capi.MATRIX_BT601, 1, 1)
            su.assert_stats(stats(glue, img, su.RECT, 40, 1, *light), su.expected(planes, geom, su.RECT, 40, light), "picture %d, rectangle, light" % k)

    n, downloads = decode(glue, emu_lib, check)
    assert n == 75 and downloads == 0, "a picture that was only measured was brought back to the host"
    assert glue.m355_glue_cpu_pixel_calls() == 0, "the decoder called into its CPU pixel table"


def test_null_rectangle_is_the_conformance_window(emu_lib, tmp_path, monkeypatch):  # noqa: F811
    monkeypatch.setenv("M355_LIB", EMU_SO)
    glue = bind(glue_lib())
    w, h, frames = 256, 128, 3
    data = make_stream(tmp_path, w, h, 8, 1, 1, frames, 116, 10, 1, 1, 0, 1, 1, G_CONFWIN)
    offsets = set()

    def check(ex, img, k):
        got = stats(glue, img, black=90)
        want_planes = host_planes(glue, img)                        # (the window: what de265.h describes for the image)
        ww, wh = want_planes[0].shape[1], want_planes[0].shape[0]
        assert (ww, wh) != (w, h), "the stream has no conformance window"
        want = su.expected(want_planes, (ww, wh, 1, 8, 8), black=90)
        assert want["box"] is not None and got["box"] is not None
        # the box is in coordinates of the coded frame: the window's offset away from the window's own
        off = (got["box"][0] - want["box"][0], got["box"][1] - want["box"][1])
        assert off != (0, 0) and off[0] >= 0 and off[1] >= 0 and off[0] + ww <= w and off[1] + wh <= h
        offsets.add(off)
        su.assert_stats(dict(got, box=tuple(v - off[i % 2] for i, v in enumerate(got["box"]))), want, "picture %d" % k)

    n, _ = decode(glue, emu_lib, check, data=data)
    assert n == frames and len(offsets) == 1
    assert glue.m355_glue_cpu_pixel_calls() == 0


def content_peak(backend, light_hist, transfer, primaries, num, den, white=203):
    """the definition of m355_glue_image_content_peak from a light histogram"""
    total, run, b = sum(light_hist), 0, 0
    for b, v in enumerate(light_hist):
        run += v
        if den * run >= num * total:
            break
    v = min(65535, (b << 8) | 255)
    lut_in = list(backend.colour_preset(transfer, primaries, 1, 1).lut_in)
    k, f = v >> 6, v & 63
    L = (lut_in[k] * (64 - f) + lut_in[k + 1] * f + 32) >> 6
    S = 10000 if transfer == 16 else (1000 if transfer == 18 else white)
    return max(white, (L * S + capi.COLOUR_ONE - 1) >> 24)


def test_content_peak_of_a_pq_stream(emu_lib, tmp_path, monkeypatch):  # noqa: F811
    monkeypatch.setenv("M355_LIB", EMU_SO)
    glue = bind(glue_lib())
    W, H, frames = 128, 64, 2
    data = with_colour_description(make_stream(tmp_path, W, H, 8, 1, 1, frames, 143, 10, 1, 1, 0, 1), 9, 16, 9)
    peaks = []

    def check(ex, img, k):
        got, raw = stats(glue, img, None, 16, 1, -1, -1, -1, raw=True)     # measured first: nothing has asked for the picture's samples
        planes = host_planes(glue, img)
        geom = (W, H, 1, 8, 8)
        signalled = (capi.MATRIX_BT2020, 0, 0)                      # matrix_coeffs 9, limited range, no chroma_loc_info
        want = su.expected(planes, geom, None, 16, signalled)
        assert want["light"] != su.expected(planes, geom, None, 16, (capi.MATRIX_BT709, 0, 0))["light"]
        su.assert_stats(got, want, "picture %d, as signalled" % k)
        su.assert_stats(stats(glue, img, None, 16, 1, *signalled), want, "picture %d, explicit" % k)
        peak = ctypes.c_int(0)
        assert glue.m355_glue_image_content_peak(img, ctypes.byref(raw), 999, 1000, 0, ctypes.byref(peak)) == 0
        assert peak.value == content_peak(emu_lib, want["light"]["hist"], 16, 9, 999, 1000)
        assert 203 <= peak.value <= 10000
        peaks.append(peak.value)
        t, default = capi.ColourTables(), capi.ColourTables()
        assert glue.m355_glue_colour_preset_for_image(img, 1, 1, capi.TONE_REINHARD, 0, peak.value, ctypes.byref(t)) == 0
        assert glue.m355_glue_colour_preset_for_image(img, 1, 1, capi.TONE_REINHARD, 0, 0, ctypes.byref(default)) == 0
        assert bytes(t) == bytes(emu_lib.colour_preset(16, 9, 1, 1, capi.TONE_REINHARD, 0, peak.value))
        if peak.value < 10000:
            assert list(t.lut_out) != list(default.lut_out), "the measured peak changes nothing"
        assert list(t.lut_in) == list(default.lut_in)
        # a lower quantile cannot give a higher peak; statistics without the light level have none
        lower = ctypes.c_int(0)
        assert glue.m355_glue_image_content_peak(img, ctypes.byref(raw), 1, 2, 0, ctypes.byref(lower)) == 0 and lower.value <= peak.value
        _, planes_only = stats(glue, img, raw=True)
        assert glue.m355_glue_image_content_peak(img, ctypes.byref(planes_only), 999, 1000, 0, ctypes.byref(lower)) == INVALID
        assert glue.m355_glue_image_content_peak(img, ctypes.byref(raw), 0, 1000, 0, ctypes.byref(lower)) == INVALID
        assert glue.m355_glue_image_content_peak(img, ctypes.byref(raw), 999, 1000, 0, None) == INVALID

    n, _ = decode(glue, emu_lib, check, data=data)
    assert n == frames
    assert any(p < 10000 for p in peaks), "no picture of the stream has a content peak below the transfer's own"
    assert glue.m355_glue_cpu_pixel_calls() == 0
