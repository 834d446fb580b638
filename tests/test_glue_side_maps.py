"""m355_glue_set_side_maps / m355_glue_image_side_maps / m355_glue_image_side_maps_host: how the pictures of the reference-API decoder
(glue/_build/libde265.so) were coded, as dense maps on the DEVICE, against the INDEPENDENT statement of the same maps from the reference's own
per-picture arrays (get_pred_mode, get_QPY, get_mv_info, refIdx -> POC -> slot ...), byte for byte, for every output picture at units of 4 and 16
samples: girlshy.h265, a P/B stream with 2x2 tiles, 16x16 CTBs and coding blocks of at least 16x16, one with three slices and parallel merge
level 4, and the first random-access stream (four references per list, a long-term picture).  The one thing the arrays cannot say — the FILL bits of
a prediction block's flags, DESIGN.md section 5 — is masked out of MAP_REF's third byte.  A run that only maps downloads nothing and never calls the
decoder's CPU pixel table.  CPU tier: the backend is the SIMT-interpreter build (M355_LIB); a gpu-marked twin runs one generated stream on the product
library."""
import ctypes

import numpy as np
import pytest

import de265_py
from libde265_amd import capi
from test_emu_picture import emu_lib, EMU_SO  # noqa: F401  (fixture)
from test_glue_live import STREAM, glue_lib
from test_streams import G_CTB16, G_MINCB16, G_PARMERGE, RA_CPU_CASES, make_stream

INVALID = 3
ALL_MAPS = (1 << capi.N_MAPS) - 1
FILL_BITS = 0x60                      # M355_PBF_FILL_L0 | M355_PBF_FILL_L1


class GlueSideMaps(ctypes.Structure):
    """m355_glue_side_maps (glue/m355_glue.cc)"""
    _fields_ = [("dst", ctypes.c_void_p * capi.N_MAPS), ("pitch", ctypes.c_int64 * capi.N_MAPS), ("log2_unit", ctypes.c_int32), ("units_w", ctypes.c_int32),
                ("units_h", ctypes.c_int32), ("ref_valid", ctypes.c_uint32), ("ref_poc", ctypes.c_int32 * 32), ("info", capi.MapsInfo)]


def bind(glue):
    vp, i, u = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint
    glue.m355_glue_set_side_maps.argtypes = [vp, u, i]
    glue.m355_glue_image_side_maps.argtypes = [vp, i, ctypes.POINTER(GlueSideMaps)]
    glue.m355_glue_image_side_maps_host.argtypes = [vp, u, i, ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_int64)]
    glue.m355_glue_backend_context.argtypes = [vp]
    glue.m355_glue_backend_context.restype = vp
    glue.m355_glue_stats.argtypes = [vp] + [ctypes.POINTER(ctypes.c_longlong)] * 3
    return de265_py.bind(glue)


def run(glue, backend, data, log2_unit, per_picture, threads=2, mask=ALL_MAPS):
    """the stream through a decoder with side maps on; per_picture(mctx, img, index) for every output picture -> (pictures, downloads)"""
    dec = glue.de265_new_decoder()
    assert dec
    try:
        assert glue.m355_glue_set_side_maps(dec, mask, log2_unit) == 0
        assert glue.de265_start_worker_threads(dec, threads) == 0
        buf = ctypes.create_string_buffer(data, len(data))
        assert glue.de265_push_data(dec, buf, len(data), 0, None) == 0 and glue.de265_flush_data(dec) == 0
        mctx = glue.m355_glue_backend_context(dec)
        n, more = 0, ctypes.c_int(1)
        while more.value:
            more.value = 0
            assert glue.de265_decode(dec, ctypes.byref(more)) == 0
            while True:
                img = glue.de265_get_next_picture(dec)
                if not img:
                    break
                per_picture(mctx, img, n)
                n += 1
        stats = [ctypes.c_longlong() for _ in range(3)]
        assert glue.m355_glue_stats(dec, *[ctypes.byref(s) for s in stats]) == 0
        return n, stats[2].value
    finally:
        glue.de265_free_decoder(dec)


def compare(glue, backend, log2_unit, seen):
    """-> per_picture: the device maps (m355_device_read) against m355_glue_image_side_maps_host, byte for byte"""
    L = backend.lib

    def check(mctx, img, k):
        out = GlueSideMaps()
        assert glue.m355_glue_image_side_maps(img, 1, ctypes.byref(out)) == 0, "picture %d" % k
        uw, uh = out.units_w, out.units_h
        assert out.log2_unit == log2_unit and uw * uh > 0
        info = out.info
        assert info.units_w == uw and info.units_h == uh
        assert info.n_intra + info.n_inter + info.n_skip == uw * uh == info.covered, "picture %d: the coding units cover every unit" % k
        assert list(info.skipped) == [0, 0, 0, 0]
        dst, pitch, host = (ctypes.c_void_p * capi.N_MAPS)(), (ctypes.c_int64 * capi.N_MAPS)(), []
        for m in range(capi.N_MAPS):
            assert out.dst[m] and out.pitch[m] == uw * capi.MAP_ELEM_BYTES[m]
            host.append(np.full(uh * out.pitch[m], 0xA5, np.uint8))
            dst[m], pitch[m] = host[m].ctypes.data, out.pitch[m]
        assert glue.m355_glue_image_side_maps_host(img, ALL_MAPS, log2_unit, dst, pitch) == 0
        bipred = 0
        for m in range(capi.N_MAPS):
            dev = np.zeros(host[m].size, np.uint8)
            assert L.m355_device_read(mctx, out.dst[m], dev.ctypes.data, dev.size) == 0
            want = host[m]
            if m == capi.MAP_REF:
                dev = dev.copy()
                dev[2::4] &= 0xFF ^ FILL_BITS               # (in no array of the reference: DESIGN.md section 5)
                bipred = int(((dev[2::4] & 3) == 3).sum())
                seen["slots"] |= set(dev[0::4][dev[0::4] != 255].tolist()) | set(dev[1::4][dev[1::4] != 255].tolist())
                seen["inter"] += int((dev[2::4] != 0).sum())
                valid = [s for s in range(32) if (out.ref_valid >> s) & 1]
                assert all(s in valid for s in set(dev[0::4].tolist()) | set(dev[1::4].tolist()) if s != 255), "a slot outside the table"
            if m == capi.MAP_INTRA:
                seen["intra"] += int((dev != 255).sum())
            if not np.array_equal(dev, want):
                d = np.flatnonzero(dev != want)
                es = capi.MAP_ELEM_BYTES[m]
                u = int(d[0]) // es
                raise AssertionError("picture %d, map %s: %d bytes differ, first in unit (%d, %d): device %s, reference's arrays %s" % (
                    k, capi.MAP_NAMES[m], len(d), u % uw, u // uw, dev[u * es:(u + 1) * es].tolist(), want[u * es:(u + 1) * es].tolist()))
        assert info.n_bipred == bipred
        seen["pictures"] += 1

    return check


def streams(tmp_path):
    ra = RA_CPU_CASES[0]
    return {
        "girlshy": lambda: open(STREAM, "rb").read(),
        "tiles_ctb16_mincb16": lambda: make_stream(tmp_path, 256, 128, 8, 2, 2, 5, 151, 10, 1, 1, 0, 1, 1, G_CTB16 | G_MINCB16),
        "slices3_parmerge": lambda: make_stream(tmp_path, 256, 128, 8, 1, 1, 5, 152, 10, 1, 1, 0, 1, 3, G_PARMERGE),
        "random_access": lambda: make_stream(tmp_path, ra[0], ra[1], ra[2], 1, 1, ra[3], ra[4], 5, 1, 1, ra[5]),
    }


@pytest.mark.parametrize("log2_unit", [2, 4])
@pytest.mark.parametrize("name", ["girlshy", "tiles_ctb16_mincb16", "slices3_parmerge", "random_access"])
def test_device_maps_equal_the_references_arrays(emu_lib, tmp_path, monkeypatch, name, log2_unit):  # noqa: F811
    monkeypatch.setenv("M355_LIB", EMU_SO)
    glue = bind(glue_lib())
    data = streams(tmp_path)[name]()
    seen = dict(pictures=0, slots=set(), inter=0, intra=0)
    n, downloads = run(glue, emu_lib, data, log2_unit, compare(glue, emu_lib, log2_unit, seen), threads=RA_CPU_CASES[0][6] if name == "random_access" else 2)
    assert n == seen["pictures"] and n >= (75 if name == "girlshy" else 5)
    assert seen["inter"] > 0 and seen["intra"] > 0 and len(seen["slots"]) >= (3 if name == "random_access" else 1), seen
    assert downloads == 0, "a picture that was only mapped was brought back to the host"
    assert glue.m355_glue_cpu_pixel_calls() == 0, "the decoder called into its CPU pixel table"


def test_maps_off_and_two_ranks(emu_lib, tmp_path, monkeypatch):  # noqa: F811
    monkeypatch.setenv("M355_LIB", EMU_SO)
    glue = bind(glue_lib())
    data = make_stream(tmp_path, 256, 128, 8, 1, 1, 3, 153, 10, 1, 1, 0, 1, 1, 0)

    def off(mctx, img, k):
        out = GlueSideMaps()
        assert glue.m355_glue_image_side_maps(img, 1, ctypes.byref(out)) == INVALID, "maps are off"
        assert glue.m355_glue_image_side_maps(img, 1, None) == INVALID and glue.m355_glue_image_side_maps(None, 1, ctypes.byref(out)) == INVALID

    n, _ = run(glue, emu_lib, data, 2, off, mask=0)
    assert n == 3
    dec = glue.de265_new_decoder()
    try:
        for mask, lu in ((1 << capi.N_MAPS, 2), (1, 1), (1, 7)):
            assert glue.m355_glue_set_side_maps(dec, mask, lu) == INVALID
        assert glue.m355_glue_set_side_maps(None, 1, 2) == INVALID
    finally:
        glue.de265_free_decoder(dec)
    monkeypatch.setenv("M355_GLUE_RANKS", "2")
    dec = glue.de265_new_decoder()
    try:
        assert glue.m355_glue_set_side_maps(dec, ALL_MAPS, 2) == INVALID, "a rank's lists hold its tiles only"
    finally:
        glue.de265_free_decoder(dec)


@pytest.mark.gpu
def test_device_maps_equal_the_references_arrays_gpu(tmp_path, monkeypatch):
    monkeypatch.delenv("M355_LIB", raising=False)
    glue = bind(glue_lib())
    backend = capi.Library()
    data = make_stream(tmp_path, 832, 480, 8, 2, 2, 9, 154, 10, 1, 1, 0, 1, 2, G_CTB16 | G_MINCB16)
    for lu in (2, 4):
        seen = dict(pictures=0, slots=set(), inter=0, intra=0)
        n, downloads = run(glue, backend, data, lu, compare(glue, backend, lu, seen), threads=4)
        assert n == seen["pictures"] == 9 and seen["inter"] > 0 and seen["intra"] > 0
        assert downloads == 0 and glue.m355_glue_cpu_pixel_calls() == 0
