"""m355_frame_export / _wait / _order and the m355_device_* trio on the SIMT-interpreter build: every layout and sample format of every
instantiation of k_export, whole frames and misaligned rectangles, rows shorter than one lane's vector, the frame hazard against a later
decode, a pinned-host destination and the argument checks.  Expected values are the planes m355_frame_download returns (first checked
against the oracle's decode) pushed through the numpy restatement in export_util.py; every comparison is exact."""
import ctypes

import numpy as np
import pytest

from test_emu_picture import emu_lib  # noqa: F401  (fixture)
from oracle_py import Oracle
from export_util import (FORMATS, LAYOUTS, SAMPLES, M355_ERR_INVALID, check_export, check_format_matrix, check_gate, check_hazard, decode_into_frame,
                         expected_export, format_id)
from synth_util import assert_planes_equal
from libde265_amd import capi


@pytest.fixture()
def ctx(emu_lib):  # noqa: F811
    c = capi.Context(emu_lib, 0)
    yield c
    c.close()


@pytest.mark.parametrize("fmt", FORMATS, ids=format_id)
def test_export_format_matrix(ctx, oracle, fmt):
    """whole frame, and a rectangle whose source starts off a vector boundary and whose rows are no whole number of 16-byte vectors"""
    check_format_matrix(ctx, Oracle(oracle), dict(fmt, width=64, height=32, log2_ctb=5), [None, (2, 2, 50, 22)])


@pytest.mark.parametrize("bit_depth", [8, 10])
def test_export_minimum_size(ctx, oracle, bit_depth):
    """a 16x8 picture and a 2x2 rectangle of it: every row is shorter than the 16 bytes one lane produces"""
    cfg = dict(width=16, height=8, bit_depth=bit_depth, seed=7200 + bit_depth, log2_ctb=4)
    check_format_matrix(ctx, Oracle(oracle), cfg, [None, (6, 4, 2, 2)])


@pytest.mark.parametrize("depth", [1, 3])
def test_export_behind_recycled_frames(ctx, depth):
    """(the interpreter runs every launch to its end at once: this walks the reader bookkeeping, the GPU tier is what can see a missing wait)"""
    check_hazard(ctx, depth)


def test_export_behind_a_rejected_decode_writes_nothing(ctx):
    check_gate(ctx)


def test_export_into_pinned_host_memory(ctx, oracle):
    frame, planes, geom, frames = decode_into_frame(ctx, Oracle(oracle), dict(width=64, height=32, bit_depth=10, seed=7301, log2_ctb=5))
    check_export(ctx, frame, planes, geom, capi.EXPORT_SEMIPLANAR, capi.EXPORT_MSB16, (2, 2, 50, 22), host=True, what="pinned")
    check_export(ctx, frame, planes, geom, capi.EXPORT_PLANAR, capi.EXPORT_U8, None, host=True, what="pinned")
    for f in frames:
        ctx.frame_destroy(f)


def test_export_order_with_the_contexts_own_stream(ctx, oracle):
    """m355_frame_export_order accepts a stream, and what is read behind it is the export"""
    frame, planes, geom, frames = decode_into_frame(ctx, Oracle(oracle), dict(width=64, height=32, bit_depth=8, seed=7302, log2_ctb=5))
    tok = ctx.frame_export(frame, capi.EXPORT_SEMIPLANAR, capi.EXPORT_NATIVE)
    ctx.frame_export_order(frame, ctx.stream())
    assert_planes_equal(ctx.frame_export_finish(tok), expected_export(planes, *geom, capi.EXPORT_SEMIPLANAR, capi.EXPORT_NATIVE), "ordered")
    with pytest.raises(capi.M355Error) as e:
        ctx.frame_export_order(frame + 100, ctx.stream())
    assert e.value.code == M355_ERR_INVALID
    with pytest.raises(capi.M355Error) as e:
        ctx.frame_export_wait(frame + 100)
    assert e.value.code == M355_ERR_INVALID
    for f in frames:
        ctx.frame_destroy(f)


def test_export_rejects_bad_arguments(ctx):
    """every rejected case returns M355_ERR_INVALID and leaves the destination as it was allocated"""
    lib = ctx.L.lib
    frame = ctx.frame_create(64, 32, 1, 10, 10)
    mono = ctx.frame_create(64, 32, 0, 8, 8)
    nbytes = 32 * 200
    bufs = [ctx.device_alloc(nbytes) for _ in range(3)]

    def desc(layout=capi.EXPORT_PLANAR, samples=capi.EXPORT_NATIVE, rect=(0, 0, 0, 0), dst=(0, 1, 2), pitch=(200, 200, 200)):
        d = capi.ExportDesc(layout=layout, samples=samples)
        d.x0, d.y0, d.width, d.height = rect
        for k in range(3):
            d.dst[k] = bufs[dst[k]] if dst[k] is not None else None
            d.pitch[k] = pitch[k]
        return d

    bad = {
        "rectangle leaves the frame (right)": desc(rect=(16, 0, 50, 16)),
        "rectangle leaves the frame (bottom)": desc(rect=(0, 20, 16, 14)),
        "negative origin": desc(rect=(-2, 0, 16, 16)),
        "negative height": desc(rect=(0, 0, 16, -2)),
        "zero height": desc(rect=(0, 0, 16, 0)),
        "odd x0 on the 4:2:0 grid": desc(rect=(1, 0, 16, 16)),
        "odd y0": desc(rect=(0, 1, 16, 16)),
        "odd width": desc(rect=(0, 0, 15, 16)),
        "odd height": desc(rect=(0, 0, 16, 15)),
        "no luma destination": desc(dst=(None, 1, 2)),
        "no Cr destination (planar)": desc(dst=(0, 1, None)),
        "no chroma destination (semi-planar)": desc(layout=capi.EXPORT_SEMIPLANAR, dst=(0, None, 2)),
        "luma pitch below the row": desc(pitch=(127, 200, 200)),
        "chroma pitch below the row": desc(pitch=(200, 200, 63)),
        "interleaved pitch below the row": desc(layout=capi.EXPORT_SEMIPLANAR, pitch=(200, 127, 200)),
        "16-bit pitch below the row": desc(samples=capi.EXPORT_MSB16, rect=(0, 0, 64, 32), pitch=(127, 200, 200)),
        "unknown layout": desc(layout=2),
        "negative layout": desc(layout=-1),
        "unknown sample format": desc(samples=3),
    }
    for what, d in bad.items():
        assert lib.m355_frame_export(ctx.h, frame, ctypes.byref(d)) == M355_ERR_INVALID, what
    assert lib.m355_frame_export(ctx.h, frame, None) == M355_ERR_INVALID
    assert lib.m355_frame_export(ctx.h, frame + 100, ctypes.byref(desc())) == M355_ERR_INVALID
    d = desc(dst=(None, 1, 2))
    assert lib.m355_frame_export(ctx.h, mono, ctypes.byref(d)) == M355_ERR_INVALID, "monochrome without a luma destination"
    ctx.wait()
    for p in bufs:
        assert np.all(ctx.device_read(p, nbytes) == capi.DEVICE_FILL), "a rejected export wrote to its destination"
    # the same descriptors are fine once the fault is mended: a monochrome frame ignores dst[1], dst[2] and their pitches in both layouts
    assert lib.m355_frame_export(ctx.h, frame, ctypes.byref(desc())) == 0, ctx.L.error()
    got = ctx.device_read(bufs[0], nbytes).reshape(32, 200)
    assert np.all(got[:, :128] == 0) and np.all(got[:, 128:] == capi.DEVICE_FILL)   # (a frame nobody wrote: zero, image.cc:164)
    for layout in LAYOUTS:
        d = desc(layout=layout, dst=(0, None, None), pitch=(64, 0, 0))
        assert lib.m355_frame_export(ctx.h, mono, ctypes.byref(d)) == 0, ctx.L.error()
    assert np.all(ctx.device_read(bufs[0], 64 * 32) == 0)
    for p in bufs:
        ctx.device_free(p)
    ctx.frame_destroy(frame)
    ctx.frame_destroy(mono)


def test_sample_formats_cover_every_value(ctx):
    """the rounding and the clip of M355_EXPORT_U8 and the shift of M355_EXPORT_MSB16 at the ends of the sample range (decoded pictures seldom
    reach them): frames uploaded with every value of the 12-bit range, and with 4096 values from 0 to 65535 of the 16-bit one"""
    for bd in (12, 16):
        frame = ctx.frame_create(128, 32, 3, bd, bd)
        ramp = (np.arange(128 * 32, dtype=np.uint32) * ((1 << bd) - 1) // (128 * 32 - 1)).astype(np.uint16).reshape(32, 128)
        planes = [ramp, ramp[::-1].copy(), ramp[:, ::-1].copy()]
        assert int(ramp.max()) == (1 << bd) - 1 and int(ramp.min()) == 0
        ctx.frame_upload(frame, planes)
        for layout in LAYOUTS:
            for samples in SAMPLES:
                check_export(ctx, frame, planes, (3, bd, bd), layout, samples, None, what="ramp %d" % bd)
        ctx.frame_destroy(frame)
