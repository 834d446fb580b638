"""m355_frame_export_scaled on the SIMT-interpreter build: every instantiation of k_export_scaled (source and destination sample size, layout,
scale), whole frames and a rectangle whose source is off a vector boundary, the smallest outputs, every sample value with the extremes of the
block sum and the rounding, the argument checks, the gate and the reader bookkeeping, a pinned-host destination.  Expected values are the planes
m355_frame_download returns pushed through the numpy restatement in export_scaled_util.py; every comparison is exact."""
import ctypes

import numpy as np
import pytest

from test_emu_picture import emu_lib  # noqa: F401  (fixture)
from oracle_py import Oracle
from export_scaled_util import (FORMATS, LAYOUTS, MATRIX_RECT, M355_ERR_INVALID, SAMPLES, SCALES, assert_export, check_export_scaled,
                                check_format_matrix_scaled, check_gate_scaled, check_hazard_scaled, check_values, decode_into_frame, format_id)
from libde265_amd import capi


@pytest.fixture()
def ctx(emu_lib):  # noqa: F811
    c = capi.Context(emu_lib, 0)
    yield c
    c.close()


@pytest.mark.parametrize("fmt", FORMATS, ids=format_id)
def test_scaled_format_matrix(ctx, oracle, fmt):
    """whole frame, and a rectangle whose source starts off a vector boundary; both a multiple of the 8x scale on every chroma grid"""
    check_format_matrix_scaled(ctx, Oracle(oracle), dict(fmt, width=64, height=32, log2_ctb=5), [None, MATRIX_RECT])


@pytest.mark.parametrize("bit_depth,layout", [(8, capi.EXPORT_PLANAR), (8, capi.EXPORT_SEMIPLANAR), (10, capi.EXPORT_PLANAR), (10, capi.EXPORT_SEMIPLANAR)])
def test_scale_one_is_the_plain_export(ctx, oracle, bit_depth, layout):
    """log2_scale 0 delivers what m355_frame_export delivers, byte for byte, the padding included"""
    frame, planes, geom, frames = decode_into_frame(ctx, Oracle(oracle), dict(width=64, height=32, bit_depth=bit_depth, seed=7600 + bit_depth, log2_ctb=5))
    try:
        for samples in SAMPLES:
            for rect in (None, (2, 2, 50, 22)):
                plain = ctx.frame_export_finish(ctx.frame_export(frame, layout, samples, rect), raw=True)
                scaled = ctx.frame_export_finish(ctx.frame_export(frame, layout, samples, rect, log2_scale=0, scaled_entry=True), raw=True)
                assert len(plain[1]) == len(scaled[1])
                for a, b in zip(plain[1], scaled[1]):
                    assert a.shape == b.shape and np.array_equal(a, b), "samples %d rect %s" % (samples, rect)
                assert not np.all(plain[1][0] == capi.DEVICE_FILL)
    finally:
        for f in frames:
            ctx.frame_destroy(f)


@pytest.mark.parametrize("bit_depth", [8, 10])
def test_scaled_minimum_size(ctx, oracle, bit_depth):
    """a 16x16 4:2:0 picture at 8x: luma 2x2, chroma 1x1; at 2x a 4x4 rectangle of it: rows of 2 and 1 samples"""
    frame, planes, geom, frames = decode_into_frame(ctx, Oracle(oracle), dict(width=16, height=16, bit_depth=bit_depth, seed=7610 + bit_depth, log2_ctb=4))
    try:
        for layout in LAYOUTS:
            for samples in SAMPLES:
                check_export_scaled(ctx, frame, planes, geom, layout, samples, 3, None, what="16x16")
                check_export_scaled(ctx, frame, planes, geom, layout, samples, 1, (4, 4, 4, 4), what="4x4")
    finally:
        for f in frames:
            ctx.frame_destroy(f)


@pytest.mark.parametrize("bit_depth", [8, 12, 16])
def test_scaled_values_and_roundings(ctx, bit_depth):
    check_values(ctx, bit_depth)


def test_scaled_export_rejects_bad_arguments(ctx):
    """every rejected case returns M355_ERR_INVALID and leaves the destination as it was allocated"""
    lib = ctx.L.lib
    frame = ctx.frame_create(64, 32, 1, 10, 10)
    odd = ctx.frame_create(72, 40, 1, 10, 10)           # whole frame: a multiple of 2 * 2 and 4 * 2, not of 8 * 2
    f422 = ctx.frame_create(72, 32, 2, 10, 10)          # 4:2:2: the height is a multiple of f = 8, the width of f only, not of f * SubWidthC
    mono = ctx.frame_create(64, 40, 0, 8, 8)
    nbytes = 48 * 200
    bufs = [ctx.device_alloc(nbytes) for _ in range(3)]

    def desc(layout=capi.EXPORT_PLANAR, samples=capi.EXPORT_NATIVE, rect=(0, 0, 0, 0), dst=(0, 1, 2), pitch=(200, 200, 200)):
        d = capi.ExportDesc(layout=layout, samples=samples)
        d.x0, d.y0, d.width, d.height = rect
        for j in range(3):
            d.dst[j] = bufs[dst[j]] if dst[j] is not None else None
            d.pitch[j] = pitch[j]
        return d

    bad = [
        ("log2_scale -1", frame, desc(), -1),
        ("log2_scale 4", frame, desc(), 4),
        ("width no multiple of 2 * 2", frame, desc(rect=(0, 0, 18, 16)), 1),
        ("height no multiple of 2 * 2", frame, desc(rect=(0, 0, 16, 18)), 1),
        ("width no multiple of 4 * 2", frame, desc(rect=(0, 0, 20, 16)), 2),
        ("height no multiple of 8 * 2", frame, desc(rect=(0, 0, 32, 24)), 3),
        ("whole 72x40 frame at 8x", odd, desc(), 3),
        ("4:2:2, whole frame, width a multiple of 8 only", f422, desc(), 3),
        ("4:2:2 rectangle, width a multiple of 8 only", f422, desc(rect=(0, 0, 24, 16)), 3),
        ("monochrome, height no multiple of 8", mono, desc(rect=(0, 0, 64, 36), dst=(0, None, None)), 3),
        ("monochrome, width no multiple of 4", mono, desc(rect=(1, 1, 10, 8), dst=(0, None, None)), 2),
        ("luma pitch below the scaled row", frame, desc(pitch=(63, 200, 200)), 1),
        ("chroma pitch below the scaled row", frame, desc(pitch=(200, 200, 15)), 2),
        ("interleaved pitch below the scaled row", frame, desc(layout=capi.EXPORT_SEMIPLANAR, pitch=(200, 63, 200)), 1),
        ("rectangle leaves the frame", frame, desc(rect=(32, 0, 48, 16)), 1),
        ("rectangle off the chroma grid", frame, desc(rect=(1, 0, 16, 16)), 1),
        ("no luma destination", frame, desc(dst=(None, 1, 2)), 1),
        ("no Cr destination (planar)", frame, desc(dst=(0, 1, None)), 2),
        ("unknown layout", frame, desc(layout=2), 1),
        ("unknown sample format", frame, desc(samples=3), 1),
    ]
    for what, f, d, k in bad:
        assert lib.m355_frame_export_scaled(ctx.h, f, ctypes.byref(d), k) == M355_ERR_INVALID, what
    assert lib.m355_frame_export_scaled(ctx.h, frame, None, 1) == M355_ERR_INVALID
    assert lib.m355_frame_export_scaled(ctx.h, frame + 100, ctypes.byref(desc()), 1) == M355_ERR_INVALID
    ctx.wait()
    for p in bufs:
        assert np.all(ctx.device_read(p, nbytes) == capi.DEVICE_FILL), "a rejected export wrote to its destination"
    # the same frames are fine at a scale that fits: the pitch is checked against the SCALED row (64 10-bit samples at 2x: 64 bytes)
    assert lib.m355_frame_export_scaled(ctx.h, frame, ctypes.byref(desc(pitch=(64, 32, 32))), 1) == 0, ctx.L.error()
    assert lib.m355_frame_export_scaled(ctx.h, odd, ctypes.byref(desc()), 2) == 0, ctx.L.error()
    assert lib.m355_frame_export_scaled(ctx.h, f422, ctypes.byref(desc()), 2) == 0, ctx.L.error()
    for p in bufs:
        ctx.device_free(p)
    for f in (frame, odd, f422):
        ctx.frame_destroy(f)
    # a monochrome frame exports luma only: dst[1], dst[2] and their pitches are ignored in both layouts
    luma = (np.arange(40 * 64, dtype=np.uint32) * 7 % 256).astype(np.uint8).reshape(40, 64)
    ctx.frame_upload(mono, [luma])
    for layout in LAYOUTS:
        got, raws = ctx.frame_export_finish(ctx.frame_export(mono, layout, capi.EXPORT_MSB16, log2_scale=2), raw=True)
        s = luma.reshape(10, 4, 16, 4).sum(axis=(1, 3), dtype=np.uint64)
        assert len(got) == 1
        assert_export(got, raws, [(((s + 8) >> np.uint64(4)) << np.uint64(8)).astype(np.uint16)], "monochrome")
    ctx.frame_destroy(mono)


def test_scaled_export_behind_a_rejected_decode_writes_nothing(ctx):
    check_gate_scaled(ctx)


@pytest.mark.parametrize("depth", [1, 3])
def test_scaled_export_behind_recycled_frames(ctx, depth):
    """(the interpreter runs every launch to its end at once: this walks the reader bookkeeping, the GPU tier is what can see a missing wait)"""
    check_hazard_scaled(ctx, depth)


def test_scaled_export_into_pinned_host_memory(ctx, oracle):
    frame, planes, geom, frames = decode_into_frame(ctx, Oracle(oracle), dict(width=64, height=32, bit_depth=10, seed=7301, log2_ctb=5))
    check_export_scaled(ctx, frame, planes, geom, capi.EXPORT_SEMIPLANAR, capi.EXPORT_MSB16, 2, (2, 2, 48, 16), host=True, what="pinned")
    for f in frames:
        ctx.frame_destroy(f)
