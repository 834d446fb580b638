"""m355_frame_export_rgb on the SIMT-interpreter build: the coefficients, every instantiation of k_export_rgb (source sample size, channel size,
layout, chroma format), whole frames and rectangles whose source is off a vector boundary, every sample value with both clips, the chroma
reconstruction filter with its frame-edge clamps, crop invariance, the smallest outputs, the argument checks, a monochrome frame, the gate and the
reader bookkeeping, a pinned-host destination, and the distance of the integer conversion to the real-valued one.  Expected values are the planes
m355_frame_download returns pushed through the Python-integer restatement in export_rgb_util.py; every comparison of pixels is exact."""
import ctypes
import itertools

import numpy as np
import pytest

from test_emu_picture import emu_lib  # noqa: F401  (fixture)
from oracle_py import Oracle
from export_rgb_util import (ALL_CONVERSIONS, COEFF_NAMES, FORMATS, LAYOUTS, MATRICES, MATRIX_RECT, M355_ERR_INVALID, SAMPLES, assert_export,
                             check_format_matrix_rgb, check_gate_rgb, check_hazard_rgb, check_rgb, check_values, chroma_at_luma, chroma_case,
                             coefficients, decode_into_frame, expected_rgb, float_rgb, format_id, matrix_rgb, value_cases, yuv_at_luma)
from libde265_amd import capi


@pytest.fixture()
def ctx(emu_lib):  # noqa: F811
    c = capi.Context(emu_lib, 0)
    yield c
    c.close()


def test_rgb_coefficients(emu_lib):  # noqa: F811
    """m355_rgb_coefficients equals the Python-integer restatement for every matrix, range, pair of bit depths and sample type"""
    for matrix, full, bdy, bdc, samples in itertools.product(MATRICES, (0, 1), (8, 9, 10, 12, 16), (8, 9, 10, 12, 16), SAMPLES):
        got = emu_lib.rgb_coefficients(matrix, full, bdy, bdc, samples)
        want = coefficients(matrix, full, bdy, bdc, samples)
        assert got == {n: want[n] for n in COEFF_NAMES}, (matrix, full, bdy, bdc, samples)
        assert max(want[n] for n in ("cy", "crv", "cgu", "cgv", "cbu")) < (1 << 23)      # (the kernel multiplies with 24-bit operands)
    k = capi.RgbCoeffs()
    lib = emu_lib.lib
    for bad in [(-1, 0, 8, 8, 0), (3, 0, 8, 8, 0), (1, -1, 8, 8, 0), (1, 2, 8, 8, 0), (1, 0, 7, 8, 0), (1, 0, 17, 8, 0), (1, 0, 8, 7, 0), (1, 0, 8, 17, 0),
                (1, 0, 8, 8, -1), (1, 0, 8, 8, 2)]:
        assert lib.m355_rgb_coefficients(*bad, ctypes.byref(k)) == M355_ERR_INVALID, bad
    assert lib.m355_rgb_coefficients(1, 0, 8, 8, 0, None) == M355_ERR_INVALID


@pytest.mark.parametrize("fmt", FORMATS, ids=format_id)
def test_rgb_format_matrix(ctx, oracle, fmt):
    """whole frame, and a rectangle whose source starts off a vector boundary: both layouts and sample types, BT.709 limited and BT.2020 full"""
    check_format_matrix_rgb(ctx, Oracle(oracle), dict(fmt, width=64, height=32, log2_ctb=5), [None, MATRIX_RECT])


@pytest.mark.parametrize("bit_depth", [8, 10, 12, 16])
def test_rgb_values_and_clips(ctx, bit_depth):
    check_values(ctx, bit_depth)


@pytest.mark.parametrize("cf,bit_depth", [(1, 8), (1, 10), (2, 8), (2, 10)])
def test_rgb_chroma_reconstruction_and_crop(ctx, cf, bit_depth):
    """uploaded chroma under constant luma: the filter (not sample replication) and its four frame-edge clamps decide the expected output, the
    export delivers it, and a rectangle whose chroma neighbours lie outside it equals the same window of the whole-frame export"""
    planes = chroma_case(cf, bit_depth, 7700 + 10 * cf + bit_depth)
    geom = (cf, bit_depth, bit_depth)
    args = (capi.RGB_PLANAR, capi.RGB_U16, capi.MATRIX_BT709, 1)
    want = expected_rgb(planes, *geom, *args)
    repl = expected_rgb(planes, *geom, *args, edge="replicate")
    differs = np.zeros(want[0].shape, bool)
    for a, b in zip(want, repl):
        differs |= a != b
    if cf == 1:
        assert differs.mean() > 0.5, "the expected output is sample replication in %d %% of the pixels" % (100 - 100 * differs.mean())
    else:
        # 4:2:2 has no vertical filter and its even columns are co-sited: they ARE the chroma samples, by definition.  Only the odd columns short of
        # the last one can differ from replication, 15 of 32 here — "more than half of the pixels" cannot hold; nine in ten of those that can, must
        assert not differs[:, 0::2].any() and not differs[:, -1].any()
        assert differs[:, 1:-1:2].mean() > 0.9, "the expected output is sample replication in %d %% of the filtered pixels" % (100 - 100 * differs[:, 1:-1:2].mean())
    wrap = expected_rgb(planes, *geom, *args, edge="wrap")
    edges = {"last column": (slice(None), -1)}
    if cf == 1:
        edges.update({"first row": (0, slice(None)), "last row": (-1, slice(None))})
    for name, idx in edges.items():
        assert any(not np.array_equal(a[idx], b[idx]) for a, b in zip(want, wrap)), "the clamp of the %s does not matter" % name
    # (the first column reads no neighbour on its left in this filter: X = 0 is co-sited with chroma column 0 — what matters there is that nothing
    #  in front of the row is read, which the wrapped restatement cannot show and the exact comparison of column 0 does)
    for a, b in zip(want, wrap):
        assert np.array_equal(a[1:-1, :-1] if cf == 1 else a[:, :-1], b[1:-1, :-1] if cf == 1 else b[:, :-1])
    frame = ctx.frame_create(32, 16, cf, bit_depth, bit_depth)
    try:
        ctx.frame_upload(frame, planes)
        for layout in LAYOUTS:
            for samples in SAMPLES:
                check_rgb(ctx, frame, planes, geom, layout, samples, capi.MATRIX_BT709, 1, what="chroma case")
                whole = ctx.frame_export_finish(ctx.frame_export_rgb(frame, layout, samples, capi.MATRIX_BT601, 0))
                crop, raws = ctx.frame_export_finish(ctx.frame_export_rgb(frame, layout, samples, capi.MATRIX_BT601, 0, (6, 6, 20, 8)), raw=True)
                n = 3 if layout == capi.RGB_PACKED else 1
                assert_export(crop, raws, [np.ascontiguousarray(p[6:14, 6 * n:26 * n]) for p in whole], "crop invariance")
    finally:
        ctx.frame_destroy(frame)


@pytest.mark.parametrize("bit_depth", [8, 10])
def test_rgb_minimum_size(ctx, oracle, bit_depth):
    """a 16x16 4:2:0 picture, whole (one partial lane per row) and a 2x2 rectangle of it"""
    frame, planes, geom, frames = decode_into_frame(ctx, Oracle(oracle), dict(width=16, height=16, bit_depth=bit_depth, seed=7710 + bit_depth, log2_ctb=4))
    try:
        for layout in LAYOUTS:
            for samples in SAMPLES:
                check_rgb(ctx, frame, planes, geom, layout, samples, capi.MATRIX_BT601, 0, None, what="16x16")
                check_rgb(ctx, frame, planes, geom, layout, samples, capi.MATRIX_BT601, 0, (4, 4, 2, 2), what="2x2")
    finally:
        for f in frames:
            ctx.frame_destroy(f)


def test_rgb_export_rejects_bad_arguments(ctx):
    """every rejected case returns M355_ERR_INVALID and leaves the destination as it was allocated"""
    lib = ctx.L.lib
    frame = ctx.frame_create(64, 32, 1, 10, 10)
    nbytes = 40 * 400
    bufs = [ctx.device_alloc(nbytes) for _ in range(3)]

    def desc(layout=capi.RGB_PLANAR, samples=capi.RGB_U8, matrix=capi.MATRIX_BT709, full=0, rect=(0, 0, 0, 0), dst=(0, 1, 2), pitch=(400, 400, 400), ofs=0):
        d = capi.RgbDesc(layout=layout, samples=samples, matrix=matrix, full_range=full)
        d.x0, d.y0, d.width, d.height = rect
        for j in range(3):
            d.dst[j] = bufs[dst[j]] + ofs if dst[j] is not None else None
            d.pitch[j] = pitch[j]
        return d

    P, U16 = capi.RGB_PACKED, capi.RGB_U16
    bad = [
        ("rectangle leaves the frame", desc(rect=(32, 0, 48, 16))),
        ("rectangle off the chroma grid (x)", desc(rect=(1, 0, 16, 16))),
        ("rectangle off the chroma grid (height)", desc(rect=(0, 0, 16, 15))),
        ("negative origin", desc(rect=(-2, 0, 16, 16))),
        ("empty height", desc(rect=(0, 0, 16, 0))),
        ("unknown layout", desc(layout=2)),
        ("negative layout", desc(layout=-1)),
        ("unknown samples", desc(samples=2)),
        ("unknown matrix", desc(matrix=3)),
        ("negative matrix", desc(matrix=-1)),
        ("full_range 2", desc(full=2)),
        ("full_range -1", desc(full=-1)),
        ("no R destination", desc(dst=(None, 1, 2))),
        ("no G destination (planar)", desc(dst=(0, None, 2))),
        ("no B destination (planar)", desc(dst=(0, 1, None))),
        ("no destination (packed)", desc(layout=P, dst=(None, 1, 2))),
        ("planar pitch below the row", desc(pitch=(400, 63, 400))),
        ("planar U16 pitch below the row", desc(samples=U16, pitch=(400, 400, 126))),
        ("packed pitch below the row", desc(layout=P, pitch=(191, 400, 400))),
        ("packed U16 pitch below the row", desc(layout=P, samples=U16, pitch=(382, 400, 400))),
        ("U16 at an odd address", desc(layout=P, samples=U16, ofs=1)),
        ("U16 with an odd pitch", desc(layout=P, samples=U16, pitch=(399, 400, 400))),
        ("planar U16, one odd pitch", desc(samples=U16, pitch=(400, 400, 399))),
    ]
    for what, d in bad:
        assert lib.m355_frame_export_rgb(ctx.h, frame, ctypes.byref(d)) == M355_ERR_INVALID, what
    assert lib.m355_frame_export_rgb(ctx.h, frame, None) == M355_ERR_INVALID
    assert lib.m355_frame_export_rgb(ctx.h, frame + 100, ctypes.byref(desc())) == M355_ERR_INVALID
    ctx.wait()
    for p in bufs:
        assert np.all(ctx.device_read(p, nbytes) == capi.DEVICE_FILL), "a rejected export wrote to its destination"
    # the limits themselves are fine: a pitch equal to the row, an odd address and pitch for 8-bit channels, dst[1..2] ignored when packed
    assert lib.m355_frame_export_rgb(ctx.h, frame, ctypes.byref(desc(pitch=(64, 64, 64)))) == 0, ctx.L.error()
    assert lib.m355_frame_export_rgb(ctx.h, frame, ctypes.byref(desc(layout=P, pitch=(193, 0, 0), dst=(0, None, None), ofs=1))) == 0, ctx.L.error()
    assert lib.m355_frame_export_rgb(ctx.h, frame, ctypes.byref(desc(layout=P, samples=U16, pitch=(384, 0, 0), dst=(0, None, None)))) == 0, ctx.L.error()
    ctx.wait()
    for p in bufs:
        ctx.device_free(p)
    ctx.frame_destroy(frame)


def test_rgb_monochrome(ctx):
    """a monochrome frame has u = v = 0: R = G = B in both layouts"""
    mono = ctx.frame_create(64, 40, 0, 8, 8)
    luma = (np.arange(40 * 64, dtype=np.uint32) * 7 % 256).astype(np.uint8).reshape(40, 64)
    ctx.frame_upload(mono, [luma])
    try:
        for samples in SAMPLES:
            for matrix, full in ((capi.MATRIX_BT601, 0), (capi.MATRIX_BT2020, 1)):
                planar, raws = ctx.frame_export_finish(ctx.frame_export_rgb(mono, capi.RGB_PLANAR, samples, matrix, full, (2, 1, 51, 30)), raw=True)
                assert_export(planar, raws, expected_rgb([luma], 0, 8, 8, capi.RGB_PLANAR, samples, matrix, full, (2, 1, 51, 30)), "monochrome planar")
                assert np.array_equal(planar[0], planar[1]) and np.array_equal(planar[0], planar[2])
                assert len(np.unique(planar[0])) > 100
                packed, raws = ctx.frame_export_finish(ctx.frame_export_rgb(mono, capi.RGB_PACKED, samples, matrix, full, (2, 1, 51, 30)), raw=True)
                assert_export(packed, raws, expected_rgb([luma], 0, 8, 8, capi.RGB_PACKED, samples, matrix, full, (2, 1, 51, 30)), "monochrome packed")
                assert np.array_equal(packed[0][:, 0::3], planar[0]) and np.array_equal(packed[0][:, 1::3], planar[0]) and np.array_equal(packed[0][:, 2::3], planar[0])
    finally:
        ctx.frame_destroy(mono)


def test_rgb_export_behind_a_rejected_decode_writes_nothing(ctx):
    check_gate_rgb(ctx)


@pytest.mark.parametrize("depth", [1, 3])
def test_rgb_export_behind_recycled_frames(ctx, depth):
    """(the interpreter runs every launch to its end at once: this walks the reader bookkeeping, the GPU tier is what can see a missing wait)"""
    check_hazard_rgb(ctx, depth)


def test_rgb_export_into_pinned_host_memory(ctx, oracle):
    frame, planes, geom, frames = decode_into_frame(ctx, Oracle(oracle), dict(width=64, height=32, bit_depth=10, seed=7301, log2_ctb=5))
    check_rgb(ctx, frame, planes, geom, capi.RGB_PACKED, capi.RGB_U16, capi.MATRIX_BT709, 0, (2, 2, 48, 16), host=True, what="pinned")
    check_rgb(ctx, frame, planes, geom, capi.RGB_PLANAR, capi.RGB_U8, capi.MATRIX_BT709, 0, (2, 2, 48, 16), host=True, what="pinned")
    for f in frames:
        ctx.frame_destroy(f)


@pytest.mark.parametrize("bit_depth", [8, 10, 16])
def test_rgb_accuracy_against_the_real_valued_conversion(bit_depth):
    """The expected RGB lies within 0.5 + 0.5 (|y| + |u| + |v|) / 2^F output LSB of the float64 BT matrix conversion: 0.5 for the one final rounding
    and at most half a unit of 2^-F per rounded coefficient times the magnitude it multiplies (G's two chroma coefficients share |u| + |v|).  Not
    tuned; numpy only."""
    for matrix, full in ALL_CONVERSIONS:
        for samples in SAMPLES:
            k = coefficients(matrix, full, bit_depth, bit_depth, samples)
            for name, planes in value_cases(bit_depth):
                Yp, Cb, Cr = yuv_at_luma(planes, 3)
                got = matrix_rgb(Yp, Cb, Cr, k)
                ref = float_rgb(Yp, Cb, Cr, k)
                bound = 0.5 + 0.5 * (np.abs(Yp - k["y0"]) + np.abs(Cb - k["c0"]) + np.abs(Cr - k["c0"])) / float(1 << k["F"])
                for c in range(3):
                    err = np.abs(got[c] - ref[c])
                    assert np.all(err <= bound + 1e-9), "%s: channel %d of matrix %d full %d samples %d: up to %.3f LSB off, %.3f beyond the bound" % (
                        name, c, matrix, full, samples, float(err.max()), float((err - bound).max()))
