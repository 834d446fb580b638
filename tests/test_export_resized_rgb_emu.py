"""m355_frame_export_resized_rgb on the SIMT-interpreter build: every instantiation of k_export_resized_rgb (source and destination sample size) under
both layouts and every chroma format at non-integer ratios, ratio 8 down and up and a rectangle off a vector boundary; the composition through the
public calls (resized export -> second frame -> R'G'B' export), the identity, the smallest sizes, tile seams, the extremes of the sample range, the
argument checks, the gate and the reader bookkeeping, a pinned-host destination, the descriptor's layout.  Expected values are the planes
m355_frame_download returns pushed through export_resized_rgb_util.py (the two existing restatements composed); every comparison is exact."""
import ctypes
import os
import re

import numpy as np
import pytest

from test_emu_picture import emu_lib  # noqa: F401  (fixture)
from oracle_py import Oracle
from synth_util import make_case, oracle_decode
from export_resized_util import MATRIX_RECT, expected_export_resized
from export_rgb_util import chroma_at_luma, coefficients, matrix_rgb
from export_resized_rgb_util import (FORMATS, LAYOUTS, MATRIX_CONVERSIONS, MINIMUM_SIZES, M355_ERR_INVALID, COMPOSITION_FORMATS, check_composition,
                                     check_format_matrix, check_gate, check_hazard, check_identity, check_minimum_sizes, check_odd_sizes, check_resized_rgb, check_tile_seams,
                                     check_values, decode_into_frame, expected_resized_rgb, format_id, minimum_case, seam_planes)
from libde265_amd import capi


@pytest.fixture()
def ctx(emu_lib):  # noqa: F811
    c = capi.Context(emu_lib, 0)
    yield c
    c.close()


@pytest.mark.parametrize("fmt", FORMATS, ids=format_id)
def test_resized_rgb_format_matrix(ctx, oracle, fmt):
    check_format_matrix(ctx, Oracle(oracle), dict(fmt, width=64, height=32, log2_ctb=5))


@pytest.mark.parametrize("fmt", COMPOSITION_FORMATS, ids=format_id)
def test_resized_rgb_is_the_two_calls_chained(ctx, oracle, fmt):
    check_composition(ctx, Oracle(oracle), fmt)


@pytest.mark.parametrize("bit_depth,layout", [(8, capi.RGB_PACKED), (8, capi.RGB_PLANAR), (10, capi.RGB_PACKED), (10, capi.RGB_PLANAR)])
def test_whole_frame_at_its_own_size_is_the_rgb_export(ctx, oracle, bit_depth, layout):
    check_identity(ctx, Oracle(oracle), bit_depth, layout)


@pytest.mark.parametrize("bit_depth", [8, 10])
def test_resized_rgb_minimum_sizes(ctx, oracle, bit_depth):
    check_minimum_sizes(ctx, Oracle(oracle), bit_depth)


def test_resized_rgb_tile_seams(ctx):
    check_tile_seams(ctx)


def test_resized_rgb_odd_sizes(ctx):
    check_odd_sizes(ctx)


def rounded_late(planes, cf, bdl, bdc, matrix, full, out_size, rect=None):
    """a WRONG composition: the chroma filter's result is not rounded to a sample of the bit depth before the matrix (two more fraction bits kept
    for 4:2:0 even columns, three for odd ones, scaled back in the matrix by exact division) — what the inputs below must be able to tell apart"""
    resized = expected_export_resized(planes, cf, bdl, bdc, capi.EXPORT_PLANAR, capi.EXPORT_NATIVE, out_size, rect)
    k = coefficients(matrix, full, bdl, bdc, capi.RGB_U16)
    Y = resized[0].astype(np.int64)
    H, W = Y.shape
    out = []
    for C in resized[1:]:
        C = C.astype(np.int64)
        CH, CW = C.shape
        X, Yy = np.arange(W), np.arange(H)
        i, j = X >> 1, Yy >> 1
        i1 = np.minimum(i + 1, CW - 1)
        jn = np.clip(np.where(Yy & 1, j + 1, j - 1), 0, CH - 1)
        T = 3 * C[j] + C[jn]
        out.append(np.where(X & 1, T[:, i] + T[:, i1], 2 * T[:, i]))       # 8 x the sample at the luma position, unrounded
    F, half = k["F"], 1 << (k["F"] - 1)
    y = Y - k["y0"]
    u, v = out[0] - 8 * k["c0"], out[1] - 8 * k["c0"]
    sums = (k["cy"] * y + (k["crv"] * v >> 3) + half, k["cy"] * y - (k["cgu"] * u >> 3) - (k["cgv"] * v >> 3) + half, k["cy"] * y + (k["cbu"] * u >> 3) + half)
    return [np.clip(s >> F, 0, k["M"]).astype(np.uint16) for s in sums]


def test_the_filters_are_under_test(oracle):
    """no library: on the inputs of the smallest sizes and of the tile seams, the composition with the chroma filter's clamps replaced (edge="replicate":
    no filter; edge="wrap": indices modulo the plane) differs from the definition, and so does a composition that skips the rounding of chroma to the
    bit depth before the matrix — else these inputs could not see a wrong halo or a skipped rounding"""
    o = Oracle(oracle)
    inputs = []
    for bd in (8, 10):
        pic, refs = make_case(**minimum_case(bd))
        planes = oracle_decode(o, pic, refs)
        inputs += [(planes, bd, size, rect) for rect, size in MINIMUM_SIZES]
    inputs += [(planes, 10, out_size, None) for _, out_size, planes in seam_planes()]
    matrix, full = MATRIX_CONVERSIONS[0]
    for planes, bd, out_size, rect in inputs:
        args = (planes, 1, bd, bd, capi.RGB_PLANAR, capi.RGB_U16, matrix, full, out_size, rect)
        want = expected_resized_rgb(*args)
        if out_size != (2, 2):           # (a resized chroma plane of 1x1 has no neighbour: every edge rule folds onto the one sample)
            for edge in ("replicate", "wrap"):
                other = expected_resized_rgb(*args, edge=edge)
                assert any(not np.array_equal(a, b) for a, b in zip(want, other)), "edge=%s is not seen at %s rect %s" % (edge, out_size, rect)
            late = rounded_late(planes, 1, bd, bd, matrix, full, out_size, rect)
            assert any(not np.array_equal(a, b) for a, b in zip(want, late)), "a skipped rounding is not seen at %s rect %s" % (out_size, rect)
        else:
            assert all(np.array_equal(a, b) for a, b in zip(want, expected_resized_rgb(*args, edge="wrap")))


@pytest.mark.parametrize("bit_depth", [8, 12, 16])
def test_resized_rgb_values_and_clips(ctx, bit_depth):
    check_values(ctx, bit_depth)


def test_resized_rgb_export_rejects_bad_arguments(ctx):
    """every rejected case returns M355_ERR_INVALID and leaves the destination as it was allocated"""
    lib = ctx.L.lib
    frame = ctx.frame_create(64, 32, 1, 10, 10)
    f422 = ctx.frame_create(64, 32, 2, 10, 10)
    mono = ctx.frame_create(64, 40, 0, 8, 8)
    nbytes = 64 * 600
    bufs = [ctx.device_alloc(nbytes) for _ in range(3)]

    def desc(out=(32, 16), layout=capi.RGB_PLANAR, samples=capi.RGB_U8, matrix=capi.MATRIX_BT709, full=0, rect=(0, 0, 0, 0), dst=(0, 1, 2), pitch=(600, 600, 600),
             odd=0):
        d = capi.ResizeRgbDesc(layout=layout, samples=samples, matrix=matrix, full_range=full, out_width=out[0], out_height=out[1])
        d.x0, d.y0, d.width, d.height = rect
        for j in range(3):
            d.dst[j] = bufs[dst[j]] + odd if dst[j] is not None else None
            d.pitch[j] = pitch[j]
        return d

    bad = [
        ("out_width 0", frame, desc(out=(0, 16))),
        ("out_width negative", frame, desc(out=(-32, 16))),
        ("out_height 0", frame, desc(out=(32, 0))),
        ("out_height negative", frame, desc(out=(32, -16))),
        ("out_width odd, 4:2:0", frame, desc(out=(33, 16))),
        ("out_height odd, 4:2:0", frame, desc(out=(32, 17))),
        ("out_width odd, 4:2:2", f422, desc(out=(33, 17))),
        ("more than 8x down, width", frame, desc(out=(6, 16))),
        ("more than 8x down, height", frame, desc(out=(32, 2))),
        ("one sample beyond 8x down, width", mono, desc(out=(7, 40), rect=(0, 0, 57, 40))),
        ("one sample beyond 8x down, height", mono, desc(out=(64, 4), rect=(0, 0, 64, 33))),
        ("one sample beyond 8x up, width", mono, desc(out=(65, 20), rect=(0, 0, 8, 20))),
        ("one sample beyond 8x up, height", mono, desc(out=(32, 33), rect=(0, 0, 32, 4))),
        ("more than 8x up", frame, desc(out=(72, 16), rect=(0, 0, 8, 8))),
        ("rectangle leaves the frame", frame, desc(rect=(32, 0, 48, 16))),
        ("rectangle off the chroma grid", frame, desc(rect=(1, 0, 16, 16))),
        ("rectangle of no width", frame, desc(rect=(0, 0, -4, 16))),
        ("unknown layout", frame, desc(layout=2)),
        ("unknown samples", frame, desc(samples=2)),
        ("unknown matrix", frame, desc(matrix=3)),
        ("negative matrix", frame, desc(matrix=-1)),
        ("full_range 2", frame, desc(full=2)),
        ("packed pitch one byte below the output row", frame, desc(layout=capi.RGB_PACKED, pitch=(3 * 32 - 1, 600, 600))),
        ("packed U16 pitch one byte below the output row", frame, desc(layout=capi.RGB_PACKED, samples=capi.RGB_U16, pitch=(3 * 32 * 2 - 1, 600, 600))),
        ("planar pitch below the output row", frame, desc(pitch=(600, 31, 600))),
        ("no destination (packed)", frame, desc(layout=capi.RGB_PACKED, dst=(None, 1, 2))),
        ("a planar plane missing", frame, desc(dst=(0, 1, None))),
        ("a planar plane missing, monochrome", mono, desc(dst=(0, None, 2))),
        ("U16 destination at an odd address", frame, desc(samples=capi.RGB_U16, odd=1)),
        ("U16 destination with an odd pitch", frame, desc(samples=capi.RGB_U16, pitch=(600, 601, 600))),
    ]
    for what, f, d in bad:
        assert lib.m355_frame_export_resized_rgb(ctx.h, f, ctypes.byref(d)) == M355_ERR_INVALID, what
    assert lib.m355_frame_export_resized_rgb(ctx.h, frame, None) == M355_ERR_INVALID
    assert lib.m355_frame_export_resized_rgb(ctx.h, frame + 100, ctypes.byref(desc())) == M355_ERR_INVALID
    ctx.wait()
    for p in bufs:
        assert np.all(ctx.device_read(p, nbytes) == capi.DEVICE_FILL), "a rejected export wrote to its destination"
    # the limits themselves: a pitch equal to the output row's bytes, ratio exactly 8 down and up
    assert lib.m355_frame_export_resized_rgb(ctx.h, frame, ctypes.byref(desc(layout=capi.RGB_PACKED, pitch=(96, 0, 0), dst=(0, None, None)))) == 0, ctx.L.error()
    assert lib.m355_frame_export_resized_rgb(ctx.h, frame, ctypes.byref(desc(samples=capi.RGB_U16, pitch=(64, 64, 64)))) == 0, ctx.L.error()
    assert lib.m355_frame_export_resized_rgb(ctx.h, frame, ctypes.byref(desc(out=(8, 4)))) == 0, ctx.L.error()
    assert lib.m355_frame_export_resized_rgb(ctx.h, mono, ctypes.byref(desc(out=(7, 40), rect=(0, 0, 56, 40)))) == 0, ctx.L.error()
    assert lib.m355_frame_export_resized_rgb(ctx.h, mono, ctypes.byref(desc(out=(64, 32), rect=(0, 0, 8, 4)))) == 0, ctx.L.error()
    ctx.wait()
    for p in bufs:
        ctx.device_free(p)
    for f in (frame, f422, mono):
        ctx.frame_destroy(f)


def test_resized_rgb_export_behind_a_rejected_decode_writes_nothing(ctx):
    check_gate(ctx)


@pytest.mark.parametrize("depth", [1, 3])
def test_resized_rgb_export_behind_recycled_frames(ctx, depth):
    """(the interpreter runs every launch to its end at once: this walks the reader bookkeeping, the GPU tier is what can see a missing wait)"""
    check_hazard(ctx, depth)


def test_resized_rgb_export_into_pinned_host_memory(ctx, oracle):
    frame, planes, geom, frames = decode_into_frame(ctx, Oracle(oracle), dict(width=64, height=32, bit_depth=10, seed=7301, log2_ctb=5))
    check_resized_rgb(ctx, frame, planes, geom, capi.RGB_PACKED, capi.RGB_U16, capi.MATRIX_BT709, 0, (36, 14), MATRIX_RECT, host=True, what="pinned")
    for f in frames:
        ctx.frame_destroy(f)


def test_resize_rgb_desc_abi():
    """sizeof and the field offsets of m355_resize_rgb_desc as the header declares it (LP64: ten int32, three pointers, three int64), against the
    ctypes structure; the header's field order is read from the header itself"""
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "de265_mi355x.h")).read()
    body = re.search(r"typedef struct m355_resize_rgb_desc \{(.*?)\} m355_resize_rgb_desc;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names, offsets, ofs = [], {}, 0
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, rest = re.match(r"(int32_t|int64_t|void\*)\s*(.*)", decl).groups()
        size = 4 if ctype == "int32_t" else 8
        for item in rest.split(","):
            name, count = re.match(r"\s*(\w+)(?:\[(\d+)\])?", item).groups()
            ofs = (ofs + size - 1) // size * size
            names.append(name); offsets[name] = ofs
            ofs += size * int(count or 1)
    assert names == [n for n, _ in capi.ResizeRgbDesc._fields_]
    for n in names:
        assert getattr(capi.ResizeRgbDesc, n).offset == offsets[n], n
    assert ctypes.sizeof(capi.ResizeRgbDesc) == (ofs + 7) // 8 * 8 == 88
