"""m355_frame_export_resized on the SIMT-interpreter build: the filter rows (m355_resize_taps against the Python-integer restatement), the restatement
against an independent float64 resize, every instantiation of k_export_resized (source and destination sample size, layout) at non-integer ratios,
ratio 8 down and up, a rectangle whose source is off a vector boundary, the smallest sizes, the extremes of the sample range, the argument checks,
the gate and the reader bookkeeping, a pinned-host destination, the descriptor's layout.  Expected values are the planes m355_frame_download returns
pushed through export_resized_util.py; every comparison of an export is exact."""
import ctypes
import math
import random
import re
import os

import numpy as np
import pytest

from test_emu_picture import emu_lib  # noqa: F401  (fixture)
from oracle_py import Oracle
from export_resized_util import (FORMATS, LAYOUTS, MATRIX_RECT, M355_ERR_INVALID, assert_export, check_export_resized, check_format_matrix_resized,
                                 check_gate_resized, check_hazard_resized, check_identity, check_minimum_sizes, check_rect_equals_cropped_frame, check_several_tiles,
                                 check_values, convert, decode_into_frame, float_resize, format_id, ratio_ok, resize_plane, taps)
from libde265_amd import capi


@pytest.fixture()
def ctx(emu_lib):  # noqa: F811
    c = capi.Context(emu_lib, 0)
    yield c
    c.close()


TAP_PAIRS = [(64, 8), (8, 64), (64, 48), (50, 64), (17, 3), (1, 1), (1, 8), (8, 1), (9, 2), (33, 32), (1920, 1280), (7680, 1920)]


def check_axis(lib, sn, dn):
    for cosited in (0, 1):
        for i in range(dn):
            want = taps(sn, dn, cosited, i)
            assert lib.resize_taps(sn, dn, cosited, i) == want, "taps %d -> %d, cosited %d, row %d" % (sn, dn, cosited, i)
            first, q = want
            assert 0 <= first and first + len(q) <= sn and 1 <= len(q) <= 16
            assert min(q) >= 0 and sum(q) == 1 << 14
            if sn == dn:
                assert want == (i, [1 << 14])


@pytest.mark.parametrize("sn,dn", TAP_PAIRS)
def test_taps_equal_the_restatement(emu_lib, sn, dn):  # noqa: F811
    check_axis(emu_lib, sn, dn)


def test_taps_of_random_pairs(emu_lib):  # noqa: F811
    rng = random.Random(7800)
    for _ in range(200):
        sn = rng.randint(1, 600)
        dn = rng.randint((sn + 7) // 8, min(8 * sn, 600))
        assert ratio_ok(sn, dn)
        check_axis(emu_lib, sn, dn)


def test_taps_reject_bad_arguments(emu_lib):  # noqa: F811
    bad = [(0, 4, 0, 0), (4, 0, 0, 0), (-3, 4, 0, 0), (65, 8, 0, 0), (8, 65, 0, 0), (8, 4, 2, 0), (8, 4, -1, 0), (8, 4, 0, -1), (8, 4, 0, 4)]
    for args in bad:
        assert emu_lib.resize_taps(*args) is None, args
    first, coeff = ctypes.c_int32(), (ctypes.c_int32 * 16)()
    assert emu_lib.lib.m355_resize_taps(8, 4, 0, 0, None, coeff) < 0
    assert emu_lib.lib.m355_resize_taps(8, 4, 0, 0, ctypes.byref(first), None) < 0
    assert emu_lib.resize_taps(64, 8, 0, 7) is not None and emu_lib.resize_taps(8, 64, 1, 63) is not None


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_the_restatement_is_an_antialiased_bilinear_resize(bd):
    """no library: the integer restatement against a float64 resize written independently, within B = 0.5 + 2^(bd-19) + (Tx + Ty) 2^(bd-14) samples —
    every coefficient is within 2^-14 of the real weight (T = ceil(2 max(1, ratio)) of them per axis, on samples below 2^bd), the rounding to the
    intermediate costs 2^(bd-19), the final rounding 0.5"""
    rng = np.random.default_rng(7810 + bd)
    for (sw, sh), (ow, oh) in [((64, 48), (8, 6)), ((64, 48), (48, 20)), ((40, 24), (64, 64)), ((17, 9), (3, 2)), ((12, 8), (96, 64)), ((96, 80), (13, 11))]:
        S = rng.integers(0, 1 << bd, (sh, sw))
        T = [math.ceil(2 * max(1.0, s / d)) for s, d in ((sw, ow), (sh, oh))]
        B = 0.5 + 2.0 ** (bd - 19) + (T[0] + T[1]) * 2.0 ** (bd - 14)
        for cosited in (0, 1):
            a = convert(resize_plane(S, ow, oh, cosited, bd), bd, capi.EXPORT_NATIVE, np.int64)
            err = float(np.abs(a - float_resize(S, ow, oh, cosited)).max())
            assert err <= B, "%dx%d -> %dx%d at %d bits, cosited %d: %.4f samples off, bound %.4f" % (sw, sh, ow, oh, bd, cosited, err, B)


@pytest.mark.parametrize("fmt", FORMATS, ids=format_id)
def test_resized_format_matrix(ctx, oracle, fmt):
    check_format_matrix_resized(ctx, Oracle(oracle), dict(fmt, width=64, height=32, log2_ctb=5))


@pytest.mark.parametrize("bit_depth,layout", [(8, capi.EXPORT_PLANAR), (8, capi.EXPORT_SEMIPLANAR), (10, capi.EXPORT_PLANAR), (10, capi.EXPORT_SEMIPLANAR)])
def test_same_size_is_the_plain_export(ctx, oracle, bit_depth, layout):
    check_identity(ctx, Oracle(oracle), bit_depth, layout)


def test_rectangle_equals_cropped_frame(ctx, oracle):
    check_rect_equals_cropped_frame(ctx, Oracle(oracle))


@pytest.mark.parametrize("bit_depth", [8, 10])
def test_resized_minimum_sizes(ctx, oracle, bit_depth):
    check_minimum_sizes(ctx, Oracle(oracle), bit_depth)


@pytest.mark.parametrize("bit_depth", [8, 12, 16])
def test_resized_values_and_roundings(ctx, bit_depth):
    check_values(ctx, bit_depth)


def test_resized_several_tiles(ctx):
    check_several_tiles(ctx)


def test_resized_export_rejects_bad_arguments(ctx):
    """every rejected case returns M355_ERR_INVALID and leaves the destination as it was allocated"""
    lib = ctx.L.lib
    frame = ctx.frame_create(64, 32, 1, 10, 10)
    f422 = ctx.frame_create(64, 32, 2, 10, 10)
    mono = ctx.frame_create(64, 40, 0, 8, 8)
    nbytes = 64 * 300
    bufs = [ctx.device_alloc(nbytes) for _ in range(3)]

    def desc(out=(32, 16), layout=capi.EXPORT_PLANAR, samples=capi.EXPORT_NATIVE, rect=(0, 0, 0, 0), dst=(0, 1, 2), pitch=(300, 300, 300)):
        d = capi.ResizeDesc(layout=layout, samples=samples, out_width=out[0], out_height=out[1])
        d.x0, d.y0, d.width, d.height = rect
        for j in range(3):
            d.dst[j] = bufs[dst[j]] if dst[j] is not None else None
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
        ("one sample beyond 8x down, width", mono, desc(out=(7, 40), rect=(0, 0, 57, 40), dst=(0, None, None))),
        ("one sample beyond 8x down, height", mono, desc(out=(64, 4), rect=(0, 0, 64, 33), dst=(0, None, None))),
        ("one sample beyond 8x up, width", mono, desc(out=(65, 20), rect=(0, 0, 8, 20), dst=(0, None, None))),
        ("one sample beyond 8x up, height", mono, desc(out=(32, 33), rect=(0, 0, 32, 4), dst=(0, None, None))),
        ("more than 8x up", frame, desc(out=(72, 16), rect=(0, 0, 8, 8))),
        ("luma pitch below the output row", frame, desc(pitch=(63, 300, 300))),
        ("chroma pitch below the output row", frame, desc(pitch=(300, 300, 31))),
        ("interleaved pitch below the output row", frame, desc(layout=capi.EXPORT_SEMIPLANAR, pitch=(300, 63, 300))),
        ("rectangle leaves the frame", frame, desc(rect=(32, 0, 48, 16))),
        ("rectangle off the chroma grid", frame, desc(rect=(1, 0, 16, 16))),
        ("rectangle of no width", frame, desc(rect=(0, 0, -4, 16))),
        ("no luma destination", frame, desc(dst=(None, 1, 2))),
        ("no Cr destination (planar)", frame, desc(dst=(0, 1, None))),
        ("no chroma destination (semi-planar)", frame, desc(layout=capi.EXPORT_SEMIPLANAR, dst=(0, None, 2))),
        ("unknown layout", frame, desc(layout=2)),
        ("unknown sample format", frame, desc(samples=3)),
    ]
    for what, f, d in bad:
        assert lib.m355_frame_export_resized(ctx.h, f, ctypes.byref(d)) == M355_ERR_INVALID, what
    assert lib.m355_frame_export_resized(ctx.h, frame, None) == M355_ERR_INVALID
    assert lib.m355_frame_export_resized(ctx.h, frame + 100, ctypes.byref(desc())) == M355_ERR_INVALID
    ctx.wait()
    for p in bufs:
        assert np.all(ctx.device_read(p, nbytes) == capi.DEVICE_FILL), "a rejected export wrote to its destination"
    # the ratio limit itself, and a pitch equal to the output row's bytes (32 10-bit samples: 64 bytes), are fine
    assert lib.m355_frame_export_resized(ctx.h, frame, ctypes.byref(desc(pitch=(64, 32, 32)))) == 0, ctx.L.error()
    assert lib.m355_frame_export_resized(ctx.h, frame, ctypes.byref(desc(layout=capi.EXPORT_SEMIPLANAR, pitch=(64, 64, 0)))) == 0, ctx.L.error()
    assert lib.m355_frame_export_resized(ctx.h, frame, ctypes.byref(desc(out=(8, 4)))) == 0, ctx.L.error()
    assert lib.m355_frame_export_resized(ctx.h, mono, ctypes.byref(desc(out=(7, 40), rect=(0, 0, 56, 40), dst=(0, None, None)))) == 0, ctx.L.error()
    assert lib.m355_frame_export_resized(ctx.h, mono, ctypes.byref(desc(out=(64, 32), rect=(0, 0, 8, 4), dst=(0, None, None)))) == 0, ctx.L.error()
    ctx.wait()
    for p in bufs:
        ctx.device_free(p)
    for f in (frame, f422):
        ctx.frame_destroy(f)
    # a monochrome frame exports luma only: dst[1], dst[2] and their pitches are ignored in both layouts
    luma = (np.arange(40 * 64, dtype=np.uint32) * 7 % 256).astype(np.uint8).reshape(40, 64)
    ctx.frame_upload(mono, [luma])
    for layout in LAYOUTS:
        got, raws = ctx.frame_export_finish(ctx.frame_export_resized(mono, layout, capi.EXPORT_MSB16, (24, 15)), raw=True)
        assert len(got) == 1
        assert_export(got, raws, [convert(resize_plane(luma, 24, 15, 0, 8), 8, capi.EXPORT_MSB16, np.uint8)], "monochrome")
    ctx.frame_destroy(mono)


def test_resized_export_behind_a_rejected_decode_writes_nothing(ctx):
    check_gate_resized(ctx)


@pytest.mark.parametrize("depth", [1, 3])
def test_resized_export_behind_recycled_frames(ctx, depth):
    """(the interpreter runs every launch to its end at once: this walks the reader bookkeeping, the GPU tier is what can see a missing wait)"""
    check_hazard_resized(ctx, depth)


def test_resized_export_into_pinned_host_memory(ctx, oracle):
    frame, planes, geom, frames = decode_into_frame(ctx, Oracle(oracle), dict(width=64, height=32, bit_depth=10, seed=7301, log2_ctb=5))
    check_export_resized(ctx, frame, planes, geom, capi.EXPORT_SEMIPLANAR, capi.EXPORT_MSB16, (36, 14), MATRIX_RECT, host=True, what="pinned")
    for f in frames:
        ctx.frame_destroy(f)


def test_resize_desc_abi():
    """sizeof and the field offsets of m355_resize_desc as the header declares it (LP64: eight int32, three pointers, three int64), against the ctypes
    structure; the header's field order is read from the header itself"""
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "de265_mi355x.h")).read()
    body = re.search(r"typedef struct m355_resize_desc \{(.*?)\} m355_resize_desc;", header, re.S).group(1)
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
    assert names == [n for n, _ in capi.ResizeDesc._fields_]
    for n in names:
        assert getattr(capi.ResizeDesc, n).offset == offsets[n], n
    assert ctypes.sizeof(capi.ResizeDesc) == (ofs + 7) // 8 * 8 == 80
    assert capi.RESIZE_MAX_TAPS == int(re.search(r"#define M355_RESIZE_MAX_TAPS (\d+)", header).group(1)) == 16
