"""m355_frames_export_tensor_rois on the SIMT-interpreter build: regions of one frame at both ratio limits, slices of different unit counts in one
grid, whole frames of different sizes, mirrored slices (the seam between two tiles, output rows that end in half a dword), the full record array, the
argument checks, the gate per slice, the reader bookkeeping and a pinned-host destination.  Every slice has two expectations
(export_tensor_rois_util.py): the restatement of the planes m355_frame_download returns, and m355_frames_export_tensor with n = 1 for the same frame
and rectangle; every comparison is bit-exact, and every byte of the destination outside the tensor's elements must be untouched.

The build holds four instantiations for this call, k_export_resized_rgb<source bytes, element bytes, RR_ROIS>; layout, F16 / BF16, chroma
format, U8 / U16 and the mirror are run-time switches.  Which test reaches which:
  <1, 2, RR_ROIS>, <1, 4, RR_ROIS>  test_regions_of_an_8bit_frame (4:2:0, two tiles across in every slice), test_mirror_at_odd_output_widths (monochrome,
                              <1, 2, RR_ROIS>), test_rois_gate_is_per_slice
  <2, 2, RR_ROIS>, <2, 4, RR_ROIS>  test_regions_of_one_frame, test_slices_of_different_unit_counts, test_whole_frames_of_different_sizes,
                              test_mirrored_regions_of_one_frame, test_mirror_across_the_seam_of_two_tiles, test_mirror_at_odd_output_widths (4:4:4,
                              <2, 2, RR_ROIS>), test_full_record_array, test_rois_export_behind_recycled_frames (<2, 2, RR_ROIS>),
                              test_rois_export_into_pinned_host_memory
The single calls they are held against run the RR_BATCH instantiations."""
import ctypes

import numpy as np
import pytest

from test_emu_picture import emu_lib  # noqa: F401  (fixture)
from oracle_py import Oracle
from export_tensor_rois_util import (M355_ERR_INVALID, MIRROR, check_composition, check_different_sizes, check_full_array, check_gate, check_hazard,
                                     check_mirror_odd_widths, check_mixed_8bit, check_mixed_units, check_pinned_host)
from libde265_amd import capi


@pytest.fixture()
def ctx(emu_lib):  # noqa: F811
    c = capi.Context(emu_lib, 0)
    yield c
    c.close()


def test_regions_of_one_frame(ctx, oracle):
    check_composition(ctx, Oracle(oracle))


def test_slices_of_different_unit_counts(ctx):
    check_mixed_units(ctx)


def test_regions_of_an_8bit_frame(ctx):
    check_mixed_8bit(ctx)


def test_whole_frames_of_different_sizes(ctx, oracle):
    check_different_sizes(ctx, Oracle(oracle))


def test_mirrored_regions_of_one_frame(ctx, oracle):
    check_composition(ctx, Oracle(oracle), mirrored=True)


def test_mirror_across_the_seam_of_two_tiles(ctx):
    check_mixed_units(ctx, mirrored=True)


def test_mirror_at_odd_output_widths(ctx, oracle):
    check_mirror_odd_widths(ctx, Oracle(oracle))


def test_full_record_array(ctx, oracle):
    check_full_array(ctx, Oracle(oracle))


def test_rois_export_rejects_bad_arguments(ctx):
    """every rejected case returns M355_ERR_INVALID, names the entry point in the message and leaves the destination as it was allocated; the limits
    themselves are accepted"""
    lib = ctx.L.lib
    frame = ctx.frame_create(64, 32, 1, 10, 10)
    large = ctx.frame_create(128, 64, 1, 10, 10)
    small = ctx.frame_create(32, 16, 1, 10, 10)
    f422 = ctx.frame_create(64, 32, 2, 10, 10)
    depth8 = ctx.frame_create(64, 32, 1, 8, 8)
    depth12 = ctx.frame_create(64, 32, 1, 12, 12)
    depth9c = ctx.frame_create(64, 32, 1, 10, 9)
    mono = ctx.frame_create(64, 40, 0, 8, 8)
    nbytes = 1 << 16
    buf = ctx.device_alloc(nbytes)
    inf, nan = float("inf"), float("nan")
    W = (0, 0, 0, 0, 0)                       # the whole frame

    def desc(out=(32, 16), layout=capi.TENSOR_NCHW, dtype=capi.TENSOR_F16, samples=capi.RGB_U8, matrix=capi.MATRIX_BT709, full=0, rect=(0, 0, 0, 0),
             scale=(1, 1, 1), bias=(0, 0, 0), dst=0, sn=4096, sc=1200, sh=72):
        d = capi.TensorDesc(layout=layout, dtype=dtype, samples=samples, matrix=matrix, full_range=full, out_width=out[0], out_height=out[1],
                            stride_n=sn, stride_c=sc, stride_h=sh)
        d.x0, d.y0, d.width, d.height = rect
        d.scale = (ctypes.c_float * 3)(*scale)
        d.bias = (ctypes.c_float * 3)(*bias)
        d.dst = None if dst is None else buf + dst
        return d

    def call(frames, rois, d, n=None):
        arr = (ctypes.c_int * max(1, len(frames)))(*frames)
        ra = (capi.TensorRoi * max(1, len(rois)))(*[capi.TensorRoi(*r) for r in rois])
        return lib.m355_frames_export_tensor_rois(ctx.h, arr, ra, len(frames) if n is None else n, ctypes.byref(d) if d is not None else None)

    two = [frame, frame]
    E = 15 * 72 + 64                          # 32x16 F16 NCHW: row 64 bytes, E = 15 * stride_h + 64; NHWC row 192 bytes
    En = 15 * 200 + 192
    bad = [
        ("n 0", [frame], [W], desc(), 0),
        ("n negative", [frame], [W], desc(), -1),
        ("n above the limit", [frame] * 33, [W] * 33, desc(), None),
        ("a bad handle", [frame, frame + 100], [W, W], desc(), None),
        ("a negative handle", [-1], [W], desc(), None),
        ("another chroma format", [frame, f422], [W, W], desc(), None),
        ("another element size", [frame, depth8], [W, W], desc(), None),
        ("another luma bit depth", [frame, depth12], [W, W], desc(), None),
        ("another chroma bit depth", [frame, depth9c], [W, W], desc(), None),
        ("a nonzero descriptor rectangle", two, [W, W], desc(rect=(0, 0, 64, 32)), None),
        ("a descriptor rectangle with x0 alone", two, [W, W], desc(rect=(2, 0, 0, 0)), None),
        ("a descriptor rectangle with a height alone", two, [W, W], desc(rect=(0, 0, 0, 8)), None),
        ("an unknown flag bit", two, [W, (0, 0, 64, 32, 2)], desc(), None),
        ("an unknown flag bit beside the known one", two, [(0, 0, 64, 32, 3), W], desc(), None),
        ("a negative flags word", two, [W, (0, 0, 64, 32, -1)], desc(), None),
        ("an entry that fits frames[0] but not its own frame", [large, frame], [(0, 0, 64, 32, 0), (64, 32, 64, 32, 0)], desc(), None),
        ("an entry that leaves its small frame", [frame, small], [W, (0, 0, 64, 32, 0)], desc(), None),
        ("the first entry leaves its frame", [small, frame], [(0, 0, 64, 32, 0), W], desc(), None),
        ("rectangle leaves the frame to the right", two, [W, (32, 0, 48, 16, 0)], desc(), None),
        ("rectangle off the chroma grid", two, [W, (1, 0, 16, 16, 0)], desc(), None),
        ("rectangle of an odd height, 4:2:0", two, [W, (0, 0, 16, 15, 0)], desc(), None),
        ("rectangle of a negative width", two, [W, (0, 0, -4, 16, 0)], desc(), None),
        ("rectangle of a negative height", two, [W, (0, 0, 16, -4, 0)], desc(), None),
        ("rectangle of no height", two, [W, (0, 0, 16, 0, 0)], desc(), None),
        ("out_width 0", two, [W, W], desc(out=(0, 16)), None),
        ("out_height negative", two, [W, W], desc(out=(32, -16)), None),
        ("out_width odd, 4:2:0", two, [W, W], desc(out=(33, 16), sh=80), None),
        ("out_height odd, 4:2:0", two, [W, W], desc(out=(32, 17), sc=1300), None),
        ("more than 8x down, every entry", two, [W, W], desc(out=(6, 16)), None),
        ("8x up exceeded by one entry only", two, [W, (0, 0, 2, 2, 0)], desc(), None),
        ("8x up exceeded by the first entry only", two, [(0, 0, 2, 32, 0), W], desc(), None),
        ("8x down exceeded by one entry only", [frame, large], [W, W], desc(out=(14, 16), sh=40), None),
        ("one sample beyond 8x down", [mono, mono], [(0, 0, 56, 40, 0), (0, 0, 57, 40, 0)], desc(out=(7, 40), sc=4000, sn=16384), None),
        ("one sample beyond 8x up", [mono, mono], [(0, 0, 9, 20, 0), (0, 0, 8, 20, 0)], desc(out=(65, 20), sh=136, sc=4000, sn=16384), None),
        ("unknown samples", two, [W, W], desc(samples=2), None),
        ("unknown matrix", two, [W, W], desc(matrix=3), None),
        ("negative matrix", two, [W, W], desc(matrix=-1), None),
        ("full_range 2", two, [W, W], desc(full=2), None),
        ("unknown layout", two, [W, W], desc(layout=2), None),
        ("unknown dtype", two, [W, W], desc(dtype=3), None),
        ("scale infinite", two, [W, W], desc(scale=(1, inf, 1)), None),
        ("bias NaN", two, [W, W], desc(bias=(0, nan, 0)), None),
        ("no destination", two, [W, W], desc(dst=None), None),
        ("F16 destination at an odd address", two, [W, W], desc(dst=1), None),
        ("F32 destination off a multiple of 4", two, [W, W], desc(dtype=capi.TENSOR_F32, dst=2, sh=128, sc=2048, sn=8192), None),
        ("F16 stride_h odd", two, [W, W], desc(sh=73), None),
        ("F16 stride_c odd", two, [W, W], desc(sc=1201), None),
        ("F16 stride_n odd", two, [W, W], desc(sn=4097), None),
        ("NCHW stride_h one element below the row", two, [W, W], desc(sh=62), None),
        ("NHWC stride_h one element below the row", two, [W, W], desc(layout=capi.TENSOR_NHWC, sh=190), None),
        ("stride_h negative", two, [W, W], desc(sh=-72), None),
        ("NCHW stride_c one element below E", two, [W, W], desc(sc=E - 2, sn=8192), None),
        ("NCHW stride_n one element below 2 stride_c + E", two, [W, W], desc(sc=E, sn=3 * E - 2), None),
        ("NHWC stride_n one element below E", two, [W, W], desc(layout=capi.TENSOR_NHWC, sh=200, sn=En - 2), None),
        ("stride_n negative", two, [W, W], desc(sn=-4096), None),
    ]
    for what, frames, rois, d, n in bad:
        assert call(frames, rois, d, n) == M355_ERR_INVALID, what
        assert "m355_frames_export_tensor_rois" in ctx.L.error() or "handle" in ctx.L.error() or "m355_rgb_coefficients" in ctx.L.error(), (what, ctx.L.error())
    one = (ctypes.c_int * 1)(frame)
    roi = (capi.TensorRoi * 1)(capi.TensorRoi(*W))
    assert lib.m355_frames_export_tensor_rois(ctx.h, one, None, 1, ctypes.byref(desc())) == M355_ERR_INVALID, "null rois"
    assert "m355_frames_export_tensor_rois" in ctx.L.error()
    assert lib.m355_frames_export_tensor_rois(ctx.h, None, roi, 1, ctypes.byref(desc())) == M355_ERR_INVALID
    assert lib.m355_frames_export_tensor_rois(ctx.h, one, roi, 1, None) == M355_ERR_INVALID
    assert lib.m355_frames_export_tensor_rois(None, one, roi, 1, ctypes.byref(desc())) == M355_ERR_INVALID
    ctx.wait()
    assert np.all(ctx.device_read(buf, nbytes) == capi.DEVICE_FILL), "a rejected export wrote to its destination"
    # the limits themselves: exactly 8x down and 8x up in one batch, 32 entries, dense strides, frames of different sizes as whole frames and with a
    # region that only its own frame contains, mirror on every entry
    good = [
        ("dense NCHW", two, [W, (0, 0, 32, 16, MIRROR)], desc(sh=64, sc=16 * 64, sn=3 * 16 * 64)),
        ("NHWC at E", two, [W, W], desc(layout=capi.TENSOR_NHWC, sh=200, sc=-7, sn=En)),
        ("one entry, stride_n unused", [frame], [W], desc(sn=-3)),
        ("32 entries", [frame] * 32, [(2 * k, 0, 64 - 2 * k, 32, k & 1) for k in range(32)], desc(out=(8, 4), sh=16, sc=64, sn=192)),
        ("exactly 8x down beside exactly 1x", [mono, mono], [(0, 0, 56, 40, 0), (3, 0, 7, 40, MIRROR)], desc(out=(7, 40), sc=4000, sn=16384)),
        ("exactly 8x up twice", [mono, mono], [(0, 0, 8, 4, 0), (1, 1, 8, 4, MIRROR)], desc(out=(64, 32), sh=128, sc=4096, sn=16384)),
        ("exactly 8x down beside exactly 8x up", [mono, mono], [(0, 0, 64, 32, 0), (5, 5, 1, 1, MIRROR)], desc(out=(8, 4), sh=16, sc=64, sn=192)),
        ("whole frames of different sizes", [frame, large, small], [W, W, W], desc(sn=4096)),
        ("a region that only its own frame contains", [frame, large], [W, (64, 32, 64, 32, 0)], desc()),
    ]
    for what, frames, rois, d in good:
        assert call(frames, rois, d) == 0, "%s: %s" % (what, ctx.L.error())
    ctx.wait()
    ctx.device_free(buf)
    for f in (frame, large, small, f422, depth8, depth12, depth9c, mono):
        ctx.frame_destroy(f)


def test_rois_gate_is_per_slice(ctx):
    check_gate(ctx)


@pytest.mark.parametrize("depth", [1, 3])
def test_rois_export_behind_recycled_frames(ctx, depth):
    """(the interpreter runs every launch to its end at once: this walks the reader bookkeeping, the GPU tier is what can see a missing wait)"""
    check_hazard(ctx, depth)


def test_rois_export_into_pinned_host_memory(ctx, oracle):
    check_pinned_host(ctx, Oracle(oracle))
