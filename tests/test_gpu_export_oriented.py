"""m355_frame_export_oriented and m355_frame_export_pixels_oriented on the GPU: the matrix of tests/test_export_oriented_emu.py through the real
k_export_oriented / k_export_pixels_oriented instantiations — all eight orientations, every layout and sample format, frames of several 64-element
tiles with partial last ones, the partial-lane rectangle, the smallest frame, odd destination addresses —, oriented rows that span several wavefronts
with a partial last one, the frame hazard (a decode into a frame waits for the oriented export of the frame's previous picture) with one and three
pictures in flight, and the gate.  Expected values: export_oriented_util — orient of the restatements and orient of the plain calls' output on the same
device; all exact, guard bytes included."""
import numpy as np
import pytest

import export_oriented_util as ou
import export_pixels_util as pu
import export_util as eu
from export_oriented_util import BIG, BIG_RECT, NON_TRANSPOSING, ORIENTATIONS, SMALL
from libde265_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    lib = capi.Library()
    assert lib.device_count() >= 1
    c = capi.Context(lib, 0)
    yield c
    c.close()


@pytest.mark.parametrize("cf,bit_depth", [(1, 8), (1, 10), (3, 10), (0, 8)])
def test_oriented_tiles_and_partial_lanes(ctx, cf, bit_depth):
    ou.check_source(ctx, cf, bit_depth, BIG, (None, BIG_RECT))
    ou.check_source(ctx, cf, bit_depth, SMALL, (None,))


def test_oriented_422_without_transpose(ctx):
    ou.check_source(ctx, 2, 10, BIG, (None, BIG_RECT), NON_TRANSPOSING)


def test_oriented_odd_address_and_odd_pitch(ctx):
    for o in ORIENTATIONS[1:]:
        ou.check_odd_destination(ctx, o)


@pytest.mark.parametrize("bit_depth", [8, 10])
def test_pixels_oriented(ctx, bit_depth):
    ou.check_pixels_source(ctx, 1, bit_depth, BIG, (None, BIG_RECT))
    ou.check_pixels_source(ctx, 1, bit_depth, SMALL, (None,), formats=(capi.PIXEL_BGRA8, capi.PIXEL_A2B10G10R10))


def test_pixels_oriented_other_chroma_formats(ctx):
    for cf, bd in ((0, 8), (3, 10), (2, 10)):
        ou.check_pixels_source(ctx, cf, bd, (136, 72), (None, (6, 2, 122, 66)), formats=(capi.PIXEL_RGBA8, capi.PIXEL_A2R10G10B10))


@pytest.mark.parametrize("o", [1, 5, 6])
def test_oriented_rows_that_span_wavefronts(ctx, o):
    """a 1040x1032 monochrome 8-bit plane: a wavefront covers 1024 destination bytes, so the oriented rows (1040 wide mirrored, 1032 wide rotated) take
    two, the second partial; the rectangle starts off a vector boundary and ends in a partial lane"""
    luma = ou.random_planes(0, 8, 9700, (1040, 1032))
    frame = pu.upload(ctx, luma, 0, 8)
    try:
        for rect in (None, (6, 2, 1027, 1029)):
            ou.check_oriented(ctx, frame, luma, (0, 8, 8), capi.EXPORT_PLANAR, capi.EXPORT_NATIVE, o, rect, what="1040x1032")
        ou.check_oriented(ctx, frame, luma, (0, 8, 8), capi.EXPORT_PLANAR, capi.EXPORT_MSB16, o, what="1040x1032")
    finally:
        ctx.frame_destroy(frame)


@pytest.mark.parametrize("o", [1, 5])
def test_pixels_oriented_rows_that_span_wavefronts(ctx, o):
    """1040x72 8-bit 4:2:0: a wavefront of the non-transposing path covers 1024 pixels, a row of tiles of the transposing one 17 tiles"""
    planes = ou.random_planes(1, 8, 9710, (1040, 72))
    frame = pu.upload(ctx, planes, 1, 8)
    try:
        for rect in (None, (6, 2, 1030, 66)):
            ou.check_pixels_oriented(ctx, frame, planes, (1, 8, 8), capi.PIXEL_BGRA8, o, rect, what="1040x72")
    finally:
        ctx.frame_destroy(frame)


def test_orientation_zero_is_the_plain_call(ctx):
    planes = ou.random_planes(1, 10, 9500, (72, 40))
    frame = pu.upload(ctx, planes, 1, 10)
    try:
        for layout in eu.LAYOUTS:
            got = ctx.frame_export_finish(ctx.frame_export_oriented(frame, layout, capi.EXPORT_MSB16, 0, (6, 2, 58, 34)), raw=True)[1]
            want = ctx.frame_export_finish(ctx.frame_export(frame, layout, capi.EXPORT_MSB16, (6, 2, 58, 34)), raw=True)[1]
            assert all(np.array_equal(g, w) for g, w in zip(got, want))
        for f in pu.FORMATS:
            got = pu.finish(ctx, ctx.frame_export_pixels_oriented(frame, f, pu.alpha_for(f), capi.MATRIX_BT709, 0, 0, (6, 2, 58, 34)))
            want = pu.finish(ctx, ctx.frame_export_pixels(frame, f, pu.alpha_for(f), capi.MATRIX_BT709, 0, (6, 2, 58, 34)))
            assert np.array_equal(got[1][0], want[1][0]), pu.NAMES[f]
    finally:
        ctx.frame_destroy(frame)


CALLS = {"nv_msb16_cw": ou.yuv_call(capi.EXPORT_SEMIPLANAR, capi.EXPORT_MSB16, capi.ORIENT_ROTATE_90_CW),
         "planar_u8_mirror": ou.yuv_call(capi.EXPORT_PLANAR, capi.EXPORT_U8, capi.ORIENT_MIRROR),
         "bgra8_ccw": ou.pixels_call(capi.PIXEL_BGRA8, capi.ORIENT_ROTATE_90_CCW),
         "a2r10_180": ou.pixels_call(capi.PIXEL_A2R10G10B10, capi.ORIENT_ROTATE_180)}


@pytest.mark.parametrize("name", list(CALLS))
@pytest.mark.parametrize("depth", [1, 3])
def test_oriented_export_is_waited_for_by_the_next_decode(ctx, depth, name):
    ou.check_hazard(ctx, depth, CALLS[name])


@pytest.mark.parametrize("name", list(CALLS))
def test_oriented_export_behind_a_rejected_decode_writes_nothing(ctx, name):
    ou.check_gate(ctx, CALLS[name])
