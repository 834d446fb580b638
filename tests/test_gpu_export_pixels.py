"""m355_frame_export_pixels and m355_frame_export_resized_pixels on the GPU: the format matrix of tests/test_export_pixels_emu.py through the real
k_export_pixels / k_export_rgb / k_export_resized_rgb instantiations, every c10 on the device, rows that span several wavefronts with a partial last
one, resized pictures of two column tiles with both filters, a colour object and a tone object, the frame hazard (a decode into a frame waits for the
pixels export of the frame's previous picture) with one and three pictures in flight, and the gate.  Expected values: the planes m355_frame_download
returns through the Python-integer restatements and export_pixels_util.pixel_pack; all exact, guard bytes included."""
import numpy as np
import pytest

import export_colour_util as cu
import export_pixels_util as pu
import export_tone_util as tu
from libde265_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    lib = capi.Library()
    assert lib.device_count() >= 1
    c = capi.Context(lib, 0)
    yield c
    c.close()


@pytest.mark.parametrize("cf,bit_depth", pu.SOURCES)
def test_pixels_format_matrix(ctx, cf, bit_depth):
    pu.check_format_matrix(ctx, cf, bit_depth)


def test_every_c10_on_the_device(ctx):
    """a 256x256 monochrome 16-bit full-range frame with sample 256 y + x: cy = 1 << F, so R = G = B = Y and every 16-bit value occurs once; all
    65536 pixels of both 10-bit formats against m355_pixel_pack"""
    luma = np.arange(65536, dtype=np.uint16).reshape(256, 256)
    k = ctx.rgb_coefficients(capi.MATRIX_BT709, 1, 16, 16, capi.RGB_U16)
    assert k["cy"] == 1 << k["F"] and k["y0"] == 0
    frame = pu.upload(ctx, [luma], 0, 16)
    try:
        for f in pu.TEN:
            got = pu.finish(ctx, ctx.frame_export_pixels(frame, f, 1, capi.MATRIX_BT709, 1))[0]
            want = np.frombuffer(b"".join(ctx.pixel_pack(f, (v, v, v), 1) for v in range(65536)), np.uint8).reshape(256, 1024)
            assert np.array_equal(got, want), pu.NAMES[f]
            assert np.array_equal(want, pu.pack_planes(f, [luma] * 3, 1))
    finally:
        ctx.frame_destroy(frame)


@pytest.mark.parametrize("width,bit_depth", [(1040, 8), (528, 10)])
def test_pixels_rows_that_span_wavefronts(ctx, width, bit_depth):
    """a wavefront covers 64 lanes x NP pixels — 1024 of an 8-bit source, 512 of a 10-bit one —, so these rows take two, the second partial; the
    rectangle starts at x = 6, off a vector boundary, and ends in a partial lane"""
    planes = cu.random_planes(bit_depth, 8900 + bit_depth, (width, 16))
    frame = pu.upload(ctx, planes, 1, bit_depth)
    try:
        for f in (capi.PIXEL_BGRA8, capi.PIXEL_A2R10G10B10):
            for rect in (None, (6, 0, width - 6, 16)):
                pu.check_pixels(ctx, frame, planes, (1, bit_depth, bit_depth), f, capi.MATRIX_BT709, 0, rect, what="%d wide" % width)
    finally:
        ctx.frame_destroy(frame)


@pytest.mark.parametrize("name", ["plain", "colour", "tone"])
def test_resized_pixels(ctx, name):
    """544x32 to 272x16 (two tiles of 256 columns, the second partial) and 64x32 to 96x48, both filters, every format; without an object, with a colour
    object and with a tone object"""
    S = {"plain": None, "colour": cu.RANDOM, "tone": tu.RANDOM}[name]
    colour = tu.create(ctx, S) if S is not None else 0
    try:
        for size, out_size, bd in (((544, 32), (272, 16), 10), ((64, 32), (96, 48), 8)):
            planes = cu.random_planes(bd, 8910 + bd, size)
            frame = pu.upload(ctx, planes, 1, bd)
            try:
                for filt in (pu.TRIANGLE, pu.CUBIC):
                    for f in pu.FORMATS:
                        pu.check_resized_pixels(ctx, frame, planes, (1, bd, bd), f, cu.MATRIX, cu.FULL, out_size, None, 2 if filt == pu.CUBIC else 0, filt, S, colour,
                                                "gpu %s" % (size,), what=name)
            finally:
                ctx.frame_destroy(frame)
    finally:
        if colour:
            ctx.colour_destroy(colour)


@pytest.mark.parametrize("resized", [False, True], ids=["plain", "resized"])
@pytest.mark.parametrize("depth", [1, 3])
def test_pixels_export_is_waited_for_by_the_next_decode(ctx, depth, resized):
    pu.check_hazard(ctx, depth, resized)


@pytest.mark.parametrize("resized", [False, True], ids=["plain", "resized"])
def test_pixels_export_behind_a_rejected_decode_writes_nothing(ctx, resized):
    pu.check_gate(ctx, resized)
