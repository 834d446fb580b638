"""m355_frame_export_oriented and m355_frame_export_pixels_oriented on the SIMT-interpreter build: all eight orientations on every layout and sample
format of 4:2:0 (8 and 10 bits), 4:4:4 and monochrome frames — and the four non-transposing ones on 4:2:2 —, on a frame whose luma and chroma planes
span several 64-element tiles with a partial last one in both directions, a rectangle of it that starts off a vector boundary and ends in a partial
lane, and the smallest frame there is (chroma below one vector and one tile); odd destination addresses and pitches; the pixels call with every
four-byte format, two chroma sample location types; identity; every rejection; the gate, the reader bookkeeping and a pinned-host destination.
Expected values: export_oriented_util — orient of the restatements and orient of the plain calls' output, all exact, guard bytes included."""
import ctypes

import numpy as np
import pytest

from test_emu_picture import emu_lib  # noqa: F401  (fixture)
import export_oriented_util as ou
import export_pixels_util as pu
import export_util as eu
from export_oriented_util import BIG, BIG_RECT, M355_ERR_INVALID, NON_TRANSPOSING, ORIENTATIONS, SMALL
from libde265_amd import capi


@pytest.fixture()
def ctx(emu_lib):  # noqa: F811
    c = capi.Context(emu_lib, 0)
    yield c
    c.close()


@pytest.mark.parametrize("cf,bit_depth", [(1, 8), (1, 10), (3, 10), (0, 8)])
def test_oriented_tiles_and_partial_lanes(ctx, cf, bit_depth):
    """264x136: 5 x 3 luma tiles and, for 4:2:0, 3 x 2 chroma tiles, the last partial in both directions; whole, and the rectangle (6, 2, 250, 130)"""
    ou.check_source(ctx, cf, bit_depth, BIG, (None, BIG_RECT))


@pytest.mark.parametrize("cf,bit_depth", [(1, 8), (1, 10), (3, 10), (0, 8)])
def test_oriented_smallest_frame(ctx, cf, bit_depth):
    """8x8: a 4:2:0 chroma plane of 4 x 4 samples, less than a 16-byte vector and less than a tile in both directions"""
    ou.check_source(ctx, cf, bit_depth, SMALL, (None,))


def test_oriented_422_without_transpose(ctx):
    ou.check_source(ctx, 2, 10, BIG, (None, BIG_RECT), NON_TRANSPOSING)
    ou.check_source(ctx, 2, 10, SMALL, (None,), NON_TRANSPOSING)


@pytest.mark.parametrize("o", ORIENTATIONS[1:])
def test_oriented_odd_address_and_odd_pitch(ctx, o):
    ou.check_odd_destination(ctx, o)


@pytest.mark.parametrize("bit_depth", [8, 10])
def test_pixels_oriented(ctx, bit_depth):
    """every four-byte format x chroma_loc 0 and 2 x the whole frame and the partial-lane rectangle x all eight orientations"""
    ou.check_pixels_source(ctx, 1, bit_depth, BIG, (None, BIG_RECT))
    ou.check_pixels_source(ctx, 1, bit_depth, SMALL, (None,), formats=(capi.PIXEL_BGRA8, capi.PIXEL_A2B10G10R10))


def test_pixels_oriented_other_chroma_formats(ctx):
    for cf, bd in ((0, 8), (3, 10)):
        ou.check_pixels_source(ctx, cf, bd, (136, 72), (None, (6, 2, 122, 66)), formats=(capi.PIXEL_RGBA8, capi.PIXEL_A2R10G10B10))
    ou.check_pixels_source(ctx, 2, 10, (136, 72), (None, (6, 2, 122, 66)), formats=(capi.PIXEL_BGRA8,))


def test_mirror_of_left_sited_chroma_differs_from_converting_mirrored_planes():
    """from the restatements alone — why the pixels call exists: R'G'B' of the mirrored 4:2:0 planes is not the mirrored R'G'B' (left-sited chroma
    mirrored sits on odd luma columns), so orientation 1 of the pixels call is not the planes call followed by a conversion"""
    planes = ou.random_planes(1, 8, 9400, (32, 16))
    f, a = capi.PIXEL_RGBA8, 255
    turned = pu.expected_pixels([ou.orient(p, 1) for p in planes], 1, 8, 8, f, a, capi.MATRIX_BT709, 0)
    want = ou.orient_rows(pu.expected_pixels(planes, 1, 8, 8, f, a, capi.MATRIX_BT709, 0), 1, 4)
    assert not np.array_equal(turned, want)


def test_orientation_zero_is_the_plain_call(ctx):
    """byte-identical to m355_frame_export / m355_frame_export_pixels, BGR8 included.  (That orientation 0 does not launch the new kernel cannot be
    asserted here: the interpreter build keeps no launch accounting — simt::launch takes the kernel's name for block ordering only.  The dispatch
    is visible in the results instead: BGR8, which the oriented kernels reject, is delivered.)"""
    planes = ou.random_planes(1, 10, 9500, (72, 40))
    frame = pu.upload(ctx, planes, 1, 10)
    try:
        for layout in eu.LAYOUTS:
            for samples in eu.SAMPLES:
                for rect in (None, (6, 2, 58, 34)):
                    got, raws = ctx.frame_export_finish(ctx.frame_export_oriented(frame, layout, samples, 0, rect), raw=True)
                    want, wraws = ctx.frame_export_finish(ctx.frame_export(frame, layout, samples, rect), raw=True)
                    assert all(np.array_equal(g, w) for g, w in zip(raws, wraws)) and len(got) == len(want)
        for f in pu.FORMATS:
            for loc in (0, 2):
                got = pu.finish(ctx, ctx.frame_export_pixels_oriented(frame, f, pu.alpha_for(f), capi.MATRIX_BT709, 0, 0, (6, 2, 58, 34), chroma_loc=loc))
                want = pu.finish(ctx, ctx.frame_export_pixels(frame, f, pu.alpha_for(f), capi.MATRIX_BT709, 0, (6, 2, 58, 34), chroma_loc=loc))
                assert np.array_equal(got[1][0], want[1][0]), pu.NAMES[f]
    finally:
        ctx.frame_destroy(frame)


def test_oriented_exports_reject_bad_arguments(ctx):
    """every rejected case of both calls returns M355_ERR_INVALID and leaves the destination as it was allocated"""
    lib = ctx.L.lib
    frame = ctx.frame_create(64, 32, 1, 10, 10)
    f422 = ctx.frame_create(64, 32, 2, 10, 10)
    nbytes = 64 * 400
    buf = ctx.device_alloc(nbytes)

    def desc(layout=capi.EXPORT_PLANAR, samples=capi.EXPORT_NATIVE, rect=(0, 0, 0, 0), dst=(True, True, True), pitch=(400, 400, 400)):
        d = capi.ExportDesc(layout=layout, samples=samples)
        d.x0, d.y0, d.width, d.height = rect
        for k in range(3):
            d.dst[k] = buf if dst[k] else None
            d.pitch[k] = pitch[k]
        return d

    def pdesc(format=capi.PIXEL_RGBA8, alpha=0, matrix=capi.MATRIX_BT709, full=0, rect=(0, 0, 0, 0), out=(0, 0), dst=True, pitch=400, ofs=0):
        d = capi.PixelDesc(format=format, alpha=alpha, matrix=matrix, full_range=full, out_width=out[0], out_height=out[1])
        d.x0, d.y0, d.width, d.height = rect
        d.dst = buf + ofs if dst else None
        d.pitch = pitch
        return d

    yuv = [
        ("orientation 8", {}, 8), ("orientation -1", {}, -1),
        ("rectangle leaves the frame", dict(rect=(32, 0, 48, 16)), 5), ("rectangle off the chroma grid", dict(rect=(1, 0, 16, 16)), 1),
        ("unknown layout", dict(layout=2), 3), ("unknown samples", dict(samples=3), 6),
        ("no chroma destination", dict(dst=(True, False, True)), 2),
        ("luma pitch below the row", dict(pitch=(127, 400, 400)), 1),
        ("chroma pitch below the row", dict(pitch=(400, 63, 400)), 3),
        ("pitch below the TRANSPOSED row of a rectangle", dict(rect=(0, 0, 16, 32), pitch=(63, 400, 400)), 4),
        ("pitch below the transposed interleaved row", dict(layout=capi.EXPORT_SEMIPLANAR, rect=(0, 0, 16, 32), pitch=(400, 63, 400)), 7),
    ]
    for what, a, o in yuv:
        assert lib.m355_frame_export_oriented(ctx.h, frame, ctypes.byref(desc(**a)), o) == M355_ERR_INVALID, what
    for o in ou.TRANSPOSING:
        assert lib.m355_frame_export_oriented(ctx.h, f422, ctypes.byref(desc()), o) == M355_ERR_INVALID, "TRANSPOSE on 4:2:2"
    assert lib.m355_frame_export_oriented(ctx.h, frame, None, 1) == M355_ERR_INVALID
    assert lib.m355_frame_export_oriented(ctx.h, frame + 100, ctypes.byref(desc()), 1) == M355_ERR_INVALID
    px = [
        ("orientation 8", {}, None, 8), ("orientation -1", {}, None, -1),
        ("BGR8", dict(format=capi.PIXEL_BGR8), None, 1), ("BGR8 transposed", dict(format=capi.PIXEL_BGR8), None, 5),
        ("unknown format", dict(format=5), None, 2), ("alpha 256", dict(alpha=256), None, 3), ("unknown matrix", dict(matrix=3), None, 4),
        ("rectangle leaves the frame", dict(rect=(32, 0, 48, 16)), None, 5),
        ("no destination", dict(dst=False), None, 6), ("an address off a dword", dict(ofs=2), None, 7), ("a pitch off a dword", dict(pitch=398), None, 1),
        ("pitch below the row", dict(pitch=252), None, 3),
        ("pitch below the TRANSPOSED row of a rectangle", dict(rect=(0, 0, 16, 32), pitch=124), None, 5),
        ("an output size", dict(out=(64, 32)), None, 1),
        ("chroma sample location type 4", {}, capi.ExportOpts(chroma_loc=4), 1), ("a filter", {}, capi.ExportOpts(filter=1), 2),
    ]
    for what, a, o, orientation in px:
        assert lib.m355_frame_export_pixels_oriented(ctx.h, frame, ctypes.byref(pdesc(**a)), None if o is None else ctypes.byref(o), orientation) == M355_ERR_INVALID, what
    assert lib.m355_frame_export_pixels_oriented(ctx.h, frame, None, None, 1) == M355_ERR_INVALID
    assert lib.m355_frame_export_pixels_oriented(ctx.h, frame + 100, ctypes.byref(pdesc()), None, 1) == M355_ERR_INVALID
    ctx.wait()
    assert np.all(ctx.device_read(buf, nbytes) == capi.DEVICE_FILL), "a rejected export wrote to its destination"
    # the limits themselves are fine: pitches equal to the oriented rows
    assert lib.m355_frame_export_oriented(ctx.h, frame, ctypes.byref(desc(rect=(0, 0, 16, 32), pitch=(64, 32, 32))), 4) == 0, ctx.L.error()
    assert lib.m355_frame_export_oriented(ctx.h, frame, ctypes.byref(desc(rect=(0, 0, 16, 32), pitch=(32, 16, 16))), 1) == 0, ctx.L.error()
    assert lib.m355_frame_export_pixels_oriented(ctx.h, frame, ctypes.byref(pdesc(rect=(0, 0, 16, 32), pitch=128)), None, 5) == 0, ctx.L.error()
    assert lib.m355_frame_export_pixels_oriented(ctx.h, f422, ctypes.byref(pdesc()), None, 5) == 0, ctx.L.error()   # (pixels have no 4:4:0)
    ctx.wait()
    ctx.device_free(buf)
    ctx.frame_destroy(frame)
    ctx.frame_destroy(f422)


CALLS = {"nv_msb16_cw": ou.yuv_call(capi.EXPORT_SEMIPLANAR, capi.EXPORT_MSB16, capi.ORIENT_ROTATE_90_CW),
         "planar_u8_mirror": ou.yuv_call(capi.EXPORT_PLANAR, capi.EXPORT_U8, capi.ORIENT_MIRROR),
         "bgra8_ccw": ou.pixels_call(capi.PIXEL_BGRA8, capi.ORIENT_ROTATE_90_CCW),
         "a2r10_180": ou.pixels_call(capi.PIXEL_A2R10G10B10, capi.ORIENT_ROTATE_180)}


@pytest.mark.parametrize("name", list(CALLS))
def test_oriented_export_behind_a_rejected_decode_writes_nothing(ctx, name):
    ou.check_gate(ctx, CALLS[name])


@pytest.mark.parametrize("name", ["nv_msb16_cw", "bgra8_ccw"])
@pytest.mark.parametrize("depth", [1, 3])
def test_oriented_export_behind_recycled_frames(ctx, depth, name):
    """(the interpreter runs every launch to its end at once: this walks the reader bookkeeping, the GPU tier is what can see a missing wait)"""
    ou.check_hazard(ctx, depth, CALLS[name])


def test_oriented_export_into_pinned_host_memory(ctx):
    planes = ou.random_planes(1, 10, 9600, (72, 40))
    frame = pu.upload(ctx, planes, 1, 10)
    try:
        for o in (1, 5):
            ou.check_oriented(ctx, frame, planes, (1, 10, 10), capi.EXPORT_SEMIPLANAR, capi.EXPORT_MSB16, o, (2, 2, 48, 16), host=True, what="pinned")
            ou.check_pixels_oriented(ctx, frame, planes, (1, 10, 10), capi.PIXEL_BGRA8, o, (2, 2, 48, 16), host=True, what="pinned")
    finally:
        ctx.frame_destroy(frame)
