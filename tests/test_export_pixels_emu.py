"""m355_frame_export_pixels and m355_frame_export_resized_pixels on the SIMT-interpreter build: m355_pixel_pack against the Python restatement over every
channel value, every rejection, every format on every chroma format and source sample size — whole frames, a rectangle off a vector boundary and one
that ends in a partial lane —, the resized call with both filters, two chroma sample location types, a colour object and a tone object, and the
contract: a monochrome frame, the gate, the reader bookkeeping, a pinned-host destination and the descriptor's layout.  Expected values are the
restatements of the R'G'B' exports pushed through export_pixels_util.pixel_pack; every comparison is exact, guard bytes included, and every case is
compared with the pack of what the existing R'G'B' call delivers on the same build as well."""
import ctypes

import numpy as np
import pytest

from test_emu_picture import emu_lib  # noqa: F401  (fixture)
import export_colour_util as cu
import export_pixels_util as pu
import export_tone_util as tu
from export_pixels_util import FORMATS, M355_ERR_INVALID, NAMES
from libde265_amd import capi


@pytest.fixture()
def ctx(emu_lib):  # noqa: F811
    c = capi.Context(emu_lib, 0)
    yield c
    c.close()


@pytest.mark.parametrize("format", FORMATS, ids=lambda f: NAMES[f])
def test_pixel_pack_every_value(emu_lib, format):  # noqa: F811
    """m355_pixel_pack equals the restatement for every value of every channel (65536 for the 10-bit formats, 256 for the 8-bit ones) in every channel
    position and for every alpha, and c10 is round(c * 1023 / 65535)"""
    top = 65535 if format in pu.TEN else 255
    other = (top // 3, top - 7)
    for v in range(top + 1):
        a = v % (pu.alpha_max(format) + 1)
        for pos in range(3):
            rgb = [other[0], other[1]]
            rgb.insert(pos, v)
            assert emu_lib.pixel_pack(format, rgb, a) == pu.pixel_pack(format, rgb, a), (format, rgb, a)
    for a in range(pu.alpha_max(format) + 1):
        assert emu_lib.pixel_pack(format, (1, 2, 3), a) == pu.pixel_pack(format, (1, 2, 3), a)
    if format in pu.TEN:
        c = np.arange(65536, dtype=np.int64)
        assert np.array_equal(pu.c10(c), (2 * c * 1023 + 65535) // (2 * 65535)) and pu.c10(0) == 0 and pu.c10(65535) == 1023
        assert np.all(np.abs(pu.c10(c) - c * 1023 / 65535) <= 0.5)


def test_pixel_pack_rejects_bad_arguments(emu_lib):  # noqa: F811
    lib = emu_lib.lib
    out, n = (ctypes.c_uint8 * 4)(0x5A, 0x5A, 0x5A, 0x5A), ctypes.c_int(-1)

    def call(format, rgb, alpha, out_=out, n_=ctypes.byref(n), null_rgb=False):
        return lib.m355_pixel_pack(format, None if null_rgb else (ctypes.c_uint32 * 3)(*rgb), alpha, out_, n_)
    bad = [(-1, (0, 0, 0), 0), (5, (0, 0, 0), 0)]
    for f in FORMATS:
        top = 65535 if f in pu.TEN else 255
        for pos in range(3):
            rgb = [0, 0, 0]
            rgb[pos] = top + 1
            bad.append((f, rgb, 0))
        bad.append((f, (0, 0, 0), pu.alpha_max(f) + 1))
    for args in bad:
        assert call(*args) == M355_ERR_INVALID, args
    assert call(0, (0, 0, 0), 0, null_rgb=True) == M355_ERR_INVALID
    assert call(0, (0, 0, 0), 0, out_=None) == M355_ERR_INVALID
    assert call(0, (0, 0, 0), 0, n_=None) == M355_ERR_INVALID
    assert bytes(out) == b"\x5a" * 4 and n.value == -1, "a rejected m355_pixel_pack wrote its results"


def test_pixel_desc_layout():
    """the ABI of m355_pixel_desc: 56 bytes, dst at offset 40, pitch at offset 48"""
    assert ctypes.sizeof(capi.PixelDesc) == 56
    assert capi.PixelDesc.dst.offset == 40 and capi.PixelDesc.pitch.offset == 48
    assert capi.PixelDesc.out_width.offset == 32 and capi.PixelDesc.format.offset == 0 and capi.PixelDesc.alpha.offset == 4


def test_pixels_export_rejects_bad_arguments(ctx):
    """every rejected case of both calls returns M355_ERR_INVALID and leaves the destination as it was allocated"""
    lib = ctx.L.lib
    frame = ctx.frame_create(64, 32, 1, 10, 10)
    mono = ctx.frame_create(64, 32, 0, 8, 8)
    nbytes = 40 * 400
    buf = ctx.device_alloc(nbytes)
    colour = ctx.colour_create(cu.to_ctypes(cu.RANDOM))
    RGBA, BGR, A2 = capi.PIXEL_RGBA8, capi.PIXEL_BGR8, capi.PIXEL_A2R10G10B10

    def desc(format=RGBA, alpha=0, matrix=capi.MATRIX_BT709, full=0, rect=(0, 0, 0, 0), out=(0, 0), dst=True, pitch=400, ofs=0):
        d = capi.PixelDesc(format=format, alpha=alpha, matrix=matrix, full_range=full, out_width=out[0], out_height=out[1])
        d.x0, d.y0, d.width, d.height = rect
        d.dst = buf + ofs if dst else None
        d.pitch = pitch
        return d

    def opts(filter=0, chroma_loc=0, colour=0, reserved=None):
        o = capi.ExportOpts(filter=filter, chroma_loc=chroma_loc)
        o.reserved[0] = colour
        if reserved is not None:
            o.reserved[reserved] = 1
        return o

    # (what, descriptor arguments, options or None) for both calls; `out` is added for the resized call
    shared = [
        ("rectangle leaves the frame", dict(rect=(32, 0, 48, 16)), None),
        ("rectangle off the chroma grid (x)", dict(rect=(1, 0, 16, 16)), None),
        ("rectangle off the chroma grid (height)", dict(rect=(0, 0, 16, 15)), None),
        ("negative origin", dict(rect=(-2, 0, 16, 16)), None),
        ("empty height", dict(rect=(0, 0, 16, 0)), None),
        ("unknown format", dict(format=5), None),
        ("negative format", dict(format=-1), None),
        ("alpha 256", dict(alpha=256), None),
        ("negative alpha", dict(alpha=-1), None),
        ("alpha 4 of a 2-bit alpha", dict(format=A2, alpha=4), None),
        ("alpha for BGR8", dict(format=BGR, alpha=1), None),
        ("unknown matrix", dict(matrix=3), None),
        ("negative matrix", dict(matrix=-1), None),
        ("full_range 2", dict(full=2), None),
        ("full_range -1", dict(full=-1), None),
        ("no destination", dict(dst=False), None),
        ("4-byte pixels at an address off a dword", dict(ofs=2), None),
        ("4-byte pixels at an odd address", dict(format=A2, ofs=1), None),
        ("4-byte pixels with a pitch off a dword", dict(pitch=398), None),
        ("a reserved option", {}, opts(reserved=3)),
        ("chroma sample location type 4", {}, opts(chroma_loc=4)),
        ("a dead colour handle", {}, opts(colour=0x7777)),
    ]
    plain = shared + [
        ("pitch below the row", dict(pitch=252), None),
        ("BGR8 pitch below the row", dict(format=BGR, pitch=191), None),
        ("10-bit pitch below the row", dict(format=A2, pitch=252), None),
        ("an output width", dict(out=(64, 0)), None),
        ("an output height", dict(out=(0, 32)), None),
        ("an output size", dict(out=(64, 32)), None),
        ("a colour object", {}, opts(colour=colour)),
        ("a filter", {}, opts(filter=1)),
    ]
    resized = [(w, dict(a, out=a.get("out", (48, 24))), o) for w, a, o in shared] + [
        ("pitch below the output row", dict(out=(48, 24), pitch=188), None),
        ("BGR8 pitch below the output row", dict(format=BGR, out=(48, 24), pitch=143), None),
        ("no output size", dict(out=(0, 0)), None),
        ("negative output width", dict(out=(-48, 24)), None),
        ("odd output width (4:2:0)", dict(out=(47, 24)), None),
        ("more than 8x down", dict(out=(6, 24)), None),
        ("more than 8x up", dict(rect=(0, 0, 4, 4), out=(34, 8)), None),
        ("more than 4x down, cubic", dict(out=(14, 24)), opts(filter=1)),
        ("unknown filter", dict(out=(48, 24)), opts(filter=2)),
    ]
    for name, cases in (("m355_frame_export_pixels", plain), ("m355_frame_export_resized_pixels", resized)):
        call = getattr(lib, name)
        for what, a, o in cases:
            assert call(ctx.h, frame, ctypes.byref(desc(**a)), None if o is None else ctypes.byref(o)) == M355_ERR_INVALID, "%s: %s" % (name, what)
        ok = desc(out=(48, 24)) if cases is resized else desc()
        assert call(ctx.h, frame, None, None) == M355_ERR_INVALID, name
        assert call(ctx.h, frame + 100, ctypes.byref(ok), None) == M355_ERR_INVALID, name
        assert call(ctx.h, mono, ctypes.byref(ok), ctypes.byref(opts(chroma_loc=2))) == M355_ERR_INVALID, name + ": a siting for a monochrome frame"
    ctx.wait()
    assert np.all(ctx.device_read(buf, nbytes) == capi.DEVICE_FILL), "a rejected export wrote to its destination"
    # the limits themselves are fine: a pitch equal to the row, BGR8 at an odd address with an odd pitch, the largest alphas
    for d in (desc(pitch=256, alpha=255), desc(format=BGR, pitch=193, ofs=1), desc(format=A2, pitch=256, alpha=3)):
        assert lib.m355_frame_export_pixels(ctx.h, frame, ctypes.byref(d), None) == 0, ctx.L.error()
    for d in (desc(out=(48, 24), pitch=192, alpha=255), desc(format=BGR, out=(48, 24), pitch=145, ofs=1), desc(format=A2, out=(48, 24), pitch=192, alpha=3)):
        assert lib.m355_frame_export_resized_pixels(ctx.h, frame, ctypes.byref(d), ctypes.byref(opts(colour=colour, chroma_loc=2, filter=1))) == 0, ctx.L.error()
    ctx.wait()
    ctx.colour_destroy(colour)
    ctx.device_free(buf)
    ctx.frame_destroy(frame)
    ctx.frame_destroy(mono)


@pytest.mark.parametrize("cf,bit_depth", pu.SOURCES)
def test_pixels_format_matrix(ctx, cf, bit_depth):
    """every format x chroma format x source sample size on 64x32 frames: whole, MATRIX_RECT, and (6, 6, 20, 8), which ends in a partial lane"""
    pu.check_format_matrix(ctx, cf, bit_depth)


@pytest.mark.parametrize("bit_depth", [8, 10])
def test_pixels_sited(ctx, bit_depth):
    """the chroma sample location types 1..3 of a 4:2:0 frame carry over from m355_frame_export_rgb_opts"""
    planes = pu.random_planes(1, bit_depth, 8870 + bit_depth)
    frame = pu.upload(ctx, planes, 1, bit_depth)
    try:
        for loc in (1, 2, 3):
            for f in FORMATS:
                for rect in (None, pu.PARTIAL_LANE_RECT):
                    pu.check_pixels(ctx, frame, planes, (1, bit_depth, bit_depth), f, capi.MATRIX_BT709, 0, rect, loc, what="sited")
    finally:
        ctx.frame_destroy(frame)


@pytest.mark.parametrize("bit_depth", [8, 10])
def test_resized_pixels(ctx, bit_depth):
    """64x32 to 32x16 and to 48x40, the output equal to the frame and to a rectangle: every format, both filters, chroma_loc 0 and 2"""
    pu.check_resized_cases(ctx, bit_depth)


@pytest.mark.parametrize("cf,bit_depth", [(0, 8), (2, 10), (3, 8), (3, 10)])
def test_resized_pixels_other_chroma_formats(ctx, cf, bit_depth):
    planes = pu.random_planes(cf, bit_depth, 8840 + 10 * cf + bit_depth)
    frame = pu.upload(ctx, planes, cf, bit_depth)
    try:
        for out_size in ((32, 16), (48, 40)):
            for filt in (pu.TRIANGLE, pu.CUBIC):
                for f in FORMATS:
                    pu.check_resized_pixels(ctx, frame, planes, (cf, bit_depth, bit_depth), f, capi.MATRIX_BT2020, 1, out_size, filt=filt, what="cf %d" % cf)
    finally:
        ctx.frame_destroy(frame)


@pytest.mark.parametrize("name", ["colour", "tone"])
@pytest.mark.parametrize("bit_depth", [8, 10])
def test_resized_pixels_with_colour(ctx, bit_depth, name):
    """a colour object and a tone object: the 8-bit formats take m355_colour_pixel's U8 delivery, the 10-bit ones c10 of its 16-bit result"""
    S = cu.RANDOM if name == "colour" else tu.RANDOM
    pu.check_resized_cases(ctx, bit_depth, S, name)


def test_ten_bit_colour_delivery_is_not_the_u8_delivery():
    """from the restatement alone: c10 of the 16-bit result differs from the U8 delivery widened to 10 bits, so the 10-bit path is under test"""
    planes = tu.census_planes(10)
    o16 = cu.colour_pixels(cu.RANDOM, cu.ints16(planes, 10, (32, 16), 0, None, pu.TRIANGLE, "census"), capi.RGB_U16)
    o8 = cu.colour_pixels(cu.RANDOM, cu.ints16(planes, 10, (32, 16), 0, None, pu.TRIANGLE, "census"), capi.RGB_U8)
    assert any(not np.array_equal(pu.c10(a), (b * 1023 + 127) // 255) for a, b in zip(o16, o8))
    assert any(len(np.unique(pu.c10(a) & 3)) == 4 for a in o16)


def test_pixels_monochrome(ctx):
    """a monochrome frame has u = v = 0: the three channels of every pixel are equal, whatever the channel order"""
    luma = (np.arange(40 * 64, dtype=np.uint32) * 7 % 256).astype(np.uint8).reshape(40, 64)
    mono = pu.upload(ctx, [luma], 0, 8)
    try:
        for f in FORMATS:
            got = pu.check_pixels(ctx, mono, [luma], (0, 8, 8), f, capi.MATRIX_BT601, 0, (2, 1, 51, 30), what="monochrome")
            n = capi.pixel_bytes(f)
            px = got.reshape(30, 51, n)
            if f in pu.TEN:
                dw = np.ascontiguousarray(px).view("<u4")[:, :, 0]
                assert np.array_equal(dw & 1023, (dw >> 10) & 1023) and np.array_equal(dw & 1023, (dw >> 20) & 1023) and np.all(dw >> 30 == pu.alpha_for(f))
            else:
                assert np.array_equal(px[:, :, 0], px[:, :, 1]) and np.array_equal(px[:, :, 0], px[:, :, 2])
                assert n == 3 or np.all(px[:, :, 3] == pu.alpha_for(f))
            assert len(np.unique(px[:, :, 0])) > 100
            pu.check_resized_pixels(ctx, mono, [luma], (0, 8, 8), f, capi.MATRIX_BT601, 0, (40, 24), (2, 2, 50, 30), what="monochrome")
    finally:
        ctx.frame_destroy(mono)


@pytest.mark.parametrize("resized", [False, True], ids=["plain", "resized"])
def test_pixels_export_behind_a_rejected_decode_writes_nothing(ctx, resized):
    pu.check_gate(ctx, resized)


@pytest.mark.parametrize("resized", [False, True], ids=["plain", "resized"])
@pytest.mark.parametrize("depth", [1, 3])
def test_pixels_export_behind_recycled_frames(ctx, depth, resized):
    """(the interpreter runs every launch to its end at once: this walks the reader bookkeeping, the GPU tier is what can see a missing wait)"""
    pu.check_hazard(ctx, depth, resized)


def test_pixels_export_into_pinned_host_memory(ctx):
    planes = pu.random_planes(1, 10, 8891)
    frame = pu.upload(ctx, planes, 1, 10)
    try:
        for f in (capi.PIXEL_BGRA8, capi.PIXEL_BGR8, capi.PIXEL_A2B10G10R10):
            pu.check_pixels(ctx, frame, planes, (1, 10, 10), f, capi.MATRIX_BT709, 0, (2, 2, 48, 16), host=True, what="pinned")
            pu.check_resized_pixels(ctx, frame, planes, (1, 10, 10), f, capi.MATRIX_BT709, 0, (48, 24), host=True, what="pinned")
    finally:
        ctx.frame_destroy(frame)
