"""Shared by the pixel-format export tests (SIMT-interpreter build, GPU and glue): m355_pixel_pack of include/de265_mi355x.h restated in Python integers
/ numpy int64, applied to what the restatements of the R'G'B' exports already compute — export_rgb_util / export_siting_util for
m355_frame_export_pixels, export_resized_rgb_util / export_cubic_util / export_siting_util for m355_frame_export_resized_pixels, export_colour_util /
export_tone_util for a colour or tone object —, and the drivers that check exports against it.  Every destination is a buffer whose every byte holds
capi.DEVICE_FILL beforehand; every comparison of pixels is exact, and every byte outside the rows must still hold the sentinel.  Each driver also
compares the pixels call with the pack of what the EXISTING R'G'B' call delivers on the same build: a second check, independent of the restatement."""
import numpy as np

import export_cubic_util
import export_resized_rgb_util
import export_tone_util as tu
from export_colour_util import FULL as COLOUR_FULL, MATRIX as COLOUR_MATRIX, ints16
from export_rgb_util import M355_ERR_INVALID, MATRIX_RECT, expected_rgb  # noqa: F401
from export_siting_util import expected_resized_rgb_sited, expected_rgb_sited
from export_util import assert_export, chroma_grid_rect
from synth_util import assert_planes_equal
from libde265_amd import capi, worklist

FORMATS = capi.PIXEL_FORMATS
NAMES = {capi.PIXEL_RGBA8: "rgba8", capi.PIXEL_BGRA8: "bgra8", capi.PIXEL_BGR8: "bgr8", capi.PIXEL_A2B10G10R10: "a2b10g10r10",
         capi.PIXEL_A2R10G10B10: "a2r10g10b10"}
TEN = (capi.PIXEL_A2B10G10R10, capi.PIXEL_A2R10G10B10)
B_FIRST = (capi.PIXEL_BGRA8, capi.PIXEL_BGR8, capi.PIXEL_A2R10G10B10)
TRIANGLE, CUBIC = capi.FILTER_TRIANGLE, capi.FILTER_CUBIC
PARTIAL_LANE_RECT = (6, 6, 20, 8)      # ends in a partial lane (20 pixels: a lane of 16 and one of 4, or two of 8 and one of 4)
# (chroma format, bit depth) of the format matrix: 64x32 frames
SOURCES = [(cf, bd) for cf in (0, 1, 2, 3) for bd in (8, 10)]


def samples_of(format):
    """S(format): the samples of the R'G'B' call underneath"""
    return capi.RGB_U16 if format in TEN else capi.RGB_U8


def alpha_max(format):
    return 0 if format == capi.PIXEL_BGR8 else (3 if format in TEN else 255)


def alpha_for(format):
    """an alpha inside the range with both bit values in it"""
    return {255: 0xA6, 3: 2, 0: 0}[alpha_max(format)]


def c10(c):
    return (2046 * c + 65535) // 131070


def pixel_dword(format, r, g, b, alpha):
    """the pixel's little-endian dword (BGR8: its low 24 bits) — Python integers or int64 arrays"""
    lo, hi = (b, r) if format in B_FIRST else (r, b)
    if format in TEN:
        return c10(lo) | (c10(g) << 10) | (c10(hi) << 20) | (alpha << 30)
    return lo | (g << 8) | (hi << 16) | (alpha << 24)


def pixel_pack(format, rgb, alpha):
    """m355_pixel_pack in Python integers -> bytes"""
    return int(pixel_dword(format, int(rgb[0]), int(rgb[1]), int(rgb[2]), int(alpha))).to_bytes(4, "little")[:capi.pixel_bytes(format)]


def pack_planes(format, rgb, alpha):
    """three (H, W) arrays -> the (H, W * bytes per pixel) uint8 rows of the destination"""
    dw = pixel_dword(format, *[c.astype(np.int64) for c in rgb], alpha).astype("<u4")
    h, w = dw.shape
    b = np.ascontiguousarray(dw).view(np.uint8).reshape(h, w, 4)
    return np.ascontiguousarray(b[:, :, :capi.pixel_bytes(format)]).reshape(h, -1)


def unpack_packed(plane):
    """a packed R'G'B' plane (H, 3 W) as the existing exports deliver it -> [R, G, B]"""
    return [plane[:, c::3] for c in range(3)]


def expected_pixels(planes, cf, bdl, bdc, format, alpha, matrix, full_range, rect=None, loc=0):
    """what m355_frame_export_pixels delivers, from the planes m355_frame_download returns"""
    s = samples_of(format)
    if loc:
        rgb = expected_rgb_sited(planes, bdl, bdc, capi.RGB_PLANAR, s, matrix, full_range, loc, rect)
    else:
        rgb = expected_rgb(planes, cf, bdl, bdc, capi.RGB_PLANAR, s, matrix, full_range, rect)
    return pack_planes(format, rgb, alpha)


def expected_resized_ints(planes, cf, bd, samples, matrix, full_range, out_size, rect=None, loc=0, filt=TRIANGLE, S=None, key=None):
    """the three channel planes m355_frame_export_resized_rgb_opts delivers.  S: a set of export_colour_util / export_tone_util (4:2:0, and the
    conversion of those modules)"""
    if S is not None:
        assert cf == 1 and (matrix, full_range) == (COLOUR_MATRIX, COLOUR_FULL)
        return tu.pixels(S, ints16(planes, bd, out_size, loc, rect, filt, key), samples)
    if cf == 1:
        return expected_resized_rgb_sited(planes, bd, bd, capi.RGB_PLANAR, samples, matrix, full_range, out_size, loc, rect, filt)
    m = export_cubic_util if filt == CUBIC else export_resized_rgb_util
    return m.expected_resized_rgb(planes, cf, bd, bd, capi.RGB_PLANAR, samples, matrix, full_range, out_size, rect)


def expected_resized_pixels(planes, cf, bd, format, alpha, matrix, full_range, out_size, rect=None, loc=0, filt=TRIANGLE, S=None, key=None):
    """what m355_frame_export_resized_pixels delivers"""
    return pack_planes(format, expected_resized_ints(planes, cf, bd, samples_of(format), matrix, full_range, out_size, rect, loc, filt, S, key), alpha)


def random_planes(cf, bd, seed, size=(64, 32)):
    w, h = size
    rng = np.random.default_rng(seed)
    dt = np.uint8 if bd == 8 else np.uint16
    return [rng.integers(0, 1 << bd, (ph, pw)).astype(dt) for pw, ph in worklist.plane_dims(w, h, cf) if pw]


def upload(ctx, planes, cf, bd):
    frame = ctx.frame_create(planes[0].shape[1], planes[0].shape[0], cf, bd, bd)
    ctx.frame_upload(frame, planes)
    return frame


def finish(ctx, token):
    (got,), raws = ctx.frame_export_finish(token, raw=True)
    return got, raws


def check_pixels(ctx, frame, planes, geom, format, matrix, full_range, rect=None, loc=0, host=False, what="", alpha=None):
    """m355_frame_export_pixels against the restatement and against the pack of m355_frame_export_rgb_opts' packed output; guard bytes untouched"""
    cf, bdl, bdc = geom
    alpha = alpha_for(format) if alpha is None else alpha
    what = "%s %s matrix %d full %d rect %s type %d" % (what, NAMES[format], matrix, full_range, rect, loc)
    got, raws = finish(ctx, ctx.frame_export_pixels(frame, format, alpha, matrix, full_range, rect, host=host, chroma_loc=loc))
    assert_export([got], raws, [expected_pixels(planes, cf, bdl, bdc, format, alpha, matrix, full_range, rect, loc)], what)
    rgb = ctx.frame_export_finish(ctx.frame_export_rgb(frame, capi.RGB_PACKED, samples_of(format), matrix, full_range, rect, chroma_loc=loc))[0]
    assert_planes_equal([got], [pack_planes(format, unpack_packed(rgb), alpha)], what + ": against the R'G'B' export")
    return got


def check_resized_pixels(ctx, frame, planes, geom, format, matrix, full_range, out_size, rect=None, loc=0, filt=TRIANGLE, S=None, colour=0, key=None,
                         host=False, what="", alpha=None):
    """m355_frame_export_resized_pixels against the restatement and against the pack of m355_frame_export_resized_rgb_opts' packed output"""
    cf, bd = geom[0], geom[1]
    alpha = alpha_for(format) if alpha is None else alpha
    what = "%s %s to %dx%d rect %s type %d filter %d colour %d" % (what, NAMES[format], out_size[0], out_size[1], rect, loc, filt, colour)
    got, raws = finish(ctx, ctx.frame_export_resized_pixels(frame, format, alpha, matrix, full_range, out_size, rect, host=host, filter=filt, chroma_loc=loc,
                                                            colour=colour))
    assert_export([got], raws, [expected_resized_pixels(planes, cf, bd, format, alpha, matrix, full_range, out_size, rect, loc, filt, S, key)], what)
    rgb = ctx.frame_export_finish(ctx.frame_export_resized_rgb(frame, capi.RGB_PACKED, samples_of(format), matrix, full_range, out_size, rect, filter=filt,
                                                               chroma_loc=loc, colour=colour))[0]
    assert_planes_equal([got], [pack_planes(format, unpack_packed(rgb), alpha)], what + ": against the R'G'B' export")
    return got


def check_format_matrix(ctx, cf, bd, rects=(None, MATRIX_RECT, PARTIAL_LANE_RECT), conversions=((capi.MATRIX_BT709, 0), (capi.MATRIX_BT2020, 1))):
    """every format on one 64x32 source: the whole frame, the rectangle off a vector boundary, the rectangle that ends in a partial lane.  B-first and
    R-first formats of the same channel bits must differ, else the channel order is not under test"""
    planes = random_planes(cf, bd, 8800 + 10 * cf + bd)
    frame = upload(ctx, planes, cf, bd)
    try:
        for rect in rects:
            r = None if rect is None else chroma_grid_rect(rect, cf)
            for k, (matrix, full) in enumerate(conversions):
                got = {f: check_pixels(ctx, frame, planes, (cf, bd, bd), f, matrix, full, r, what="cf %d %d bit" % (cf, bd)) for f in FORMATS}
                if cf:
                    assert not np.array_equal(got[capi.PIXEL_RGBA8], got[capi.PIXEL_BGRA8]) and not np.array_equal(got[capi.PIXEL_A2B10G10R10], got[capi.PIXEL_A2R10G10B10])
    finally:
        ctx.frame_destroy(frame)


# the resized call on a 64x32 4:2:0 source: (rectangle, output size); None as the size: the output equals the rectangle
RESIZED_CASES = ((None, (32, 16)), (None, (48, 40)), (None, (64, 32)), ((2, 2, 44, 26), (44, 26)))


def check_resized_cases(ctx, bd, S=None, name="plain", cases=RESIZED_CASES, formats=FORMATS, filters=(TRIANGLE, CUBIC), locs=(0, 2)):
    """every format x case x filter x chroma sample location type on the 4:2:0 source of the colour tests, without an object or with the set S"""
    planes = tu.census_planes(bd)
    frame = upload(ctx, planes, 1, bd)
    colour = tu.create(ctx, S) if S is not None else 0
    try:
        for rect, out_size in cases:
            for filt in filters:
                for loc in locs:
                    for f in formats:
                        check_resized_pixels(ctx, frame, planes, (1, bd, bd), f, COLOUR_MATRIX, COLOUR_FULL, out_size, rect, loc, filt, S, colour, "census",
                                             what="%s %d bit" % (name, bd))
    finally:
        ctx.frame_destroy(frame)
        if colour:
            ctx.colour_destroy(colour)


def check_gate(ctx, resized, format=capi.PIXEL_BGRA8, matrix=capi.MATRIX_BT709, full=0, out_size=(80, 48)):
    """export_rgb_util.check_gate_rgb's scenario for a pixels call: behind a decode whose lists the device rejected it writes nothing, behind an accepted
    decode of the same lists it does"""
    from synth_util import make_case
    cfg = dict(width=128, height=64, bit_depth=8, seed=7501, intra_pct=30)
    pic, refs = make_case(**cfg)
    pp = pic.pp[0]
    handles = []
    for planes in refs:
        f = ctx.frame_create_for(pp)
        ctx.frame_upload(f, planes)
        handles.append(f)
    dst = ctx.frame_create_for(pp)
    ctx.frame_fill(dst, 77, 99)
    alpha = alpha_for(format)
    tokens, serials = [], []
    for corrupt in (False, True):
        p = make_case(**cfg)[0]
        p.ref_frames = [handles[i] if i < len(handles) else -1 for i in range(worklist.MAX_REF_FRAMES)]
        p.dst_frame = dst
        if corrupt:
            arr = p.ibs.copy(); arr["mode"][len(arr) // 2] = 77; p.ibs = arr
        ctx.submit_in_place(p, fill_threads=1)
        serials.append(ctx.last_serial())
        tokens.append(ctx.frame_export_resized_pixels(dst, format, alpha, matrix, full, out_size) if resized else
                      ctx.frame_export_pixels(dst, format, alpha, matrix, full))
    good, bad = [finish(ctx, t) for t in tokens]
    assert ctx.decode_status(serials[0]) == 0 and ctx.decode_status(serials[1]) == M355_ERR_INVALID
    with_planes = ctx.frame_download(dst)           # (the rejected decode left the accepted picture in the frame)
    want = (expected_resized_pixels(with_planes, 1, 8, format, alpha, matrix, full, out_size) if resized else
            expected_pixels(with_planes, 1, 8, 8, format, alpha, matrix, full))
    assert_export([good[0]], good[1], [want], "behind the accepted decode")
    for raw in bad[1]:
        assert np.all(raw == capi.DEVICE_FILL), "a pixels export behind a rejected decode wrote to its destination"
    ctx.wait()
    for f in handles + [dst]:
        ctx.frame_destroy(f)


def check_hazard(ctx, depth, resized, format=capi.PIXEL_A2R10G10B10, matrix=capi.MATRIX_BT709, full=0, out_size=(80, 36)):
    """export_rgb_util.check_hazard_rgb's scenario for a pixels call: four 128x64 10-bit pictures decoded alternately into a pool of two frames, each
    exported right behind its decode into a buffer of its own, no host wait in between; every export must deliver what the export of the same picture
    decoded alone delivers.  (On the GPU with several pictures in flight this sees a decode that does not wait for the export of its frame's previous
    picture; the SIMT interpreter finishes every launch before the next call and checks the bookkeeping's results only.)"""
    from libde265_amd import synth
    ctx.set_pipeline_depth(depth)
    try:
        cfg = dict(width=128, height=64, bit_depth=10, seed=5, n_refs=1)
        pics = [synth.picture(**dict(cfg, seed=5 + j)) for j in range(4)]
        pp = pics[0].pp[0]
        r0 = ctx.frame_create_for(pp)
        ctx.frame_upload(r0, synth.ref_planes(5, 128, 64, 1, 10))
        pool = [ctx.frame_create_for(pp) for _ in range(2)]
        rect = (2, 2, 122, 58)
        alpha = alpha_for(format)

        def export(f):
            if resized:
                return ctx.frame_export_resized_pixels(f, format, alpha, matrix, full, out_size, rect)
            return ctx.frame_export_pixels(f, format, alpha, matrix, full, rect)
        handles, tokens = [], []
        for j, pic in enumerate(pics):
            pic.ref_frames = [r0] + [-1] * (worklist.MAX_REF_FRAMES - 1)
            pic.dst_frame = pool[j % 2]
            handles.append(ctx.upload(pic))
            ctx.decode_resident(handles[-1])
            tokens.append(export(pool[j % 2]))
        got = [finish(ctx, t) for t in tokens]
        ctx.wait()
        for j in range(4):
            ctx.decode_resident(handles[j])
            ctx.wait()
            planes = ctx.frame_download(pool[j % 2])
            alone = finish(ctx, export(pool[j % 2]))[0]
            want = (expected_resized_pixels(planes, 1, 10, format, alpha, matrix, full, out_size, rect) if resized else
                    expected_pixels(planes, 1, 10, 10, format, alpha, matrix, full, rect))
            assert_planes_equal([alone], [want], "picture %d alone" % j)
            assert_export([got[j][0]], got[j][1], [alone], "picture %d, depth %d" % (j, depth))
        for j in (0, 1):
            assert not np.array_equal(got[j][0], got[j + 2][0]), "the pictures that share a frame must differ for this test to see a hazard"
        for h in handles:
            ctx.release(h)
        for f in pool + [r0]:
            ctx.frame_destroy(f)
    finally:
        ctx.set_pipeline_depth(1)
