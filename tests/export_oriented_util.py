"""Shared by the oriented export tests (host, SIMT-interpreter build, GPU and glue): the definition of an orientation in numpy (include/de265_mi355x.h,
M355_ORIENT_*), and the drivers that check m355_frame_export_oriented and m355_frame_export_pixels_oriented against it.  Expected values come twice:
from the existing restatements (export_util.expected_export, export_pixels_util.expected_pixels) pushed through orient, and from what the existing
un-oriented call delivers on the same build pushed through orient.  Every destination is filled with capi.DEVICE_FILL beforehand; every comparison is
exact, and every byte outside the oriented rows must still hold the sentinel."""
import ctypes

import numpy as np

import export_pixels_util as pu
import export_util as eu
from export_util import M355_ERR_INVALID, assert_export  # noqa: F401
from synth_util import assert_planes_equal
from libde265_amd import capi, worklist

ORIENTATIONS = capi.ORIENTATIONS
TRANSPOSING = tuple(o for o in ORIENTATIONS if o & capi.ORIENT_TRANSPOSE)
NON_TRANSPOSING = tuple(o for o in ORIENTATIONS if not o & capi.ORIENT_TRANSPOSE)
TILE = 64                                # M355_ORIENT_TILE: the transposing kernel's tile, in elements
BIG = (264, 136)                         # 4:2:0: luma 5 x 3 tiles, chroma (132 x 68) 3 x 2 tiles, the last one partial in both directions on both grids
BIG_RECT = (6, 2, BIG[0] - 14, BIG[1] - 6)   # starts off a vector boundary, ends in a partial lane (luma 250 x 130, 4:2:0 chroma 125 x 65)
SMALL = (8, 8)                           # the smallest frame m355_frame_create accepts: 4:2:0 chroma 4 x 4, below a 16-byte vector and a tile
FOUR_BYTE_FORMATS = tuple(f for f in pu.FORMATS if capi.pixel_bytes(f) == 4)


def orient(a, o):
    """the definition: (H, W, ...) elements -> the oriented array; trailing axes belong to the element"""
    t = np.swapaxes(a, 0, 1) if o & capi.ORIENT_TRANSPOSE else a
    t = t[::-1] if o & capi.ORIENT_FLIP else t
    t = t[:, ::-1] if o & capi.ORIENT_MIRROR else t
    return np.ascontiguousarray(t)


def orient_pointwise(a, o):
    """the same from the formula of the header, evaluated point by point"""
    h, w = a.shape[:2]
    W, H = (h, w) if o & capi.ORIENT_TRANSPOSE else (w, h)
    d = np.empty((H, W) + a.shape[2:], a.dtype)
    for Y in range(H):
        for X in range(W):
            u = W - 1 - X if o & capi.ORIENT_MIRROR else X
            v = H - 1 - Y if o & capi.ORIENT_FLIP else Y
            d[Y, X] = a[u, v] if o & capi.ORIENT_TRANSPOSE else a[v, u]
    return d


def orient_rows(plane, o, group):
    """a destination plane (H, W * group) whose elements are `group` consecutive values — the (Cb, Cr) pair of an interleaved row, the four bytes of a
    pixel — oriented as whole elements"""
    h, n = plane.shape
    t = orient(plane.reshape(h, n // group, group), o)
    return t.reshape(t.shape[0], -1)


def groups(n_planes, cf, layout):
    """values per element of each destination plane of a YUV export"""
    return [2 if layout == capi.EXPORT_SEMIPLANAR and cf != 0 and k == 1 else 1 for k in range(n_planes)]


def random_planes(cf, bd, seed, size):
    return pu.random_planes(cf, bd, seed, size)


def check_oriented(ctx, frame, planes, geom, layout, samples, o, rect=None, host=False, plain=None, what=""):
    """m355_frame_export_oriented against orient of the restatement and against orient of m355_frame_export's output (plain: that output, if the caller
    has it already); guard bytes untouched"""
    cf, bdl, bdc = geom
    what = "%s layout %d samples %d rect %s orientation %d" % (what, layout, samples, rect, o)
    got, raws = ctx.frame_export_finish(ctx.frame_export_oriented(frame, layout, samples, o, rect, host=host), raw=True)
    want = eu.expected_export(planes, cf, bdl, bdc, layout, samples, rect)
    g = groups(len(want), cf, layout)
    assert_export(got, raws, [orient_rows(p, o, k) for p, k in zip(want, g)], what)
    if plain is None:
        plain = ctx.frame_export_finish(ctx.frame_export(frame, layout, samples, rect))
    assert_planes_equal(got, [orient_rows(p, o, k) for p, k in zip(plain, g)], what + ": against the plain export")
    return got


def check_source(ctx, cf, bd, size, rects, orientations=ORIENTATIONS, seed=9100):
    """every layout x sample format x rectangle x orientation of one random frame"""
    planes = random_planes(cf, bd, seed + 10 * cf + bd, size)
    frame = pu.upload(ctx, planes, cf, bd)
    try:
        for rect in rects:
            r = None if rect is None else eu.chroma_grid_rect(rect, cf)
            for layout in eu.LAYOUTS:
                for samples in eu.SAMPLES:
                    plain = ctx.frame_export_finish(ctx.frame_export(frame, layout, samples, r))
                    for o in orientations:
                        check_oriented(ctx, frame, planes, (cf, bd, bd), layout, samples, o, r, plain=plain, what="cf %d %d bit %s" % (cf, bd, size))
    finally:
        ctx.frame_destroy(frame)


def check_pixels_oriented(ctx, frame, planes, geom, format, o, rect=None, loc=0, host=False, plain=None, matrix=capi.MATRIX_BT709, full=0, what=""):
    """m355_frame_export_pixels_oriented against orient of the restatement and of m355_frame_export_pixels' output"""
    cf, bdl, bdc = geom
    alpha = pu.alpha_for(format)
    what = "%s %s rect %s type %d orientation %d" % (what, pu.NAMES[format], rect, loc, o)
    got, raws = pu.finish(ctx, ctx.frame_export_pixels_oriented(frame, format, alpha, matrix, full, o, rect, host=host, chroma_loc=loc))
    want = pu.expected_pixels(planes, cf, bdl, bdc, format, alpha, matrix, full, rect, loc)
    assert_export([got], raws, [orient_rows(want, o, 4)], what)
    if plain is None:
        plain = pu.finish(ctx, ctx.frame_export_pixels(frame, format, alpha, matrix, full, rect, chroma_loc=loc))[0]
    assert_planes_equal([got], [orient_rows(plain, o, 4)], what + ": against the plain export")
    return got


def check_pixels_source(ctx, cf, bd, size, rects, formats=FOUR_BYTE_FORMATS, locs=(0, 2), orientations=ORIENTATIONS, seed=9200):
    planes = random_planes(cf, bd, seed + 10 * cf + bd, size)
    frame = pu.upload(ctx, planes, cf, bd)
    try:
        for rect in rects:
            r = None if rect is None else eu.chroma_grid_rect(rect, cf)
            for f in formats:
                for loc in (locs if cf == 1 else (0,)):
                    plain = pu.finish(ctx, ctx.frame_export_pixels(frame, f, pu.alpha_for(f), capi.MATRIX_BT709, 0, r, chroma_loc=loc))[0]
                    for o in orientations:
                        check_pixels_oriented(ctx, frame, planes, (cf, bd, bd), f, o, r, loc, plain=plain, what="cf %d %d bit %s" % (cf, bd, size))
    finally:
        ctx.frame_destroy(frame)


def check_odd_destination(ctx, o, size=(72, 40)):
    """a u8 planar export whose destinations start at an ODD address and whose pitches are ODD: the oriented rows, and every other byte the sentinel"""
    lib = ctx.L.lib
    planes = random_planes(1, 8, 9300 + o, size)
    frame = pu.upload(ctx, planes, 1, 8)
    want = [orient(p, o) for p in eu.expected_export(planes, 1, 8, 8, capi.EXPORT_PLANAR, capi.EXPORT_NATIVE)]
    desc = capi.ExportDesc(layout=capi.EXPORT_PLANAR, samples=capi.EXPORT_NATIVE)
    bufs = []
    try:
        for k, p in enumerate(want):
            pitch = p.shape[1] + 21 + 2 * k
            assert pitch % 2 == 1
            bufs.append((ctx.device_alloc(p.shape[0] * pitch + 1), pitch))
            desc.dst[k] = bufs[-1][0] + 1
            desc.pitch[k] = pitch
        ctx.L.check(lib.m355_frame_export_oriented(ctx.h, frame, ctypes.byref(desc), o))
        ctx.wait()
        for k, (p, (buf, pitch)) in enumerate(zip(want, bufs)):
            raw = ctx.device_read(buf, p.shape[0] * pitch + 1)
            assert raw[0] == capi.DEVICE_FILL
            rows = raw[1:].reshape(p.shape[0], pitch)
            assert np.array_equal(rows[:, :p.shape[1]], p), "plane %d orientation %d at an odd address" % (k, o)
            assert np.all(rows[:, p.shape[1]:] == capi.DEVICE_FILL), "plane %d orientation %d: bytes behind the row end were written" % (k, o)
    finally:
        for buf, _ in bufs:
            ctx.device_free(buf)
        ctx.frame_destroy(frame)


def yuv_call(layout, samples, o):
    """(export(ctx, frame, rect) -> token, expected(planes, bd, rect) -> planes) of one m355_frame_export_oriented"""
    def export(ctx, f, rect=None):
        return ctx.frame_export_oriented(f, layout, samples, o, rect)

    def expected(planes, bd, rect=None):
        want = eu.expected_export(planes, 1, bd, bd, layout, samples, rect)
        return [orient_rows(p, o, k) for p, k in zip(want, groups(len(want), 1, layout))]
    return export, expected


def pixels_call(format, o, matrix=capi.MATRIX_BT709, full=0):
    """the same of one m355_frame_export_pixels_oriented"""
    alpha = pu.alpha_for(format)

    def export(ctx, f, rect=None):
        return ctx.frame_export_pixels_oriented(f, format, alpha, matrix, full, o, rect)

    def expected(planes, bd, rect=None):
        return [orient_rows(pu.expected_pixels(planes, 1, bd, bd, format, alpha, matrix, full, rect), o, 4)]
    return export, expected


def check_gate(ctx, call):
    """export_util.check_gate's scenario for an oriented call: behind a decode whose lists the device rejected it writes nothing, behind an accepted
    decode of the same lists it does"""
    from synth_util import make_case
    export, expected = call
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
    tokens, serials = [], []
    for corrupt in (False, True):
        p = make_case(**cfg)[0]
        p.ref_frames = [handles[i] if i < len(handles) else -1 for i in range(worklist.MAX_REF_FRAMES)]
        p.dst_frame = dst
        if corrupt:
            arr = p.ibs.copy(); arr["mode"][len(arr) // 2] = 77; p.ibs = arr
        ctx.submit_in_place(p, fill_threads=1)
        serials.append(ctx.last_serial())
        tokens.append(export(ctx, dst))
    good, bad = [ctx.frame_export_finish(t, raw=True) for t in tokens]
    assert ctx.decode_status(serials[0]) == 0 and ctx.decode_status(serials[1]) == M355_ERR_INVALID
    with_planes = ctx.frame_download(dst)           # (the rejected decode left the accepted picture in the frame)
    assert_export(good[0], good[1], expected(with_planes, 8), "behind the accepted decode")
    for raw in bad[1]:
        assert np.all(raw == capi.DEVICE_FILL), "an oriented export behind a rejected decode wrote to its destination"
    ctx.wait()
    for f in handles + [dst]:
        ctx.frame_destroy(f)


def check_hazard(ctx, depth, call):
    """export_util.check_hazard's scenario for an oriented call: four 128x64 10-bit pictures decoded alternately into a pool of two frames, each exported
    right behind its decode into a buffer of its own, no host wait in between; every export must deliver what the export of the same picture decoded
    alone delivers.  (On the GPU with several pictures in flight this sees a decode that does not wait for the export of its frame's previous picture;
    the SIMT interpreter finishes every launch before the next call and checks the bookkeeping's results only.)"""
    from libde265_amd import synth
    export, expected = call
    ctx.set_pipeline_depth(depth)
    try:
        cfg = dict(width=128, height=64, bit_depth=10, seed=5, n_refs=1)
        pics = [synth.picture(**dict(cfg, seed=5 + j)) for j in range(4)]
        pp = pics[0].pp[0]
        r0 = ctx.frame_create_for(pp)
        ctx.frame_upload(r0, synth.ref_planes(5, 128, 64, 1, 10))
        pool = [ctx.frame_create_for(pp) for _ in range(2)]
        rect = (2, 2, 122, 58)
        handles, tokens = [], []
        for j, pic in enumerate(pics):
            pic.ref_frames = [r0] + [-1] * (worklist.MAX_REF_FRAMES - 1)
            pic.dst_frame = pool[j % 2]
            handles.append(ctx.upload(pic))
            ctx.decode_resident(handles[-1])
            tokens.append(export(ctx, pool[j % 2], rect))
        got = [ctx.frame_export_finish(t, raw=True) for t in tokens]
        ctx.wait()
        for j in range(4):
            ctx.decode_resident(handles[j])
            ctx.wait()
            planes = ctx.frame_download(pool[j % 2])
            alone = ctx.frame_export_finish(export(ctx, pool[j % 2], rect))
            assert_planes_equal(alone, expected(planes, 10, rect), "picture %d alone" % j)
            assert_export(got[j][0], got[j][1], alone, "picture %d, depth %d" % (j, depth))
        for j in (0, 1):
            assert not np.array_equal(got[j][0][0], got[j + 2][0][0]), "the pictures that share a frame must differ for this test to see a hazard"
        for h in handles:
            ctx.release(h)
        for f in pool + [r0]:
            ctx.frame_destroy(f)
    finally:
        ctx.set_pipeline_depth(1)
