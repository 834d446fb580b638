"""Shared by the m355_frame_export_resized tests (SIMT-interpreter build and GPU): the restatement of what a resized export delivers — taps() in
Python integers, straight from the definition in include/de265_mi355x.h, and the two passes in numpy int64, one gather-multiply-add per tap — and
the drivers that check exports against it, exactly, the untouched padding of the destination rows included."""
import functools

import numpy as np

from export_util import FORMATS, LAYOUTS, SAMPLES, M355_ERR_INVALID, assert_export, chroma_grid_rect, decode_into_frame, expected_export, format_id, sub_sampling  # noqa: F401
from synth_util import assert_planes_equal, make_case
from libde265_amd import capi, worklist

MAX_TAPS = 16
MATRIX_RECT = (2, 2, 50, 22)      # its source starts off a vector boundary
# (rectangle, output size) of the format matrix: a non-integer ratio, ratio exactly 8, upscaling, and the rectangle down and up
MATRIX_SIZES = [(None, (48, 20)), (None, (8, 4)), (None, (128, 64)), (MATRIX_RECT, (36, 14)), (MATRIX_RECT, (64, 30))]


def rdiv(a, b):
    return (2 * a + b) // (2 * b)


def ratio_ok(sn, dn):
    return sn >= 1 and dn >= 1 and sn <= 8 * dn and dn <= 8 * sn


def taps(sn, dn, cosited, i):
    """row i of the axis sn -> dn: (first source index, [coefficients]), folded at the ends of [0, sn - 1]"""
    M = 2 * max(sn, dn)
    C = 2 * i * sn if cosited else (2 * i + 1) * sn - dn
    ks = [k for k in range((C - M) // (2 * dn) - 1, (C + M) // (2 * dn) + 2) if abs(2 * dn * k - C) < M]
    assert 1 <= len(ks) <= MAX_TAPS and ks == list(range(ks[0], ks[-1] + 1))
    n = [M - abs(2 * dn * k - C) for k in ks]
    N, P, q = sum(n), 0, []
    for nk in n:
        q.append(rdiv((P + nk) << 14, N) - rdiv(P << 14, N))
        P += nk
    folded = {}
    for k, qk in zip(ks, q):
        kk = min(max(k, 0), sn - 1)
        folded[kk] = folded.get(kk, 0) + qk
    first = min(folded)
    assert sorted(folded) == list(range(first, first + len(folded)))
    return first, [folded[first + j] for j in range(len(folded))]


@functools.lru_cache(maxsize=64)
def axis_table(sn, dn, cosited):
    """every row of an axis -> (first[dn], coeff[dn][16] padded with zeros)"""
    first = np.zeros(dn, np.int64)
    coeff = np.zeros((dn, MAX_TAPS), np.int64)
    for i in range(dn):
        f, q = taps(sn, dn, cosited, i)
        first[i] = f
        coeff[i, :len(q)] = q
    return first, coeff


_planes_done = {}


def resize_plane(S, ow, oh, cosited_x, bd):
    """the horizontal sums v of one plane (computed once per plane and size: every layout and sample format starts from the same v, which is
    left unchanged)"""
    key = (S.shape, str(S.dtype), S.tobytes(), ow, oh, cosited_x, bd)
    if key not in _planes_done:
        if len(_planes_done) >= 32:
            _planes_done.clear()
        v = _resize_plane(S, ow, oh, cosited_x, bd)
        v.setflags(write=False)
        _planes_done[key] = v
    return _planes_done[key]


def _resize_plane(S, ow, oh, cosited_x, bd):
    """vertical pass, the rounding to the 18-bit intermediate, horizontal pass (int64, a gather per tap)"""
    S = S.astype(np.int64)
    sh, sw = S.shape
    fy, qy = axis_table(sh, oh, 0)
    fx, qx = axis_table(sw, ow, cosited_x)
    u = np.zeros((oh, sw), np.int64)
    for k in range(MAX_TAPS):
        if qy[:, k].any():
            u += qy[:, k, None] * S[np.minimum(fy + k, sh - 1)]
    assert int(u.max()) < 1 << (bd + 14)
    t = (u + (1 << (bd - 5))) >> (bd - 4)
    assert int(t.max()) < 1 << 18
    v = np.zeros((oh, ow), np.int64)
    for k in range(MAX_TAPS):
        if qx[:, k].any():
            v += qx[None, :, k] * t[:, np.minimum(fx + k, sw - 1)]
    assert int(v.max()) < 1 << 32
    return v


def convert(v, bd, samples, native_dtype):
    a = (v + (1 << (31 - bd))) >> (32 - bd)
    if samples == capi.EXPORT_NATIVE:
        assert int(a.max()) < 1 << bd
        return a.astype(native_dtype)
    if samples == capi.EXPORT_MSB16:
        return ((a << (16 - bd)) & 0xFFFF).astype(np.uint16)
    u8 = np.minimum(255, (v + (1 << 23)) >> 24)
    assert np.array_equal(u8, np.minimum(255, ((v >> 1) + (1 << 22)) >> 23))
    return u8.astype(np.uint8)


def expected_export_resized(planes, cf, bdl, bdc, layout, samples, out_size, rect=None):
    """what m355_frame_export_resized delivers, from the planes m355_frame_download returns"""
    sw, sh = sub_sampling(cf)
    out = []
    for c, p in enumerate(expected_export(planes, cf, bdl, bdc, capi.EXPORT_PLANAR, capi.EXPORT_NATIVE, rect)):
        bd = bdc if c else bdl
        ow, oh = (out_size[0] // sw, out_size[1] // sh) if c else out_size
        v = resize_plane(p, ow, oh, 1 if c and sw == 2 else 0, bd)
        out.append(np.ascontiguousarray(convert(v, bd, samples, p.dtype)))
    if layout == capi.EXPORT_SEMIPLANAR and len(out) == 3:
        out = [out[0], np.stack([out[1], out[2]], axis=-1).reshape(out[1].shape[0], -1)]
    return out


def float_resize(S, ow, oh, cosited_x):
    """an antialiased bilinear resize written independently, in float64: weights max(0, 1 - |k - c| / s) around the output sample's centre c in source
    coordinates, s = max(1, ratio), indices clamped to the plane, each row normalised"""
    def weights(sn, dn, cosited):
        W = np.zeros((dn, sn))
        s = max(1.0, sn / dn)
        for i in range(dn):
            c = i * sn / dn if cosited else (i + 0.5) * sn / dn - 0.5
            row = {}
            for k in range(int(np.floor(c - s)) - 1, int(np.ceil(c + s)) + 2):
                w = max(0.0, 1.0 - abs(k - c) / s)
                if w > 0:
                    kk = min(max(k, 0), sn - 1)
                    row[kk] = row.get(kk, 0.0) + w
            tot = sum(row.values())
            for kk, w in row.items():
                W[i, kk] = w / tot
        return W
    sh, sw = S.shape
    return weights(sh, oh, 0) @ S.astype(np.float64) @ weights(sw, ow, cosited_x).T


def check_export_resized(ctx, frame, planes, geom, layout, samples, out_size, rect=None, host=False, what=""):
    cf, bdl, bdc = geom
    got, raws = ctx.frame_export_finish(ctx.frame_export_resized(frame, layout, samples, out_size, rect, host=host), raw=True)
    assert_export(got, raws, expected_export_resized(planes, cf, bdl, bdc, layout, samples, out_size, rect),
                  "%s to %dx%d layout %d samples %d rect %s" % (what, out_size[0], out_size[1], layout, samples, rect))


def check_all_formats(ctx, frame, planes, geom, sizes, what=""):
    """every (rectangle, output size) x layout x sample format of one frame"""
    for rect, out_size in sizes:
        r = None if rect is None else chroma_grid_rect(rect, geom[0])
        for layout in LAYOUTS:
            for samples in SAMPLES:
                check_export_resized(ctx, frame, planes, geom, layout, samples, out_size, r, what=what)


def check_format_matrix_resized(ctx, o, cfg, sizes=MATRIX_SIZES):
    frame, planes, geom, frames = decode_into_frame(ctx, o, cfg)
    try:
        check_all_formats(ctx, frame, planes, geom, sizes, what=format_id(cfg))
    finally:
        for f in frames:
            ctx.frame_destroy(f)


def check_identity(ctx, o, bit_depth, layout):
    """out == rectangle delivers what m355_frame_export delivers, byte for byte, the padding included"""
    frame, planes, geom, frames = decode_into_frame(ctx, o, dict(width=64, height=32, bit_depth=bit_depth, seed=7700 + bit_depth, log2_ctb=5))
    try:
        for samples in SAMPLES:
            for rect in (None, MATRIX_RECT):
                size = (64, 32) if rect is None else rect[2:]
                plain = ctx.frame_export_finish(ctx.frame_export(frame, layout, samples, rect), raw=True)
                resized = ctx.frame_export_finish(ctx.frame_export_resized(frame, layout, samples, size, rect), raw=True)
                assert len(plain[1]) == len(resized[1])
                for a, b in zip(plain[1], resized[1]):
                    assert a.shape == b.shape and np.array_equal(a, b), "samples %d rect %s" % (samples, rect)
                assert not np.all(plain[1][0] == capi.DEVICE_FILL)
    finally:
        for f in frames:
            ctx.frame_destroy(f)


def check_minimum_sizes(ctx, o, bit_depth):
    """a 16x16 4:2:0 picture to 2x2 (chroma 1x1) and to 128x128; its 4x4 rectangle at (4, 4) to 2x2 and to 32x32"""
    frame, planes, geom, frames = decode_into_frame(ctx, o, dict(width=16, height=16, bit_depth=bit_depth, seed=7710 + bit_depth, log2_ctb=4))
    try:
        check_all_formats(ctx, frame, planes, geom, [(None, (2, 2)), (None, (128, 128)), ((4, 4, 4, 4), (2, 2)), ((4, 4, 4, 4), (32, 32))], what="16x16")
    finally:
        for f in frames:
            ctx.frame_destroy(f)


VALUE_SIZE = (32, 16)
VALUE_OUT = [(4, 2), (20, 10), (64, 32)]       # ratios 8, 3/2 (of 30x15) and 1/8 (of the 8x4 samples at (16, 4))
VALUE_RECTS = [None, (0, 0, 30, 15), (16, 4, 8, 4)]


def check_several_tiles(ctx):
    """more than one tile of output columns with a partial last one, more than one run of output rows, and at ratio 8 with 16-bit samples a span of
    more source vectors than a workgroup has lanes: 2400x16 to 300x2 and 48x8 to 384x40, 4:2:0, 10 bits, planes put there by frame_upload"""
    rng = np.random.default_rng(7730)
    for (w, h), out_size in (((2400, 16), (300, 2)), ((48, 8), (384, 40))):
        frame = ctx.frame_create(w, h, 1, 10, 10)
        try:
            planes = [rng.integers(0, 1024, (ph, pw)).astype(np.uint16) for pw, ph in worklist.plane_dims(w, h, 1)]
            ctx.frame_upload(frame, planes)
            check_all_formats(ctx, frame, planes, (1, 10, 10), [(None, out_size)], what="%dx%d" % (w, h))
        finally:
            ctx.frame_destroy(frame)


def value_cases(bd):
    """4:4:4 frames of 64x32 that reach what decoded pictures seldom do -> [(name, planes)]"""
    dt = np.uint8 if bd <= 8 else np.uint16
    w, h = VALUE_SIZE
    top = (1 << bd) - 1
    cases = [("zero", [np.zeros((h, w), dt)] * 3), ("maximum", [np.full((h, w), top, dt)] * 3)]
    one = np.zeros((h, w), dt)
    one[5, 19] = top
    cases.append(("single", [one, one[::-1].copy(), one[:, ::-1].copy()]))
    cols = np.zeros((h, w), dt); cols[:, 1::2] = top
    rows = np.zeros((h, w), dt); rows[1::2, :] = top
    cases.append(("alternating", [cols, rows, (cols ^ rows).astype(dt)]))
    ramp = (np.arange(w * h, dtype=np.uint64) * top // (w * h - 1)).astype(dt).reshape(h, w)
    assert int(ramp.max()) == top and int(ramp.min()) == 0
    cases.append(("ramp", [ramp, ramp[::-1].copy(), ramp[:, ::-1].copy()]))
    return cases


def check_values(ctx, bd):
    frame = ctx.frame_create(VALUE_SIZE[0], VALUE_SIZE[1], 3, bd, bd)
    try:
        for name, planes in value_cases(bd):
            ctx.frame_upload(frame, planes)
            for out_size, rect in zip(VALUE_OUT, VALUE_RECTS):
                if name in ("zero", "maximum"):
                    top = 0 if name == "zero" else (1 << bd) - 1
                    nat = expected_export_resized(planes, 3, bd, bd, capi.EXPORT_PLANAR, capi.EXPORT_NATIVE, out_size, rect)
                    u8 = expected_export_resized(planes, 3, bd, bd, capi.EXPORT_PLANAR, capi.EXPORT_U8, out_size, rect)
                    assert all(np.all(p == top) for p in nat), "the restatement does not keep a constant plane constant"
                    assert all(np.all(p == (255 if top else 0)) for p in u8)
                check_all_formats(ctx, frame, planes, (3, bd, bd), [(rect, out_size)], what="%s %d bit" % (name, bd))
    finally:
        ctx.frame_destroy(frame)


def check_rect_equals_cropped_frame(ctx, o):
    """the rectangle's planes uploaded into a second frame of that size: both resizes are identical (the clamps go to the rectangle).  The rectangle
    is 48x24 at (2, 2): a frame's size is a multiple of 8"""
    frame, planes, geom, frames = decode_into_frame(ctx, o, dict(width=64, height=32, bit_depth=10, seed=7720, log2_ctb=5))
    cf, bdl, bdc = geom
    rect = (2, 2, 48, 24)
    crop = ctx.frame_create(rect[2], rect[3], cf, bdl, bdc)
    try:
        ctx.frame_upload(crop, expected_export(planes, cf, bdl, bdc, capi.EXPORT_PLANAR, capi.EXPORT_NATIVE, rect))
        for out_size in ((36, 14), (64, 30), (8, 4)):
            for layout in LAYOUTS:
                a = ctx.frame_export_finish(ctx.frame_export_resized(frame, layout, capi.EXPORT_NATIVE, out_size, rect))
                b = ctx.frame_export_finish(ctx.frame_export_resized(crop, layout, capi.EXPORT_NATIVE, out_size))
                assert_planes_equal(a, b, "rectangle vs cropped frame to %dx%d" % out_size)
    finally:
        for f in frames + [crop]:
            ctx.frame_destroy(f)


def check_gate_resized(ctx, out_size=(80, 48)):
    """export_util.check_gate for the resized export: behind a decode whose lists the device rejected it writes nothing, behind an accepted decode of
    the same lists it does"""
    layout, samples = capi.EXPORT_SEMIPLANAR, capi.EXPORT_MSB16
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
        tokens.append(ctx.frame_export_resized(dst, layout, samples, out_size))
    good, bad = [ctx.frame_export_finish(t, raw=True) for t in tokens]
    assert ctx.decode_status(serials[0]) == 0 and ctx.decode_status(serials[1]) == M355_ERR_INVALID
    with_planes = ctx.frame_download(dst)           # (the rejected decode left the accepted picture in the frame)
    assert_export(good[0], good[1], expected_export_resized(with_planes, 1, 8, 8, layout, samples, out_size), "behind the accepted decode")
    for raw in bad[1]:
        assert np.all(raw == capi.DEVICE_FILL), "a resized export behind a rejected decode wrote to its destination"
    ctx.wait()
    for f in handles + [dst]:
        ctx.frame_destroy(f)


def check_hazard_resized(ctx, depth, out_size=(80, 36), layout=capi.EXPORT_SEMIPLANAR, samples=capi.EXPORT_MSB16):
    """export_util.check_hazard for the resized export: four pictures decoded alternately into a pool of two frames, each exported right behind its
    decode into a buffer of its own, no host wait in between; every export must deliver what the export of the same picture decoded alone
    delivers.  (On the GPU with several pictures in flight this sees a decode that does not wait for the resized export of its frame's previous
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
        rect = (2, 2, 120, 56)
        handles, tokens = [], []
        for j, pic in enumerate(pics):
            pic.ref_frames = [r0] + [-1] * (worklist.MAX_REF_FRAMES - 1)
            pic.dst_frame = pool[j % 2]
            handles.append(ctx.upload(pic))
            ctx.decode_resident(handles[-1])
            tokens.append(ctx.frame_export_resized(pool[j % 2], layout, samples, out_size, rect))
        got = [ctx.frame_export_finish(t, raw=True) for t in tokens]
        ctx.wait()
        for j in range(4):
            ctx.decode_resident(handles[j])
            ctx.wait()
            planes = ctx.frame_download(pool[j % 2])
            alone = ctx.frame_export_finish(ctx.frame_export_resized(pool[j % 2], layout, samples, out_size, rect))
            assert_planes_equal(alone, expected_export_resized(planes, 1, 10, 10, layout, samples, out_size, rect), "picture %d alone" % j)
            assert_export(got[j][0], got[j][1], alone, "picture %d, depth %d" % (j, depth))
        for j in (0, 1):
            assert not np.array_equal(got[j][0][0], got[j + 2][0][0]), "the pictures that share a frame must differ for this test to see a hazard"
        for h in handles:
            ctx.release(h)
        for f in pool + [r0]:
            ctx.frame_destroy(f)
    finally:
        ctx.set_pipeline_depth(1)
