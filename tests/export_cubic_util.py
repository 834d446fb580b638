"""Shared by the tests of M355_FILTER_CUBIC (SIMT-interpreter build, GPU and glue): the restatement of the cubic filter of include/de265_mi355x.h —
taps() in Python integers straight from the definition, the two signed passes in numpy int64 with asserts on the 32-bit bounds the header states, the
three conversions — and what the four _filtered exports deliver with it.  The composed exports are the existing restatements with "the resized export"
meaning the cubic one: export_rgb_util.expected_rgb and export_tensor_util.expected_tensor behind expected_export_resized below.

The drivers of the triangle's tests (format matrix, value cases, identity, gate, hazard; export_resized_util.py, export_resized_rgb_util.py,
export_tensor_util.py, export_tensor_rois_util.py) know one filter.  `cubic(ctx)` runs them for the cubic one: it yields the context with filter =
FILTER_CUBIC in its four export helpers and, for its duration, puts this module's resize_plane and convert in the place of export_resized_util's — the
only two functions of the filter; every composition above them is the one the triangle's tests use.  Every comparison of an export is exact."""
import contextlib
import functools

import numpy as np

import export_resized_util
import export_tensor_util
from export_util import LAYOUTS, SAMPLES, assert_export, chroma_grid_rect, expected_export, sub_sampling  # noqa: F401
from export_rgb_util import MATRIX_CONVERSIONS, expected_rgb
from export_tensor_util import expected_tensor
from synth_util import assert_planes_equal
from libde265_amd import capi, worklist

CUBIC = capi.FILTER_CUBIC
MAX_TAPS = 16
MAX_N = 16384
ABS_SUM_BOUND = 23000             # of a row's |q_k|: 4 * 23000^2 + 2^21 < 2^31
MATRIX_RECT = (2, 2, 50, 22)      # its source starts off a vector boundary
# (rectangle, output size) of the format matrix at 64x32: a non-integer ratio, ratio exactly 4, upscaling, and the rectangle down and up
MATRIX_SIZES = [(None, (48, 20)), (None, (16, 8)), (None, (128, 64)), (MATRIX_RECT, (36, 14)), (MATRIX_RECT, (64, 30))]


def rdiv(a, b):
    return (2 * a + b) // (2 * b)      # (floor, on signed values)


def ratio_ok(sn, dn):
    return 1 <= sn <= MAX_N and 1 <= dn <= MAX_N and sn <= 4 * dn and dn <= 8 * sn


def max_taps(sn, dn):
    return min(MAX_TAPS, -(-4 * max(sn, dn) // dn))


def weight(d, M):
    """2 M^3 w(d / M), w = Catmull-Rom"""
    if d <= M:
        return 3 * d ** 3 - 5 * M * d ** 2 + 2 * M ** 3
    return -d ** 3 + 5 * M * d ** 2 - 8 * M ** 2 * d + 4 * M ** 3


def taps(sn, dn, cosited, i):
    """row i of the axis sn -> dn: (first source index, [coefficients]), folded at the ends of [0, sn - 1]"""
    D, M = 2 * dn, 2 * max(sn, dn)
    C = 2 * i * sn if cosited else (2 * i + 1) * sn - dn
    ks = [k for k in range((C - 2 * M) // D - 1, (C + 2 * M) // D + 2) if abs(D * k - C) < 2 * M]
    assert 1 <= len(ks) <= MAX_TAPS and ks == list(range(ks[0], ks[-1] + 1))
    n = [weight(abs(D * k - C), M) for k in ks]
    N, P, q = sum(n), 0, []
    assert N > 0
    for nk in n:
        q.append(rdiv((P + nk) << 14, N) - rdiv(P << 14, N))
        P += nk
    assert sum(q) == 1 << 14
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
    """the horizontal sums v of one plane (computed once per plane and size, left unchanged)"""
    key = (S.shape, str(S.dtype), S.tobytes(), ow, oh, cosited_x, bd)
    if key not in _planes_done:
        if len(_planes_done) >= 32:
            _planes_done.clear()
        v = _resize_plane(S, ow, oh, cosited_x, bd)
        v.setflags(write=False)
        _planes_done[key] = v
    return _planes_done[key]


def _resize_plane(S, ow, oh, cosited_x, bd):
    """vertical pass, the rounding to the intermediate of 16 bits of fraction, horizontal pass (signed int64, a gather per tap)"""
    S = S.astype(np.int64)
    sh, sw = S.shape
    fy, qy = axis_table(sh, oh, 0)
    fx, qx = axis_table(sw, ow, cosited_x)
    u = np.zeros((oh, sw), np.int64)
    for k in range(MAX_TAPS):
        if qy[:, k].any():
            u += qy[:, k, None] * S[np.minimum(fy + k, sh - 1)]
    assert int(np.abs(u).max()) < 1 << 31
    t = (u + (1 << (bd - 3))) >> (bd - 2)
    v = np.zeros((oh, ow), np.int64)
    for k in range(MAX_TAPS):
        if qx[:, k].any():
            v += qx[None, :, k] * t[:, np.minimum(fx + k, sw - 1)]
    assert int(np.abs(v).max()) + (1 << 21) < 1 << 31
    return v


def convert(v, bd, samples, native_dtype):
    a = np.clip((v + (1 << (29 - bd))) >> (30 - bd), 0, (1 << bd) - 1)
    if samples == capi.EXPORT_NATIVE:
        return a.astype(native_dtype)
    if samples == capi.EXPORT_MSB16:
        return (a << (16 - bd)).astype(np.uint16)
    return np.clip((v + (1 << 21)) >> 22, 0, 255).astype(np.uint8)


def expected_export_resized(planes, cf, bdl, bdc, layout, samples, out_size, rect=None):
    """what m355_frame_export_resized_filtered delivers with M355_FILTER_CUBIC, from the planes m355_frame_download returns"""
    sw, sh = sub_sampling(cf)
    out = []
    for c, p in enumerate(expected_export(planes, cf, bdl, bdc, capi.EXPORT_PLANAR, capi.EXPORT_NATIVE, rect)):
        bd = bdc if c else bdl
        ow, oh = (out_size[0] // sw, out_size[1] // sh) if c else out_size
        out.append(np.ascontiguousarray(convert(resize_plane(p, ow, oh, 1 if c and sw == 2 else 0, bd), bd, samples, p.dtype)))
    if layout == capi.EXPORT_SEMIPLANAR and len(out) == 3:
        out = [out[0], np.stack([out[1], out[2]], axis=-1).reshape(out[1].shape[0], -1)]
    return out


def expected_resized_rgb(planes, cf, bdl, bdc, layout, samples, matrix, full_range, out_size, rect=None):
    """m355_frame_export_resized_rgb_filtered: the cubic resize (planar, NATIVE) through export_rgb_util.expected_rgb as a frame of the output size"""
    return expected_rgb(expected_export_resized(planes, cf, bdl, bdc, capi.EXPORT_PLANAR, capi.EXPORT_NATIVE, out_size, rect), cf, bdl, bdc, layout, samples, matrix, full_range)


def expected_ints(planes, geom, samples, matrix, full_range, out_size, rect=None):
    """the integer stage of the two tensor exports: planar R, G, B"""
    cf, bdl, bdc = geom
    return expected_resized_rgb(planes, cf, bdl, bdc, capi.RGB_PLANAR, samples, matrix, full_range, out_size, rect)


def float_resize(S, ow, oh, cosited_x):
    """an antialiased Catmull-Rom resize written independently, in float64: weights w(|k - c| / s) around the output sample's centre c in source
    coordinates, s = max(1, ratio), indices clamped to the plane, each row normalised; nothing is rounded or clipped"""
    def w(x):
        x = abs(x)
        if x <= 1.0:
            return 1.5 * x ** 3 - 2.5 * x ** 2 + 1.0
        return -0.5 * x ** 3 + 2.5 * x ** 2 - 4.0 * x + 2.0 if x < 2.0 else 0.0

    def weights(sn, dn, cosited):
        W = np.zeros((dn, sn))
        s = max(1.0, sn / dn)
        for i in range(dn):
            c = i * sn / dn if cosited else (i + 0.5) * sn / dn - 0.5
            row = {}
            for k in range(int(np.floor(c - 2 * s)) - 1, int(np.ceil(c + 2 * s)) + 2):
                kk = min(max(k, 0), sn - 1)
                row[kk] = row.get(kk, 0.0) + w((k - c) / s)
            tot = sum(row.values())
            for kk, x in row.items():
                W[i, kk] = x / tot
        return W
    sh, sw = S.shape
    return weights(sh, oh, 0) @ S.astype(np.float64) @ weights(sw, ow, cosited_x).T


class CubicContext:
    """a capi.Context whose four resizing export helpers pass filter = FILTER_CUBIC; everything else is the context's"""

    def __init__(self, ctx):
        self._ctx = ctx

    def __getattr__(self, name):
        return getattr(self._ctx, name)

    def frame_export_resized(self, *args, **kw):
        return self._ctx.frame_export_resized(*args, filter=CUBIC, **kw)

    def frame_export_resized_rgb(self, *args, **kw):
        return self._ctx.frame_export_resized_rgb(*args, filter=CUBIC, **kw)

    def frames_export_tensor(self, *args, **kw):
        return self._ctx.frames_export_tensor(*args, filter=CUBIC, **kw)

    def frames_export_tensor_rois(self, *args, **kw):
        return self._ctx.frames_export_tensor_rois(*args, filter=CUBIC, **kw)


VALUE_OUT = [(8, 4), (20, 10), (64, 32)]       # of export_resized_util.VALUE_RECTS: ratios 4, 3/2 (of 30x15) and 1/8 (of the 8x4 samples at (16, 4))


@contextlib.contextmanager
def cubic(ctx):
    """-> the context for the triangle's drivers, which then check the cubic filter (the module's docstring says how)"""
    saved = (export_resized_util.resize_plane, export_resized_util.convert, export_resized_util.VALUE_OUT, export_tensor_util.MATRIX_SIZES)
    export_resized_util.resize_plane, export_resized_util.convert = resize_plane, convert
    export_resized_util.VALUE_OUT, export_tensor_util.MATRIX_SIZES = VALUE_OUT, MATRIX_SIZES
    try:
        yield CubicContext(ctx)
    finally:
        export_resized_util.resize_plane, export_resized_util.convert, export_resized_util.VALUE_OUT, export_tensor_util.MATRIX_SIZES = saved


def check_export_resized(ctx, frame, planes, geom, layout, samples, out_size, rect=None, what=""):
    cf, bdl, bdc = geom
    got, raws = ctx.frame_export_finish(ctx.frame_export_resized(frame, layout, samples, out_size, rect, filter=CUBIC), raw=True)
    assert_export(got, raws, expected_export_resized(planes, cf, bdl, bdc, layout, samples, out_size, rect),
                  "%s cubic to %dx%d layout %d samples %d rect %s" % (what, out_size[0], out_size[1], layout, samples, rect))


def check_resized_rgb(ctx, frame, planes, geom, layout, samples, matrix, full_range, out_size, rect=None, what=""):
    cf, bdl, bdc = geom
    got, raws = ctx.frame_export_finish(ctx.frame_export_resized_rgb(frame, layout, samples, matrix, full_range, out_size, rect, filter=CUBIC), raw=True)
    assert_export(got, raws, expected_resized_rgb(planes, cf, bdl, bdc, layout, samples, matrix, full_range, out_size, rect),
                  "%s cubic to %dx%d layout %d samples %d matrix %d full %d rect %s" % (what, out_size[0], out_size[1], layout, samples, matrix, full_range, rect))


def check_all_formats(ctx, frame, planes, geom, sizes, what=""):
    """every (rectangle, output size) x layout x sample format of one frame through the resized export"""
    for rect, out_size in sizes:
        r = None if rect is None else chroma_grid_rect(rect, geom[0])
        for layout in LAYOUTS:
            for samples in SAMPLES:
                check_export_resized(ctx, frame, planes, geom, layout, samples, out_size, r, what=what)


def check_all_rgb(ctx, frame, planes, geom, sizes, what=""):
    """every (rectangle, output size) x layout x sample type of one frame through the resized R'G'B' export, the two conversions alternating"""
    k = 0
    for rect, out_size in sizes:
        r = None if rect is None else chroma_grid_rect(rect, geom[0])
        for layout in (capi.RGB_PACKED, capi.RGB_PLANAR):
            for samples in (capi.RGB_U8, capi.RGB_U16):
                matrix, full = MATRIX_CONVERSIONS[k % 2]
                check_resized_rgb(ctx, frame, planes, geom, layout, samples, matrix, full, out_size, r, what=what)
                k += 1


def upload_random(ctx, size, cf, bd, seed):
    """a frame of random samples over the whole range of bd bits, put there by frame_upload -> (frame, planes)"""
    rng = np.random.default_rng(seed)
    dt = np.uint8 if bd <= 8 else np.uint16
    planes = [rng.integers(0, 1 << bd, (ph, pw)).astype(dt) for pw, ph in worklist.plane_dims(size[0], size[1], cf) if pw]
    frame = ctx.frame_create(size[0], size[1], cf, bd, bd)
    ctx.frame_upload(frame, planes)
    return frame, planes


def check_16_bit_formats(ctx, rgb=False):
    """the format matrix at 64x32 for 16-bit samples (no decoded picture has them: random planes), 4:2:0 — the operands of the signed dot product are
    the samples less 2^15 there"""
    frame, planes = upload_random(ctx, (64, 32), 1, 16, 8516)
    try:
        (check_all_rgb if rgb else check_all_formats)(ctx, frame, planes, (1, 16, 16), MATRIX_SIZES, what="bd16 random")
    finally:
        ctx.frame_destroy(frame)


def value_cases(bd):
    """4:4:4 frames of 32x16: single samples of the maximum in a plane of zeros and of zero in a plane of the maximum, near a corner and inside — the
    filter's negative lobes around them go below zero and above the maximum, so both clips are reached — and checkerboards of 0 and the maximum
    -> [(name, planes)]"""
    dt = np.uint8 if bd <= 8 else np.uint16
    top = (1 << bd) - 1
    out = []
    for name, back, fore in (("impulse of the maximum", 0, top), ("impulse of zero", top, 0)):
        planes = []
        for y, x in ((5, 19), (0, 1), (15, 30)):
            p = np.full((16, 32), back, dt)
            p[y, x] = fore
            planes.append(p)
        out.append((name, planes))
    cols = np.zeros((16, 32), dt); cols[:, 1::2] = top
    rows = np.zeros((16, 32), dt); rows[1::2, :] = top
    out.append(("checkerboard", [cols, rows, (cols ^ rows).astype(dt)]))
    return out


VALUE_SIZES = ((20, 10), (64, 32), (8, 4))        # ratios 8/5, 1/2 and exactly 4


def check_value_cases(ctx, bd, rgb=False):
    frame = ctx.frame_create(32, 16, 3, bd, bd)
    top = (1 << bd) - 1
    try:
        for name, planes in value_cases(bd):
            ctx.frame_upload(frame, planes)
            for out_size in VALUE_SIZES:
                if name.startswith("impulse") and out_size != (8, 4):
                    # the sums overshoot before the clip, or the case would not reach it
                    v = resize_plane(planes[0], out_size[0], out_size[1], 0, bd)
                    a = (v + (1 << (29 - bd))) >> (30 - bd)
                    assert (int(a.min()) < 0) if planes[0].flat[0] == 0 else (int(a.max()) > top), "%s to %s: no overshoot" % (name, out_size)
                (check_all_rgb if rgb else check_all_formats)(ctx, frame, planes, (3, bd, bd), [(None, out_size)], what="%s %d bit" % (name, bd))
    finally:
        ctx.frame_destroy(frame)


def check_rect_equals_cropped_frame(ctx, rgb=False):
    """the rectangle's planes uploaded into a second frame of that size: both resizes are identical (the clamps go to the rectangle).  The rectangle
    is 48x24 at (2, 2): a frame's size is a multiple of 8"""
    frame, planes = upload_random(ctx, (64, 32), 1, 10, 8520)
    rect = (2, 2, 48, 24)
    crop = ctx.frame_create(rect[2], rect[3], 1, 10, 10)
    try:
        ctx.frame_upload(crop, expected_export(planes, 1, 10, 10, capi.EXPORT_PLANAR, capi.EXPORT_NATIVE, rect))
        for out_size in ((36, 14), (64, 30), (12, 6)):
            if rgb:
                a = ctx.frame_export_finish(ctx.frame_export_resized_rgb(frame, capi.RGB_PLANAR, capi.RGB_U16, capi.MATRIX_BT709, 0, out_size, rect, filter=CUBIC))
                b = ctx.frame_export_finish(ctx.frame_export_resized_rgb(crop, capi.RGB_PLANAR, capi.RGB_U16, capi.MATRIX_BT709, 0, out_size, filter=CUBIC))
                assert_planes_equal(a, b, "rectangle vs cropped frame to %dx%d" % out_size)
                continue
            for layout in LAYOUTS:
                a = ctx.frame_export_finish(ctx.frame_export_resized(frame, layout, capi.EXPORT_NATIVE, out_size, rect, filter=CUBIC))
                b = ctx.frame_export_finish(ctx.frame_export_resized(crop, layout, capi.EXPORT_NATIVE, out_size, filter=CUBIC))
                assert_planes_equal(a, b, "rectangle vs cropped frame to %dx%d" % out_size)
    finally:
        ctx.frame_destroy(frame)
        ctx.frame_destroy(crop)


def check_minimum_sizes(ctx, rgb=False):
    """1x1 luma of a monochrome frame (from 4x4 down and from 1x1 — a rectangle — at its own size and up to 8x8) and 2x2 of a 4:2:0 frame (chroma 1x1:
    every clamp folds onto one sample), from 8x8 and from its 2x2 rectangle, which also goes up to 16x16"""
    mono, mplanes = upload_random(ctx, (8, 8), 0, 8, 8530)
    f420, planes = upload_random(ctx, (8, 8), 1, 10, 8531)
    check = check_all_rgb if rgb else check_all_formats
    try:
        check(ctx, mono, mplanes, (0, 8, 8), [((0, 0, 4, 4), (1, 1)), ((3, 5, 1, 1), (1, 1)), ((3, 5, 1, 1), (8, 8)), ((0, 0, 3, 4), (1, 2))], what="monochrome")
        check(ctx, f420, planes, (1, 10, 10), [(None, (2, 2)), ((4, 2, 2, 2), (2, 2)), ((4, 2, 2, 2), (16, 16))], what="4:2:0")
    finally:
        ctx.frame_destroy(mono)
        ctx.frame_destroy(f420)


# (frame size, output size), 4:2:0, 10 bits: ratio 4 with a span of more source vectors than a workgroup has lanes and a partial last tile of output
# columns; upscaling over two tiles and three runs of rows; a non-integer ratio over three tiles
TILE_CASES = (((2400, 16), (600, 4)), ((48, 8), (384, 40)), ((1040, 16), (694, 10)))


def check_several_tiles(ctx, rgb=False):
    for k, ((w, h), out_size) in enumerate(TILE_CASES):
        frame, planes = upload_random(ctx, (w, h), 1, 10, 8540 + k)
        try:
            if rgb:
                check_all_rgb(ctx, frame, planes, (1, 10, 10), [(None, out_size)], what="%dx%d" % (w, h))
            else:
                check_all_formats(ctx, frame, planes, (1, 10, 10), [(None, out_size)], what="%dx%d" % (w, h))
        finally:
            ctx.frame_destroy(frame)


TENSOR_ROIS = [(0, 0, 128, 64, 0), (34, 6, 62, 34, 0), (34, 6, 62, 34, capi.ROI_MIRROR), (112, 56, 16, 8, 0)]   # ratios 2, ~1, ~1 mirrored, 1/8 to 64x32 ... 1/4


def check_tensor_batch(ctx, n=3, out_size=(48, 20)):
    """n frames of 128x64 (4:2:0, 10 bits, random), one rectangle, as one tensor: NCHW F32 and NHWC F16, against the restatement"""
    made = [upload_random(ctx, (128, 64), 1, 10, 8550 + i) for i in range(n)]
    frames, planes = [f for f, _ in made], [p for _, p in made]
    geom = (1, 10, 10)
    try:
        for layout, dtype, samples, rect in ((capi.TENSOR_NCHW, capi.TENSOR_F32, capi.RGB_U8, None), (capi.TENSOR_NHWC, capi.TENSOR_F16, capi.RGB_U16, (2, 2, 124, 60)),
                                             (capi.TENSOR_NCHW, capi.TENSOR_BF16, capi.RGB_U8, (2, 2, 124, 60))):
            scale, bias = export_tensor_util.imagenet(samples)
            ints = [expected_ints(p, geom, samples, capi.MATRIX_BT709, 0, out_size, rect) for p in planes]
            got = ctx.tensor_export_finish(ctx.frames_export_tensor(frames, layout, dtype, samples, capi.MATRIX_BT709, 0, out_size, scale, bias, rect, filter=CUBIC))
            export_tensor_util.assert_tensor(got, expected_tensor(ints, layout, dtype, scale, bias), "cubic batch of %d, layout %d dtype %d" % (n, layout, dtype))
    finally:
        for f in frames:
            ctx.frame_destroy(f)


def check_tensor_rois(ctx, rois=TENSOR_ROIS, out_size=(64, 32)):
    """regions of different ratios of two 128x64 frames (4:2:0, 10 bits, random), one mirrored beside its unmirrored twin, as one tensor"""
    made = [upload_random(ctx, (128, 64), 1, 10, 8560 + i) for i in range(2)]
    geom = (1, 10, 10)
    frames = [made[i % 2][0] for i in range(len(rois))]
    planes = [made[i % 2][1] for i in range(len(rois))]
    frames[2], planes[2] = frames[1], planes[1]                # (the mirrored entry and its twin share a frame)
    try:
        for layout, dtype, samples in ((capi.TENSOR_NCHW, capi.TENSOR_F32, capi.RGB_U8), (capi.TENSOR_NHWC, capi.TENSOR_BF16, capi.RGB_U16)):
            scale, bias = export_tensor_util.imagenet(samples)
            want = []
            for p, r in zip(planes, rois):
                w = expected_tensor([expected_ints(p, geom, samples, capi.MATRIX_BT2020, 1, out_size, r[:4])], layout, dtype, scale, bias)[0]
                if r[4] & capi.ROI_MIRROR:
                    w = w[:, :, ::-1] if layout == capi.TENSOR_NCHW else w[:, ::-1, :]
                want.append(w)
            got = ctx.tensor_export_finish(ctx.frames_export_tensor_rois(frames, rois, layout, dtype, samples, capi.MATRIX_BT2020, 1, out_size, scale, bias, filter=CUBIC))
            export_tensor_util.assert_tensor(got, np.stack(want), "cubic regions, layout %d dtype %d" % (layout, dtype))
            assert not np.array_equal(got[0][1], got[0][2]), "a slice that equals its reversal shows nothing"
    finally:
        for f, _ in made:
            ctx.frame_destroy(f)
