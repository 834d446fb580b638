"""Shared by the chroma sample location tests (SIMT-interpreter build, GPU and glue): the definition of m355_export_opts in include/de265_mi355x.h
restated in Python integers / numpy int64, parameterised by chroma_loc — the reconstruction filter with weights in quarters per axis, the resize grids
that keep the siting, and the composed exports as compositions — on top of the restatements of the type-0 exports, which are imported, not copied.
Every comparison of pixels is exact, the untouched padding of the destinations included."""
import numpy as np

import export_cubic_util
import export_resized_util
from export_util import assert_export, expected_export, sub_sampling
from export_rgb_util import M355_ERR_INVALID, chroma_at_luma, chroma_case, coefficients, expected_rgb, matrix_rgb, shape_rgb  # noqa: F401
from export_tensor_util import assert_tensor, expected_tensor
from export_tensor_rois_util import reverse_columns, upload_random  # noqa: F401
from synth_util import assert_planes_equal, make_case
from libde265_amd import capi, worklist

TRIANGLE, CUBIC = capi.FILTER_TRIANGLE, capi.FILTER_CUBIC
LOCS = (0, 1, 2, 3)
RGB_LAYOUTS = (capi.RGB_PACKED, capi.RGB_PLANAR)
RGB_SAMPLES = (capi.RGB_U8, capi.RGB_U16)
CHROMA_RECT = (6, 6, 20, 8)
# source 64x32: (rectangle, output size, filters).  16x8 is 4x down, the cubic limit; 8x4 is 8x down, the triangle's
RESIZE_CASES = [(None, (48, 24), (TRIANGLE, CUBIC)), (None, (128, 64), (TRIANGLE, CUBIC)), (None, (16, 8), (TRIANGLE, CUBIC)), (None, (8, 4), (TRIANGLE,)),
                ((2, 2, 44, 26), (30, 18), (TRIANGLE, CUBIC))]
WIDE_CASE = ((96, 32), (528, 40))     # wider than one tile of 256 columns, taller than two tile rows of 16: the last tile row is partial


def axis_weights(n, cn, second, sited):
    """one axis of the reconstruction filter for luma positions 0 .. n - 1 over cn chroma samples -> (index a, index b, weight of a in quarters);
    b has weight 4 - that.  `second` = hx for the horizontal axis and vy for the vertical one; `sited` says which table applies: "h" — LEFT / CENTRE,
    "v" — MID / TOP"""
    P = np.arange(n)
    i, odd = P >> 1, (P & 1) == 1
    if (sited == "h" and second == 0) or (sited == "v" and second == 1):       # LEFT / TOP: the chroma sample sits on the even luma position
        return i, np.clip(i + 1, 0, cn - 1), np.where(odd, 2, 4)
    return i, np.clip(np.where(odd, i + 1, i - 1), 0, cn - 1), np.full(n, 3)   # CENTRE / MID: midway between the even and the odd position


def chroma_at_luma_sited(C, W, H, loc, clamp=True):
    """the 4:2:0 chroma plane C brought to the W x H luma positions for chroma sample location type loc -> int64 (H, W); clamp=False leaves the rim
    to the caller (indices wrap: only the samples whose taps are not clamped mean anything)"""
    assert loc in LOCS
    C = C.astype(np.int64)
    CH, CW = C.shape
    hx, vy = loc & 1, loc >> 1
    ia, ib, wa = axis_weights(W, CW if clamp else 1 << 30, hx, "h")
    ja, jb, va = axis_weights(H, CH if clamp else 1 << 30, vy, "v")
    if not clamp:
        ib, jb = ib % CW, jb % CH
    T = va[:, None] * C[ja] + (4 - va)[:, None] * C[jb]                        # (H, CW), quarters
    s = wa[None, :] * T[:, ia] + (4 - wa)[None, :] * T[:, ib]
    assert int(s.max()) < 1 << 20
    return (s + 8) >> 4


def unclamped(W, H, loc):
    """mask (H, W) of the luma positions whose taps all lie inside a plane of W / 2 x H / 2"""
    hx, vy = loc & 1, loc >> 1
    X, Y = np.arange(W), np.arange(H)
    okx = np.where(X & 1, (X >> 1) + 1 <= W // 2 - 1, (X >> 1) - 1 >= 0 if hx else True)
    oky = np.where(Y & 1, (Y >> 1) + 1 <= H // 2 - 1, True if vy else (Y >> 1) - 1 >= 0)
    return oky[:, None] & okx[None, :]


def ramp_plane(cw, ch, loc, base, g, gv):
    """the ramp base + 2 g X + 2 gv Y over luma positions, sampled where type loc puts chroma sample (i, j): X = 2 i (LEFT) or 2 i + 1/2 (CENTRE),
    Y = 2 j (TOP) or 2 j + 1/2 (MID)"""
    hx, vy = loc & 1, loc >> 1
    i, j = np.arange(cw)[None, :], np.arange(ch)[:, None]
    return base + g * (4 * i + hx) + gv * (4 * j + (0 if vy else 1))


def expected_rgb_sited(planes, bdl, bdc, layout, samples, matrix, full_range, loc, rect=None):
    """what m355_frame_export_rgb_opts delivers for a 4:2:0 frame: the whole frame is converted and the rectangle cut from it"""
    H, W = planes[0].shape
    k = coefficients(matrix, full_range, bdl, bdc, samples)
    rgb = matrix_rgb(planes[0].astype(np.int64), chroma_at_luma_sited(planes[1], W, H, loc), chroma_at_luma_sited(planes[2], W, H, loc), k)
    return shape_rgb(rgb, layout, samples, rect)


def resize_plane_sited(S, ow, oh, cosited_x, cosited_y, bd, filter):
    """the horizontal sums v of one plane with a siting per axis: the passes of export_resized_util / export_cubic_util._resize_plane, whose vertical
    axis is centre-aligned by construction, with that axis' table chosen too"""
    m = export_cubic_util if filter == CUBIC else export_resized_util
    S = S.astype(np.int64)
    sh, sw = S.shape
    fy, qy = m.axis_table(sh, oh, cosited_y)
    fx, qx = m.axis_table(sw, ow, cosited_x)
    u = np.zeros((oh, sw), np.int64)
    for k in range(m.MAX_TAPS):
        u += qy[:, k, None] * S[np.minimum(fy + k, sh - 1)]
    t = (u + (1 << (bd - 3))) >> (bd - 2) if filter == CUBIC else (u + (1 << (bd - 5))) >> (bd - 4)
    v = np.zeros((oh, ow), np.int64)
    for k in range(m.MAX_TAPS):
        v += qx[None, :, k] * t[:, np.minimum(fx + k, sw - 1)]
    return v


def expected_export_resized_sited(planes, bdl, bdc, layout, samples, out_size, loc, rect=None, filter=TRIANGLE):
    """what m355_frame_export_resized_opts delivers for a 4:2:0 frame: chroma horizontally co-sited iff LEFT, vertically co-sited iff TOP"""
    m = export_cubic_util if filter == CUBIC else export_resized_util
    out = []
    for c, p in enumerate(expected_export(planes, 1, bdl, bdc, capi.EXPORT_PLANAR, capi.EXPORT_NATIVE, rect)):
        bd = bdc if c else bdl
        ow, oh = (out_size[0] // 2, out_size[1] // 2) if c else out_size
        v = resize_plane_sited(p, ow, oh, 1 if c and not loc & 1 else 0, 1 if c and loc >> 1 else 0, bd, filter)
        out.append(np.ascontiguousarray(m.convert(v, bd, samples, p.dtype)))
    if layout == capi.EXPORT_SEMIPLANAR:
        out = [out[0], np.stack([out[1], out[2]], axis=-1).reshape(out[1].shape[0], -1)]
    return out


def expected_resized_rgb_sited(planes, bdl, bdc, layout, samples, matrix, full_range, out_size, loc, rect=None, filter=TRIANGLE):
    """the composition: the sited resize (planar, NATIVE) through the sited R'G'B' export of a frame of the output size"""
    R = expected_export_resized_sited(planes, bdl, bdc, capi.EXPORT_PLANAR, capi.EXPORT_NATIVE, out_size, loc, rect, filter)
    return expected_rgb_sited(R, bdl, bdc, layout, samples, matrix, full_range, loc)


def expected_ints_sited(planes, bd, samples, matrix, full_range, out_size, loc, rect=None, filter=TRIANGLE):
    return expected_resized_rgb_sited(planes, bd, bd, capi.RGB_PLANAR, samples, matrix, full_range, out_size, loc, rect, filter)


# ---- the restatement against itself -------------------------------------------------------------------------------------------------------------

def check_restatement():
    """type 0 is the filter of export_rgb_util and the grids of export_resized_util / export_cubic_util; every type reconstructs a ramp sampled at
    its own chroma positions exactly"""
    rng = np.random.default_rng(9100)
    C = rng.integers(0, 1 << 10, (8, 16))
    assert np.array_equal(chroma_at_luma_sited(C, 32, 16, 0), chroma_at_luma(C, 1, 32, 16))
    planes = [rng.integers(0, 1 << 10, (32, 64)).astype(np.uint16)] + [rng.integers(0, 1 << 10, (16, 32)).astype(np.uint16) for _ in range(2)]
    for filt, m in ((TRIANGLE, export_resized_util), (CUBIC, export_cubic_util)):
        for layout, samples in ((capi.EXPORT_PLANAR, capi.EXPORT_NATIVE), (capi.EXPORT_SEMIPLANAR, capi.EXPORT_U8)):
            assert_planes_equal(expected_export_resized_sited(planes, 10, 10, layout, samples, (48, 24), 0, None, filt),
                                m.expected_export_resized(planes, 1, 10, 10, layout, samples, (48, 24)), "type 0, filter %d" % filt)
    W, H = 32, 16
    for loc in LOCS:
        for base, g, gv in ((100, 3, 5), (900, -4, 2), (37, 0, 7), (512, 6, 0)):
            want = base + 2 * g * np.arange(W)[None, :] + 2 * gv * np.arange(H)[:, None]
            got = chroma_at_luma_sited(ramp_plane(W // 2, H // 2, loc, base, g, gv), W, H, loc, clamp=False)
            ok = unclamped(W, H, loc)
            assert ok.sum() >= (W - 2) * (H - 2) and np.array_equal(got[ok], np.broadcast_to(want, got.shape)[ok]), "type %d does not reconstruct its own ramp" % loc
            # a type's filter on another type's sampling is off by the shift between the two sitings: the four definitions are four
            for other in LOCS:
                if other != loc:
                    assert not np.array_equal(chroma_at_luma_sited(ramp_plane(W // 2, H // 2, other, 100, 3, 5), W, H, loc, clamp=False)[ok],
                                              np.broadcast_to(100 + 6 * np.arange(W)[None, :] + 10 * np.arange(H)[:, None], got.shape)[ok])


# ---- drivers: each runs on the interpreter build and on the GPU ------------------------------------------------------------------------------------

def finish(ctx, token):
    return ctx.frame_export_finish(token, raw=True)


def assert_same_bytes(a, b, what):
    """two finished exports (planes, raw buffers): byte for byte, padding included"""
    assert len(a[1]) == len(b[1]), what
    for k, (x, y) in enumerate(zip(a[1], b[1])):
        assert np.array_equal(x, y), "%s: buffer %d differs" % (what, k)


def random_frame(ctx, bd, seed, size=(64, 32)):
    return upload_random(ctx, size, 1, bd, seed)


def check_type0_is_plain(ctx, bd):
    """type 0 through each _opts entry point, and a NULL options pointer, deliver what the plain (filter 0) or _filtered entry point delivers"""
    frame, planes = random_frame(ctx, bd, 9200 + bd)
    other, _ = random_frame(ctx, bd, 9300 + bd)
    try:
        rgb = (frame, capi.RGB_PACKED, capi.RGB_U8, capi.MATRIX_BT709, 0, (2, 2, 44, 26))
        plain = finish(ctx, ctx.frame_export_rgb(*rgb))
        assert_same_bytes(finish(ctx, ctx.frame_export_rgb(*rgb, opts_entry=True)), plain, "rgb, type 0")
        assert_same_bytes(finish(ctx, ctx.frame_export_rgb(*rgb, opts_entry=None)), plain, "rgb, NULL options")
        scale, bias = [1.0 / 255, 0.5 / 255, 2.0 / 255], [0.0, -1.0, 0.25]
        rois = [(0, 0, 64, 32, 0), (2, 2, 44, 26, capi.ROI_MIRROR), (16, 8, 32, 16, 0)]
        for filt in (TRIANGLE, CUBIC):
            base = dict(filter=filt, filtered_entry=filt != 0)
            rs = (frame, capi.EXPORT_SEMIPLANAR, capi.EXPORT_MSB16, (48, 24), (2, 2, 44, 26))
            plain = finish(ctx, ctx.frame_export_resized(*rs, **base))
            assert_same_bytes(finish(ctx, ctx.frame_export_resized(*rs, filter=filt, opts_entry=True)), plain, "resized, type 0, filter %d" % filt)
            rr = (frame, capi.RGB_PLANAR, capi.RGB_U16, capi.MATRIX_BT2020, 1, (48, 24), (2, 2, 44, 26))
            plain = finish(ctx, ctx.frame_export_resized_rgb(*rr, **base))
            assert_same_bytes(finish(ctx, ctx.frame_export_resized_rgb(*rr, filter=filt, opts_entry=True)), plain, "resized rgb, type 0, filter %d" % filt)
            te = ([frame, other, frame], capi.TENSOR_NCHW, capi.TENSOR_F16, capi.RGB_U8, capi.MATRIX_BT709, 0, (32, 16), scale, bias)
            plain = ctx.tensor_export_finish(ctx.frames_export_tensor(*te, **base))
            assert np.array_equal(ctx.tensor_export_finish(ctx.frames_export_tensor(*te, filter=filt, opts_entry=True))[1], plain[1]), "tensor, filter %d" % filt
            tr = ([frame, other, frame], rois, capi.TENSOR_NHWC, capi.TENSOR_F32, capi.RGB_U16, capi.MATRIX_BT709, 0, (32, 16), scale, bias)
            plain = ctx.tensor_export_finish(ctx.frames_export_tensor_rois(*tr, **base))
            assert np.array_equal(ctx.tensor_export_finish(ctx.frames_export_tensor_rois(*tr, filter=filt, opts_entry=True))[1], plain[1]), "rois, filter %d" % filt
            if filt == TRIANGLE:                 # NULL options: the triangle filter, type 0
                assert_same_bytes(finish(ctx, ctx.frame_export_resized(*rs, opts_entry=None)), finish(ctx, ctx.frame_export_resized(*rs)), "resized, NULL options")
                assert_same_bytes(finish(ctx, ctx.frame_export_resized_rgb(*rr, opts_entry=None)), finish(ctx, ctx.frame_export_resized_rgb(*rr)), "resized rgb, NULL options")
                assert np.array_equal(ctx.tensor_export_finish(ctx.frames_export_tensor(*te, opts_entry=None))[1], ctx.tensor_export_finish(ctx.frames_export_tensor(*te))[1])
                assert np.array_equal(ctx.tensor_export_finish(ctx.frames_export_tensor_rois(*tr, opts_entry=None))[1], ctx.tensor_export_finish(ctx.frames_export_tensor_rois(*tr))[1])
    finally:
        ctx.frame_destroy(frame)
        ctx.frame_destroy(other)


def check_rgb_sited(ctx, frame, planes, bd, loc, rects, what="", layouts=RGB_LAYOUTS, samples_set=RGB_SAMPLES, must_differ=True):
    """m355_frame_export_rgb_opts of an uploaded 4:2:0 frame against the restatement; must_differ: the expected output is not type 0's (an
    implementation that ignores chroma_loc cannot pass)"""
    for rect in rects:
        for layout in layouts:
            for samples in samples_set:
                want = expected_rgb_sited(planes, bd, bd, layout, samples, capi.MATRIX_BT709, 1, loc, rect)
                if must_differ:
                    zero = expected_rgb_sited(planes, bd, bd, layout, samples, capi.MATRIX_BT709, 1, 0, rect)
                    assert any(not np.array_equal(a, b) for a, b in zip(want, zero)), "%s: type %d expects what type 0 expects" % (what, loc)
                got, raws = finish(ctx, ctx.frame_export_rgb(frame, layout, samples, capi.MATRIX_BT709, 1, rect, chroma_loc=loc))
                assert_export(got, raws, want, "%s type %d layout %d samples %d rect %s" % (what, loc, layout, samples, rect))


def check_chroma_case(ctx, bd, loc):
    planes = chroma_case(1, bd, 9400 + bd)
    frame = ctx.frame_create(32, 16, 1, bd, bd)
    try:
        ctx.frame_upload(frame, planes)
        check_rgb_sited(ctx, frame, planes, bd, loc, (None, CHROMA_RECT), "chroma case %d bit" % bd)
    finally:
        ctx.frame_destroy(frame)


def check_resized_sited(ctx, bd, loc):
    """the resizing and the composed export of one random 64x32 frame for one type: every size and filter of RESIZE_CASES"""
    frame, planes = random_frame(ctx, bd, 9500 + bd)
    try:
        for rect, out_size, filters in RESIZE_CASES:
            for filt in filters:
                what = "type %d %d bit rect %s to %dx%d filter %d" % (loc, bd, rect, out_size[0], out_size[1], filt)
                sited = expected_export_resized_sited(planes, bd, bd, capi.EXPORT_PLANAR, capi.EXPORT_NATIVE, out_size, loc, rect, filt)
                zero = expected_export_resized_sited(planes, bd, bd, capi.EXPORT_PLANAR, capi.EXPORT_NATIVE, out_size, 0, rect, filt)
                assert np.array_equal(sited[0], zero[0]) and not np.array_equal(sited[1], zero[1]), "%s: luma moves, or chroma expects what type 0 expects" % what
                for layout, samples in ((capi.EXPORT_PLANAR, capi.EXPORT_NATIVE), (capi.EXPORT_SEMIPLANAR, capi.EXPORT_U8)):
                    got, raws = finish(ctx, ctx.frame_export_resized(frame, layout, samples, out_size, rect, filter=filt, chroma_loc=loc))
                    assert_export(got, raws, expected_export_resized_sited(planes, bd, bd, layout, samples, out_size, loc, rect, filt), what)
                layout, samples = (capi.RGB_PACKED, capi.RGB_U8) if filt == TRIANGLE else (capi.RGB_PLANAR, capi.RGB_U16)
                got, raws = finish(ctx, ctx.frame_export_resized_rgb(frame, layout, samples, capi.MATRIX_BT2020, 0, out_size, rect, filter=filt, chroma_loc=loc))
                assert_export(got, raws, expected_resized_rgb_sited(planes, bd, bd, layout, samples, capi.MATRIX_BT2020, 0, out_size, loc, rect, filt), what + " rgb")
        # out == rectangle: the rows are {1 << 14} on every grid, whatever the siting
        for rect in (None, (2, 2, 44, 26)):
            size = (64, 32) if rect is None else rect[2:]
            for filt in (TRIANGLE, CUBIC):
                got, raws = finish(ctx, ctx.frame_export_resized(frame, capi.EXPORT_PLANAR, capi.EXPORT_NATIVE, size, rect, filter=filt, chroma_loc=loc))
                assert_export(got, raws, ctx.frame_export_finish(ctx.frame_export(frame, capi.EXPORT_PLANAR, capi.EXPORT_NATIVE, rect)), "identity, type %d" % loc)
    finally:
        ctx.frame_destroy(frame)


def check_constant_stays_constant(ctx, bd, loc):
    dt = np.uint8 if bd == 8 else np.uint16
    vals = (37 << (bd - 8), 201 << (bd - 8), 90 << (bd - 8))
    planes = [np.full((32, 64), vals[0], dt), np.full((16, 32), vals[1], dt), np.full((16, 32), vals[2], dt)]
    frame = ctx.frame_create(64, 32, 1, bd, bd)
    try:
        ctx.frame_upload(frame, planes)
        for filt in (TRIANGLE, CUBIC):
            got = ctx.frame_export_finish(ctx.frame_export_resized(frame, capi.EXPORT_PLANAR, capi.EXPORT_NATIVE, (48, 24), filter=filt, chroma_loc=loc))
            for c in range(3):
                assert np.all(got[c] == vals[c]), "plane %d, type %d, filter %d" % (c, loc, filt)
            rgb = ctx.frame_export_finish(ctx.frame_export_resized_rgb(frame, capi.RGB_PLANAR, capi.RGB_U8, capi.MATRIX_BT709, 0, (48, 24), filter=filt, chroma_loc=loc))
            for c in range(3):
                assert len(np.unique(rgb[c])) == 1
    finally:
        ctx.frame_destroy(frame)


def check_wide(ctx, loc, bd=10):
    """several tiles across and a partial last tile row: a tile's first luma column takes chroma column cc0 - 1 from outside its own range"""
    size, out_size = WIDE_CASE
    frame, planes = random_frame(ctx, bd, 9600 + loc, size)
    try:
        got, raws = finish(ctx, ctx.frame_export_resized_rgb(frame, capi.RGB_PACKED, capi.RGB_U8, capi.MATRIX_BT709, 0, out_size, chroma_loc=loc))
        assert_export(got, raws, expected_resized_rgb_sited(planes, bd, bd, capi.RGB_PACKED, capi.RGB_U8, capi.MATRIX_BT709, 0, out_size, loc), "wide, type %d" % loc)
    finally:
        ctx.frame_destroy(frame)


TENSOR_ROIS = [(0, 0, 64, 32, 0), (2, 2, 44, 26, 0), (2, 2, 44, 26, capi.ROI_MIRROR)]


def check_tensors_sited(ctx, loc=2, bd=10, out_size=(32, 16)):
    """3 frames as one tensor and 3 regions (one mirrored) as one tensor, F16 NCHW and F32 NHWC, against the restatement through the float stage"""
    made = [random_frame(ctx, bd, 9700 + k) for k in range(3)]
    frames, planes = [f for f, _ in made], [p for _, p in made]
    scale, bias = [1.0 / 255, 0.5 / 255, 2.0 / 255], [0.0, -1.0, 0.25]
    try:
        for layout, dtype, samples in ((capi.TENSOR_NCHW, capi.TENSOR_F16, capi.RGB_U8), (capi.TENSOR_NHWC, capi.TENSOR_F32, capi.RGB_U16)):
            ints = [expected_ints_sited(p, bd, samples, capi.MATRIX_BT2020, 0, out_size, loc) for p in planes]
            zero = [expected_ints_sited(p, bd, samples, capi.MATRIX_BT2020, 0, out_size, 0) for p in planes]
            assert any(not np.array_equal(a, b) for x, y in zip(ints, zero) for a, b in zip(x, y)), "type %d expects what type 0 expects" % loc
            got = ctx.tensor_export_finish(ctx.frames_export_tensor(frames, layout, dtype, samples, capi.MATRIX_BT2020, 0, out_size, scale, bias, chroma_loc=loc))
            assert_tensor(got, expected_tensor(ints, layout, dtype, scale, bias), "tensor, type %d layout %d dtype %d" % (loc, layout, dtype))
            want = []
            for k, (x0, y0, w, h, flags) in enumerate(TENSOR_ROIS):
                one = expected_tensor([expected_ints_sited(planes[k], bd, samples, capi.MATRIX_BT2020, 0, out_size, loc, (x0, y0, w, h))], layout, dtype, scale, bias)[0]
                want.append(reverse_columns(one, layout) if flags & capi.ROI_MIRROR else one)
            got = ctx.tensor_export_finish(ctx.frames_export_tensor_rois(frames, TENSOR_ROIS, layout, dtype, samples, capi.MATRIX_BT2020, 0, out_size, scale, bias,
                                                                         chroma_loc=loc))
            assert_tensor(got, np.stack(want), "rois, type %d layout %d dtype %d" % (loc, layout, dtype))
    finally:
        for f in frames:
            ctx.frame_destroy(f)


def check_lane_boundaries(ctx, size, bd, loc):
    """an uploaded frame just wider than one wavefront's chunk of k_export_rgb (64 lanes x 16 bytes of luma): the CENTRE form's left neighbour crosses
    a lane, a wave and a vector boundary; whole, and a rectangle that starts at x0 = 6"""
    frame, planes = random_frame(ctx, bd, 9800 + bd, size)
    try:
        check_rgb_sited(ctx, frame, planes, bd, loc, (None, (6, 2, size[0] - 6, size[1] - 4)), "%dx%d" % size, layouts=(capi.RGB_PACKED,),
                        samples_set=(capi.RGB_U8 if bd == 8 else capi.RGB_U16,))
    finally:
        ctx.frame_destroy(frame)


def check_gate_rgb_sited(ctx, loc=2, layout=capi.RGB_PACKED, samples=capi.RGB_U8, matrix=capi.MATRIX_BT709, full=0):
    """export_rgb_util.check_gate_rgb's scenario through m355_frame_export_rgb_opts: behind a decode whose lists the device rejected the export
    writes nothing, behind an accepted decode of the same lists it does"""
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
        tokens.append(ctx.frame_export_rgb(dst, layout, samples, matrix, full, chroma_loc=loc))
    good, bad = [ctx.frame_export_finish(t, raw=True) for t in tokens]
    assert ctx.decode_status(serials[0]) == 0 and ctx.decode_status(serials[1]) == M355_ERR_INVALID
    with_planes = ctx.frame_download(dst)
    assert_export(good[0], good[1], expected_rgb_sited(with_planes, 8, 8, layout, samples, matrix, full, loc), "behind the accepted decode")
    for raw in bad[1]:
        assert np.all(raw == capi.DEVICE_FILL), "an RGB export behind a rejected decode wrote to its destination"
    ctx.wait()
    for f in handles + [dst]:
        ctx.frame_destroy(f)


def check_hazard_rgb_sited(ctx, depth, loc=2, layout=capi.RGB_PACKED, samples=capi.RGB_U8, matrix=capi.MATRIX_BT709, full=0):
    """export_rgb_util.check_hazard_rgb's scenario through m355_frame_export_rgb_opts: four pictures decoded alternately into a pool of two frames,
    each exported right behind its decode, no host wait in between; every export delivers what the export of the same picture decoded alone does"""
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
        handles, tokens = [], []
        for j, pic in enumerate(pics):
            pic.ref_frames = [r0] + [-1] * (worklist.MAX_REF_FRAMES - 1)
            pic.dst_frame = pool[j % 2]
            handles.append(ctx.upload(pic))
            ctx.decode_resident(handles[-1])
            tokens.append(ctx.frame_export_rgb(pool[j % 2], layout, samples, matrix, full, rect, chroma_loc=loc))
        got = [ctx.frame_export_finish(t, raw=True) for t in tokens]
        ctx.wait()
        for j in range(4):
            ctx.decode_resident(handles[j])
            ctx.wait()
            planes = ctx.frame_download(pool[j % 2])
            alone = ctx.frame_export_finish(ctx.frame_export_rgb(pool[j % 2], layout, samples, matrix, full, rect, chroma_loc=loc))
            assert_planes_equal(alone, expected_rgb_sited(planes, 10, 10, layout, samples, matrix, full, loc, rect), "picture %d alone" % j)
            assert_export(got[j][0], got[j][1], alone, "picture %d, depth %d" % (j, depth))
        for j in (0, 1):
            assert not np.array_equal(got[j][0][0], got[j + 2][0][0]), "the pictures that share a frame must differ for this test to see a hazard"
        for h in handles:
            ctx.release(h)
        for f in pool + [r0]:
            ctx.frame_destroy(f)
    finally:
        ctx.set_pipeline_depth(1)
