"""Shared by the colour transform tests (SIMT-interpreter build, GPU and glue): the contract of COLOUR TRANSFORM in include/de265_mi355x.h restated in
Python integers / numpy int64 — the pixel function, the preset builder in doubles, and the composed exports with a colour transform as the composed
exports of export_siting_util.py (imported, not copied) with samples = U16, sent through the pixel function.  Three table sets: RANDOM (a), EXTREME (b)
and the preset PQ / BT.2020 -> gamma 2.4 / BT.709, Reinhard, 203 / 1000 nits (c).  Every comparison of pixels is exact, destination padding included."""
import math

import numpy as np

from export_rgb_util import M355_ERR_INVALID, coefficients, matrix_rgb, shape_rgb  # noqa: F401
from export_siting_util import (CUBIC, TRIANGLE, TENSOR_ROIS, WIDE_CASE, assert_same_bytes, expected_ints_sited, finish)
from export_tensor_util import assert_tensor, expected_tensor
from export_tensor_rois_util import reverse_columns
from export_util import assert_export
from synth_util import assert_planes_equal, make_case
from libde265_amd import capi, worklist

ONE, IN_KNOTS, OUT_KNOTS = capi.COLOUR_ONE, capi.COLOUR_IN_KNOTS, capi.COLOUR_OUT_KNOTS
U8, U16 = capi.RGB_U8, capi.RGB_U16
MATRIX, FULL = capi.MATRIX_BT2020, 0          # the YCbCr conversion of every kernel case


# ---- the pixel function ------------------------------------------------------------------------------------------------------------------------------

def out_index(P):
    """step 3's index: P (int64 array, 0..ONE) -> (idx, fr)"""
    P = np.asarray(P, np.int64)
    e = np.floor(np.log2(np.maximum(P, 1).astype(np.float64))).astype(np.int64)      # exact: P < 2^53
    e = np.where((np.int64(1) << e) > P, e - 1, e)
    e = np.where((np.int64(2) << e) <= P, e + 1, e)
    big = P >= 64
    es = np.where(big, e, 24)
    n = P << (24 - es)
    return np.where(big, 64 * (es - 5) + ((n >> 18) & 63), P), np.where(big, (n >> 10) & 255, 0)


def exponent(P):
    """floor(log2 P) for P >= 64, else -1"""
    idx, _ = out_index(P)
    return np.where(np.asarray(P) >= 64, (idx >> 6) + 5, -1)


def knot(i):
    return i if i < 64 else (64 + i % 64) << (i // 64 - 1)


def linear_and_sums(T, rgb16):
    """steps 1 and 2 before the clip -> (L per channel, the shifted sums per output channel)"""
    lin = T["lut_in"].astype(np.int64)
    L = []
    for v in rgb16:
        v = np.asarray(v, np.int64)
        k, f = v >> 6, v & 63
        L.append((lin[k] * (64 - f) + lin[k + 1] * f + 32) >> 6)
    m = [int(x) for x in T["matrix"]]
    return L, [(m[3 * c] * L[0] + m[3 * c + 1] * L[1] + m[3 * c + 2] * L[2] + (1 << 13)) >> 14 for c in range(3)]


def colour_pixels(T, rgb16, samples):
    """m355_colour_pixel over arrays: rgb16 = three int64 arrays of 0..65535 -> three int64 arrays"""
    lo = T["lut_out"].astype(np.int64)
    out = []
    for s in linear_and_sums(T, rgb16)[1]:
        P = np.clip(s, 0, ONE)
        idx, fr = out_index(P)
        o = (lo[idx] * (256 - fr) + lo[np.minimum(idx + 1, OUT_KNOTS - 1)] * fr + 128) >> 8
        out.append(o if samples == U16 else (2 * o + 257) // 514)
    return out


def to_ctypes(T, pad=0):
    return capi.colour_tables(T["lut_in"], T["matrix"], T["lut_out"], pad)


def from_ctypes(t):
    return dict(lut_in=np.array(t.lut_in[:], np.int64), matrix=np.array(t.matrix[:], np.int64), lut_out=np.array(t.lut_out[:], np.int64))


# ---- the presets in doubles ----------------------------------------------------------------------------------------------------------------------------

XY = {1: (0.640, 0.330, 0.300, 0.600, 0.150, 0.060), 5: (0.640, 0.330, 0.290, 0.600, 0.150, 0.060), 6: (0.630, 0.340, 0.310, 0.595, 0.155, 0.070),
      9: (0.708, 0.292, 0.170, 0.797, 0.131, 0.046)}


def _transfer(t):
    return 1 if t in (2, 6, 14, 15) else t


def eotf(t, e, white):
    if t == 1:
        return white * e ** 2.4
    if t == 13:
        return white * (e / 12.92 if e <= 0.04045 else ((e + 0.055) / 1.055) ** 2.4)
    if t == 8:
        return white * e
    if t == 16:
        m1, m2, c1, c2, c3 = 2610 / 16384, 2523 / 4096 * 128, 3424 / 4096, 2413 / 4096 * 32, 2392 / 4096 * 32
        p = e ** (1 / m2)
        return 10000.0 * (max(p - c1, 0.0) / (c2 - c3 * p)) ** (1 / m1)
    a = 0.17883277
    b, c = 1 - 4 * a, 0.5 - a * math.log(4 * a)
    s = e * e / 3 if e <= 0.5 else (math.exp((e - c) / a) + b) / 12
    return 1000.0 * s ** 1.2


def oetf(t, y):
    if t == 1:
        return y ** (1 / 2.4)
    if t == 13:
        return 12.92 * y if y <= 0.0031308 else 1.055 * y ** (1 / 2.4) - 0.055
    return y


def rgb_to_xyz(p):
    q = XY[p]
    xw, yw = 0.3127, 0.3290
    m = np.array([[q[2 * i] / q[2 * i + 1] for i in range(3)], [1.0] * 3, [(1 - q[2 * i] - q[2 * i + 1]) / q[2 * i + 1] for i in range(3)]])
    s = np.linalg.solve(m, np.array([xw / yw, 1.0, (1 - xw - yw) / yw]))
    return m * s[None, :]


def preset_tables(in_transfer, in_primaries, out_transfer, out_primaries, tone, white_nits=0, peak_nits=0):
    """m355_colour_preset in Python doubles -> the table set"""
    it, ot = _transfer(in_transfer), _transfer(out_transfer)
    ip, op = (1 if in_primaries == 2 else in_primaries), (1 if out_primaries == 2 else out_primaries)
    white = float(white_nits) if white_nits else 203.0
    S = eotf(it, 1.0, white)
    lut_in = [min(ONE, int(math.floor(eotf(it, min(64 * k, 65535) / 65535, white) / S * ONE + 0.5))) for k in range(IN_KNOTS)]
    if ip == op:
        matrix = [16384, 0, 0, 0, 16384, 0, 0, 0, 16384]
    else:
        M = np.linalg.solve(rgb_to_xyz(op), rgb_to_xyz(ip))
        matrix = []
        for r in range(3):
            row = [int(math.floor(M[r][c] * 16384 + 0.5)) for c in range(3)]
            big = max(range(3), key=lambda c: (abs(row[c]), -c))
            row[big] += 16384 - sum(row)
            matrix += row
    peak = float(peak_nits) if peak_nits else S
    w = max(1.0, peak / white)
    lut_out = []
    for i in range(OUT_KNOTS):
        x = knot(i) / ONE * S / white
        y = min(1.0, x * (1 + x / (w * w)) / (1 + x) if tone == capi.TONE_REINHARD else x)
        lut_out.append(int(math.floor(oetf(ot, y) * 65535 + 0.5)))
    return dict(lut_in=np.array(lut_in, np.int64), matrix=np.array(matrix, np.int64), lut_out=np.array(lut_out, np.int64))


# ---- the three table sets --------------------------------------------------------------------------------------------------------------------------------

def random_tables(seed=20240):
    rng = np.random.default_rng(seed)
    return dict(lut_in=rng.integers(0, ONE + 1, IN_KNOTS), matrix=rng.integers(-65535, 65536, 9), lut_out=rng.integers(0, 65536, OUT_KNOTS))


RANDOM = random_tables()
EXTREME = dict(lut_in=np.full(IN_KNOTS, ONE, np.int64), matrix=np.array([65535] * 3 + [-65535] * 3 + [16384, 0, 0], np.int64),
               lut_out=np.random.default_rng(20241).integers(0, 65536, OUT_KNOTS))
PRESET_ARGS = (16, 9, 1, 1, capi.TONE_REINHARD, 203, 1000)
PRESET = preset_tables(*PRESET_ARGS)
TABLE_SETS = {"random": RANDOM, "extreme": EXTREME, "preset": PRESET}


# ---- the picture inputs ---------------------------------------------------------------------------------------------------------------------------------

CONDITIONS = ["P<64", "P=ONE", "fr!=0", "clip low", "clip high"] + ["e=%d" % e for e in range(6, 25)]


def conditions_reached(T, rgb16):
    """the names of CONDITIONS that the pixels rgb16 reach under the tables T"""
    got = set()
    for s in linear_and_sums(T, rgb16)[1]:
        P = np.clip(s, 0, ONE)
        _, fr = out_index(P)
        if np.any(P < 64): got.add("P<64")
        if np.any(P == ONE): got.add("P=ONE")
        if np.any(fr != 0): got.add("fr!=0")
        if np.any(s < 0): got.add("clip low")
        if np.any(s > ONE): got.add("clip high")
        got.update("e=%d" % e for e in np.unique(exponent(P)) if e >= 6)
    return got


_frames = {}


def census_planes(bd, size=(64, 32)):
    """the 4:2:0 source of the kernel cases: seeded random samples over the whole range, and in the right half flat patches of 8 x 4 luma samples
    (Y, Cb, Cr constant: their inner pixels pass the chroma filter and an identity resize unchanged) whose colours were searched, among seeded
    random ones, for those that bring table set (a) to every exponent of the output table — random samples alone reach the small ones too rarely"""
    if (bd, size) in _frames:
        return _frames[(bd, size)]
    w, h = size
    rng = np.random.default_rng(9900 + bd)
    dt = np.uint8 if bd == 8 else np.uint16
    planes = [rng.integers(0, 1 << bd, (h, w)).astype(dt)] + [rng.integers(0, 1 << bd, (h // 2, w // 2)).astype(dt) for _ in range(2)]
    k = coefficients(MATRIX, FULL, bd, bd, U16)
    yuv = rng.integers(0, 1 << bd, (3, 1 << 22))
    rgb = matrix_rgb(yuv[0], yuv[1], yuv[2], k)
    sums = linear_and_sums(RANDOM, rgb)[1]
    es = [np.where(s < 0, -1, exponent(np.clip(s, 0, ONE))) for s in sums]       # (e = 24 is P = ONE, mostly through the clip)
    picks = []
    for e in range(6, 25):
        hit = (es[0] == e) | (es[1] == e) | (es[2] == e)
        assert hit.any(), "no colour among the candidates brings table set (a) to exponent %d" % e
        picks.append(int(np.argmax(hit)))
    slots = [(x, y) for y in range(0, h, 4) for x in range(w // 2, w, 8)]
    assert len(slots) >= len(picks)
    for (x, y), p in zip(slots, picks):
        planes[0][y:y + 4, x:x + 8] = yuv[0][p]
        planes[1][y // 2:y // 2 + 2, x // 2:x // 2 + 4] = yuv[1][p]
        planes[2][y // 2:y // 2 + 2, x // 2:x // 2 + 4] = yuv[2][p]
    _frames[(bd, size)] = planes
    return planes


def upload(ctx, planes, bd):
    frame = ctx.frame_create(planes[0].shape[1], planes[0].shape[0], 1, bd, bd)
    ctx.frame_upload(frame, planes)
    return frame


def random_planes(bd, seed, size=(64, 32)):
    w, h = size
    rng = np.random.default_rng(seed)
    dt = np.uint8 if bd == 8 else np.uint16
    return [rng.integers(0, 1 << bd, (h, w)).astype(dt)] + [rng.integers(0, 1 << bd, (h // 2, w // 2)).astype(dt) for _ in range(2)]


# ---- the composed exports with a colour transform ---------------------------------------------------------------------------------------------------------

_ints = {}


def ints16(planes, bd, out_size, loc, rect, filt, key=None):
    """the U16 integers of the composed export without a colour transform (export_siting_util) -> [R, G, B] int64; key: cache them under it"""
    if key is not None and (key, bd, out_size, loc, rect, filt) in _ints:
        return _ints[(key, bd, out_size, loc, rect, filt)]
    v = [c.astype(np.int64) for c in expected_ints_sited(planes, bd, U16, MATRIX, FULL, out_size, loc, rect, filt)]
    if key is not None:
        _ints[(key, bd, out_size, loc, rect, filt)] = v
    return v


def expected_colour_ints(T, planes, bd, samples, out_size, loc=0, rect=None, filt=TRIANGLE, key=None):
    return colour_pixels(T, ints16(planes, bd, out_size, loc, rect, filt, key), samples)


def expected_colour_rgb(T, planes, bd, layout, samples, out_size, loc=0, rect=None, filt=TRIANGLE, key=None):
    return shape_rgb(expected_colour_ints(T, planes, bd, samples, out_size, loc, rect, filt, key), layout, samples)


# source 64x32: (rectangle, output size, filters); None as the size: out == rectangle
KERNEL_CASES = [(None, (48, 24), (TRIANGLE, CUBIC)), (None, (128, 64), (TRIANGLE,)), ((2, 2, 44, 26), (30, 18), (TRIANGLE,)), (None, (64, 32), (TRIANGLE,)),
                ((2, 2, 44, 26), (44, 26), (TRIANGLE,))]
KERNEL_LOCS = (0, 2)


def kernel_case_inputs(bd):
    """every (planes, out_size, loc, rect, filter) the kernel cases of one bit depth put through the stage, for the census"""
    planes = census_planes(bd)
    return [(planes, out_size, loc, rect, filt) for rect, out_size, filters in KERNEL_CASES for filt in filters for loc in KERNEL_LOCS]


def check_census():
    """from the restatement alone: the picture inputs of the kernel cases reach every condition with table set (a), and with (b) those it can reach"""
    got_a, got_b = set(), set()
    for bd in (8, 10):
        for planes, out_size, loc, rect, filt in kernel_case_inputs(bd):
            rgb = ints16(planes, bd, out_size, loc, rect, filt, "census")
            got_a |= conditions_reached(RANDOM, rgb)
        got_b |= conditions_reached(EXTREME, ints16(census_planes(bd), bd, (48, 24), 0, None, TRIANGLE, "census"))
    assert got_a == set(CONDITIONS), "table set (a) misses %s" % sorted(set(CONDITIONS) - got_a)
    assert {"P<64", "P=ONE", "clip low", "clip high", "e=24"} <= got_b, "table set (b) reaches only %s" % sorted(got_b)


def check_kernel_cases(ctx, bd, T, name):
    """the 64x32 cases of one bit depth under one table set: packed and planar, U8 and U16, chroma_loc 0 and 2"""
    planes = census_planes(bd)
    frame, handle = upload(ctx, planes, bd), ctx.colour_create(to_ctypes(T))
    try:
        for rect, out_size, filters in KERNEL_CASES:
            for filt in filters:
                for loc in KERNEL_LOCS:
                    for layout in (capi.RGB_PACKED, capi.RGB_PLANAR):
                        for samples in (U8, U16):
                            what = "%s %d bit rect %s to %dx%d filter %d type %d layout %d samples %d" % (name, bd, rect, out_size[0], out_size[1], filt, loc, layout, samples)
                            want = expected_colour_rgb(T, planes, bd, layout, samples, out_size, loc, rect, filt, "census")
                            got, raws = finish(ctx, ctx.frame_export_resized_rgb(frame, layout, samples, MATRIX, FULL, out_size, rect, filter=filt, chroma_loc=loc, colour=handle))
                            assert_export(got, raws, want, what)
    finally:
        ctx.frame_destroy(frame)
        ctx.colour_destroy(handle)


def check_differs_from_plain(T=RANDOM, bd=10):
    """the expectations themselves: with a colour transform they are not the plain call's (an implementation that ignores the handle cannot pass)"""
    planes = census_planes(bd)
    for samples in (U8, U16):
        plain = expected_ints_sited(planes, bd, samples, MATRIX, FULL, (48, 24), 0)
        assert any(not np.array_equal(a, b) for a, b in zip(plain, expected_colour_ints(T, planes, bd, samples, (48, 24), key="census")))


def check_wide(ctx, T, name, bd=10):
    size, out_size = WIDE_CASE
    planes = random_planes(bd, 9910, size)
    frame, handle = upload(ctx, planes, bd), ctx.colour_create(to_ctypes(T))
    try:
        got, raws = finish(ctx, ctx.frame_export_resized_rgb(frame, capi.RGB_PACKED, U8, MATRIX, FULL, out_size, chroma_loc=2, colour=handle))
        assert_export(got, raws, expected_colour_rgb(T, planes, bd, capi.RGB_PACKED, U8, out_size, 2, key="wide"), "wide, " + name)
    finally:
        ctx.frame_destroy(frame)
        ctx.colour_destroy(handle)


TENSOR_FORMATS = ((capi.TENSOR_NCHW, capi.TENSOR_F32, U16), (capi.TENSOR_NHWC, capi.TENSOR_F16, U8), (capi.TENSOR_NCHW, capi.TENSOR_BF16, U16))
SCALE, BIAS = [1.0 / 255, 0.5 / 255, 2.0 / 255], [0.0, -1.0, 0.25]


def check_tensors(ctx, T, name, bd=10, out_size=(48, 24), loc=2):
    """3 frames as one tensor, and 3 regions (one mirrored) as one tensor"""
    planes = [random_planes(bd, 9920 + k) for k in range(3)]
    frames, handle = [upload(ctx, p, bd) for p in planes], ctx.colour_create(to_ctypes(T))
    try:
        for layout, dtype, samples in TENSOR_FORMATS:
            what = "%s layout %d dtype %d samples %d" % (name, layout, dtype, samples)
            ints = [expected_colour_ints(T, p, bd, samples, out_size, loc, key="tensor%d" % k) for k, p in enumerate(planes)]
            got = ctx.tensor_export_finish(ctx.frames_export_tensor(frames, layout, dtype, samples, MATRIX, FULL, out_size, SCALE, BIAS, chroma_loc=loc, colour=handle))
            assert_tensor(got, expected_tensor(ints, layout, dtype, SCALE, BIAS), "tensor, " + what)
            want = []
            for k, (x0, y0, w, h, flags) in enumerate(TENSOR_ROIS):
                one = expected_tensor([expected_colour_ints(T, planes[0], bd, samples, out_size, loc, (x0, y0, w, h), key="roi")], layout, dtype, SCALE, BIAS)[0]
                want.append(reverse_columns(one, layout) if flags & capi.ROI_MIRROR else one)
            got = ctx.tensor_export_finish(ctx.frames_export_tensor_rois([frames[0]] * 3, TENSOR_ROIS, layout, dtype, samples, MATRIX, FULL, out_size, SCALE, BIAS,
                                                                         chroma_loc=loc, colour=handle))
            assert_tensor(got, np.stack(want), "rois, " + what)
    finally:
        for f in frames:
            ctx.frame_destroy(f)
        ctx.colour_destroy(handle)


def check_extreme(ctx, bd=10):
    planes = census_planes(bd)
    frame, handle = upload(ctx, planes, bd), ctx.colour_create(to_ctypes(EXTREME))
    try:
        got, raws = finish(ctx, ctx.frame_export_resized_rgb(frame, capi.RGB_PLANAR, U16, MATRIX, FULL, (48, 24), colour=handle))
        assert_export(got, raws, expected_colour_rgb(EXTREME, planes, bd, capi.RGB_PLANAR, U16, (48, 24), key="census"), "extreme")
    finally:
        ctx.frame_destroy(frame)
        ctx.colour_destroy(handle)


def check_grey(ctx, bd=10):
    """a constant neutral-grey frame under the preset: R = G = B, constant"""
    planes = [np.full((32, 64), 400, np.uint16), np.full((16, 32), 512, np.uint16), np.full((16, 32), 512, np.uint16)]
    frame, handle = upload(ctx, planes, bd), ctx.colour_create(to_ctypes(PRESET))
    try:
        for samples in (U8, U16):
            got = ctx.frame_export_finish(ctx.frame_export_resized_rgb(frame, capi.RGB_PLANAR, samples, MATRIX, FULL, (48, 24), colour=handle))
            assert len(np.unique(got[0])) == 1 and np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2])
            assert_planes_equal(got, expected_colour_rgb(PRESET, planes, bd, capi.RGB_PLANAR, samples, (48, 24)), "grey")
    finally:
        ctx.frame_destroy(frame)
        ctx.colour_destroy(handle)


def check_destroy_after_export(ctx, bd=10):
    """m355_colour_destroy directly behind an export: it waits for the context's work, the export's bytes are exact"""
    planes = census_planes(bd)
    frame, handle = upload(ctx, planes, bd), ctx.colour_create(to_ctypes(RANDOM))
    try:
        token = ctx.frame_export_resized_rgb(frame, capi.RGB_PACKED, U16, MATRIX, FULL, (128, 64), colour=handle)
        ctx.colour_destroy(handle)
        got, raws = finish(ctx, token)
        assert_export(got, raws, expected_colour_rgb(RANDOM, planes, bd, capi.RGB_PACKED, U16, (128, 64), key="census"), "destroy behind the export")
    finally:
        ctx.frame_destroy(frame)


def check_gate_colour(ctx, T=RANDOM, layout=capi.RGB_PACKED, samples=U8, out_size=(96, 48)):
    """export_siting_util.check_gate_rgb_sited's scenario through the composed export with a colour transform: behind a decode whose lists the
    device rejected the export writes nothing, behind an accepted decode of the same lists it does"""
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
    colour = ctx.colour_create(to_ctypes(T))
    tokens, serials = [], []
    for corrupt in (False, True):
        p = make_case(**cfg)[0]
        p.ref_frames = [handles[i] if i < len(handles) else -1 for i in range(worklist.MAX_REF_FRAMES)]
        p.dst_frame = dst
        if corrupt:
            arr = p.ibs.copy(); arr["mode"][len(arr) // 2] = 77; p.ibs = arr
        ctx.submit_in_place(p, fill_threads=1)
        serials.append(ctx.last_serial())
        tokens.append(ctx.frame_export_resized_rgb(dst, layout, samples, MATRIX, FULL, out_size, chroma_loc=2, colour=colour))
    good, bad = [ctx.frame_export_finish(t, raw=True) for t in tokens]
    assert ctx.decode_status(serials[0]) == 0 and ctx.decode_status(serials[1]) == M355_ERR_INVALID
    with_planes = ctx.frame_download(dst)
    assert_export(good[0], good[1], expected_colour_rgb(T, with_planes, 8, layout, samples, out_size, 2), "behind the accepted decode")
    for raw in bad[1]:
        assert np.all(raw == capi.DEVICE_FILL), "a colour export behind a rejected decode wrote to its destination"
    ctx.wait()
    ctx.colour_destroy(colour)
    for f in handles + [dst]:
        ctx.frame_destroy(f)


def check_hazard_colour(ctx, depth, T=RANDOM, layout=capi.RGB_PACKED, samples=U8, out_size=(96, 48)):
    """export_siting_util.check_hazard_rgb_sited's scenario: four pictures decoded alternately into a pool of two frames, each exported with a colour
    transform right behind its decode, no host wait in between; every export delivers what the export of the same picture decoded alone does"""
    from libde265_amd import synth
    ctx.set_pipeline_depth(depth)
    try:
        cfg = dict(width=128, height=64, bit_depth=10, seed=5, n_refs=1)
        pics = [synth.picture(**dict(cfg, seed=5 + j)) for j in range(4)]
        pp = pics[0].pp[0]
        r0 = ctx.frame_create_for(pp)
        ctx.frame_upload(r0, synth.ref_planes(5, 128, 64, 1, 10))
        pool = [ctx.frame_create_for(pp) for _ in range(2)]
        colour = ctx.colour_create(to_ctypes(T))
        rect = (2, 2, 122, 58)
        handles, tokens = [], []
        for j, pic in enumerate(pics):
            pic.ref_frames = [r0] + [-1] * (worklist.MAX_REF_FRAMES - 1)
            pic.dst_frame = pool[j % 2]
            handles.append(ctx.upload(pic))
            ctx.decode_resident(handles[-1])
            tokens.append(ctx.frame_export_resized_rgb(pool[j % 2], layout, samples, MATRIX, FULL, out_size, rect, chroma_loc=2, colour=colour))
        got = [ctx.frame_export_finish(t, raw=True) for t in tokens]
        ctx.wait()
        for j in range(4):
            ctx.decode_resident(handles[j])
            ctx.wait()
            planes = ctx.frame_download(pool[j % 2])
            alone = ctx.frame_export_finish(ctx.frame_export_resized_rgb(pool[j % 2], layout, samples, MATRIX, FULL, out_size, rect, chroma_loc=2, colour=colour))
            assert_planes_equal(alone, expected_colour_rgb(T, planes, 10, layout, samples, out_size, 2, rect), "picture %d alone" % j)
            assert_export(got[j][0], got[j][1], alone, "picture %d, depth %d" % (j, depth))
        for j in (0, 1):
            assert not np.array_equal(got[j][0][0], got[j + 2][0][0]), "the pictures that share a frame must differ for this test to see a hazard"
        for h in handles:
            ctx.release(h)
        ctx.colour_destroy(colour)
        for f in pool + [r0]:
            ctx.frame_destroy(f)
    finally:
        ctx.set_pipeline_depth(1)


def check_handle_zero_is_plain(ctx, bd=10):
    """handle 0 through the _opts entry points is the plain call, byte for byte"""
    planes = census_planes(bd)
    frame = upload(ctx, planes, bd)
    try:
        rr = (frame, capi.RGB_PLANAR, U16, MATRIX, FULL, (48, 24), (2, 2, 44, 26))
        assert_same_bytes(finish(ctx, ctx.frame_export_resized_rgb(*rr, opts_entry=True, colour=0)), finish(ctx, ctx.frame_export_resized_rgb(*rr)), "resized rgb")
        te = ([frame, frame], capi.TENSOR_NHWC, capi.TENSOR_F16, U8, MATRIX, FULL, (32, 16), SCALE, BIAS)
        assert np.array_equal(ctx.tensor_export_finish(ctx.frames_export_tensor(*te, opts_entry=True, colour=0))[1], ctx.tensor_export_finish(ctx.frames_export_tensor(*te))[1])
        tr = ([frame] * 3, TENSOR_ROIS, capi.TENSOR_NCHW, capi.TENSOR_F32, U16, MATRIX, FULL, (32, 16), SCALE, BIAS)
        assert np.array_equal(ctx.tensor_export_finish(ctx.frames_export_tensor_rois(*tr, opts_entry=True, colour=0))[1],
                              ctx.tensor_export_finish(ctx.frames_export_tensor_rois(*tr))[1])
    finally:
        ctx.frame_destroy(frame)
