"""Scenarios of the MS-SSIM-request tests (m355_frame_msssim_async / m355_frame_msssim_result), shared by the CPU tier (SIMT-interpreter build,
tests/test_msssim_emu.py) and the GPU tier (tests/test_gpu_msssim.py), and the numpy restatement of the definition (include/de265_mi355x.h) their
expected values come from: level j = the f x f box sums of the ORIGINAL samples with one rounding, per level the window sums and the point q of
tests/ssim_util.py plus the contrast-structure point qc.  Every integer comparison is exact; msssim is compared exactly where it is 0.0 or 1.0 and
to 2^-49 relative (8 ulp: five pow results of at most 1 ulp each and four multiplications) elsewhere."""
import ctypes
import math

import numpy as np
import pytest

import ssim_util as su
from hash_util import CRC, make_planes
from measure_util import BUSY, INVALID, PIC_A, PIC_B, PIC_C, PIC_D, REJECT_CASE, _upload_refs, crop, frame_with
from oracle_py import Oracle
from synth_util import assert_planes_equal, make_case, oracle_decode
from libde265_amd import capi

SLOTS = 4                           # M355_MSSSIM_REQUESTS
LEVELS = 5                          # M355_MSSSIM_LEVELS
ONE = su.ONE
TW, TH = su.TW, su.TH               # the tile of k_ssim.h, which k_msssim.hip takes over
WANG = [0.0448, 0.2856, 0.3001, 0.2363, 0.1333]
# (levels, plane size): one window at the last level; odd sizes (the trailing column / row dropped); windows fill two tiles exactly while the samples
# need a third that has no window; a tile's rim over and short; level 1 one column over a tile
SIZES_2 = [(22, 22), (23, 25), (2 * TW + 10, TH + 10), (2 * TW + 11, 2 * TH + 9), (4 * TW + 21, 2 * TH + 22)]
SIZES_3 = [(44, 47), (4 * TW + 43, 91)]
SIZES_5 = [(176, 176), (191, 192)]  # one window at level 4; 11 x 12 samples there, 15 columns dropped there and none at level 0
SIZE_5_WIDE = (16 * (TW + 11) + 3, 180)   # more than one tile at level 4
PLANE_SIZES = [(2, s) for s in SIZES_2] + [(3, s) for s in SIZES_3] + [(5, s) for s in SIZES_5]


# ---- the definition, restated ----
def level(plane, j):
    """level j of a plane: (S + f f / 2) >> 2j of the f x f blocks of the plane itself, (ph >> j) x (pw >> j)"""
    if j == 0:
        return plane
    f = 1 << j
    lh, lw = plane.shape[0] >> j, plane.shape[1] >> j
    s = plane[:lh * f, :lw * f].astype(np.int64).reshape(lh, f, lw, f).sum(axis=(1, 3))
    return ((s + f * f // 2) >> (2 * j)).astype(plane.dtype)


def point_cs(sums, bd):
    """the five sums (uint64 arrays) -> qc, int64 array: the operations of m355_ssim_point_cs, one rounding each"""
    _, c2 = su.constants(bd)
    MA, MB, SAA, SBB, SAB = [np.asarray(s, np.uint64) for s in sums]
    k28 = np.float64(2.0 ** 28)
    fa, fb = MA.astype(np.float64), MB.astype(np.float64)
    ab, aa, bb = fa * fb, fa * fa, fb * fb
    cov, va, vb = k28 * SAB.astype(np.float64) - ab, k28 * SAA.astype(np.float64) - aa, k28 * SBB.astype(np.float64) - bb
    cs = (2.0 * cov + c2) / ((va + vb) + c2)
    return np.clip(np.floor(cs * 2.0 ** 30 + 0.5), -2.0 ** 30, 2.0 ** 30).astype(np.int64)


def means(r, levels):
    return [float(r["sum_cs"][j] if j < levels - 1 else r["sum_q"][j]) / (float(r["n"][j]) * 2.0 ** 30) for j in range(levels)]


def combine(m, weights=None):
    v = 1.0
    for x, w in zip(m, WANG if weights is None else weights):
        v *= math.pow(max(x, 0.0), w)
    return v


def msssim_plane(a, b, bd, levels):
    """one plane against another -> the fields of m355_msssim for it"""
    r = dict(sum_q=[0] * LEVELS, sum_cs=[0] * LEVELS, n=[0] * LEVELS, msssim=0.0)
    for j in range(levels):
        sums = su.window_sums(level(a, j), level(b, j))
        r["sum_q"][j], r["sum_cs"][j], r["n"][j] = int(su.point(sums, bd).sum()), int(point_cs(sums, bd).sum()), int(sums[0].size)
    if levels == LEVELS:
        r["msssim"] = combine(means(r, levels))
    return r


def zero():
    return dict(sum_q=[0] * LEVELS, sum_cs=[0] * LEVELS, n=[0] * LEVELS, msssim=0.0)


def expected(frame_planes, ref_rect_planes, rect, geom, planes=0, levels=LEVELS):
    """what a request on a frame holding frame_planes delivers against the RECTANGLE's reference planes -> [3 dicts]"""
    _, _, cf, bdl, bdc = geom
    res = []
    for c in range(3):
        if c >= len(frame_planes) or (planes and not (planes >> c) & 1):
            res.append(zero())
        else:
            res.append(msssim_plane(crop(frame_planes, rect, cf)[c], ref_rect_planes[c], bdc if c else bdl, levels))
    return res


def assert_result(got, want, what=""):
    assert len(got) == 3, what
    for c, (g, w) in enumerate(zip(got, want)):
        for k in ("sum_q", "sum_cs", "n"):
            assert g[k] == w[k], "%s: plane %d: %s is %r, expected %r" % (what, c, k, g[k], w[k])
        if w["msssim"] in (0.0, 1.0):
            assert g["msssim"] == w["msssim"], "%s: plane %d: msssim is %r, expected exactly %r" % (what, c, g["msssim"], w["msssim"])
        else:
            assert abs(g["msssim"] - w["msssim"]) <= 2.0 ** -49 * w["msssim"], "%s: plane %d: msssim is %r, expected %r" % (what, c, g["msssim"], w["msssim"])


def check_pair(ctx, geom, a, b, rect=None, planes=0, levels=LEVELS, against_frame=True, against_memory=True, host=False, what="", want=None):
    """a frame holding planes `a` against whole-frame planes `b`: as memory (the rectangle's part of b) and as a second frame"""
    cf = geom[2]
    if want is None:
        want = expected(a, crop(b, rect, cf), rect, geom, planes, levels)
    fa = frame_with(ctx, geom, a)
    fb = frame_with(ctx, geom, b) if against_frame else None
    try:
        runs = []
        for how in [h for h, on in (("memory", against_memory), ("frame", against_frame)) if on]:
            kw = dict(ref_planes=crop(b, rect, cf), host=host) if how == "memory" else dict(ref_frame=fb)
            runs.append((how, ctx.frame_msssim_async(fa, rect=rect, planes=planes, levels=levels, **kw)))
        for how, tk in runs:
            assert_result(ctx.frame_msssim_result(tk), want, "%s %s rect %s planes %d levels %d against %s" % (what, geom, rect, planes, levels, how))
    finally:
        ctx.frame_destroy(fa)
        if fb is not None:
            ctx.frame_destroy(fb)
    return want


# ---- values ----
def check_plane_size(ctx, levels, pw, ph, bd):
    """a pw x ph rectangle of a monochrome frame whose origin is off every multiple of the tile"""
    w, h = (pw + 3 + 7) & ~7, (ph + 5 + 7) & ~7
    geom = (w, h, 0, bd, bd)
    a = make_planes(w, h, 0, bd, bd, seed=pw + 7 * ph + bd)
    want = check_pair(ctx, geom, a, su.perturbed(a, (bd,), seed=3 * pw + ph), rect=(3, 5, pw, ph), levels=levels, against_frame=False, what="plane size")
    assert want[0]["n"][:levels] == [((pw >> j) - 10) * ((ph >> j) - 10) for j in range(levels)] and want[0]["n"][levels:] == [0] * (LEVELS - levels)
    assert want[1] == zero() and want[2] == zero()


def most_levels(w, h, cf):
    sw, sh = (2 if cf in (1, 2) else 1), (2 if cf == 1 else 1)
    pw, ph = (w // sw, h // sh) if cf else (w, h)
    return max(L for L in range(1, LEVELS + 1) if min(pw, ph) >> (L - 1) >= 11)


def check_format(ctx, cf, bdl, bdc, size=352):
    """a whole size x size frame with as many levels as its chroma planes allow (five at 352), each plane with its own constants"""
    geom = (size, size, cf, bdl, bdc)
    levels = most_levels(size, size, cf)
    a = make_planes(*geom, seed=20 + cf + bdl)
    want = check_pair(ctx, geom, a, su.perturbed(a, (bdl, bdc, bdc), seed=30 + cf + bdc), levels=levels, against_memory=False, what="format")
    assert [w["n"][levels - 1] != 0 for w in want] == [True, cf != 0, cf != 0]
    if levels == LEVELS:
        assert all(0 < w["msssim"] < 1 for w in want if w["n"][0])


def check_extremes(ctx, bd, size=176):
    peak = (1 << bd) - 1
    dt = np.uint8 if bd <= 8 else np.uint16
    geom = (size, size, 0, bd, bd)
    levels = most_levels(size, size, 0)
    full = levels == LEVELS
    hi, lo = [np.full((size, size), peak, dt)], [np.zeros((size, size), dt)]
    mid = [np.full((size, size), peak // 3, dt)]
    want = check_pair(ctx, geom, hi, lo, levels=levels, against_memory=False, what="peak against zero")
    assert want[0]["sum_q"][0] == su.PEAK_AGAINST_ZERO * want[0]["n"][0] and want[0]["sum_cs"][:levels] == [ONE * n for n in want[0]["n"][:levels]]
    want = check_pair(ctx, geom, mid, hi, levels=levels, against_memory=False, what="a constant against another constant")
    assert want[0]["sum_cs"][:levels] == [ONE * n for n in want[0]["n"][:levels]] and 0 < want[0]["sum_q"][levels - 1] < ONE * want[0]["n"][levels - 1]
    noise = make_planes(size, size, 0, bd, bd, seed=bd)
    for a in (noise, hi):
        want = check_pair(ctx, geom, a, [a[0].copy()], levels=levels, against_frame=False, what="identical")
        assert want[0]["sum_q"][:levels] == want[0]["sum_cs"][:levels] == [ONE * n for n in want[0]["n"][:levels]] and (not full or want[0]["msssim"] == 1.0)
    want = check_pair(ctx, geom, noise, [(peak - noise[0].astype(np.int64)).astype(dt)], levels=levels, against_memory=False, what="inversion")
    assert min(want[0]["sum_cs"]) < 0 and want[0]["msssim"] == 0.0


# (chroma format, bit depth, frame size, rectangle, levels); the first one has five levels
RECTANGLES = [(1, 8, (400, 368), (6, 2, 354, 352), 5), (2, 10, (104, 96), (6, 3, 90, 91), 3), (3, 8, (64, 56), (5, 3, 51, 45), 3), (0, 12, (64, 48), (1, 1, 62, 46), 2)]


def check_rectangles(ctx, cases=RECTANGLES):
    """rectangles whose origin is off every multiple of 32 and on the chroma grid: tiles and blocks count from the rectangle, not from the frame"""
    for cf, bd, (w, h), rect, levels in cases:
        geom = (w, h, cf, bd, bd)
        a = make_planes(*geom, seed=40 + cf)
        check_pair(ctx, geom, a, su.perturbed(a, (bd,) * 3, seed=50 + cf), rect=rect, levels=levels, what="rectangle")


def check_pinned_reference(ctx):
    geom = (96, 96, 1, 8, 8)
    a = make_planes(*geom, seed=70)
    check_pair(ctx, geom, a, su.perturbed(a, (8,) * 3, seed=71), levels=3, against_frame=False, host=True, what="reference in m355_host_alloc memory")


def check_plane_selection(ctx):
    for geom, levels in (((96, 96, 1, 8, 8), 3), ((48, 48, 3, 10, 10), 3)):
        a = make_planes(*geom, seed=80)
        b = su.perturbed(a, (geom[3], geom[4], geom[4]), seed=81)
        want = check_pair(ctx, geom, a, b, planes=1, levels=levels + (geom[2] == 1), what="luma only")
        assert want[0]["n"][0] and want[1] == zero() and want[2] == zero()
        want = check_pair(ctx, geom, a, b, planes=6, levels=levels, what="chroma only")
        assert want[0] == zero() and want[1]["n"][levels - 1] and want[2]["n"][levels - 1]
        check_pair(ctx, geom, a, b, planes=4, levels=levels, against_memory=False, what="Cr alone")


# ---- cross-checks against the calls the library had before, on the same build ----
def check_level_0_is_the_ssim_request(ctx):
    for geom, rect in (((96, 80, 1, 8, 8), None), ((64, 48, 2, 10, 9), (6, 3, 50, 41))):
        a = make_planes(*geom, seed=60)
        b = su.perturbed(a, (geom[3], geom[4], geom[4]), seed=61)
        fa, fb = frame_with(ctx, geom, a), frame_with(ctx, geom, b)
        try:
            single = ctx.frame_ssim_result(ctx.frame_ssim_async(fa, ref_frame=fb, rect=rect))
            for levels in (1, 2):
                multi = ctx.frame_msssim_result(ctx.frame_msssim_async(fa, ref_frame=fb, rect=rect, levels=levels))
                for c in range(3):
                    assert (multi[c]["sum_q"][0], multi[c]["n"][0]) == (single[c]["sum_q"], single[c]["n"]), "plane %d, levels %d" % (c, levels)
        finally:
            ctx.frame_destroy(fa)
            ctx.frame_destroy(fb)


def check_levels_are_the_scaled_export(ctx):
    """levels 1..3 of a 4:2:0 frame whose size is a multiple of 16 per axis = the SSIM request on frames that hold what m355_frame_export_scaled
    delivers for the two frames (native samples)"""
    geom = (256, 192, 1, 8, 8)
    a = make_planes(*geom, seed=62)
    b = su.perturbed(a, (8,) * 3, seed=63)
    fa, fb = frame_with(ctx, geom, a), frame_with(ctx, geom, b)
    made = [fa, fb]
    try:
        multi = ctx.frame_msssim_result(ctx.frame_msssim_async(fa, ref_frame=fb, levels=4))
        for j in (1, 2, 3):
            small = []
            for f in (fa, fb):
                planes = ctx.frame_export_finish(ctx.frame_export(f, capi.EXPORT_PLANAR, capi.EXPORT_NATIVE, log2_scale=j))
                small.append(frame_with(ctx, (256 >> j, 192 >> j, 1, 8, 8), planes))
            made += small
            single = ctx.frame_ssim_result(ctx.frame_ssim_async(small[0], ref_frame=small[1]))
            for c in range(3):
                assert (multi[c]["sum_q"][j], multi[c]["n"][j]) == (single[c]["sum_q"], single[c]["n"]), "plane %d, level %d" % (c, j)
    finally:
        for f in made:
            ctx.frame_destroy(f)


# ---- the request as a reader of its frames (the scenarios of ssim_util with these calls) ----
GEOM_420 = (64, 64, 1, 8, 8)


def check_reader_hazard(lib, oracle, depth, as_ref_frame, with_others):
    """decode A into F, request on F (or on G with F as ref_frame), [export F, hash F,] decode B into F — nothing waited for in between:
    the values are A's.  The other side holds picture B, so a request that saw B in F would report identical planes."""
    o = Oracle(oracle)
    (pa, ra), (pb, rb) = make_case(**PIC_A), make_case(**PIC_B)
    want_a, want_b = oracle_decode(o, pa, ra), oracle_decode(o, pb, rb)
    want = expected(want_a, want_b, None, GEOM_420, levels=2)
    assert all(w["sum_q"][j] < ONE * w["n"][j] for w in want for j in range(2)), "the two pictures must differ on both levels"
    ctx = capi.Context(lib, 0)
    try:
        _upload_refs(ctx, pa, ra)
        _upload_refs(ctx, pb, rb)
        F = ctx.frame_create_for(pa.pp[0])
        G = ctx.frame_create_for(pa.pp[0])
        ctx.frame_upload(G, want_b)
        ctx.set_pipeline_depth(depth)
        in_memory = None if as_ref_frame else ctx.measure_reference(want_b)
        ctx.frame_msssim_result(ctx.frame_msssim_async(G, ref_frame=G, levels=2))     # (the slot's scratch exists from here on: no allocation below)
        ctx.wait()
        # ---- no host wait from here ...
        pa.dst_frame = pb.dst_frame = F
        ctx.submit(pa)
        tk = ctx.frame_msssim_async(G, ref_frame=F, levels=2) if as_ref_frame else ctx.frame_msssim_async(F, ref_planes=in_memory, levels=2)
        token = ctx.frame_export(F, capi.EXPORT_PLANAR, capi.EXPORT_NATIVE, host=True) if with_others else None
        htk = ctx.frame_hash_async(F, CRC) if with_others else None
        ctx.submit(pb)
        # ---- ... to here
        assert_result(ctx.frame_msssim_result(tk), want, "depth %d, F as %s" % (depth, "ref_frame" if as_ref_frame else "the frame"))   # (q and qc are symmetric)
        if with_others:
            assert_planes_equal(ctx.frame_export_finish(token), want_a, "export between the request and the next decode")
            hash_a = ctx.frame_hash_result(htk)
        ctx.wait()
        assert_planes_equal(ctx.frame_download(F), want_b, "the later picture")
        if with_others:
            assert hash_a != ctx.frame_hash(F, CRC)
        assert_result(ctx.frame_msssim_result(ctx.frame_msssim_async(F, ref_frame=G, levels=2)), expected(want_b, want_b, None, GEOM_420, levels=2), "the later picture against itself")
    finally:
        ctx.close()


def check_two_writers(lib, oracle, depth=3):
    """the frame and its ref_frame written by decodes on DIFFERENT lanes, nothing waited for (ssim_util.check_two_writers): D into G, D into H, C into
    F, then a request on G and one on H, both with ref_frame = F, then D into F"""
    o = Oracle(oracle)
    (pc, rc_), (pd, rd) = make_case(**PIC_C), make_case(**PIC_D)
    want_c, want_d = oracle_decode(o, pc, rc_), oracle_decode(o, pd, rd)
    want = expected(want_d, want_c, None, (256, 192, 1, 8, 8), levels=4)
    assert all(w["sum_q"][0] < ONE * w["n"][0] for w in want), "the two pictures must differ"
    ctx = capi.Context(lib, 0)
    try:
        _upload_refs(ctx, pc, rc_)
        _upload_refs(ctx, pd, rd)
        F, G, H = [ctx.frame_create_for(pc.pp[0]) for _ in range(3)]
        ctx.set_pipeline_depth(depth)
        warm = [ctx.frame_msssim_async(F, ref_frame=F, levels=4) for _ in range(2)]   # (two slots' scratch: no allocation below)
        for tk in warm:
            ctx.frame_msssim_result(tk)
        ctx.wait()
        # ---- no host wait from here ...
        pd.dst_frame = G
        ctx.submit(pd)
        pd.dst_frame = H
        ctx.submit(pd)
        pc.dst_frame = F
        ctx.submit(pc)
        tk_g = ctx.frame_msssim_async(G, ref_frame=F, levels=4)
        tk_h = ctx.frame_msssim_async(H, ref_frame=F, levels=4)
        pd.dst_frame = F
        ctx.submit(pd)
        # ---- ... to here
        assert_result(ctx.frame_msssim_result(tk_g), want, "G against F, written on another lane (depth %d)" % depth)
        assert_result(ctx.frame_msssim_result(tk_h), want, "H against F, behind the first request's mark (depth %d)" % depth)
        ctx.wait()
        assert_planes_equal(ctx.frame_download(F), want_d, "the later picture")
    finally:
        ctx.close()


# ---- verdicts, slots and tickets ----
def check_rejected_decode(lib, oracle, depth):
    """a request behind a decode whose lists the device rejected — into the frame, or into its ref_frame — has no value and has read nothing; the
    slot it used (record, scratch) serves the next request correctly"""
    pic, refs = make_case(**REJECT_CASE)
    geom = (256, 192, 1, 8, 8)
    want = oracle_decode(Oracle(oracle), pic, refs)
    ctx = capi.Context(lib, 0)
    try:
        _upload_refs(ctx, pic, refs)
        ctx.set_pipeline_depth(depth)
        d = ctx.frame_create_for(pic.pp[0])
        ctx.frame_fill(d, 77, 99)
        other = ctx.frame_create_for(pic.pp[0])
        ctx.frame_fill(other, 77, 99)
        filled = ctx.frame_download(other)
        bad = make_case(**REJECT_CASE)[0]
        bad.ref_frames = pic.ref_frames
        arr = bad.tus.copy()
        arr["log2_size"][len(arr) // 2] = 9
        bad.tus = arr
        w = expected(want, filled, None, geom, levels=4)
        for as_ref_frame in (False, True):
            bad.dst_frame = d
            ctx.submit_in_place(bad, fill_threads=1)
            serial = ctx.last_serial()
            tk = ctx.frame_msssim_async(other, ref_frame=d, levels=4) if as_ref_frame else ctx.frame_msssim_async(d, ref_frame=other, levels=4)
            with pytest.raises(capi.M355Error) as e:
                ctx.frame_msssim_result(tk)
            assert e.value.code == INVALID and "rejected" in str(e.value)
            st = ctx.decode_status(serial)                      # (reported here, so that m355_wait stays quiet)
            while st == BUSY:
                st = ctx.decode_status(serial)
            assert st == INVALID
            with pytest.raises(capi.M355Error):                 # the failed collection freed the ticket
                ctx.frame_msssim_result(tk)
            pic.dst_frame = d
            ctx.submit_in_place(pic, fill_threads=1)
            tk = ctx.frame_msssim_async(other, ref_frame=d, levels=4) if as_ref_frame else ctx.frame_msssim_async(d, ref_frame=other, levels=4)
            assert_result(ctx.frame_msssim_result(tk), w, "in the slot a gated request left (ref_frame: %s)" % as_ref_frame)
        ctx.wait()
    finally:
        ctx.close()


def check_concurrency(lib):
    """four requests on four frames before any is collected, collected in reverse; the fifth is refused; a collected slot is free again"""
    ctx = capi.Context(lib, 0)
    try:
        frames, refs, want, lv = [], [], [], []
        for i in range(SLOTS):
            geom, levels = [((96, 48, 1, 8, 8), 2), ((72, 56, 0, 8, 8), 3), ((56, 48, 2, 10, 10), 2), ((48, 24, 3, 12, 12), 2)][i]
            a = make_planes(*geom, seed=900 + i)
            b = su.perturbed(a, (geom[3], geom[4], geom[4]), seed=950 + i)
            frames.append(frame_with(ctx, geom, a))
            refs.append(frame_with(ctx, geom, b) if i % 2 else ctx.measure_reference(b))
            want.append(expected(a, b, None, geom, levels=levels))
            lv.append(levels)
        tickets = [ctx.frame_msssim_async(f, ref_frame=r, levels=n) if i % 2 else ctx.frame_msssim_async(f, ref_planes=r, levels=n) for i, (f, r, n) in enumerate(zip(frames, refs, lv))]
        assert tickets == list(range(1, SLOTS + 1)), "tickets count 1, 2, ... per context"
        with pytest.raises(capi.M355Error) as e:
            ctx.frame_msssim_async(frames[0], ref_frame=frames[0], levels=1)
        assert e.value.code == BUSY
        assert_result(ctx.frame_msssim_result(tickets[-1]), want[-1], "the last request")
        extra = ctx.frame_msssim_async(frames[3], ref_frame=refs[3], levels=lv[3])       # the refused call took no ticket and enqueued nothing
        assert extra == SLOTS + 1
        assert_result(ctx.frame_msssim_result(extra), want[3], "the slot collected first, reused")
        for i in reversed(range(SLOTS - 1)):
            assert_result(ctx.frame_msssim_result(tickets[i]), want[i], "request %d" % i)
    finally:
        ctx.close()


def check_nonblocking(lib):
    ctx = capi.Context(lib, 0)
    try:
        geom = (88, 56, 1, 8, 8)
        a = make_planes(*geom, seed=5)
        b = su.perturbed(a, (8,) * 3, seed=6)
        fa, fb = frame_with(ctx, geom, a), frame_with(ctx, geom, b)
        want = expected(a, b, None, geom, levels=2)
        for k in range(3):
            tk = ctx.frame_msssim_async(fa, ref_frame=fb, levels=2)
            assert tk == k + 1
            got = ctx.frame_msssim_result(tk, block=False)
            while got is None:                                      # BUSY: nothing was waited for, the request stays
                got = ctx.frame_msssim_result(tk, block=False)
            assert_result(got, want, "non-blocking collection")
            for bad in (tk, tk + 1000, 0):                          # collected / unknown
                with pytest.raises(capi.M355Error) as e:
                    ctx.frame_msssim_result(bad, block=False)
                assert e.value.code == INVALID
        # m355_wait completes a request and does not collect it; a frame may be destroyed with a request pending
        tk = ctx.frame_msssim_async(fa, ref_frame=fb, levels=2)
        ctx.wait()
        tk2 = ctx.frame_msssim_async(fb, ref_frame=fa, levels=2)
        ctx.frame_destroy(fa)
        assert_result(ctx.frame_msssim_result(tk, block=False), want, "collected behind m355_wait")
        assert_result(ctx.frame_msssim_result(tk2), want, "collected behind the frame's destruction")
    finally:
        ctx.close()


def check_slot_reuse(ctx, rounds=40):
    """one slot, request after request, sizes and level counts alternating large, small, large: the small request's levels lie where the large one's
    lay, and every frame holds other noise, so a level sample or an accumulator the predecessor left would change a sum"""
    cases = []
    for k, (geom, levels) in enumerate((((112, 96, 0, 8, 8), 4), ((48, 56, 0, 8, 8), 3), ((96, 112, 3, 8, 8), 4), ((64, 48, 2, 10, 9), 2))):
        a = make_planes(*geom, seed=77 + k)
        b = su.perturbed(a, (geom[3], geom[4], geom[4]), seed=87 + k)
        cases.append((frame_with(ctx, geom, a), frame_with(ctx, geom, b), levels, expected(a, b, None, geom, levels=levels)))
    try:
        for k in range(rounds):
            fa, fb, levels, want = cases[k % len(cases)]
            assert_result(ctx.frame_msssim_result(ctx.frame_msssim_async(fa, ref_frame=fb, levels=levels)), want, "round %d" % k)
    finally:
        for case in cases:
            for f in case[:2]:
                ctx.frame_destroy(f)


def check_invalid(lib):
    """every M355_ERR_INVALID case of the header enqueues nothing: the next ticket is consecutive"""
    ctx = capi.Context(lib, 0)
    shard = capi.Context(lib, 0)
    try:
        L = lib.lib
        f8 = ctx.frame_create(64, 32, 1, 8, 8)
        f10 = ctx.frame_create(64, 32, 1, 10, 10)
        f9 = ctx.frame_create(64, 32, 1, 10, 9)
        f422 = ctx.frame_create(64, 32, 2, 8, 8)
        mono = ctx.frame_create(64, 32, 0, 8, 8)
        small = ctx.frame_create(32, 32, 1, 8, 8)
        big = ctx.frame_create(192, 176, 1, 8, 8)
        assert ctx.frame_msssim_async(f8, ref_frame=f8, levels=1) == 1
        tk = ctypes.c_ulonglong(0)
        mem = ctx.device_alloc(3 * 40 * 80)

        def desc(ref_frame=-1, rect=None, ref=(mem, mem, mem), pitch=(80, 80, 80), planes=0, levels=1, reserved=None):
            d = capi.MsssimDesc(ref_frame=ref_frame, planes=planes, levels=levels)
            if rect:
                d.x0, d.y0, d.width, d.height = rect
            for k in range(3):
                d.ref[k] = ref[k]; d.pitch[k] = pitch[k]
            if reserved is not None:
                d.reserved[reserved] = 1
            return d

        def refused(frame, d, what):
            rc = L.m355_frame_msssim_async(ctx.h, frame, d, tk)
            assert rc == INVALID, "%s: returned %d" % (what, rc)

        # what m355_frame_ssim_async rejects
        refused(f8 + 99, ctypes.byref(desc()), "bad frame handle")
        refused(-1, ctypes.byref(desc()), "negative frame handle")
        refused(f8, None, "null descriptor")
        assert L.m355_frame_msssim_async(ctx.h, f8, ctypes.byref(desc()), None) == INVALID, "null ticket"
        for rect in ((56, 0, 12, 12), (0, 28, 12, 12), (-2, 0, 12, 12), (0, -2, 12, 12), (0, 0, 12, -2), (0, 0, -12, 12), (0, 0, 66, 32), (0, 0, 12, 0)):
            refused(f8, ctypes.byref(desc(rect=rect)), "rectangle %s leaves the frame" % (rect,))
        for rect in ((1, 0, 24, 24), (0, 1, 24, 24), (0, 0, 23, 24), (0, 0, 24, 23)):
            refused(f8, ctypes.byref(desc(rect=rect)), "rectangle %s off the 4:2:0 chroma grid" % (rect,))
        refused(f422, ctypes.byref(desc(rect=(1, 0, 24, 24))), "4:2:2: odd x0")
        assert L.m355_frame_msssim_async(ctx.h, f422, ctypes.byref(desc(rect=(0, 1, 24, 23))), tk) == 0 and tk.value == 2, "4:2:2 has no vertical grid"
        for r, what in ((f8 + 99, "unknown ref_frame"), (-2, "ref_frame -2"), (f10, "other bit depths"), (f422, "other chroma format")):
            refused(f8, ctypes.byref(desc(ref_frame=r)), what)
        refused(f10, ctypes.byref(desc(ref_frame=f9)), "other chroma bit depth")
        refused(f10, ctypes.byref(desc(ref_frame=f8)), "other element size")
        refused(f8, ctypes.byref(desc(ref_frame=small)), "ref_frame smaller than the whole frame")
        refused(f8, ctypes.byref(desc(ref_frame=small, rect=(16, 0, 32, 32))), "ref_frame does not contain the rectangle")
        assert L.m355_frame_msssim_async(ctx.h, f8, ctypes.byref(desc(ref_frame=small, rect=(0, 0, 32, 32))), tk) == 0 and tk.value == 3
        for p in range(3):
            ref = [mem] * 3; ref[p] = None
            refused(f8, ctypes.byref(desc(ref=ref)), "null ref[%d]" % p)
            pitch = [80] * 3; pitch[p] = 63 if p == 0 else 31
            refused(f8, ctypes.byref(desc(pitch=pitch)), "pitch of plane %d below the row" % p)
            pitch = [160] * 3; pitch[p] = 161
            refused(f10, ctypes.byref(desc(pitch=pitch)), "odd pitch of 16-bit plane %d" % p)
            ref = [mem] * 3; ref[p] = mem + 1
            refused(f10, ctypes.byref(desc(ref=ref, rect=(0, 0, 24, 24), pitch=(160, 160, 160))), "odd pointer of 16-bit plane %d" % p)
        assert L.m355_frame_msssim_async(ctx.h, f8, ctypes.byref(desc(ref=(mem + 1, mem + 3, mem + 5), pitch=(65, 33, 33))), tk) == 0 and tk.value == 4, "8-bit planes: any pointer, any pitch"
        for t in (1, 2, 3, 4):                                      # (the four slots are taken)
            assert L.m355_frame_msssim_result(ctx.h, t, 1, ctypes.byref(capi.Msssim())) == 0
        shard.shard_set(0, 2)
        fs = shard.frame_create(64, 32, 1, 8, 8)
        assert L.m355_frame_msssim_async(shard.h, fs, ctypes.byref(desc(ref_frame=fs)), tk) == INVALID, "tile-sharded context"
        for planes in (8, 9, 15, 16, -1, 1 << 30):
            refused(f8, ctypes.byref(desc(ref_frame=f8, planes=planes)), "planes %d: bits above 2" % planes)
        for planes in (2, 4, 3, 6, 7):
            refused(mono, ctypes.byref(desc(ref_frame=mono, planes=planes)), "planes %d of a monochrome frame" % planes)
        for k in range(6):
            refused(f8, ctypes.byref(desc(ref_frame=f8, reserved=k)), "reserved[%d]" % k)
        # the call's own cases
        for levels in (0, -1, 6, 7, 1 << 20):
            refused(big, ctypes.byref(desc(ref_frame=big, planes=1, levels=levels)), "levels %d" % levels)
        for rect, planes, levels, what in (((0, 0, 10, 32), 1, 1, "luma 10 samples wide"), ((0, 0, 32, 20), 4, 1, "Cr 10 rows"), ((0, 0, 44, 32), 0, 2, "chroma 22 x 16, 2 levels"),
                                           ((0, 0, 64, 32), 1, 3, "luma 32 rows, 3 levels")):
            refused(f8, ctypes.byref(desc(ref_frame=f8, rect=rect, planes=planes, levels=levels)), what)
        for rect, what in (((0, 0, 21, 32), "21 samples wide, 2 levels"), ((0, 0, 44, 21), "21 rows, 2 levels")):
            refused(mono, ctypes.byref(desc(ref_frame=mono, rect=rect, levels=2)), what)
        refused(big, ctypes.byref(desc(ref_frame=big, rect=(0, 0, 176, 174), planes=1, levels=5)), "174 rows, 5 levels")
        refused(big, ctypes.byref(desc(ref_frame=big, planes=0, levels=5)), "chroma 96 x 88, 5 levels")
        rc = L.m355_frame_msssim_async(ctx.h, big, ctypes.byref(desc(ref_frame=big, planes=2, levels=5)), tk)
        assert rc == INVALID and all(s in lib.error() for s in ("plane 1", "96x88", "level 4")), "the message names the plane, its size and the level: %s" % lib.error()
        assert L.m355_frame_msssim_async(ctx.h, f8, ctypes.byref(desc(ref_frame=f8, rect=(0, 0, 44, 22), planes=1, levels=2)), tk) == 0 and tk.value == 5, "a narrow chroma plane that is not selected"
        assert L.m355_frame_msssim_async(ctx.h, big, ctypes.byref(desc(ref_frame=big, rect=(0, 0, 176, 176), planes=1, levels=5)), tk) == 0 and tk.value == 6, "the smallest plane of five levels"
        out = capi.Msssim()
        assert L.m355_frame_msssim_result(ctx.h, 5, 1, None) == INVALID, "null result"
        for t in (5, 6):
            assert L.m355_frame_msssim_result(ctx.h, t, 1, ctypes.byref(out)) == 0
        assert out.n[0][4] == 1 and out.sum_q[0][4] == ONE and out.msssim[0] == 1.0
        assert L.m355_frame_msssim_result(ctx.h, 7, 1, ctypes.byref(out)) == INVALID
        ctx.device_free(mem)
    finally:
        shard.close()
        ctx.close()


# ---- a decoded picture ----
def check_decoded_picture(lib):
    """one girlshy picture measured behind its decode with three pictures in flight: against the planes an earlier decode of it delivered and against
    that decode's frame (identical on every level) and against a perturbed copy; luma on five levels, all planes on four"""
    from golden_io import load_gold
    hdr, pics = load_gold("girlshy_full.m355gold.gz")
    c = capi.Context(lib, 0)
    try:
        pic = pics[0]
        saved = pic.dst_frame
        first = c.frame_create_for(pic.pp[0])
        pic.dst_frame = first
        c.submit(pic)
        c.wait()
        planes = c.frame_download(first)
        geom = (planes[0].shape[1], planes[0].shape[0], 1, 8, 8)
        all_levels = most_levels(geom[0], geom[1], 1)
        other = su.perturbed(planes, (8, 8, 8), seed=9)
        same, changed, changed_luma = c.measure_reference(planes), c.measure_reference(other), c.measure_reference(other)
        dst = c.frame_create_for(pic.pp[0])
        c.set_pipeline_depth(3)
        pic.dst_frame = dst
        c.submit(pic)
        pic.dst_frame = saved
        tickets = [c.frame_msssim_async(dst, ref_planes=same, levels=all_levels), c.frame_msssim_async(dst, ref_planes=changed, levels=all_levels),
                   c.frame_msssim_async(dst, ref_frame=first, levels=all_levels), c.frame_msssim_async(dst, ref_planes=changed_luma, planes=1, levels=most_levels(geom[0], geom[1], 0))]
        identical = expected(planes, planes, None, geom, levels=all_levels)
        assert all(w["sum_cs"][j] == w["sum_q"][j] == ONE * w["n"][j] for w in identical for j in range(all_levels))
        assert_result(c.frame_msssim_result(tickets[0]), identical, "against its own planes")
        assert_result(c.frame_msssim_result(tickets[1]), expected(planes, other, None, geom, levels=all_levels), "against the perturbed copy")
        assert_result(c.frame_msssim_result(tickets[2]), identical, "against the earlier decode's frame")
        want = expected(planes, other, None, geom, planes=1, levels=most_levels(geom[0], geom[1], 0))
        assert most_levels(geom[0], geom[1], 0) < LEVELS or 0 < want[0]["msssim"] < 1
        assert_result(c.frame_msssim_result(tickets[3]), want, "luma against the perturbed copy")
    finally:
        c.close()
