"""Scenarios of the SSIM-request tests (m355_frame_ssim_async / m355_frame_ssim_result), shared by the CPU tier (SIMT-interpreter build,
tests/test_ssim_emu.py) and the GPU tier (tests/test_gpu_ssim.py), and the numpy restatement of the definition (csrc/ssim_window.h) their
expected values come from: uint64 window sums, float64 elementwise operations in the header's order (numpy rounds every operation by itself),
q in Q30.  Every comparison is exact: sum_q, n, min_q, every map element, and ssim as the 8 bytes of the double."""
import ctypes
import re
import struct
from pathlib import Path

import numpy as np
import pytest

from hash_util import CRC, make_planes
from measure_util import BUSY, INVALID, PIC_A, PIC_B, PIC_C, PIC_D, REJECT_CASE, _upload_refs, crop, frame_with, sub_sampling
from oracle_py import Oracle
from synth_util import assert_planes_equal, make_case, oracle_decode
from libde265_amd import capi

SLOTS = 16                          # M355_SSIM_REQUESTS
ONE = 1 << 30
WEIGHTS = [17, 124, 590, 1792, 3490, 4358, 3490, 1792, 590, 124, 17]
PEAK_AGAINST_ZERO = 107363          # q of a window of `peak` against a window of 0, at every bit depth
_K_SSIM_H = (Path(__file__).resolve().parent.parent / "libde265_amd" / "csrc" / "k_ssim.h").read_text()
TW = int(re.search(r"#define SSIM_TILE_W (\d+)", _K_SSIM_H).group(1))
TH = int(re.search(r"#define SSIM_TILE_H (\d+)", _K_SSIM_H).group(1))
# one window; one more column / row; a tile whose last column / row is short by one, full, over by one; two tiles and a third of one column / row
PLANE_SIZES = [(11, 11), (12, 11), (11, 12), (TW + 9, TH + 9), (TW + 10, TH + 10), (TW + 11, TH + 11), (2 * TW + 11, 2 * TH + 11), (TW + 9, 2 * TH + 11),
               (2 * TW + 11, TH + 10)]
FORMATS = [(cf, 8, 8) for cf in range(4)] + [(cf, 10, 10) for cf in range(4)] + [(1, 16, 16), (3, 16, 16), (1, 10, 9), (2, 10, 9)]
MAP_FILL = 0xA5A5A5A5 - (1 << 32)   # capi.DEVICE_FILL in every byte of an int32


# ---- the definition, restated ----
def window_sums(a, b):
    """two planes of one shape -> MA, MB, SAA, SBB, SAB of every valid window: five uint64 arrays of (ph - 10, pw - 10)"""
    a, b = a.astype(np.uint64), b.astype(np.uint64)
    w = np.array(WEIGHTS, np.uint64)
    ph, pw = a.shape
    out = []
    for f in (a, b, a * a, b * b, a * b):
        rows = sum(w[k] * f[:, k:k + pw - 10] for k in range(11))
        out.append(sum(w[k] * rows[k:k + ph - 10, :] for k in range(11)))
    return out


def constants(bd):
    peak = (1 << bd) - 1
    return float(peak * peak) * 2.0 ** 56 / 10000.0, float(peak * peak * 9) * 2.0 ** 56 / 10000.0


def point(sums, bd):
    """the five sums (uint64 arrays) -> q, int64 array: the operations of m355_ssim_point, one rounding each"""
    c1, c2 = constants(bd)
    MA, MB, SAA, SBB, SAB = [np.asarray(s, np.uint64) for s in sums]
    k28 = np.float64(2.0 ** 28)
    fa, fb = MA.astype(np.float64), MB.astype(np.float64)
    ab, aa, bb = fa * fb, fa * fa, fb * fb
    cov, va, vb = k28 * SAB.astype(np.float64) - ab, k28 * SAA.astype(np.float64) - aa, k28 * SBB.astype(np.float64) - bb
    s = ((2.0 * ab + c1) * (2.0 * cov + c2)) / (((aa + bb) + c1) * ((va + vb) + c2))
    return np.clip(np.floor(s * 2.0 ** 30 + 0.5), -2.0 ** 30, 2.0 ** 30).astype(np.int64)


def ssim_plane(a, b, bd):
    """one plane against another -> the fields of m355_ssim for it, and the map"""
    q = point(window_sums(a, b), bd)
    sum_q, n = int(q.sum()), int(q.size)
    return dict(sum_q=sum_q, n=n, min_q=int(q.min()), ssim=float(sum_q) / (float(n) * 2.0 ** 30)), q.astype(np.int32)


ZERO = dict(sum_q=0, n=0, min_q=0, ssim=0.0)


def expected(frame_planes, ref_rect_planes, rect, geom, planes=0):
    """what a request on a frame holding frame_planes delivers against the RECTANGLE's reference planes -> ([3 dicts], [3 maps or None])"""
    _, _, cf, bdl, bdc = geom
    res, maps = [], []
    for c in range(3):
        if c >= len(frame_planes) or (planes and not (planes >> c) & 1):
            res.append(dict(ZERO)); maps.append(None)
            continue
        r, m = ssim_plane(crop(frame_planes, rect, cf)[c], ref_rect_planes[c], bdc if c else bdl)
        res.append(r); maps.append(m)
    return res, maps


def assert_result(got, want, what=""):
    assert len(got) == 3, what
    for c, (g, w) in enumerate(zip(got, want)):
        for k in ("sum_q", "n", "min_q"):
            assert g[k] == w[k], "%s: plane %d: %s is %r, expected %r" % (what, c, k, g[k], w[k])
        assert struct.pack("<d", g["ssim"]) == struct.pack("<d", w["ssim"]), "%s: plane %d: ssim is %r, expected %r" % (what, c, g["ssim"], w["ssim"])


def perturbed(planes, bds, seed):
    """the planes with noise of a few percent of the range and a patch of stronger damage: SSIM in the middle of its range"""
    rng = np.random.default_rng(seed)
    out = []
    for c, p in enumerate(planes):
        peak = (1 << bds[c]) - 1
        d = rng.integers(-(peak // 16) - 1, peak // 16 + 2, p.shape)
        d[: p.shape[0] // 2, : p.shape[1] // 3] *= 5
        out.append(np.clip(p.astype(np.int64) + d, 0, peak).astype(p.dtype))
    return out


# ---- maps ----
GUARD = 64


class Maps:
    """per measured plane a device buffer for the map at a pitch above the row, with a guard band behind it, every byte capi.DEVICE_FILL"""

    def __init__(self, ctx, want_maps, extra=12):
        self.ctx, self.bufs = ctx, []
        for m in want_maps:
            if m is None:
                self.bufs.append(None)
                continue
            pitch = 4 * m.shape[1] + extra
            self.bufs.append((ctx.device_alloc(m.shape[0] * pitch + GUARD), pitch, m.shape))
        self.arg = [None if b is None else (b[0], b[1]) for b in self.bufs]

    def read(self, c):
        p, pitch, (rows, cols) = self.bufs[c]
        raw = self.ctx.device_read(p, rows * pitch + GUARD)
        body = raw[:rows * pitch].reshape(rows, pitch)
        return body[:, :4 * cols].copy().view(np.int32), body[:, 4 * cols:], raw[rows * pitch:]

    def check(self, want_maps, what, untouched=False):
        for c, m in enumerate(want_maps):
            if m is None:
                continue
            got, tails, guard = self.read(c)
            assert (tails == capi.DEVICE_FILL).all() and (guard == capi.DEVICE_FILL).all(), "%s: plane %d: bytes behind a map row or behind the map were written" % (what, c)
            if untouched:
                assert (got == MAP_FILL).all(), "%s: plane %d: the map was written" % (what, c)
            else:
                bad = np.argwhere(got != m)
                assert not len(bad), "%s: plane %d: %d map elements differ, first at (x, y) = (%d, %d): %d, expected %d" % (
                    what, c, len(bad), bad[0][1], bad[0][0], got[tuple(bad[0])], m[tuple(bad[0])])

    def free(self):
        for b in self.bufs:
            if b is not None:
                self.ctx.device_free(b[0])


def check_pair(ctx, geom, a, b, rect=None, planes=0, against_frame=True, against_memory=True, host=False, with_maps=True, what=""):
    """a frame holding planes `a` against whole-frame planes `b`: as memory (the rectangle's part of b) and as a second frame, with maps"""
    cf = geom[2]
    want, want_maps = expected(a, crop(b, rect, cf), rect, geom, planes)
    fa = frame_with(ctx, geom, a)
    fb = frame_with(ctx, geom, b) if against_frame else None
    runs = []
    try:
        for how in [h for h, on in (("memory", against_memory), ("frame", against_frame)) if on]:
            maps = Maps(ctx, want_maps) if with_maps else None
            kw = dict(ref_planes=crop(b, rect, cf), host=host) if how == "memory" else dict(ref_frame=fb)
            runs.append((how, ctx.frame_ssim_async(fa, rect=rect, planes=planes, maps=maps.arg if maps else None, **kw), maps))
        for how, tk, maps in runs:
            text = "%s %s rect %s planes %d against %s" % (what, geom, rect, planes, how)
            assert_result(ctx.frame_ssim_result(tk), want, text)
            if maps:
                maps.check(want_maps, text)
    finally:
        for _, _, maps in runs:
            if maps:
                maps.free()
        ctx.frame_destroy(fa)
        if fb is not None:
            ctx.frame_destroy(fb)
    return want, want_maps


# ---- values ----
def check_plane_size(ctx, pw, ph, bd):
    """a pw x ph rectangle of a monochrome frame, off the frame's origin"""
    w, h = (pw + 3 + 7) & ~7, (ph + 5 + 7) & ~7
    geom = (w, h, 0, bd, bd)
    a = make_planes(w, h, 0, bd, bd, seed=pw + 7 * ph + bd)
    want, _ = check_pair(ctx, geom, a, perturbed(a, (bd,), seed=3 * pw + ph), rect=(3, 5, pw, ph), what="plane size")
    assert want[0]["n"] == (pw - 10) * (ph - 10) and want[1] == ZERO and want[2] == ZERO


def check_format(ctx, cf, bdl, bdc):
    """a whole 64 x 48 frame: chroma planes of 32 x 24 (4:2:0), 32 x 48 (4:2:2), 64 x 48 (4:4:4), each with its own constants"""
    geom = (64, 48, cf, bdl, bdc)
    a = make_planes(*geom, seed=20 + cf + bdl)
    want, _ = check_pair(ctx, geom, a, perturbed(a, (bdl, bdc, bdc), seed=30 + cf + bdc), what="format")
    assert [w["n"] != 0 for w in want] == [True, cf != 0, cf != 0]
    assert all(0 < w["ssim"] < 1 for w in want if w["n"])


def check_extremes(ctx, bd):
    peak = (1 << bd) - 1
    dt = np.uint8 if bd <= 8 else np.uint16
    w, h = TW + 16, TH + 16
    geom = (w, h, 0, bd, bd)
    hi, lo = [np.full((h, w), peak, dt)], [np.zeros((h, w), dt)]
    for a, b in ((hi, lo), (lo, hi)):
        want, maps = check_pair(ctx, geom, a, b, what="peak against zero")
        assert (maps[0] == PEAK_AGAINST_ZERO).all() and want[0]["min_q"] == PEAK_AGAINST_ZERO
    noise = make_planes(w, h, 0, bd, bd, seed=bd)
    for a in (noise, hi, lo):
        want, maps = check_pair(ctx, geom, a, [a[0].copy()], what="identical")
        assert (maps[0] == ONE).all() and want[0]["min_q"] == ONE and want[0]["sum_q"] == ONE * want[0]["n"] and want[0]["ssim"] == 1.0
    want, _ = check_pair(ctx, geom, noise, [(peak - noise[0].astype(np.int64)).astype(dt)], what="inversion")
    assert want[0]["sum_q"] < 0 and want[0]["min_q"] < 0 and want[0]["ssim"] < -0.5


def check_rectangles(ctx):
    for cf, bd, rect in ((1, 8, (6, 2, 50, 40)), (2, 10, (6, 3, 50, 41)), (3, 8, (5, 3, 51, 13)), (0, 12, (1, 1, 62, 46))):
        geom = (64, 48, cf, bd, bd)
        a = make_planes(*geom, seed=40 + cf)
        check_pair(ctx, geom, a, perturbed(a, (bd,) * 3, seed=50 + cf), rect=rect, what="rectangle")


def check_pinned_reference(ctx):
    geom = (64, 48, 1, 8, 8)
    a = make_planes(*geom, seed=70)
    check_pair(ctx, geom, a, perturbed(a, (8,) * 3, seed=71), against_frame=False, host=True, what="pinned host reference")


def check_plane_selection(ctx):
    for geom in ((64, 48, 1, 8, 8), (64, 48, 3, 10, 10)):
        a = make_planes(*geom, seed=80)
        b = perturbed(a, (geom[3], geom[4], geom[4]), seed=81)
        want, _ = check_pair(ctx, geom, a, b, planes=1, what="luma only")
        assert want[0]["n"] and want[1] == ZERO and want[2] == ZERO
        want, _ = check_pair(ctx, geom, a, b, planes=6, rect=(8, 4, 48, 40), what="chroma only")
        assert want[0] == ZERO and want[1]["n"] and want[2]["n"]
        check_pair(ctx, geom, a, b, planes=5, what="luma and Cr")


# ---- the request as a reader of its frames (the scenarios of measure_util with these calls) ----
GEOM_420 = (64, 64, 1, 8, 8)


def check_reader_hazard(lib, oracle, depth, as_ref_frame, with_others):
    """decode A into F, request on F (or on G with F as ref_frame), [export F, hash F,] decode B into F — nothing waited for in between:
    the values are A's.  The other side holds picture B, so a request that saw B in F would report 1.0."""
    o = Oracle(oracle)
    (pa, ra), (pb, rb) = make_case(**PIC_A), make_case(**PIC_B)
    want_a, want_b = oracle_decode(o, pa, ra), oracle_decode(o, pb, rb)
    want, _ = expected(want_a, want_b, None, GEOM_420)
    assert all(w["min_q"] < ONE for w in want), "the two pictures must differ"
    ctx = capi.Context(lib, 0)
    try:
        _upload_refs(ctx, pa, ra)
        _upload_refs(ctx, pb, rb)
        F = ctx.frame_create_for(pa.pp[0])
        G = ctx.frame_create_for(pa.pp[0])
        ctx.frame_upload(G, want_b)
        ctx.set_pipeline_depth(depth)
        in_memory = None if as_ref_frame else ctx.measure_reference(want_b)
        ctx.wait()
        # ---- no host wait from here ...
        pa.dst_frame = pb.dst_frame = F
        ctx.submit(pa)
        tk = ctx.frame_ssim_async(G, ref_frame=F) if as_ref_frame else ctx.frame_ssim_async(F, ref_planes=in_memory)
        token = ctx.frame_export(F, capi.EXPORT_PLANAR, capi.EXPORT_NATIVE, host=True) if with_others else None
        htk = ctx.frame_hash_async(F, CRC) if with_others else None
        ctx.submit(pb)
        # ---- ... to here
        assert_result(ctx.frame_ssim_result(tk), want, "depth %d, F as %s" % (depth, "ref_frame" if as_ref_frame else "the frame"))   # (q is symmetric)
        if with_others:
            assert_planes_equal(ctx.frame_export_finish(token), want_a, "export between the request and the next decode")
            hash_a = ctx.frame_hash_result(htk)
        ctx.wait()
        assert_planes_equal(ctx.frame_download(F), want_b, "the later picture")
        if with_others:
            assert hash_a != ctx.frame_hash(F, CRC)
        assert_result(ctx.frame_ssim_result(ctx.frame_ssim_async(F, ref_frame=G)), expected(want_b, want_b, None, GEOM_420)[0], "the later picture against itself")
    finally:
        ctx.close()


def check_two_writers(lib, oracle, depth=3):
    """the frame and its ref_frame written by decodes on DIFFERENT lanes, nothing waited for (measure_util.check_two_writers): D into G, D into H, C into
    F, then a request on G and one on H, both with ref_frame = F, then D into F"""
    o = Oracle(oracle)
    (pc, rc_), (pd, rd) = make_case(**PIC_C), make_case(**PIC_D)
    want_c, want_d = oracle_decode(o, pc, rc_), oracle_decode(o, pd, rd)
    want, _ = expected(want_d, want_c, None, (256, 192, 1, 8, 8))
    assert all(w["min_q"] < ONE for w in want), "the two pictures must differ"
    ctx = capi.Context(lib, 0)
    try:
        _upload_refs(ctx, pc, rc_)
        _upload_refs(ctx, pd, rd)
        F, G, H = [ctx.frame_create_for(pc.pp[0]) for _ in range(3)]
        ctx.set_pipeline_depth(depth)
        ctx.wait()
        # ---- no host wait from here ...
        pd.dst_frame = G
        ctx.submit(pd)
        pd.dst_frame = H
        ctx.submit(pd)
        pc.dst_frame = F
        ctx.submit(pc)
        tk_g = ctx.frame_ssim_async(G, ref_frame=F)
        tk_h = ctx.frame_ssim_async(H, ref_frame=F)
        pd.dst_frame = F
        ctx.submit(pd)
        # ---- ... to here
        assert_result(ctx.frame_ssim_result(tk_g), want, "G against F, written on another lane (depth %d)" % depth)
        assert_result(ctx.frame_ssim_result(tk_h), want, "H against F, behind the first request's mark (depth %d)" % depth)
        ctx.wait()
        assert_planes_equal(ctx.frame_download(F), want_d, "the later picture")
    finally:
        ctx.close()


# ---- verdicts, slots and tickets ----
def check_rejected_decode(lib, oracle, depth):
    """a request behind a decode whose lists the device rejected — into the frame, or into its ref_frame — has no value, has read nothing and has left
    a pre-filled map as it was; the slot it used is clean for the next request"""
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
        w, want_maps = expected(want, filled, None, geom)
        for as_ref_frame in (False, True):
            maps = Maps(ctx, want_maps)
            try:
                bad.dst_frame = d
                ctx.submit_in_place(bad, fill_threads=1)
                serial = ctx.last_serial()
                tk = ctx.frame_ssim_async(other, ref_frame=d, maps=maps.arg) if as_ref_frame else ctx.frame_ssim_async(d, ref_frame=other, maps=maps.arg)
                with pytest.raises(capi.M355Error) as e:
                    ctx.frame_ssim_result(tk)
                assert e.value.code == INVALID and "rejected" in str(e.value)
                st = ctx.decode_status(serial)                      # (reported here, so that m355_wait stays quiet)
                while st == BUSY:
                    st = ctx.decode_status(serial)
                assert st == INVALID
                maps.check(want_maps, "behind a rejected decode (ref_frame: %s)" % as_ref_frame, untouched=True)
                with pytest.raises(capi.M355Error):                 # the failed collection freed the ticket
                    ctx.frame_ssim_result(tk)
                pic.dst_frame = d
                ctx.submit_in_place(pic, fill_threads=1)
                tk = ctx.frame_ssim_async(other, ref_frame=d, maps=maps.arg) if as_ref_frame else ctx.frame_ssim_async(d, ref_frame=other, maps=maps.arg)
                assert_result(ctx.frame_ssim_result(tk), w, "in the slot a gated request left (ref_frame: %s)" % as_ref_frame)
                maps.check(want_maps, "in the slot a gated request left (ref_frame: %s)" % as_ref_frame)
            finally:
                maps.free()
        ctx.wait()
    finally:
        ctx.close()


def check_concurrency(lib):
    """16 requests on 16 frames before any is collected, collected in reverse; the 17th is refused; a collected slot is free again"""
    ctx = capi.Context(lib, 0)
    try:
        frames, refs, want = [], [], []
        for i in range(SLOTS):
            geom = [(64, 48, 1, 8, 8), (72, 40, 0, 8, 8), (56, 32, 2, 10, 10), (40, 16, 3, 12, 12)][i % 4]
            a = make_planes(*geom, seed=900 + i)
            b = perturbed(a, (geom[3], geom[4], geom[4]), seed=950 + i)
            frames.append(frame_with(ctx, geom, a))
            refs.append(frame_with(ctx, geom, b) if i % 2 else ctx.measure_reference(b))
            want.append(expected(a, b, None, geom)[0])
        tickets = [ctx.frame_ssim_async(f, ref_frame=r) if i % 2 else ctx.frame_ssim_async(f, ref_planes=r) for i, (f, r) in enumerate(zip(frames, refs))]
        assert tickets == list(range(1, SLOTS + 1)), "tickets count 1, 2, ... per context"
        with pytest.raises(capi.M355Error) as e:
            ctx.frame_ssim_async(frames[0], ref_frame=frames[0])
        assert e.value.code == BUSY
        assert_result(ctx.frame_ssim_result(tickets[-1]), want[-1], "the last request")
        extra = ctx.frame_ssim_async(frames[3], ref_frame=refs[3])         # the refused call took no ticket and enqueued nothing
        assert extra == SLOTS + 1
        assert_result(ctx.frame_ssim_result(extra), want[3], "the slot collected first, reused")
        for i in reversed(range(SLOTS - 1)):
            assert_result(ctx.frame_ssim_result(tickets[i]), want[i], "request %d" % i)
    finally:
        ctx.close()


def check_nonblocking(lib):
    ctx = capi.Context(lib, 0)
    try:
        geom = (88, 56, 1, 8, 8)
        a = make_planes(*geom, seed=5)
        b = perturbed(a, (8,) * 3, seed=6)
        fa, fb = frame_with(ctx, geom, a), frame_with(ctx, geom, b)
        want = expected(a, b, None, geom)[0]
        for k in range(3):
            tk = ctx.frame_ssim_async(fa, ref_frame=fb)
            assert tk == k + 1
            got = ctx.frame_ssim_result(tk, block=False)
            while got is None:                                      # BUSY: nothing was waited for, the request stays
                got = ctx.frame_ssim_result(tk, block=False)
            assert_result(got, want, "non-blocking collection")
            for bad in (tk, tk + 1000, 0):                          # collected / unknown
                with pytest.raises(capi.M355Error) as e:
                    ctx.frame_ssim_result(bad, block=False)
                assert e.value.code == INVALID
        # m355_wait completes a request (and its map) and does not collect it; a frame may be destroyed with a request pending
        _, want_maps = expected(a, b, None, geom)
        maps = Maps(ctx, want_maps)
        tk = ctx.frame_ssim_async(fa, ref_frame=fb, maps=maps.arg)
        ctx.wait()
        maps.check(want_maps, "the map behind m355_wait")
        maps.free()
        tk2 = ctx.frame_ssim_async(fb, ref_frame=fa)
        ctx.frame_destroy(fa)
        assert_result(ctx.frame_ssim_result(tk, block=False), want, "collected behind m355_wait")
        assert_result(ctx.frame_ssim_result(tk2), want, "collected behind the frame's destruction")
    finally:
        ctx.close()


def check_slot_reuse(ctx, rounds=40):
    """one slot, request after request, alternately "identical" and "differs", 8 and 10 bit: a device record not left zero shows in the next result"""
    cases = []
    for geom in ((72, 40, 1, 8, 8), (56, 24, 2, 10, 9)):
        a = make_planes(*geom, seed=77)
        b = perturbed(a, (geom[3], geom[4], geom[4]), seed=78)
        cases.append((frame_with(ctx, geom, a), frame_with(ctx, geom, b), frame_with(ctx, geom, a), expected(a, b, None, geom)[0], expected(a, a, None, geom)[0]))
    try:
        for k in range(rounds):
            fa, fb, fa2, differs, same = cases[(k // 2) % 2]
            tk = ctx.frame_ssim_async(fa, ref_frame=fb if k % 2 else fa2)
            assert_result(ctx.frame_ssim_result(tk), differs if k % 2 else same, "round %d" % k)
    finally:
        for case in cases:
            for f in case[:3]:
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
        assert ctx.frame_ssim_async(f8, ref_frame=f8) == 1
        tk = ctypes.c_ulonglong(0)
        mem = ctx.device_alloc(3 * 40 * 80)
        mapmem = ctx.device_alloc(3 * 64 * 4 * 32)

        def desc(ref_frame=-1, rect=None, ref=(mem, mem, mem), pitch=(80, 80, 80), planes=0, reserved=None, maps=(None, None, None), map_pitch=(0, 0, 0)):
            d = capi.SsimDesc(ref_frame=ref_frame, planes=planes)
            if rect:
                d.x0, d.y0, d.width, d.height = rect
            for k in range(3):
                d.ref[k] = ref[k]; d.pitch[k] = pitch[k]; d.map[k] = maps[k]; d.map_pitch[k] = map_pitch[k]
            if reserved is not None:
                d.reserved[reserved] = 1
            return d

        def refused(frame, d, what):
            rc = L.m355_frame_ssim_async(ctx.h, frame, d, tk)
            assert rc == INVALID, "%s: returned %d" % (what, rc)

        # what m355_frame_measure_async rejects
        refused(f8 + 99, ctypes.byref(desc()), "bad frame handle")
        refused(-1, ctypes.byref(desc()), "negative frame handle")
        refused(f8, None, "null descriptor")
        assert L.m355_frame_ssim_async(ctx.h, f8, ctypes.byref(desc()), None) == INVALID, "null ticket"
        for rect in ((56, 0, 12, 12), (0, 28, 12, 12), (-2, 0, 12, 12), (0, -2, 12, 12), (0, 0, 12, -2), (0, 0, -12, 12), (0, 0, 66, 32), (0, 0, 12, 0)):
            refused(f8, ctypes.byref(desc(rect=rect)), "rectangle %s leaves the frame" % (rect,))
        for rect in ((1, 0, 24, 24), (0, 1, 24, 24), (0, 0, 23, 24), (0, 0, 24, 23)):
            refused(f8, ctypes.byref(desc(rect=rect)), "rectangle %s off the 4:2:0 chroma grid" % (rect,))
        refused(f422, ctypes.byref(desc(rect=(1, 0, 24, 24))), "4:2:2: odd x0")
        assert L.m355_frame_ssim_async(ctx.h, f422, ctypes.byref(desc(rect=(0, 1, 24, 23))), tk) == 0 and tk.value == 2, "4:2:2 has no vertical grid"
        for r, what in ((f8 + 99, "unknown ref_frame"), (-2, "ref_frame -2"), (f10, "other bit depths"), (f422, "other chroma format")):
            refused(f8, ctypes.byref(desc(ref_frame=r)), what)
        refused(f10, ctypes.byref(desc(ref_frame=f9)), "other chroma bit depth")
        refused(f10, ctypes.byref(desc(ref_frame=f8)), "other element size")
        refused(f8, ctypes.byref(desc(ref_frame=small)), "ref_frame smaller than the whole frame")
        refused(f8, ctypes.byref(desc(ref_frame=small, rect=(16, 0, 32, 32))), "ref_frame does not contain the rectangle")
        assert L.m355_frame_ssim_async(ctx.h, f8, ctypes.byref(desc(ref_frame=small, rect=(0, 0, 32, 32))), tk) == 0 and tk.value == 3
        for p in range(3):
            ref = [mem] * 3; ref[p] = None
            refused(f8, ctypes.byref(desc(ref=ref)), "null ref[%d]" % p)
            pitch = [80] * 3; pitch[p] = 63 if p == 0 else 31
            refused(f8, ctypes.byref(desc(pitch=pitch)), "pitch of plane %d below the row" % p)
            pitch = [160] * 3; pitch[p] = 161
            refused(f10, ctypes.byref(desc(pitch=pitch)), "odd pitch of 16-bit plane %d" % p)
            ref = [mem] * 3; ref[p] = mem + 1
            refused(f10, ctypes.byref(desc(ref=ref, rect=(0, 0, 24, 24), pitch=(160, 160, 160))), "odd pointer of 16-bit plane %d" % p)
        assert L.m355_frame_ssim_async(ctx.h, f8, ctypes.byref(desc(ref=(mem + 1, mem + 3, mem + 5), pitch=(65, 33, 33))), tk) == 0 and tk.value == 4, "8-bit planes: any pointer, any pitch"
        shard.shard_set(0, 2)
        fs = shard.frame_create(64, 32, 1, 8, 8)
        assert L.m355_frame_ssim_async(shard.h, fs, ctypes.byref(desc(ref_frame=fs)), tk) == INVALID, "tile-sharded context"
        # the calls' own cases
        for rect, planes, what in (((0, 0, 10, 32), 1, "luma 10 samples wide"), ((0, 0, 32, 10), 1, "luma 10 rows"), ((0, 0, 20, 32), 0, "chroma 10 samples wide"),
                                   ((0, 0, 32, 20), 4, "Cr 10 rows"), ((0, 0, 20, 20), 6, "chroma 10 x 10")):
            refused(f8, ctypes.byref(desc(ref_frame=f8, rect=rect, planes=planes)), what)
        assert L.m355_frame_ssim_async(ctx.h, f8, ctypes.byref(desc(ref_frame=f8, rect=(0, 0, 20, 20), planes=1)), tk) == 0 and tk.value == 5, "a narrow chroma plane that is not selected"
        for planes in (8, 9, 15, 16, -1, 1 << 30):
            refused(f8, ctypes.byref(desc(ref_frame=f8, planes=planes)), "planes %d: bits above 2" % planes)
        for planes in (2, 4, 3, 6, 7):
            refused(mono, ctypes.byref(desc(ref_frame=mono, planes=planes)), "planes %d of a monochrome frame" % planes)
        for k in range(7):
            refused(f8, ctypes.byref(desc(ref_frame=f8, reserved=k)), "reserved[%d]" % k)
        row = 4 * 54                                                # the whole 64 x 32 frame: luma 54 x 22 windows, chroma 22 x 6
        for p in range(3):
            need = row if p == 0 else 4 * 22
            for ptr, mp, what in ((mapmem + 2, 256, "map pointer off by 2"), (mapmem + 1, 256, "odd map pointer"), (mapmem, 258, "map pitch off by 2"),
                                  (mapmem, need - 4, "map pitch below the row"), (mapmem, 0, "map pitch 0"), (mapmem, -256, "negative map pitch")):
                maps, pitches = [None] * 3, [0] * 3
                maps[p], pitches[p] = ptr, mp
                refused(f8, ctypes.byref(desc(ref_frame=f8, maps=maps, map_pitch=pitches)), "%s, plane %d" % (what, p))
        refused(f8, ctypes.byref(desc(ref_frame=f8, planes=1, maps=(None, mapmem, None), map_pitch=(0, 256, 0))), "a map for a plane that is not selected")
        refused(f8, ctypes.byref(desc(ref_frame=f8, planes=6, maps=(mapmem, None, None), map_pitch=(256, 0, 0))), "a map for luma, which is not selected")
        refused(mono, ctypes.byref(desc(ref_frame=mono, maps=(None, None, mapmem), map_pitch=(0, 0, 256))), "a map for a plane the frame does not have")
        assert L.m355_frame_ssim_async(ctx.h, f8, ctypes.byref(desc(ref_frame=f8, maps=(mapmem, None, None), map_pitch=(row, 0, 0))), tk) == 0 and tk.value == 6, "the smallest map pitch"
        out = capi.Ssim()
        assert L.m355_frame_ssim_result(ctx.h, 1, 1, None) == INVALID, "null result"
        for t in (1, 2, 3, 4, 5, 6):
            assert L.m355_frame_ssim_result(ctx.h, t, 1, ctypes.byref(out)) == 0
        assert L.m355_frame_ssim_result(ctx.h, 7, 1, ctypes.byref(out)) == INVALID
        ctx.device_free(mem)
        ctx.device_free(mapmem)
    finally:
        shard.close()
        ctx.close()


# ---- a decoded picture ----
def check_decoded_picture(lib):
    """one girlshy picture measured behind its decode with three pictures in flight: against the planes an earlier decode of it delivered and against
    that decode's frame (all 2^30) and against a copy with three samples changed"""
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
        other = [p.copy() for p in planes]
        other[0][5, 17] ^= 1
        other[0][planes[0].shape[0] - 1, planes[0].shape[1] - 1] ^= 0x80
        other[2][3, 0] ^= 0x22
        same, changed = c.measure_reference(planes), c.measure_reference(other)
        dst = c.frame_create_for(pic.pp[0])
        c.set_pipeline_depth(3)
        pic.dst_frame = dst
        c.submit(pic)
        pic.dst_frame = saved
        tickets = [c.frame_ssim_async(dst, ref_planes=same), c.frame_ssim_async(dst, ref_planes=changed), c.frame_ssim_async(dst, ref_frame=first)]
        identical = expected(planes, planes, None, geom)[0]
        assert all(w["min_q"] == ONE and w["ssim"] == 1.0 for w in identical)
        assert_result(c.frame_ssim_result(tickets[0]), identical, "against its own planes")
        want = expected(planes, other, None, geom)[0]
        assert [w["min_q"] < ONE for w in want] == [True, False, True]
        assert_result(c.frame_ssim_result(tickets[1]), want, "against the changed copy")
        assert_result(c.frame_ssim_result(tickets[2]), identical, "against the earlier decode's frame")
    finally:
        c.close()
