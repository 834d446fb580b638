"""Scenarios of the comparison-request tests (m355_frame_measure_async / m355_frame_measure_result), shared by the CPU tier (SIMT-interpreter
build, tests/test_measure_emu.py) and the GPU tier (tests/test_gpu_measure.py), and the numpy restatement their expected values come from:
int64 differences, the MSE as quality.cc sums it (row by row, in double) — tests/test_measure_ref.py holds the restatement against the
reference's own SSD / SAD / MSE.  Every comparison is exact; mse is compared as the 8 bytes of the double."""
import ctypes
import struct

import numpy as np
import pytest

from hash_util import CRC, make_planes
from oracle_py import Oracle
from synth_util import assert_planes_equal, make_case, oracle_decode
from libde265_amd import capi, worklist

BUSY, INVALID = 6, 3                # M355_ERR_BUSY, M355_ERR_INVALID
SLOTS = 16                          # M355_MEASURE_REQUESTS

# rows of one 1 KB block plus a tail that is no multiple of 16 bytes (1032 bytes; chroma 516) and of a block plus one lane (520 samples of 10 bit),
# in all four chroma formats; the minimum of rows; several rows per wavefront with the last span short (12296 rows, three per wavefront)
SHAPES = [(1032, 16, cf, 8, 8) for cf in range(4)] + [(520, 16, cf, 10, 10) for cf in range(4)] + [(64, 8, 0, 8, 8), (64, 12296, 0, 8, 8)]
RECT = (6, 2, 50, 22)               # on 64x32
PIC_A = dict(width=64, height=64, bit_depth=8, seed=301, intra_pct=30)
PIC_B = dict(width=64, height=64, bit_depth=8, seed=302, intra_pct=30)
PIC_C = dict(width=256, height=192, bit_depth=8, seed=311, intra_pct=30)
PIC_D = dict(width=256, height=192, bit_depth=8, seed=312, intra_pct=30)
REJECT_CASE = dict(width=256, height=192, bit_depth=8, seed=71, intra_pct=30, tile_cols=2, features=2)


def sub_sampling(cf):
    return (2 if cf in (1, 2) else 1), (2 if cf == 1 else 1)


def mse_rows(row_ssd, width):
    """MSE() of quality.cc: from 0.0, plus (double)row / width row by row, divided by the number of rows"""
    s = 0.0
    for r in row_ssd:
        s += float(int(r)) / width
    return s / len(row_ssd)


def measure_plane(a, b, px=0, py=0):
    """one plane against another of the same shape -> the fields of m355_measure; px, py: where a[0, 0] lies in the frame's plane"""
    d = a.astype(np.int64) - b.astype(np.int64)
    rows = (d * d).sum(axis=1)
    nz = np.argwhere(d != 0)
    return dict(ssd=int(rows.sum()), sad=int(np.abs(d).sum()), n_diff=int(len(nz)), max_abs=int(np.abs(d).max()),
                first=None if not len(nz) else (int(nz[0][1]) + px, int(nz[0][0]) + py), mse=mse_rows(rows, a.shape[1]))


def crop(planes, rect, cf):
    if rect is None:
        return [np.ascontiguousarray(p) for p in planes]
    sw, sh = sub_sampling(cf)
    x0, y0, w, h = rect
    return [np.ascontiguousarray(p[y0 // (sh if c else 1):(y0 + h) // (sh if c else 1), x0 // (sw if c else 1):(x0 + w) // (sw if c else 1)]) for c, p in enumerate(planes)]


def expected(frame_planes, ref_rect_planes, rect, cf):
    """what a request on a frame holding frame_planes delivers against the RECTANGLE's reference planes"""
    sw, sh = sub_sampling(cf)
    x0, y0 = (rect[0], rect[1]) if rect is not None else (0, 0)
    return [measure_plane(a, b, x0 // (sw if c else 1), y0 // (sh if c else 1)) for c, (a, b) in enumerate(zip(crop(frame_planes, rect, cf), ref_rect_planes))]


def assert_result(got, want, what=""):
    assert len(got) == len(want), what
    for c, (g, w) in enumerate(zip(got, want)):
        for k in ("ssd", "sad", "n_diff", "max_abs", "first"):
            assert g[k] == w[k], "%s: plane %d: %s is %r, expected %r" % (what, c, k, g[k], w[k])
        assert struct.pack("<d", g["mse"]) == struct.pack("<d", w["mse"]), "%s: plane %d: mse is %r, expected %r" % (what, c, g["mse"], w["mse"])


def frame_with(ctx, geom, planes):
    f = ctx.frame_create(*geom)
    ctx.frame_upload(f, planes)
    return f


def check_pair(ctx, geom, a, b, rect=None, against_frame=True, against_memory=True, host=False, what=""):
    """a frame holding planes `a` against whole-frame planes `b`: as memory (the rectangle's part of b) and as a second frame"""
    cf = geom[2]
    want = expected(a, crop(b, rect, cf), rect, cf)
    fa = frame_with(ctx, geom, a)
    fb = frame_with(ctx, geom, b) if against_frame else None
    try:
        tickets = []
        if against_memory:
            tickets.append(("memory", ctx.frame_measure_async(fa, ref_planes=crop(b, rect, cf), rect=rect, host=host)))
        if against_frame:
            tickets.append(("frame", ctx.frame_measure_async(fa, ref_frame=fb, rect=rect)))
        for how, tk in tickets:
            assert_result(ctx.frame_measure_result(tk), want, "%s %s rect %s against %s" % (what, geom, rect, how))
    finally:
        ctx.frame_destroy(fa)
        if fb is not None:
            ctx.frame_destroy(fb)
    return want


# ---- values ----
def check_values(ctx, geom):
    w, h, cf, bdl, bdc = geom
    check_pair(ctx, geom, make_planes(w, h, cf, bdl, bdc, seed=w + 7 * h), make_planes(w, h, cf, bdl, bdc, seed=11 * w + h + cf), what="values")


def check_rectangles(ctx):
    for cf, bd in ((1, 8), (2, 10), (3, 8), (0, 12)):
        geom = (64, 32, cf, bd, bd)
        a, b = make_planes(64, 32, cf, bd, bd, seed=40 + cf), make_planes(64, 32, cf, bd, bd, seed=50 + cf)
        check_pair(ctx, geom, a, b, rect=RECT, what="rectangle")
    for bd in (8, 10):                      # rows shorter than one lane's vector
        geom = (16, 8, 1, bd, bd)
        check_pair(ctx, geom, make_planes(16, 8, 1, bd, bd, seed=60), make_planes(16, 8, 1, bd, bd, seed=61), rect=(6, 4, 2, 2), what="2x2")


def check_pinned_reference(ctx):
    geom = (1032, 16, 1, 8, 8)
    check_pair(ctx, geom, make_planes(*geom, seed=70), make_planes(*geom, seed=71), against_frame=False, host=True, what="pinned host reference")


# ---- ranges ----
def check_extremes(ctx, w, h, bd):
    """all (1 << bd) - 1 against all 0 and the reverse, monochrome: the largest difference everywhere"""
    top = (1 << bd) - 1
    dt = np.uint8 if bd <= 8 else np.uint16
    hi, lo = [np.full((h, w), top, dt)], [np.zeros((h, w), dt)]
    # (the direction exercises the arithmetic, the kind of reference the addressing: the tall shape takes one kind per direction)
    for a, b, memory in ((hi, lo, True), (lo, hi, False)):
        want = check_pair(ctx, (w, h, 0, bd, bd), a, b, against_memory=memory or h < 1000, against_frame=not memory or h < 1000, what="extremes")
        assert want[0]["ssd"] == w * h * top * top and want[0]["sad"] == w * h * top and want[0]["max_abs"] == top and want[0]["first"] == (0, 0)


def check_ramps(ctx):
    for bd in (12, 16):
        ramp = (np.arange(128 * 32, dtype=np.uint32) * ((1 << bd) - 1) // (128 * 32 - 1)).astype(np.uint16).reshape(32, 128)
        a = [ramp, ramp[::-1].copy(), ramp[:, ::-1].copy()]
        b = [p[::-1, ::-1].copy() for p in a]
        want = check_pair(ctx, (128, 32, 3, bd, bd), a, b, what="ramp %d" % bd)
        assert want[0]["max_abs"] == (1 << bd) - 1


# ---- first difference and counts ----
def check_first_and_counts(ctx):
    geom = (64, 32, 1, 8, 8)
    base = make_planes(*geom, seed=90)

    def changed(*edits):
        out = [p.copy() for p in base]
        for c, x, y in edits:
            out[c][y, x] ^= 0x15
        return out

    want = check_pair(ctx, geom, base, changed(), what="identical")
    assert all(w == dict(ssd=0, sad=0, n_diff=0, max_abs=0, first=None, mse=0.0) for w in want)
    assert check_pair(ctx, geom, base, changed((0, 0, 0)), what="first sample")[0]["first"] == (0, 0)
    want = check_pair(ctx, geom, base, changed((0, 63, 31), (1, 31, 15), (2, 31, 15)), what="last sample of the last row")
    assert [w["first"] for w in want] == [(63, 31), (31, 15), (31, 15)] and [w["n_diff"] for w in want] == [1, 1, 1]
    want = check_pair(ctx, geom, base, changed((0, 55, 23), (1, 27, 11)), rect=RECT, what="last sample of the rectangle")
    assert [w["first"] for w in want] == [(55, 23), (27, 11), None]
    # the raster-first one has the larger x and lies in an earlier row (another wavefront's span)
    want = check_pair(ctx, geom, base, changed((0, 50, 3), (0, 2, 20)), what="two samples")
    assert want[0]["first"] == (50, 3) and want[0]["n_diff"] == 2
    want = check_pair(ctx, geom, base, changed((2, 9, 7)), what="Cr only")
    assert [w["n_diff"] for w in want] == [0, 0, 1] and want[2]["first"] == (9, 7)
    # just outside the rectangle (6, 2, 50, 22) on each side, luma and chroma: not seen
    outside = changed((0, 5, 10), (0, 56, 10), (0, 20, 1), (0, 20, 24), (1, 2, 5), (1, 28, 5), (2, 10, 0), (2, 10, 12))
    want = check_pair(ctx, geom, base, outside, rect=RECT, what="outside the rectangle")
    assert all(w["n_diff"] == 0 and w["first"] is None for w in want)
    assert [w["n_diff"] for w in check_pair(ctx, geom, base, outside, what="the same, whole frame")] == [4, 2, 2]


# ---- the request as a reader of its frames ----
def _upload_refs(ctx, pic, refs):
    handles = []
    for planes in refs:
        f = ctx.frame_create_for(pic.pp[0])
        ctx.frame_upload(f, planes)
        handles.append(f)
    pic.ref_frames = [handles[i] if i < len(handles) else -1 for i in range(worklist.MAX_REF_FRAMES)]


def check_reader_hazard(lib, oracle, depth, as_ref_frame, with_others):
    """decode A into F, request on F (or on G with F as ref_frame), [export F, hash F,] decode B into F — nothing waited for in between:
    the values are A's.  The other side holds picture B, so a request that saw B in F would report no difference."""
    o = Oracle(oracle)
    (pa, ra), (pb, rb) = make_case(**PIC_A), make_case(**PIC_B)
    want_a, want_b = oracle_decode(o, pa, ra), oracle_decode(o, pb, rb)
    want = expected(want_a, want_b, None, 1)
    assert all(w["n_diff"] for w in want), "the two pictures must differ"
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
        tk = ctx.frame_measure_async(G, ref_frame=F) if as_ref_frame else ctx.frame_measure_async(F, ref_planes=in_memory)
        token = ctx.frame_export(F, capi.EXPORT_PLANAR, capi.EXPORT_NATIVE, host=True) if with_others else None
        htk = ctx.frame_hash_async(F, CRC) if with_others else None
        ctx.submit(pb)
        # ---- ... to here
        got = ctx.frame_measure_result(tk)
        if as_ref_frame:                                            # (a - b with the sides swapped: the same magnitudes)
            assert_result(got, expected(want_b, want_a, None, 1), "F as ref_frame, depth %d" % depth)
        else:
            assert_result(got, want, "request on F, depth %d" % depth)
        if with_others:
            assert_planes_equal(ctx.frame_export_finish(token), want_a, "export between the request and the next decode")
            hash_a = ctx.frame_hash_result(htk)
        ctx.wait()
        assert_planes_equal(ctx.frame_download(F), want_b, "the later picture")
        if with_others:
            assert hash_a != ctx.frame_hash(F, CRC)
        assert_result(ctx.frame_measure_result(ctx.frame_measure_async(F, ref_frame=G)), expected(want_b, want_b, None, 1), "the later picture against itself")
    finally:
        ctx.close()


def check_two_writers(lib, oracle, depth=3):
    """the frame and its ref_frame written by decodes on DIFFERENT lanes, nothing waited for: D into G, D into H, C into F (three lanes), then a
    request on G and one on H, both with ref_frame = F, then D into F.  The requests run on the streams of G's and H's writers, not of F's:
    what orders them behind the decode of C is the wait for the reference frame's last writer, and what keeps the second decode into F
    behind BOTH requests is that the second one — on another stream — continued behind the first one's mark on F before it replaced it.
    F is zero before C, so a request that ran early reports other values."""
    o = Oracle(oracle)
    (pc, rc_), (pd, rd) = make_case(**PIC_C), make_case(**PIC_D)
    want_c, want_d = oracle_decode(o, pc, rc_), oracle_decode(o, pd, rd)
    want = expected(want_d, want_c, None, 1)
    assert all(w["n_diff"] for w in want), "the two pictures must differ"
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
        tk_g = ctx.frame_measure_async(G, ref_frame=F)
        tk_h = ctx.frame_measure_async(H, ref_frame=F)
        pd.dst_frame = F
        ctx.submit(pd)
        # ---- ... to here
        assert_result(ctx.frame_measure_result(tk_g), want, "G against F, written on another lane (depth %d)" % depth)
        assert_result(ctx.frame_measure_result(tk_h), want, "H against F, behind the first request's mark (depth %d)" % depth)
        ctx.wait()
        assert_planes_equal(ctx.frame_download(F), want_d, "the later picture")
    finally:
        ctx.close()


def check_rejected_ref_frame_other_lane(lib, oracle, depth=3):
    """the gate of ref_frame when the two frames were written on different lanes: an accepted decode into G on one lane, a rejected one into F
    on the next, a request on G with ref_frame = F — it runs on G's writer's stream and must carry F's decode's verdict"""
    pic, refs = make_case(**REJECT_CASE)
    want = oracle_decode(Oracle(oracle), pic, refs)
    ctx = capi.Context(lib, 0)
    try:
        _upload_refs(ctx, pic, refs)
        ctx.set_pipeline_depth(depth)
        F, G = ctx.frame_create_for(pic.pp[0]), ctx.frame_create_for(pic.pp[0])
        ctx.frame_fill(F, 77, 99)
        bad = make_case(**REJECT_CASE)[0]
        bad.ref_frames = pic.ref_frames
        arr = bad.tus.copy()
        arr["log2_size"][len(arr) // 2] = 9
        bad.tus = arr
        good_state, bad_state = {}, {}
        pic.dst_frame = G
        ctx.submit_in_place(pic, fill_threads=1, state=good_state)
        bad.dst_frame = F
        ctx.submit_in_place(bad, fill_threads=1, state=bad_state)
        serial = ctx.last_serial()
        tk = ctx.frame_measure_async(G, ref_frame=F)
        with pytest.raises(capi.M355Error) as e:
            ctx.frame_measure_result(tk)
        assert e.value.code == INVALID and "rejected" in str(e.value)
        st = ctx.decode_status(serial)                              # (reported here, so that m355_wait stays quiet)
        while st == BUSY:
            st = ctx.decode_status(serial)
        assert st == INVALID
        # an accepted decode into F on yet another lane, and the request has a value again
        pic.dst_frame = F
        ctx.submit_in_place(pic, fill_threads=1, state=good_state)
        tk = ctx.frame_measure_async(G, ref_frame=F)
        assert_result(ctx.frame_measure_result(tk), expected(want, want, None, 1), "behind an accepted decode into F")
        ctx.wait()
    finally:
        ctx.close()


# ---- slots and tickets ----
def check_concurrency(lib):
    """16 requests on 16 frames before any is collected, collected in reverse; the 17th is refused; a collected slot is free again"""
    ctx = capi.Context(lib, 0)
    try:
        frames, refs, want = [], [], []
        for i in range(SLOTS):
            w, h, cf, bd = [(64, 48, 1, 8), (72, 40, 0, 8), (136, 72, 2, 10), (264, 16, 3, 12)][i % 4]
            a, b = make_planes(w, h, cf, bd, bd, seed=900 + i), make_planes(w, h, cf, bd, bd, seed=950 + i)
            frames.append(frame_with(ctx, (w, h, cf, bd, bd), a))
            refs.append(frame_with(ctx, (w, h, cf, bd, bd), b) if i % 2 else ctx.measure_reference(b))
            want.append(expected(a, b, None, cf))
        tickets = [ctx.frame_measure_async(f, ref_frame=r) if i % 2 else ctx.frame_measure_async(f, ref_planes=r) for i, (f, r) in enumerate(zip(frames, refs))]
        assert tickets == list(range(1, SLOTS + 1)), "tickets count 1, 2, ... per context"
        with pytest.raises(capi.M355Error) as e:
            ctx.frame_measure_async(frames[0], ref_frame=frames[0])
        assert e.value.code == BUSY
        assert_result(ctx.frame_measure_result(tickets[-1]), want[-1], "the last request")
        extra = ctx.frame_measure_async(frames[3], ref_frame=refs[3])       # the refused call took no ticket and enqueued nothing
        assert extra == SLOTS + 1
        assert_result(ctx.frame_measure_result(extra), want[3], "the slot collected first, reused")
        for i in reversed(range(SLOTS - 1)):
            assert_result(ctx.frame_measure_result(tickets[i]), want[i], "request %d" % i)
    finally:
        ctx.close()


def check_nonblocking(lib):
    ctx = capi.Context(lib, 0)
    try:
        geom = (200, 120, 1, 8, 8)
        a, b = make_planes(*geom, seed=5), make_planes(*geom, seed=6)
        fa, fb = frame_with(ctx, geom, a), frame_with(ctx, geom, b)
        for k in range(3):
            tk = ctx.frame_measure_async(fa, ref_frame=fb)
            assert tk == k + 1
            got = ctx.frame_measure_result(tk, block=False)
            while got is None:                                      # BUSY: nothing was waited for, the request stays
                got = ctx.frame_measure_result(tk, block=False)
            assert_result(got, expected(a, b, None, 1), "non-blocking collection")
            for bad in (tk, tk + 1000, 0):                          # collected / unknown
                with pytest.raises(capi.M355Error) as e:
                    ctx.frame_measure_result(bad, block=False)
                assert e.value.code == INVALID
        # m355_wait completes a request and does not collect it; a frame may be destroyed with a request pending
        tk = ctx.frame_measure_async(fa, ref_frame=fb)
        ctx.wait()
        tk2 = ctx.frame_measure_async(fb, ref_frame=fa)
        ctx.frame_destroy(fa)
        assert_result(ctx.frame_measure_result(tk, block=False), expected(a, b, None, 1), "collected behind m355_wait")
        assert_result(ctx.frame_measure_result(tk2), expected(b, a, None, 1), "collected behind the frame's destruction")
    finally:
        ctx.close()


def check_slot_reuse(ctx, rounds=40):
    """one slot, request after request, alternately "no difference" and "differs", 8 and 10 bit: a device record not left zero shows in the next result"""
    cases = []
    for geom in ((72, 40, 1, 8, 8), (136, 24, 2, 10, 9)):
        a, b = make_planes(*geom, seed=77), make_planes(*geom, seed=78)
        cases.append((frame_with(ctx, geom, a), frame_with(ctx, geom, b), frame_with(ctx, geom, a), expected(a, b, None, geom[2]), expected(a, a, None, geom[2])))
    try:
        for k in range(rounds):
            fa, fb, fa2, differs, same = cases[(k // 2) % 2]
            tk = ctx.frame_measure_async(fa, ref_frame=fb if k % 2 else fa2)
            assert_result(ctx.frame_measure_result(tk), differs if k % 2 else same, "round %d" % k)
    finally:
        for case in cases:
            for f in case[:3]:
                ctx.frame_destroy(f)


def check_rejected_decode(lib, oracle, depth):
    """a request behind a decode whose lists the device rejected — into the frame, or into its ref_frame — has no value and has read nothing;
    the slot it used is clean for the next request"""
    pic, refs = make_case(**REJECT_CASE)
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
        for as_ref_frame in (False, True):
            bad.dst_frame = d
            ctx.submit_in_place(bad, fill_threads=1)
            serial = ctx.last_serial()
            tk = ctx.frame_measure_async(other, ref_frame=d) if as_ref_frame else ctx.frame_measure_async(d, ref_frame=other)
            with pytest.raises(capi.M355Error) as e:
                ctx.frame_measure_result(tk)
            assert e.value.code == INVALID and "rejected" in str(e.value)
            st = ctx.decode_status(serial)                          # (reported here, so that m355_wait stays quiet)
            while st == BUSY:
                st = ctx.decode_status(serial)
            assert st == INVALID
            with pytest.raises(capi.M355Error):                     # the failed collection freed the ticket
                ctx.frame_measure_result(tk)
            pic.dst_frame = d
            ctx.submit_in_place(pic, fill_threads=1)
            tk = ctx.frame_measure_async(other, ref_frame=d) if as_ref_frame else ctx.frame_measure_async(d, ref_frame=other)
            w = expected(filled, want, None, 1) if as_ref_frame else expected(want, filled, None, 1)
            assert_result(ctx.frame_measure_result(tk), w, "in the slot a gated request left (ref_frame: %s)" % as_ref_frame)
        ctx.wait()
    finally:
        ctx.close()


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
        small = ctx.frame_create(32, 32, 1, 8, 8)
        assert ctx.frame_measure_async(f8, ref_frame=f8) == 1
        tk = ctypes.c_ulonglong(0)
        mem = ctx.device_alloc(3 * 40 * 80)

        def desc(ref_frame=-1, rect=None, ref=(mem, mem, mem), pitch=(80, 80, 80)):
            d = capi.MeasureDesc(ref_frame=ref_frame)
            if rect:
                d.x0, d.y0, d.width, d.height = rect
            for k in range(3):
                d.ref[k] = ref[k]; d.pitch[k] = pitch[k]
            return d

        def refused(frame, d, what):
            rc = L.m355_frame_measure_async(ctx.h, frame, d, tk)
            assert rc == INVALID, "%s: returned %d" % (what, rc)

        refused(f8 + 99, ctypes.byref(desc()), "bad frame handle")
        refused(-1, ctypes.byref(desc()), "negative frame handle")
        refused(f8, None, "null descriptor")
        assert L.m355_frame_measure_async(ctx.h, f8, ctypes.byref(desc()), None) == INVALID, "null ticket"
        for rect in ((60, 0, 8, 8), (0, 30, 8, 4), (-2, 0, 8, 8), (0, -2, 8, 8), (0, 0, 8, -2), (0, 0, -8, 2), (0, 0, 66, 32), (0, 0, 8, 0)):
            refused(f8, ctypes.byref(desc(rect=rect)), "rectangle %s leaves the frame" % (rect,))
        for rect in ((1, 0, 8, 8), (0, 1, 8, 8), (0, 0, 7, 8), (0, 0, 8, 7)):
            refused(f8, ctypes.byref(desc(rect=rect)), "rectangle %s off the 4:2:0 chroma grid" % (rect,))
        refused(f422, ctypes.byref(desc(rect=(1, 0, 8, 8))), "4:2:2: odd x0")
        assert L.m355_frame_measure_async(ctx.h, f422, ctypes.byref(desc(rect=(0, 1, 8, 7))), tk) == 0 and tk.value == 2, "4:2:2 has no vertical grid"
        for r, what in ((f8 + 99, "unknown ref_frame"), (-2, "ref_frame -2"), (f10, "other bit depths"), (f422, "other chroma format")):
            refused(f8, ctypes.byref(desc(ref_frame=r)), what)
        refused(f10, ctypes.byref(desc(ref_frame=f9)), "other chroma bit depth")
        refused(f10, ctypes.byref(desc(ref_frame=f8)), "other element size")
        refused(f8, ctypes.byref(desc(ref_frame=small)), "ref_frame smaller than the whole frame")
        refused(f8, ctypes.byref(desc(ref_frame=small, rect=(16, 0, 32, 32))), "ref_frame does not contain the rectangle")
        assert L.m355_frame_measure_async(ctx.h, f8, ctypes.byref(desc(ref_frame=small, rect=(0, 0, 32, 32))), tk) == 0 and tk.value == 3
        for p in range(3):
            ref = [mem] * 3; ref[p] = None
            refused(f8, ctypes.byref(desc(ref=ref)), "null ref[%d]" % p)
            pitch = [80] * 3; pitch[p] = 63 if p == 0 else 31
            refused(f8, ctypes.byref(desc(pitch=pitch)), "pitch of plane %d below the row" % p)
            pitch = [160] * 3; pitch[p] = 161
            refused(f10, ctypes.byref(desc(pitch=pitch)), "odd pitch of 16-bit plane %d" % p)
            ref = [mem] * 3; ref[p] = mem + 1
            refused(f10, ctypes.byref(desc(ref=ref, rect=(0, 0, 16, 8), pitch=(160, 160, 160))), "odd pointer of 16-bit plane %d" % p)
        assert L.m355_frame_measure_async(ctx.h, f8, ctypes.byref(desc(ref=(mem + 1, mem + 3, mem + 5), pitch=(65, 33, 33))), tk) == 0 and tk.value == 4, "8-bit planes: any pointer, any pitch"
        shard.shard_set(0, 2)
        fs = shard.frame_create(64, 32, 1, 8, 8)
        assert L.m355_frame_measure_async(shard.h, fs, ctypes.byref(desc(ref_frame=fs)), tk) == INVALID, "tile-sharded context"
        out = capi.Measure()
        assert L.m355_frame_measure_result(ctx.h, 1, 1, None) == INVALID, "null result"
        for t in (1, 2, 3, 4):
            assert L.m355_frame_measure_result(ctx.h, t, 1, ctypes.byref(out)) == 0
        assert L.m355_frame_measure_result(ctx.h, 5, 1, ctypes.byref(out)) == INVALID
        ctx.device_free(mem)
    finally:
        shard.close()
        ctx.close()


# ---- a decoded picture ----
def check_decoded_picture(lib):
    """one girlshy picture measured behind its decode with three pictures in flight: against the planes an earlier decode of it delivered (no
    difference) and against a copy of them with three samples changed"""
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
        tickets = [c.frame_measure_async(dst, ref_planes=same), c.frame_measure_async(dst, ref_planes=changed), c.frame_measure_async(dst, ref_frame=first)]
        assert_result(c.frame_measure_result(tickets[0]), expected(planes, planes, None, 1), "against its own planes")
        want = expected(planes, other, None, 1)
        assert [w["n_diff"] for w in want] == [2, 0, 1] and want[0]["first"] == (17, 5)
        assert_result(c.frame_measure_result(tickets[1]), want, "against the changed copy")
        assert_result(c.frame_measure_result(tickets[2]), expected(planes, planes, None, 1), "against the earlier decode's frame")
    finally:
        c.close()
