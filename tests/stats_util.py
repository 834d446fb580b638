"""Scenarios of the statistics-request tests (m355_frame_stats_async / m355_frame_stats_result), shared by the CPU tier (SIMT-interpreter build,
tests/test_stats_emu.py) and the GPU tier (tests/test_gpu_stats.py), and the numpy restatement their expected values come from: per plane the
256-bin histogram of s >> (bit depth - 8), min, max, sum and sum of squares in int64; the box of the luma samples above `black`; and the light level
m = max(R, G, B) of the 16-bit R'G'B' that the restatements of the R'G'B' export (tests/export_rgb_util.py, tests/export_siting_util.py) expect for
the WHOLE frame, cut to the rectangle.  Every comparison is exact."""
import ctypes

import numpy as np
import pytest

import measure_util as mu
from export_rgb_util import expected_rgb
from export_siting_util import expected_rgb_sited
from hash_util import CRC, make_planes
from oracle_py import Oracle
from synth_util import assert_planes_equal, make_case, oracle_decode
from libde265_amd import capi

BUSY, INVALID = 6, 3                # M355_ERR_BUSY, M355_ERR_INVALID
SLOTS = 16                          # M355_STATS_REQUESTS
SHAPES = mu.SHAPES                  # the smallest shapes at which the span / tail code can go wrong: measure_util states why
RECT = mu.RECT                      # (6, 2, 50, 22) on 64x32
CONVERSIONS = tuple((m, r) for m in (capi.MATRIX_BT601, capi.MATRIX_BT709, capi.MATRIX_BT2020) for r in (0, 1))


def dtype_of(bd):
    return np.uint8 if bd <= 8 else np.uint16


def plane_stats(p, bd):
    s = p.astype(np.int64).ravel()
    return dict(hist=[int(v) for v in np.bincount(s >> (bd - 8), minlength=256)], min=int(s.min()), max=int(s.max()), sum=int(s.sum()), sum_sq=int((s * s).sum()))


def light_values(planes, geom, matrix, full_range, chroma_loc):
    """m = max(R, G, B) of the 16-bit R'G'B' of the WHOLE frame -> int64 (H, W)"""
    w, h, cf, bdl, bdc = geom
    if cf == 1:
        rgb = expected_rgb_sited(planes, bdl, bdc, capi.RGB_PLANAR, capi.RGB_U16, matrix, full_range, chroma_loc)
    else:
        assert chroma_loc == 0
        rgb = expected_rgb(planes, cf, bdl, bdc, capi.RGB_PLANAR, capi.RGB_U16, matrix, full_range)
    return np.maximum(np.maximum(rgb[0], rgb[1]), rgb[2]).astype(np.int64)


def light_stats(m):
    m = m.ravel()
    return dict(hist=[int(v) for v in np.bincount(m >> 8, minlength=256)], min=int(m.min()), max=int(m.max()), sum=int(m.sum()))


def expected(planes, geom, rect=None, black=0, light=None):
    """what a request on a frame holding `planes` delivers; light = None or (matrix, full_range, chroma_loc)"""
    w, h, cf, bdl, bdc = geom
    x0, y0, rw, rh = rect if rect is not None else (0, 0, w, h)
    cut = mu.crop(planes, rect, cf)
    above = np.argwhere(cut[0].astype(np.int64) > black)
    box = None if not len(above) else (x0 + int(above[:, 1].min()), y0 + int(above[:, 0].min()), x0 + int(above[:, 1].max()), y0 + int(above[:, 0].max()))
    lt = None
    if light is not None:
        lt = light_stats(light_values(planes, geom, *light)[y0:y0 + rh, x0:x0 + rw])
    return dict(planes=[plane_stats(p, bdc if c else bdl) for c, p in enumerate(cut)], box=box, n_active=int(len(above)), light=lt)


def assert_stats(got, want, what=""):
    assert len(got["planes"]) == len(want["planes"]), what
    for c, (g, w) in enumerate(zip(got["planes"], want["planes"])):
        for k in ("min", "max", "sum", "sum_sq", "hist"):
            assert g[k] == w[k], "%s: plane %d: %s is %r, expected %r" % (what, c, k, g[k], w[k])
    assert got["box"] == want["box"] and got["n_active"] == want["n_active"], "%s: box %r with %d samples, expected %r with %d" % (
        what, got["box"], got["n_active"], want["box"], want["n_active"])
    assert (got["light"] is None) == (want["light"] is None), what
    if want["light"] is not None:
        for k in ("min", "max", "sum", "hist"):
            assert got["light"][k] == want["light"][k], "%s: light %s is %r, expected %r" % (what, k, got["light"][k], want["light"][k])


def request(ctx, f, rect=None, black=0, light=None):
    m, r, loc = light if light is not None else (0, 0, 0)
    return ctx.frame_stats_async(f, rect=rect, black=black, light=light is not None, matrix=m, full_range=r, chroma_loc=loc)


def check(ctx, geom, planes, rect=None, black=0, light=None, what=""):
    want = expected(planes, geom, rect, black, light)
    f = mu.frame_with(ctx, geom, planes)
    try:
        assert_stats(ctx.frame_stats_result(request(ctx, f, rect, black, light)), want, "%s %s rect %s black %d light %s" % (what, geom, rect, black, light))
    finally:
        ctx.frame_destroy(f)
    return want


# ---- values ----
def check_values(ctx, geom):
    w, h, cf, bdl, bdc = geom
    check(ctx, geom, make_planes(w, h, cf, bdl, bdc, seed=w + 7 * h + cf), black=1 << (bdl - 2), what="values")


def check_extremes(ctx, w, h, bd):
    """every sample (1 << bd) - 1, monochrome: bin 255 alone; at 16 bit the sum of squares of ONE ROW leaves 32 bits"""
    top = (1 << bd) - 1
    want = check(ctx, (w, h, 0, bd, bd), [np.full((h, w), top, dtype_of(bd))], black=top - 1, what="extremes")
    p = want["planes"][0]
    assert p["hist"][255] == w * h and sum(p["hist"]) == w * h and p["min"] == p["max"] == top and p["sum_sq"] == w * h * top * top
    assert bd < 16 or w * top * top >= 1 << 32
    assert want["box"] == (0, 0, w - 1, h - 1) and want["n_active"] == w * h


def check_plane_depths(ctx):
    """the bin shift is the PLANE's: 4:0:0 at 12 bit, and luma 12 / chroma 10"""
    check(ctx, (64, 32, 0, 12, 12), make_planes(64, 32, 0, 12, 12, seed=21), what="4:0:0")
    planes = make_planes(64, 32, 1, 12, 10, seed=22)
    want = check(ctx, (64, 32, 1, 12, 10), planes, what="12 / 10 bit")
    assert want["planes"][1]["hist"] != plane_stats(planes[1], 12)["hist"]


def content_cases(w, h, cf, bd):
    """-> [(name, planes)]: a constant frame, all zero, a ramp that hits every bin equally, and 0 / maximum in alternating lanes (16-byte vectors)"""
    dt, top, (sw, sh) = dtype_of(bd), (1 << bd) - 1, mu.sub_sampling(cf)
    shapes = [(h, w)] + ([(h // sh, w // sw)] * 2 if cf else [])
    per_lane = 16 // np.dtype(dt).itemsize
    out = [("constant", [np.full(s, v, dt) for s, v in zip(shapes, (37 << (bd - 8), 1 << (bd - 1), top))]), ("zero", [np.zeros(s, dt) for s in shapes])]
    out.append(("ramp", [(((np.arange(s[0] * s[1], dtype=np.int64) * 256) // (s[0] * s[1])) << (bd - 8)).astype(dt).reshape(s) for s in shapes]))
    out.append(("alternating lanes", [np.broadcast_to(np.where((np.arange(s[1]) // per_lane) % 2, top, 0).astype(dt), s).copy() for s in shapes]))
    return out


def check_content(ctx):
    for geom in ((1032, 16, 1, 8, 8), (520, 16, 1, 10, 10), (1024, 16, 0, 12, 12)):
        w, h, cf, bd, _ = geom
        for name, planes in content_cases(w, h, cf, bd):
            want = check(ctx, geom, planes, what=name)
            for c, p in enumerate(want["planes"]):
                n = planes[c].size
                if name in ("constant", "zero"):
                    assert max(p["hist"]) == n and p["min"] == p["max"]
                if name == "ramp" and n % 256 == 0:
                    assert p["hist"] == [n // 256] * 256
                if name == "alternating lanes":
                    assert p["hist"][0] + p["hist"][255] == n and p["hist"][0] and p["hist"][255]
            if name == "zero":
                assert want["box"] is None and want["n_active"] == 0


# ---- rectangles ----
def check_rectangles(ctx):
    for cf, bd in ((1, 8), (2, 10), (3, 8), (0, 12)):
        geom = (64, 32, cf, bd, bd)
        planes = make_planes(64, 32, cf, bd, bd, seed=40 + cf)
        check(ctx, geom, planes, rect=RECT, black=1 << (bd - 1), what="rectangle")
        # light: the rectangle's values are the whole frame's, cut — its rim reads chroma outside the rectangle
        light = (capi.MATRIX_BT709, 0, 0)
        want = check(ctx, geom, planes, rect=RECT, light=light, what="rectangle, light")
        if cf in (1, 2):
            inside = [np.ascontiguousarray(p) for p in mu.crop(planes, RECT, cf)]
            alone = light_stats(light_values(inside, (RECT[2], RECT[3], cf, bd, bd), *light))
            assert alone["hist"] != want["light"]["hist"], "the rim of the rectangle must depend on chroma outside it for this case to see the clamp"
    for bd in (8, 10):                      # rows shorter than one lane's vector
        geom = (16, 8, 1, bd, bd)
        planes = make_planes(16, 8, 1, bd, bd, seed=60)
        check(ctx, geom, planes, rect=(6, 4, 2, 2), what="2x2")
        check(ctx, geom, planes, rect=(6, 4, 2, 2), light=(capi.MATRIX_BT601, 1, 1), what="2x2, light")


# ---- active area ----
def check_active_area(ctx):
    geom, black = (64, 32, 1, 8, 8), 20
    base = [np.full((32, 64), black, np.uint8), np.full((16, 32), 128, np.uint8), np.full((16, 32), 128, np.uint8)]

    def with_luma(fill):
        out = [p.copy() for p in base]
        fill(out[0])
        return out

    def content(y):
        y[4:20, 10:42] = 200

    want = check(ctx, geom, with_luma(content), black=black, what="content")
    assert want["box"] == (10, 4, 41, 19) and want["n_active"] == 32 * 16
    want = check(ctx, geom, base, black=black, what="samples equal to black do not count")
    assert want["box"] is None and want["n_active"] == 0
    want = check(ctx, geom, base, black=black - 1, what="one below the threshold: everything counts")
    assert want["box"] == (0, 0, 63, 31)

    def first(y):
        y[0, 0] = black + 1

    def last(y):
        y[31, 63] = black + 1

    assert check(ctx, geom, with_luma(first), black=black, what="sample (0, 0)")["box"] == (0, 0, 0, 0)
    assert check(ctx, geom, with_luma(last), black=black, what="the last sample")["box"] == (63, 31, 63, 31)
    want = check(ctx, geom, with_luma(content), rect=(20, 8, 44, 24), black=black, what="a rectangle that cuts the content")
    assert want["box"] == (20, 8, 41, 19)
    want = check(ctx, geom, with_luma(content), rect=RECT, black=black, what="the box is in frame coordinates")
    assert want["box"] == (10, 4, 41, 19)
    want = check(ctx, geom, with_luma(content), rect=(44, 0, 20, 32), black=black, what="a rectangle beside the content")
    assert want["box"] is None


# ---- light ----
def check_light_conversions(ctx):
    geom = (64, 16, 1, 10, 10)
    planes = make_planes(*geom, seed=81)
    seen = set()
    for matrix, full in CONVERSIONS:
        want = check(ctx, geom, planes, light=(matrix, full, 0), what="conversion")
        seen.add(tuple(want["light"]["hist"]))
    assert len(seen) == len(CONVERSIONS), "the six conversions must expect six histograms"


def check_light_siting(ctx, geom):
    planes = make_planes(*geom, seed=82 + geom[0])
    seen = set()
    for loc in range(4):
        want = check(ctx, geom, planes, light=(capi.MATRIX_BT2020, 0, loc), what="siting")
        seen.add(want["light"]["sum"])
    assert len(seen) == 4, "the four sitings must expect four sums"


def check_light_formats(ctx):
    for cf, bd in ((2, 10), (3, 8), (0, 12)):
        geom = (72, 16, cf, bd, bd)
        check(ctx, geom, make_planes(*geom, seed=83 + cf), light=(capi.MATRIX_BT709, 1, 0), what="chroma format")


def check_light_clips(ctx):
    """limited range, neutral chroma: luma 0 lies below black — R = G = B clip at 0 —, the largest luma above white: they clip at 65535"""
    for bd in (8, 10):
        geom, top = (64, 16, 3, bd, bd), (1 << bd) - 1
        y = np.zeros((16, 64), dtype_of(bd))
        y[:, 32:] = top
        planes = [y, np.full((16, 64), 1 << (bd - 1), dtype_of(bd)), np.full((16, 64), 1 << (bd - 1), dtype_of(bd))]
        want = check(ctx, geom, planes, light=(capi.MATRIX_BT709, 0, 0), what="clips")
        lt = want["light"]
        assert lt["min"] == 0 and lt["max"] == 65535 and lt["hist"][0] == 512 and lt["hist"][255] == 512 and lt["sum"] == 512 * 65535


def check_light_against_export(ctx):
    """the composition on the device itself: the light values are those of the frame's own m355_frame_export_rgb_opts, U16, with the same siting"""
    geom = (1032, 16, 1, 8, 8)
    planes = make_planes(*geom, seed=84)
    f = mu.frame_with(ctx, geom, planes)
    try:
        for loc, rect in ((2, None), (1, (6, 2, 1000, 12))):
            rgb = ctx.frame_export_finish(ctx.frame_export_rgb(f, capi.RGB_PLANAR, capi.RGB_U16, capi.MATRIX_BT2020, 0, rect, chroma_loc=loc))
            want = light_stats(np.maximum(np.maximum(rgb[0], rgb[1]), rgb[2]).astype(np.int64))
            got = ctx.frame_stats_result(request(ctx, f, rect, 0, (capi.MATRIX_BT2020, 0, loc)))
            assert got["light"] == want, "type %d rect %s" % (loc, rect)
    finally:
        ctx.frame_destroy(f)


# ---- the request as a reader of its frame ----
def check_reader_hazard(lib, oracle, depth, with_others):
    """decode A into F, request on F, [hash F, measure F,] decode B into F — nothing waited for in between: the values are A's"""
    o = Oracle(oracle)
    (pa, ra), (pb, rb) = make_case(**mu.PIC_A), make_case(**mu.PIC_B)
    want_a, want_b = oracle_decode(o, pa, ra), oracle_decode(o, pb, rb)
    geom, light = (64, 64, 1, 8, 8), (capi.MATRIX_BT709, 0, 0)
    wa, wb = expected(want_a, geom, black=60, light=light), expected(want_b, geom, black=60, light=light)
    assert wa["planes"][0]["sum"] != wb["planes"][0]["sum"] and wa["light"]["sum"] != wb["light"]["sum"], "the two pictures must differ"
    ctx = capi.Context(lib, 0)
    try:
        mu._upload_refs(ctx, pa, ra)
        mu._upload_refs(ctx, pb, rb)
        F = ctx.frame_create_for(pa.pp[0])
        G = ctx.frame_create_for(pa.pp[0])
        ctx.frame_upload(G, want_b)
        ctx.set_pipeline_depth(depth)
        ctx.wait()
        # ---- no host wait from here ...
        pa.dst_frame = pb.dst_frame = F
        ctx.submit(pa)
        tk = request(ctx, F, None, 60, light)
        htk = ctx.frame_hash_async(F, CRC) if with_others else None
        mtk = ctx.frame_measure_async(F, ref_frame=G) if with_others else None
        ctx.submit(pb)
        # ---- ... to here
        assert_stats(ctx.frame_stats_result(tk), wa, "request on F, depth %d" % depth)
        if with_others:
            hash_a = ctx.frame_hash_result(htk)
            mu.assert_result(ctx.frame_measure_result(mtk), mu.expected(want_a, want_b, None, 1), "the comparison pending beside it")
        ctx.wait()
        assert_planes_equal(ctx.frame_download(F), want_b, "the later picture")
        if with_others:
            assert hash_a != ctx.frame_hash(F, CRC)
        assert_stats(ctx.frame_stats_result(request(ctx, F, None, 60, light)), wb, "the later picture")
    finally:
        ctx.close()


def check_rejected_decode(lib, oracle, depth):
    """a request behind a decode whose lists the device rejected has no value and has read nothing; the slot it used is clean for the next request"""
    pic, refs = make_case(**mu.REJECT_CASE)
    want = oracle_decode(Oracle(oracle), pic, refs)
    geom = (256, 192, 1, 8, 8)
    ctx = capi.Context(lib, 0)
    try:
        mu._upload_refs(ctx, pic, refs)
        ctx.set_pipeline_depth(depth)
        d = ctx.frame_create_for(pic.pp[0])
        ctx.frame_fill(d, 77, 99)
        bad = make_case(**mu.REJECT_CASE)[0]
        bad.ref_frames = pic.ref_frames
        arr = bad.tus.copy()
        arr["log2_size"][len(arr) // 2] = 9
        bad.tus = arr
        for light in (None, (capi.MATRIX_BT601, 1, 3)):
            bad.dst_frame = d
            ctx.submit_in_place(bad, fill_threads=1)
            serial = ctx.last_serial()
            tk = request(ctx, d, None, 0, light)
            with pytest.raises(capi.M355Error) as e:
                ctx.frame_stats_result(tk)
            assert e.value.code == INVALID and "rejected" in str(e.value)
            st = ctx.decode_status(serial)                          # (reported here, so that m355_wait stays quiet)
            while st == BUSY:
                st = ctx.decode_status(serial)
            assert st == INVALID
            with pytest.raises(capi.M355Error):                     # the failed collection freed the ticket
                ctx.frame_stats_result(tk)
            pic.dst_frame = d
            ctx.submit_in_place(pic, fill_threads=1)
            assert_stats(ctx.frame_stats_result(request(ctx, d, None, 30, light)), expected(want, geom, black=30, light=light), "in the slot a gated request left")
        ctx.wait()
    finally:
        ctx.close()


# ---- slots and tickets ----
def check_concurrency(lib):
    """16 requests on 16 frames before any is collected, collected in reverse; the 17th is refused; a collected slot is free again"""
    ctx = capi.Context(lib, 0)
    try:
        frames, want, args = [], [], []
        for i in range(SLOTS):
            w, h, cf, bd = [(64, 48, 1, 8), (72, 40, 0, 8), (136, 72, 2, 10), (264, 16, 3, 12)][i % 4]
            planes = make_planes(w, h, cf, bd, bd, seed=900 + i)
            light = (i % 3, i % 2, 0) if i % 2 else None
            frames.append(mu.frame_with(ctx, (w, h, cf, bd, bd), planes))
            args.append((None, 5 * i, light))
            want.append(expected(planes, (w, h, cf, bd, bd), None, 5 * i, light))
        tickets = [request(ctx, f, *a) for f, a in zip(frames, args)]
        assert tickets == list(range(1, SLOTS + 1)), "tickets count 1, 2, ... per context"
        with pytest.raises(capi.M355Error) as e:
            request(ctx, frames[0])
        assert e.value.code == BUSY
        assert_stats(ctx.frame_stats_result(tickets[-1]), want[-1], "the last request")
        extra = request(ctx, frames[3], *args[3])                   # the refused call took no ticket and enqueued nothing
        assert extra == SLOTS + 1
        assert_stats(ctx.frame_stats_result(extra), want[3], "the slot collected first, reused")
        for i in reversed(range(SLOTS - 1)):
            assert_stats(ctx.frame_stats_result(tickets[i]), want[i], "request %d" % i)
    finally:
        ctx.close()


def check_nonblocking(lib):
    ctx = capi.Context(lib, 0)
    try:
        geom = (200, 120, 1, 8, 8)
        a, b = make_planes(*geom, seed=5), make_planes(*geom, seed=6)
        fa, fb = mu.frame_with(ctx, geom, a), mu.frame_with(ctx, geom, b)
        light = (capi.MATRIX_BT709, 0, 2)
        wa, wb = expected(a, geom, light=light), expected(b, geom, black=9)
        for k in range(3):
            tk = request(ctx, fa, light=light)
            assert tk == k + 1
            got = ctx.frame_stats_result(tk, block=False)
            while got is None:                                      # BUSY: nothing was waited for, the request stays
                got = ctx.frame_stats_result(tk, block=False)
            assert_stats(got, wa, "non-blocking collection")
            for bad in (tk, tk + 1000, 0):                          # collected / unknown
                with pytest.raises(capi.M355Error) as e:
                    ctx.frame_stats_result(bad, block=False)
                assert e.value.code == INVALID
        # m355_wait completes a request and does not collect it; a frame may be destroyed with a request pending
        tk = request(ctx, fa, light=light)
        ctx.wait()
        tk2 = request(ctx, fb, black=9)
        ctx.frame_destroy(fb)
        assert_stats(ctx.frame_stats_result(tk, block=False), wa, "collected behind m355_wait")
        assert_stats(ctx.frame_stats_result(tk2), wb, "collected behind the frame's destruction")
    finally:
        ctx.close()


def check_slot_reuse(ctx, rounds=40):
    """one slot, request after request on alternating frames whose min rises, whose max falls and whose box shrinks from round to round: a device
    record not left neutral shows in the next result (a stale smaller min, larger max, wider box, or counts added up)"""
    geoms = ((72, 40, 1, 8, 8), (136, 24, 2, 10, 9))
    frames = [ctx.frame_create(*g) for g in geoms]
    try:
        for k in range(rounds):
            w, h, cf, bdl, bdc = geom = geoms[k % 2]
            top, q = (1 << bdl) - 1, k // 2
            planes = make_planes(w, h, cf, bdl, bdc, seed=77 + k)
            planes[0] = np.clip(planes[0].astype(np.int64), 2 * q, top - 3 * q).astype(planes[0].dtype)
            planes[0][:q % 8] = 2 * q
            planes[0][:, :q] = 2 * q                                # rows and columns at the (rising) minimum: not above `black`
            light = (capi.MATRIX_BT601, 0, 0) if k % 4 < 2 else None
            ctx.frame_upload(frames[k % 2], planes)
            want = expected(planes, geom, None, 2 * q, light)
            assert want["box"][:2] == (q, q % 8)
            assert_stats(ctx.frame_stats_result(request(ctx, frames[k % 2], None, 2 * q, light)), want, "round %d" % k)
    finally:
        for f in frames:
            ctx.frame_destroy(f)


def check_invalid(lib):
    """every M355_ERR_INVALID case of the header enqueues nothing: the next ticket is consecutive"""
    ctx = capi.Context(lib, 0)
    shard = capi.Context(lib, 0)
    try:
        L = lib.lib
        f8 = ctx.frame_create(64, 32, 1, 8, 8)
        f10 = ctx.frame_create(64, 32, 1, 10, 10)
        f422 = ctx.frame_create(64, 32, 2, 8, 8)
        f400 = ctx.frame_create(64, 32, 0, 8, 8)
        assert ctx.frame_stats_async(f8) == 1
        tk = ctypes.c_ulonglong(0)

        def desc(rect=None, reserved=None, **kw):
            d = capi.StatsDesc(**kw)
            if rect:
                d.x0, d.y0, d.width, d.height = rect
            if reserved is not None:
                d.reserved[reserved] = 1
            return d

        def refused(frame, d, what):
            rc = L.m355_frame_stats_async(ctx.h, frame, d, tk)
            assert rc == INVALID, "%s: returned %d" % (what, rc)

        refused(f8 + 99, ctypes.byref(desc()), "bad frame handle")
        refused(-1, ctypes.byref(desc()), "negative frame handle")
        refused(f8, None, "null descriptor")
        assert L.m355_frame_stats_async(ctx.h, f8, ctypes.byref(desc()), None) == INVALID, "null ticket"
        for rect in ((60, 0, 8, 8), (0, 30, 8, 4), (-2, 0, 8, 8), (0, -2, 8, 8), (0, 0, 8, -2), (0, 0, -8, 2), (0, 0, 66, 32), (0, 0, 8, 0)):
            refused(f8, ctypes.byref(desc(rect=rect)), "rectangle %s leaves the frame" % (rect,))
        for rect in ((1, 0, 8, 8), (0, 1, 8, 8), (0, 0, 7, 8), (0, 0, 8, 7)):
            refused(f8, ctypes.byref(desc(rect=rect)), "rectangle %s off the 4:2:0 chroma grid" % (rect,))
        refused(f422, ctypes.byref(desc(rect=(1, 0, 8, 8))), "4:2:2: odd x0")
        assert L.m355_frame_stats_async(ctx.h, f422, ctypes.byref(desc(rect=(0, 1, 8, 7))), tk) == 0 and tk.value == 2, "4:2:2 has no vertical grid"
        for black in (-1, 256):
            refused(f8, ctypes.byref(desc(black=black)), "black %d at 8 bit" % black)
        refused(f10, ctypes.byref(desc(black=1024)), "black 1024 at 10 bit")
        assert L.m355_frame_stats_async(ctx.h, f10, ctypes.byref(desc(black=1023)), tk) == 0 and tk.value == 3
        for light in (-1, 2):
            refused(f8, ctypes.byref(desc(light=light)), "light %d" % light)
        for kw in (dict(matrix=3), dict(matrix=-1), dict(full_range=2), dict(full_range=-1), dict(chroma_loc=4), dict(chroma_loc=-1)):
            refused(f8, ctypes.byref(desc(light=1, **kw)), "light with %s" % kw)
        refused(f422, ctypes.byref(desc(light=1, chroma_loc=2)), "a siting for 4:2:2")
        refused(f400, ctypes.byref(desc(light=1, chroma_loc=1)), "a siting for 4:0:0")
        for kw in (dict(matrix=1), dict(full_range=1), dict(chroma_loc=2)):
            refused(f8, ctypes.byref(desc(**kw)), "%s without light" % kw)
        for k in range(7):
            refused(f8, ctypes.byref(desc(reserved=k)), "reserved[%d]" % k)
        assert L.m355_frame_stats_async(ctx.h, f8, ctypes.byref(desc(light=1, matrix=2, full_range=1, chroma_loc=3)), tk) == 0 and tk.value == 4
        shard.shard_set(0, 2)
        fs = shard.frame_create(64, 32, 1, 8, 8)
        assert L.m355_frame_stats_async(shard.h, fs, ctypes.byref(desc()), tk) == INVALID, "tile-sharded context"
        out = capi.Stats()
        assert L.m355_frame_stats_result(ctx.h, 1, 1, None) == INVALID, "null result"
        for t in (1, 2, 3, 4):
            assert L.m355_frame_stats_result(ctx.h, t, 1, ctypes.byref(out)) == 0
        assert L.m355_frame_stats_result(ctx.h, 5, 1, ctypes.byref(out)) == INVALID
    finally:
        shard.close()
        ctx.close()


# ---- a decoded picture ----
def check_decoded_picture(lib, oracle):
    """one girlshy picture's statistics behind its decode with three pictures in flight, against the numpy statistics of the oracle's planes"""
    from golden_io import load_gold
    hdr, pics = load_gold("girlshy_full.m355gold.gz")
    o = Oracle(oracle)
    pic = pics[0]
    od = o.frame_new(pic.pp[0])
    assert o.decode(pic, od, {}) == 0
    planes = o.frame_planes(od)
    geom = (planes[0].shape[1], planes[0].shape[0], 1, 8, 8)
    c = capi.Context(lib, 0)
    try:
        dst = c.frame_create_for(pic.pp[0])
        c.set_pipeline_depth(3)
        saved, pic.dst_frame = pic.dst_frame, dst
        c.submit(pic)
        pic.dst_frame = saved
        light = (capi.MATRIX_BT709, 0, 0)
        rect = (16, 8, geom[0] - 32, geom[1] - 16)
        tickets = [request(c, dst, None, 16, None), request(c, dst, None, 40, light), request(c, dst, rect, 16, light)]
        assert_stats(c.frame_stats_result(tickets[0]), expected(planes, geom, None, 16, None), "planes")
        assert_stats(c.frame_stats_result(tickets[1]), expected(planes, geom, None, 40, light), "with light")
        assert_stats(c.frame_stats_result(tickets[2]), expected(planes, geom, rect, 16, light), "a rectangle")
    finally:
        c.close()
