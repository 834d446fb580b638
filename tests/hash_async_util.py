"""Scenarios of the hash-request tests (m355_frame_hash_async / m355_frame_hash_result), shared by the CPU tier (SIMT-interpreter
build, tests/test_hash_async_emu.py) and the GPU tier (tests/test_gpu_hash_async.py): each takes a loaded library and the oracle.
Every comparison is exact — a hash has no tolerance."""
import pytest

from hash_util import MD5, CRC, CHECKSUM, make_planes, oracle_hash
from oracle_py import Oracle
from synth_util import assert_planes_equal, make_case, oracle_decode
from libde265_amd import capi, worklist

TYPES = (MD5, CRC, CHECKSUM)
BUSY, INVALID = 6, 3                # M355_ERR_BUSY, M355_ERR_INVALID
SLOTS = 16                          # M355_HASH_REQUESTS

# two small pictures of one geometry whose outputs differ (the reader-hazard test) and the picture of tests/test_decode_status.py
PIC_A = dict(width=64, height=64, bit_depth=8, seed=301, intra_pct=30)
PIC_B = dict(width=64, height=64, bit_depth=8, seed=302, intra_pct=30)
REJECT_CASE = dict(width=256, height=192, bit_depth=8, seed=71, intra_pct=30, tile_cols=2, features=2)


def want_hashes(oracle, planes, bds, t):
    return [oracle_hash(oracle, p, bds[c], t) for c, p in enumerate(planes)]


def check_values(ctx, oracle, geom):
    """async == m355_frame_hash == the oracle, three types, the requests of one frame in flight together"""
    w, h, cf, bdl, bdc = geom
    planes = make_planes(w, h, cf, bdl, bdc, seed=w + 7 * h)
    f = ctx.frame_create(w, h, cf, bdl, bdc)
    try:
        ctx.frame_upload(f, planes)
        tickets = [ctx.frame_hash_async(f, t) for t in TYPES]
        for t, tk in zip(TYPES, tickets):
            got = ctx.frame_hash_result(tk)
            assert got == want_hashes(oracle, planes, [bdl, bdc, bdc], t), "hash type %d against the oracle" % t
            assert got == ctx.frame_hash(f, t), "hash type %d against m355_frame_hash" % t
    finally:
        ctx.frame_destroy(f)


def _upload_refs(ctx, pic, refs):
    handles = []
    for planes in refs:
        f = ctx.frame_create_for(pic.pp[0])
        ctx.frame_upload(f, planes)
        handles.append(f)
    pic.ref_frames = [handles[i] if i < len(handles) else -1 for i in range(worklist.MAX_REF_FRAMES)]


def check_reader_hazard(lib, oracle, types, with_export):
    """decode A into F, request F's hash(es), [export F,] decode B into F — nothing waited for in between: the values are A's"""
    o = Oracle(oracle)
    (pa, ra), (pb, rb) = make_case(**PIC_A), make_case(**PIC_B)
    want_a, want_b = oracle_decode(o, pa, ra), oracle_decode(o, pb, rb)
    assert any((x != y).any() for x, y in zip(want_a, want_b)), "the two pictures must differ"
    ctx = capi.Context(lib, 0)
    try:
        _upload_refs(ctx, pa, ra)
        _upload_refs(ctx, pb, rb)
        F = ctx.frame_create_for(pa.pp[0])
        ctx.set_pipeline_depth(3)
        ctx.wait()
        # ---- no host wait from here ...
        pa.dst_frame = pb.dst_frame = F
        ctx.submit(pa)
        tickets = [ctx.frame_hash_async(F, t) for t in types]
        token = ctx.frame_export(F, capi.EXPORT_PLANAR, capi.EXPORT_NATIVE, host=True) if with_export else None
        ctx.submit(pb)
        # ---- ... to here
        for t, tk in zip(types, tickets):
            assert ctx.frame_hash_result(tk) == want_hashes(oracle, want_a, [8, 8, 8], t), "hash type %d is not the earlier picture's" % t
        if token is not None:
            assert_planes_equal(ctx.frame_export_finish(token), want_a, "export between the hash and the next decode")
        ctx.wait()
        assert_planes_equal(ctx.frame_download(F), want_b, "the later picture")
    finally:
        ctx.close()


def check_concurrency(lib, oracle):
    """16 requests on 16 frames before any is collected, collected in reverse; the 17th is refused; a collected slot is free again"""
    ctx = capi.Context(lib, 0)
    try:
        frames, want = [], []
        for i in range(SLOTS):
            w, h, cf, bd = [(64, 48, 1, 8), (72, 40, 0, 8), (136, 72, 2, 10), (264, 16, 3, 12)][i % 4]
            planes = make_planes(w, h, cf, bd, bd, seed=900 + i)
            f = ctx.frame_create(w, h, cf, bd, bd)
            ctx.frame_upload(f, planes)
            frames.append(f)
            want.append(ctx.frame_hash(f, TYPES[i % 3]))
            assert want[i] == want_hashes(oracle, planes, [bd] * 3, TYPES[i % 3])
        tickets = [ctx.frame_hash_async(f, TYPES[i % 3]) for i, f in enumerate(frames)]
        assert tickets == list(range(1, SLOTS + 1)), "tickets count 1, 2, ... per context"
        with pytest.raises(capi.M355Error) as e:
            ctx.frame_hash_async(frames[0], CRC)
        assert e.value.code == BUSY
        assert ctx.frame_hash_result(tickets[-1]) == want[-1]
        extra = ctx.frame_hash_async(frames[3], CHECKSUM)          # the refused call took no ticket
        assert extra == SLOTS + 1
        assert ctx.frame_hash_result(extra) == ctx.frame_hash(frames[3], CHECKSUM)
        for i in reversed(range(SLOTS - 1)):
            assert ctx.frame_hash_result(tickets[i]) == want[i], "request %d" % i
    finally:
        ctx.close()


def check_nonblocking(lib, oracle):
    ctx = capi.Context(lib, 0)
    try:
        planes = make_planes(200, 120, 1, 8, 8, seed=5)
        f = ctx.frame_create(200, 120, 1, 8, 8)
        ctx.frame_upload(f, planes)
        for t in TYPES:
            tk = ctx.frame_hash_async(f, t)
            got = ctx.frame_hash_result(tk, block=False)
            while got is None:                                      # BUSY: nothing was waited for, the request stays
                got = ctx.frame_hash_result(tk, block=False)
            assert got == want_hashes(oracle, planes, [8, 8, 8], t)
            for bad in (tk, tk + 1000, 0):                          # collected / unknown
                with pytest.raises(capi.M355Error) as e:
                    ctx.frame_hash_result(bad, block=False)
                assert e.value.code == INVALID
        # bad arguments enqueue nothing and take no ticket
        for args in ((f + 99, CRC), (f, 7)):
            with pytest.raises(capi.M355Error) as e:
                ctx.frame_hash_async(*args)
            assert e.value.code == INVALID
        assert lib.lib.m355_frame_hash_async(ctx.h, f, CRC, None) == INVALID
        assert ctx.frame_hash_async(f, CRC) == len(TYPES) + 1
    finally:
        ctx.close()


def check_rejected_decode(lib, oracle, depth):
    """a hash behind a decode whose lists the device rejected has no value; the slot it used is clean for the next request"""
    pic, refs = make_case(**REJECT_CASE)
    want = oracle_decode(Oracle(oracle), pic, refs)
    ctx = capi.Context(lib, 0)
    try:
        _upload_refs(ctx, pic, refs)
        ctx.set_pipeline_depth(depth)
        d = ctx.frame_create_for(pic.pp[0])
        ctx.frame_fill(d, 77, 99)
        bad = make_case(**REJECT_CASE)[0]
        bad.ref_frames = pic.ref_frames
        arr = bad.tus.copy()
        arr["log2_size"][len(arr) // 2] = 9
        bad.tus = arr
        for t in TYPES:
            bad.dst_frame = d
            ctx.submit_in_place(bad, fill_threads=1)
            serial = ctx.last_serial()
            tk = ctx.frame_hash_async(d, t)                         # the context's only request: always the first slot
            with pytest.raises(capi.M355Error) as e:
                ctx.frame_hash_result(tk)
            assert e.value.code == INVALID and "rejected" in str(e.value)
            st = ctx.decode_status(serial)                          # (reported here, so that m355_wait stays quiet)
            while st == BUSY:
                st = ctx.decode_status(serial)
            assert st == INVALID
            with pytest.raises(capi.M355Error):                     # the failed collection freed the ticket
                ctx.frame_hash_result(tk)
            pic.dst_frame = d
            ctx.submit_in_place(pic, fill_threads=1)
            tk = ctx.frame_hash_async(d, t)
            assert ctx.frame_hash_result(tk) == want_hashes(oracle, want, [8, 8, 8], t), "hash type %d in the slot a gated request left" % t
        ctx.wait()
    finally:
        ctx.close()


def check_slot_reuse(ctx, oracle, rounds=40):
    """one slot, request after request on alternating frames and types: a record not re-zeroed or a stale verdict shows at once"""
    geoms = [(200, 120, 1, 8, 8), (136, 72, 2, 10, 9)]
    frames, want = [], []
    for k, (w, h, cf, bdl, bdc) in enumerate(geoms):
        planes = make_planes(w, h, cf, bdl, bdc, seed=77 + k)
        f = ctx.frame_create(w, h, cf, bdl, bdc)
        ctx.frame_upload(f, planes)
        frames.append(f)
        want.append({t: want_hashes(oracle, planes, [bdl, bdc, bdc], t) for t in (CRC, CHECKSUM)})
    try:
        for k in range(rounds):
            t = (CRC, CHECKSUM)[(k // 2) % 2]
            tk = ctx.frame_hash_async(frames[k % 2], t)
            assert ctx.frame_hash_result(tk) == want[k % 2][t], "round %d" % k
    finally:
        for f in frames:
            ctx.frame_destroy(f)
