"""Scenarios for the readers of a frame — downloads (m355_frame_download_async), exports (m355_frame_export) and hash requests
(m355_frame_hash_async) queued behind the decode that wrote it, which the next decode into the frame waits for — shared by the CPU
tier (SIMT-interpreter build, tests/test_reader_marks_emu.py) and the GPU tier (tests/test_gpu_reader_marks.py): each takes a loaded
library and the oracle.  Every comparison is exact.

The interpreter finishes every launch before the next call, so a missing wait cannot show there: that tier checks the bookkeeping (no
mark lost, none waited for after it was cleared, nothing left over at close()); the ordering itself is exercised on the device."""
from hash_async_util import PIC_A, _upload_refs, want_hashes
from hash_util import MD5, CRC, make_planes
from oracle_py import Oracle
from synth_util import assert_planes_equal, make_case, oracle_decode
from libde265_amd import capi

# the geometry of tests/test_gpu_pipeline.py's download test, and a picture whose copies last long enough for an unordered decode to land inside them
PIPE_A = dict(width=832, height=480, bit_depth=10, seed=311, n_refs=2, tile_cols=2, tile_rows=1)
PIPE_B = dict(PIPE_A, seed=412)
HD_A = dict(width=1920, height=1080, bit_depth=8, seed=301, intra_pct=30)
HD_B = dict(HD_A, seed=302)

_cases = {}


def case(oracle, cfg):
    """(picture, reference planes, the oracle's decode) of a configuration: made once, the planes are never written to"""
    key = tuple(sorted(cfg.items()))
    if key not in _cases:
        pic, refs = make_case(**cfg)
        _cases[key] = (pic, refs, oracle_decode(Oracle(oracle), pic, refs))
    return _cases[key]


def _geom(pic):
    pp = pic.pp[0]
    return tuple(int(pp[k]) for k in ("width", "height", "chroma_format_idc", "bit_depth_luma", "bit_depth_chroma"))


def check_all_kinds(lib, oracle, cfg_a, cfg_b, depth, reverse):
    """decode A into F; download, export and hash request of F; decode B into F — no host wait in between: every reader holds A"""
    (pa, ra, want_a), (pb, rb, want_b) = case(oracle, cfg_a), case(oracle, cfg_b)
    assert any((x != y).any() for x, y in zip(want_a, want_b)), "the two pictures must differ"
    bds = list(_geom(pa)[3:]) + [_geom(pa)[4]]
    ctx = capi.Context(lib, 0)
    try:
        _upload_refs(ctx, pa, ra)
        _upload_refs(ctx, pb, rb)
        F = ctx.frame_create_for(pa.pp[0])
        ctx.set_pipeline_depth(depth)
        ctx.wait()
        start = {"download": lambda: ctx.frame_download_async(F),
                 "export": lambda: ctx.frame_export(F, capi.EXPORT_PLANAR, capi.EXPORT_NATIVE, host=True),
                 "hash": lambda: ctx.frame_hash_async(F, CRC)}
        finish = {"download": ctx.frame_download_finish, "export": ctx.frame_export_finish, "hash": ctx.frame_hash_result}
        order = ["download", "export", "hash"][::-1 if reverse else 1]
        # ---- no host wait from here ...
        pa.dst_frame = pb.dst_frame = F
        ctx.submit(pa)
        tokens = [start[kind]() for kind in order]
        ctx.submit(pb)
        # ---- ... to here
        for kind, token in reversed(list(zip(order, tokens))):
            got = finish[kind](token)
            if kind == "hash":
                assert got == want_hashes(oracle, want_a, bds, CRC), "the hash is not the earlier picture's"
            else:
                assert_planes_equal(got, want_a, "%s behind the earlier picture" % kind)
        ctx.wait()
        assert_planes_equal(ctx.frame_download(F), want_b, "the later picture")
    finally:
        ctx.close()


def check_waits_per_kind(lib, oracle, geom):
    """an export and an MD5 request on one frame: the host's wait for one kind leaves the other collectable, in either order"""
    w, h, cf, bdl, bdc = geom
    planes = make_planes(w, h, cf, bdl, bdc, seed=w + 3 * h)
    want = want_hashes(oracle, planes, [bdl, bdc, bdc], MD5)
    ctx = capi.Context(lib, 0)
    try:
        f = ctx.frame_create(w, h, cf, bdl, bdc)
        ctx.frame_upload(f, planes)
        for hash_first in (False, True):
            token = ctx.frame_export(f, capi.EXPORT_PLANAR, capi.EXPORT_NATIVE, host=True)
            ticket = ctx.frame_hash_async(f, MD5)
            if hash_first:
                assert ctx.frame_hash_result(ticket) == want, "hash collected in front of the export"
            assert_planes_equal(ctx.frame_export_finish(token), planes, "export (hash collected first: %s)" % hash_first)
            if not hash_first:
                assert ctx.frame_hash_result(ticket) == want, "hash collected behind the export's wait"
    finally:
        ctx.close()


def check_two_downloads(lib, oracle, cfg):
    """two downloads of a frame no decode wrote, queued while different lanes are active, then a decode into the frame: both hold the uploaded planes"""
    (pic, refs, want), (small, srefs, swant) = case(oracle, cfg), case(oracle, PIC_A)
    w, h, cf, bdl, bdc = _geom(pic)
    planes = make_planes(w, h, cf, bdl, bdc, seed=w + 5 * h)
    ctx = capi.Context(lib, 0)
    try:
        _upload_refs(ctx, pic, refs)
        _upload_refs(ctx, small, srefs)
        F, G = ctx.frame_create_for(pic.pp[0]), ctx.frame_create_for(small.pp[0])
        ctx.set_pipeline_depth(2)
        ctx.frame_upload(F, planes)
        ctx.wait()
        # ---- no host wait from here ...
        first = ctx.frame_download_async(F)
        small.dst_frame = G
        ctx.submit(small)                                           # the active lane moves on: the second download is queued on another stream
        second = ctx.frame_download_async(F)
        pic.dst_frame = F
        ctx.submit(pic)
        # ---- ... to here
        assert_planes_equal(ctx.frame_download_finish(first), planes, "first download")
        assert_planes_equal(ctx.frame_download_finish(second), planes, "second download")
        ctx.wait()
        assert_planes_equal(ctx.frame_download(F), want, "the picture decoded into the frame")
        assert_planes_equal(ctx.frame_download(G), swant, "the picture in between")
    finally:
        ctx.close()


def check_collected_hash(lib, oracle, cfg_a, cfg_b):
    """a request collected before the next decode into its frame leaves nothing behind: the decode is right, the next request is the next ticket"""
    (pa, ra, want_a), (pb, rb, want_b) = case(oracle, cfg_a), case(oracle, cfg_b)
    bds = list(_geom(pa)[3:]) + [_geom(pa)[4]]
    ctx = capi.Context(lib, 0)
    try:
        _upload_refs(ctx, pa, ra)
        _upload_refs(ctx, pb, rb)
        F = ctx.frame_create_for(pa.pp[0])
        pa.dst_frame = pb.dst_frame = F
        ctx.submit(pa)
        ticket = ctx.frame_hash_async(F, CRC)
        assert ctx.frame_hash_result(ticket) == want_hashes(oracle, want_a, bds, CRC)
        ctx.submit(pb)
        ctx.wait()
        assert_planes_equal(ctx.frame_download(F), want_b, "decode into a frame whose request was collected")
        again = ctx.frame_hash_async(F, CRC)
        assert again == ticket + 1
        assert ctx.frame_hash_result(again) == want_hashes(oracle, want_b, bds, CRC), "the request behind the later picture"
    finally:
        ctx.close()
