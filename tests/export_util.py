"""Shared by the m355_frame_export tests (SIMT-interpreter build and GPU): the numpy restatement of what an export delivers — a closed-form
integer function of the planes m355_frame_download returns — and the driver that checks one export against it, the untouched
padding of the destination rows included."""
import numpy as np

from synth_util import assert_planes_equal, make_case, oracle_decode
from libde265_amd import capi, worklist

LAYOUTS = (capi.EXPORT_PLANAR, capi.EXPORT_SEMIPLANAR)
SAMPLES = (capi.EXPORT_NATIVE, capi.EXPORT_MSB16, capi.EXPORT_U8)
M355_ERR_INVALID = 3   # (capi.ERRORS)

# 64x32 pictures of every sample type and chroma format the export kernel is instantiated for
FORMATS = [
    dict(bit_depth=8, seed=7101),
    dict(bit_depth=10, seed=7102),
    dict(bit_depth=12, chroma_format=2, seed=7103),
    dict(bit_depth=10, chroma_format=3, seed=7104),
    dict(bit_depth=8, chroma_format=4, seed=7105),
    dict(bit_depth=10, bit_depth_chroma=9, seed=7106),
]


def format_id(cfg):
    return "bd%d_%d_cf%d" % (cfg["bit_depth"], cfg.get("bit_depth_chroma", cfg["bit_depth"]), cfg.get("chroma_format", 1))


def sub_sampling(cf):
    return (2 if cf in (1, 2) else 1), (2 if cf == 1 else 1)


def chroma_grid_rect(rect, cf):
    """the rectangle with every coordinate rounded down to the chroma grid of the format"""
    sw, sh = sub_sampling(cf)
    x0, y0, w, h = rect
    return (x0 // sw * sw, y0 // sh * sh, w // sw * sw, h // sh * sh)


def expected_export(planes, cf, bdl, bdc, layout, samples, rect=None):
    """what m355_frame_export delivers, from the planes m355_frame_download returns"""
    sw, sh = sub_sampling(cf)
    out = []
    for c, p in enumerate(planes):
        bd = bdc if c else bdl
        if rect is not None:
            x0, y0, w, h = rect
            dx, dy = (sw, sh) if c else (1, 1)
            p = p[y0 // dy:(y0 + h) // dy, x0 // dx:(x0 + w) // dx]
        if samples == capi.EXPORT_MSB16:
            p = (p.astype(np.uint32) << (16 - bd)).astype(np.uint16)
        elif samples == capi.EXPORT_U8 and bd > 8:
            p = np.minimum(255, (p.astype(np.uint32) + (1 << (bd - 9))) >> (bd - 8)).astype(np.uint8)
        out.append(np.ascontiguousarray(p))
    if layout == capi.EXPORT_SEMIPLANAR and len(out) == 3:
        out = [out[0], np.stack([out[1], out[2]], axis=-1).reshape(out[1].shape[0], -1)]
    return out


def assert_export(got, raws, want, what):
    """the planes are the expected ones, sample for sample, and no byte between a row's end and the pitch was written"""
    assert [g.dtype for g in got] == [w.dtype for w in want], what
    assert_planes_equal(got, want, what)
    for k, (g, raw) in enumerate(zip(got, raws)):
        pad = raw[:, g.shape[1] * g.dtype.itemsize:]
        assert pad.size and np.all(pad == capi.DEVICE_FILL), "%s: plane %d: bytes behind the row end were written" % (what, k)


def check_export(ctx, frame, planes, geom, layout, samples, rect=None, host=False, what=""):
    cf, bdl, bdc = geom
    got, raws = ctx.frame_export_finish(ctx.frame_export(frame, layout, samples, rect, host=host), raw=True)
    assert_export(got, raws, expected_export(planes, cf, bdl, bdc, layout, samples, rect), "%s layout %d samples %d rect %s" % (what, layout, samples, rect))


def decode_into_frame(ctx, o, cfg):
    """one synthetic picture through the library -> (frame handle, downloaded planes == the oracle's decode, (cf, bdl, bdc), frames to destroy)"""
    pic, refs = make_case(**cfg)
    want = oracle_decode(o, pic, refs)
    pp = pic.pp[0]
    handles = []
    for planes in refs:
        f = ctx.frame_create_for(pp)
        ctx.frame_upload(f, planes)
        handles.append(f)
    dst = ctx.frame_create_for(pp)
    pic.dst_frame = dst
    pic.ref_frames = [handles[i] if i < len(handles) else -1 for i in range(worklist.MAX_REF_FRAMES)]
    ctx.submit(pic)
    ctx.wait()
    planes = ctx.frame_download(dst)
    assert_planes_equal(planes, want, "download vs oracle")
    return dst, planes, (int(pp["chroma_format_idc"]), int(pp["bit_depth_luma"]), int(pp["bit_depth_chroma"])), handles + [dst]


def check_format_matrix(ctx, o, cfg, rects):
    """every layout x sample format x rectangle of one picture"""
    frame, planes, geom, frames = decode_into_frame(ctx, o, cfg)
    try:
        for rect in rects:
            r = None if rect is None else chroma_grid_rect(rect, geom[0])
            for layout in LAYOUTS:
                for samples in SAMPLES:
                    check_export(ctx, frame, planes, geom, layout, samples, r, what=format_id(cfg))
    finally:
        for f in frames:
            ctx.frame_destroy(f)


def check_gate(ctx):
    """an export queued behind a decode whose lists the device rejected writes nothing (the frame carries that decode's gate), and an export
    behind an accepted decode of the same lists does"""
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
        tokens.append(ctx.frame_export(dst, capi.EXPORT_SEMIPLANAR, capi.EXPORT_MSB16))
    good, bad = [ctx.frame_export_finish(t, raw=True) for t in tokens]
    assert ctx.decode_status(serials[0]) == 0 and ctx.decode_status(serials[1]) == M355_ERR_INVALID
    with_planes = ctx.frame_download(dst)           # (the rejected decode left the accepted picture in the frame)
    assert_export(good[0], good[1], expected_export(with_planes, 1, 8, 8, capi.EXPORT_SEMIPLANAR, capi.EXPORT_MSB16), "behind the accepted decode")
    for raw in bad[1]:
        assert np.all(raw == capi.DEVICE_FILL), "an export behind a rejected decode wrote to its destination"
    ctx.wait()
    for f in handles + [dst]:
        ctx.frame_destroy(f)


def check_hazard(ctx, depth, layout=capi.EXPORT_SEMIPLANAR, samples=capi.EXPORT_MSB16):
    """four pictures decoded alternately into a pool of two frames, each exported right behind its decode into a buffer of its own, no host wait
    in between: every export must deliver what the export of the same picture decoded alone delivers.  On the GPU with several pictures in
    flight this is what sees a decode that does not wait for the export of its frame's previous picture; the SIMT interpreter finishes every
    launch before the next call, so there the test checks the bookkeeping's results only, not the ordering."""
    from libde265_amd import synth
    ctx.set_pipeline_depth(depth)
    try:
        cfg = dict(width=128, height=64, bit_depth=10, seed=5, n_refs=1)
        pics = [synth.picture(**dict(cfg, seed=5 + k)) for k in range(4)]
        pp = pics[0].pp[0]
        r0 = ctx.frame_create_for(pp)
        ctx.frame_upload(r0, synth.ref_planes(5, 128, 64, 1, 10))
        pool = [ctx.frame_create_for(pp) for _ in range(2)]
        rect = (2, 2, 122, 58)
        handles, tokens = [], []
        for k, pic in enumerate(pics):
            pic.ref_frames = [r0] + [-1] * (worklist.MAX_REF_FRAMES - 1)
            pic.dst_frame = pool[k % 2]
            handles.append(ctx.upload(pic))
            ctx.decode_resident(handles[-1])
            tokens.append(ctx.frame_export(pool[k % 2], layout, samples, rect))
        got = [ctx.frame_export_finish(t, raw=True) for t in tokens]
        ctx.wait()
        for k in range(4):
            ctx.decode_resident(handles[k])
            ctx.wait()
            planes = ctx.frame_download(pool[k % 2])
            alone = ctx.frame_export_finish(ctx.frame_export(pool[k % 2], layout, samples, rect))
            assert_planes_equal(alone, expected_export(planes, 1, 10, 10, layout, samples, rect), "picture %d alone" % k)
            assert_export(got[k][0], got[k][1], alone, "picture %d, depth %d" % (k, depth))
        for k in (0, 1):
            assert not np.array_equal(got[k][0][0], got[k + 2][0][0]), "the pictures that share a frame must differ for this test to see a hazard"
        for h in handles:
            ctx.release(h)
        for f in pool + [r0]:
            ctx.frame_destroy(f)
    finally:
        ctx.set_pipeline_depth(1)
