"""Shared by the m355_frame_export_scaled tests (SIMT-interpreter build and GPU): the numpy restatement of what a scaled export delivers — the
exact box average of the planes m355_frame_download returns, one rounding from the block sum per sample format — and the drivers that check
exports against it, the untouched padding of the destination rows included."""
import numpy as np

from export_util import FORMATS, LAYOUTS, SAMPLES, M355_ERR_INVALID, assert_export, chroma_grid_rect, decode_into_frame, expected_export, format_id  # noqa: F401
from synth_util import assert_planes_equal, make_case
from libde265_amd import capi, worklist

SCALES = (1, 2, 3)
# the rectangle of the format matrix: its source starts off a vector boundary, its size is a multiple of 8 * SubWidthC x 8 * SubHeightC for every format
MATRIX_RECT = (2, 2, 48, 16)


def expected_export_scaled(planes, cf, bdl, bdc, layout, samples, k, rect=None):
    """what m355_frame_export_scaled delivers, from the planes m355_frame_download returns"""
    f = 1 << k
    out = []
    for c, p in enumerate(expected_export(planes, cf, bdl, bdc, capi.EXPORT_PLANAR, capi.EXPORT_NATIVE, rect)):
        bd = bdc if c else bdl
        h, w = p.shape
        assert h % f == 0 and w % f == 0, "the rectangle is no multiple of the scale on plane %d" % c
        s = p.reshape(h // f, f, w // f, f).sum(axis=(1, 3), dtype=np.uint64)
        a = (s + (f * f) // 2) >> np.uint64(2 * k)
        if samples == capi.EXPORT_NATIVE:
            q = a.astype(p.dtype)
        elif samples == capi.EXPORT_MSB16:
            q = ((a << np.uint64(16 - bd)) & np.uint64(0xFFFF)).astype(np.uint16)
        else:
            q = np.minimum(255, (s + (1 << (2 * k + bd - 9))) >> np.uint64(2 * k + bd - 8)).astype(np.uint8)
        out.append(np.ascontiguousarray(q))
    if layout == capi.EXPORT_SEMIPLANAR and len(out) == 3:
        out = [out[0], np.stack([out[1], out[2]], axis=-1).reshape(out[1].shape[0], -1)]
    return out


def check_export_scaled(ctx, frame, planes, geom, layout, samples, k, rect=None, host=False, what=""):
    cf, bdl, bdc = geom
    got, raws = ctx.frame_export_finish(ctx.frame_export(frame, layout, samples, rect, host=host, log2_scale=k), raw=True)
    assert_export(got, raws, expected_export_scaled(planes, cf, bdl, bdc, layout, samples, k, rect),
                  "%s scale %d layout %d samples %d rect %s" % (what, 1 << k, layout, samples, rect))


def check_all_formats(ctx, frame, planes, geom, rects, scales=SCALES, what=""):
    """every scale x layout x sample format x rectangle of one frame"""
    for rect in rects:
        r = None if rect is None else chroma_grid_rect(rect, geom[0])
        for k in scales:
            for layout in LAYOUTS:
                for samples in SAMPLES:
                    check_export_scaled(ctx, frame, planes, geom, layout, samples, k, r, what=what)


def check_format_matrix_scaled(ctx, o, cfg, rects, scales=SCALES):
    frame, planes, geom, frames = decode_into_frame(ctx, o, cfg)
    try:
        check_all_formats(ctx, frame, planes, geom, rects, scales, what=format_id(cfg))
    finally:
        for f in frames:
            ctx.frame_destroy(f)


def value_cases(bd):
    """4:4:4 frames of 128x32 that reach what decoded pictures seldom do -> [(name, planes)]: the ramps over the whole sample range, planes of the
    constant maximum (the largest block sum: what a signed or a 16-bit accumulator gets wrong, and what U8 must clip from 256 to 255), and per scale
    a plane that is zero except one sample per block, n/2 in even block columns and n/2 - 1 in odd ones (NATIVE: 1 and 0 — round half up)"""
    dt = np.uint8 if bd <= 8 else np.uint16
    cases = []
    ramp = (np.arange(128 * 32, dtype=np.uint32) * ((1 << bd) - 1) // (128 * 32 - 1)).astype(dt).reshape(32, 128)
    assert int(ramp.max()) == (1 << bd) - 1 and int(ramp.min()) == 0
    cases.append(("ramp", (1, 2, 3), [ramp, ramp[::-1].copy(), ramp[:, ::-1].copy()]))
    top = np.full((32, 128), (1 << bd) - 1, dt)
    cases.append(("maximum", (1, 2, 3), [top, top.copy(), top.copy()]))
    for k in (1, 2, 3):
        f, n = 1 << k, 1 << (2 * k)
        planes = []
        for c in range(3):                       # (the one sample at another place of the block on every plane)
            p = np.zeros((32, 128), dt)
            y, x = (c * 3) % f, (c * 5 + 1) % f
            p[y::f, x::2 * f] = n // 2
            p[y::f, x + f::2 * f] = n // 2 - 1
            planes.append(p)
        cases.append(("half %d" % f, (k,), planes))
    return cases


def check_values(ctx, bd):
    frame = ctx.frame_create(128, 32, 3, bd, bd)
    try:
        for name, scales, planes in value_cases(bd):
            ctx.frame_upload(frame, planes)
            if name.startswith("half"):
                k = scales[0]
                want = expected_export_scaled(planes, 3, bd, bd, capi.EXPORT_PLANAR, capi.EXPORT_NATIVE, k)
                assert np.all(want[0][:, 0::2] == 1) and np.all(want[0][:, 1::2] == 0), "the restatement does not round half up"
            if name == "maximum" and bd > 8:
                want = expected_export_scaled(planes, 3, bd, bd, capi.EXPORT_PLANAR, capi.EXPORT_U8, 3)
                assert np.all(want[0] == 255)
            check_all_formats(ctx, frame, planes, (3, bd, bd), [None], scales, what="%s %d bit" % (name, bd))
    finally:
        ctx.frame_destroy(frame)


def check_gate_scaled(ctx, k=1):
    """export_util.check_gate for the scaled export: behind a decode whose lists the device rejected it writes nothing, behind an accepted decode of
    the same lists it does"""
    layout, samples = capi.EXPORT_SEMIPLANAR, capi.EXPORT_MSB16
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
        tokens.append(ctx.frame_export(dst, layout, samples, log2_scale=k))
    good, bad = [ctx.frame_export_finish(t, raw=True) for t in tokens]
    assert ctx.decode_status(serials[0]) == 0 and ctx.decode_status(serials[1]) == M355_ERR_INVALID
    with_planes = ctx.frame_download(dst)           # (the rejected decode left the accepted picture in the frame)
    assert_export(good[0], good[1], expected_export_scaled(with_planes, 1, 8, 8, layout, samples, k), "behind the accepted decode")
    for raw in bad[1]:
        assert np.all(raw == capi.DEVICE_FILL), "a scaled export behind a rejected decode wrote to its destination"
    ctx.wait()
    for f in handles + [dst]:
        ctx.frame_destroy(f)


def check_hazard_scaled(ctx, depth, k=1, layout=capi.EXPORT_SEMIPLANAR, samples=capi.EXPORT_MSB16):
    """export_util.check_hazard for the scaled export: four pictures decoded alternately into a pool of two frames, each exported right behind its
    decode into a buffer of its own, no host wait in between; every export must deliver what the export of the same picture decoded alone
    delivers.  (On the GPU with several pictures in flight this sees a decode that does not wait for the scaled export of its frame's previous
    picture; the SIMT interpreter finishes every launch before the next call and checks the bookkeeping's results only.)"""
    from libde265_amd import synth
    ctx.set_pipeline_depth(depth)
    try:
        cfg = dict(width=128, height=64, bit_depth=10, seed=5, n_refs=1)
        pics = [synth.picture(**dict(cfg, seed=5 + j)) for j in range(4)]
        pp = pics[0].pp[0]
        r0 = ctx.frame_create_for(pp)
        ctx.frame_upload(r0, synth.ref_planes(5, 128, 64, 1, 10))
        pool = [ctx.frame_create_for(pp) for _ in range(2)]
        rect = (2, 2, 120, 56)
        handles, tokens = [], []
        for j, pic in enumerate(pics):
            pic.ref_frames = [r0] + [-1] * (worklist.MAX_REF_FRAMES - 1)
            pic.dst_frame = pool[j % 2]
            handles.append(ctx.upload(pic))
            ctx.decode_resident(handles[-1])
            tokens.append(ctx.frame_export(pool[j % 2], layout, samples, rect, log2_scale=k))
        got = [ctx.frame_export_finish(t, raw=True) for t in tokens]
        ctx.wait()
        for j in range(4):
            ctx.decode_resident(handles[j])
            ctx.wait()
            planes = ctx.frame_download(pool[j % 2])
            alone = ctx.frame_export_finish(ctx.frame_export(pool[j % 2], layout, samples, rect, log2_scale=k))
            assert_planes_equal(alone, expected_export_scaled(planes, 1, 10, 10, layout, samples, k, rect), "picture %d alone" % j)
            assert_export(got[j][0], got[j][1], alone, "picture %d, depth %d" % (j, depth))
        for j in (0, 1):
            assert not np.array_equal(got[j][0][0], got[j + 2][0][0]), "the pictures that share a frame must differ for this test to see a hazard"
        for h in handles:
            ctx.release(h)
        for f in pool + [r0]:
            ctx.frame_destroy(f)
    finally:
        ctx.set_pipeline_depth(1)
