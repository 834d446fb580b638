"""Shared by the m355_frame_export_resized_rgb tests (SIMT-interpreter build, GPU and glue): what the call delivers is the COMPOSITION of the two
existing restatements — export_resized_util.expected_export_resized (planar, NATIVE) pushed through export_rgb_util.expected_rgb as a frame of the
output size — and the drivers that check exports against it.  Every comparison of pixels is exact, the untouched padding of the destination rows
included."""
import numpy as np

from export_util import FORMATS, assert_export, chroma_grid_rect, decode_into_frame, expected_export, format_id  # noqa: F401
from export_resized_util import MATRIX_SIZES, expected_export_resized
from export_rgb_util import ALL_CONVERSIONS, LAYOUTS, MATRIX_CONVERSIONS, SAMPLES, M355_ERR_INVALID, expected_rgb, value_cases  # noqa: F401
from synth_util import assert_planes_equal, make_case
from libde265_amd import capi, worklist


def expected_resized_rgb(planes, cf, bdl, bdc, layout, samples, matrix, full_range, out_size, rect=None, edge="clamp"):
    """what m355_frame_export_resized_rgb delivers, from the planes m355_frame_download returns (edge: export_rgb_util.chroma_at_luma's, for the tests
    that show that the chroma filter's clamps are under test)"""
    resized = expected_export_resized(planes, cf, bdl, bdc, capi.EXPORT_PLANAR, capi.EXPORT_NATIVE, out_size, rect)
    return expected_rgb(resized, cf, bdl, bdc, layout, samples, matrix, full_range, edge=edge)


def check_resized_rgb(ctx, frame, planes, geom, layout, samples, matrix, full_range, out_size, rect=None, host=False, what=""):
    cf, bdl, bdc = geom
    got, raws = ctx.frame_export_finish(ctx.frame_export_resized_rgb(frame, layout, samples, matrix, full_range, out_size, rect, host=host), raw=True)
    assert_export(got, raws, expected_resized_rgb(planes, cf, bdl, bdc, layout, samples, matrix, full_range, out_size, rect),
                  "%s to %dx%d layout %d samples %d matrix %d full %d rect %s" % (what, out_size[0], out_size[1], layout, samples, matrix, full_range, rect))


def check_all(ctx, frame, planes, geom, sizes, conversions, what=""):
    """every (rectangle, output size) x layout x sample type x conversion of one frame"""
    for rect, out_size in sizes:
        r = None if rect is None else chroma_grid_rect(rect, geom[0])
        for layout in LAYOUTS:
            for samples in SAMPLES:
                for matrix, full in conversions:
                    check_resized_rgb(ctx, frame, planes, geom, layout, samples, matrix, full, out_size, r, what=what)


def check_format_matrix(ctx, o, cfg, sizes=MATRIX_SIZES, conversions=MATRIX_CONVERSIONS):
    frame, planes, geom, frames = decode_into_frame(ctx, o, cfg)
    try:
        check_all(ctx, frame, planes, geom, sizes, conversions, what=format_id(cfg))
    finally:
        for f in frames:
            ctx.frame_destroy(f)


# the composition through the public calls: a 64x32 picture, (rectangle, output size) with output sizes that a frame can have (multiples of 8)
COMPOSITION_SIZES = [(None, (48, 24)), (None, (128, 64)), (None, (8, 8)), ((2, 2, 50, 22), (40, 16)), ((2, 2, 50, 22), (64, 32))]
COMPOSITION_FORMATS = [dict(bit_depth=10, seed=7901), dict(bit_depth=12, chroma_format=2, seed=7902), dict(bit_depth=10, chroma_format=3, seed=7903),
                       dict(bit_depth=8, chroma_format=4, seed=7904)]


def check_composition(ctx, o, cfg):
    """independent of any Python arithmetic: frame_export_resized (planar, NATIVE) read back and uploaded into a second frame of the output size,
    frame_export_rgb of that frame taken whole — identical to the one call"""
    frame, planes, geom, frames = decode_into_frame(ctx, o, dict(cfg, width=64, height=32, log2_ctb=5))
    cf, bdl, bdc = geom
    try:
        for rect, out_size in COMPOSITION_SIZES:
            r = None if rect is None else chroma_grid_rect(rect, cf)
            resized = ctx.frame_export_finish(ctx.frame_export_resized(frame, capi.EXPORT_PLANAR, capi.EXPORT_NATIVE, out_size, r))
            second = ctx.frame_create(out_size[0], out_size[1], cf, bdl, bdc)
            frames.append(second)
            ctx.frame_upload(second, resized)
            for layout in LAYOUTS:
                for samples in SAMPLES:
                    for matrix, full in MATRIX_CONVERSIONS:
                        chained = ctx.frame_export_finish(ctx.frame_export_rgb(second, layout, samples, matrix, full))
                        got, raws = ctx.frame_export_finish(ctx.frame_export_resized_rgb(frame, layout, samples, matrix, full, out_size, r), raw=True)
                        assert_export(got, raws, chained, "%s rect %s to %dx%d layout %d samples %d matrix %d" % (format_id(cfg), r, out_size[0], out_size[1], layout, samples, matrix))
                        assert not np.all(got[0] == got[0].flat[0]), "a constant picture shows nothing"
    finally:
        for f in frames:
            ctx.frame_destroy(f)


def check_identity(ctx, o, bit_depth, layout):
    """the whole frame at its own size equals frame_export_rgb of the whole frame, byte for byte, the padding included"""
    frame, planes, geom, frames = decode_into_frame(ctx, o, dict(width=64, height=32, bit_depth=bit_depth, seed=7910 + bit_depth, log2_ctb=5))
    try:
        for samples in SAMPLES:
            for matrix, full in MATRIX_CONVERSIONS:
                plain = ctx.frame_export_finish(ctx.frame_export_rgb(frame, layout, samples, matrix, full), raw=True)
                both = ctx.frame_export_finish(ctx.frame_export_resized_rgb(frame, layout, samples, matrix, full, (64, 32)), raw=True)
                assert len(plain[1]) == len(both[1])
                for a, b in zip(plain[1], both[1]):
                    assert a.shape == b.shape and np.array_equal(a, b), "samples %d matrix %d" % (samples, matrix)
                assert not np.all(plain[1][0] == capi.DEVICE_FILL)
    finally:
        for f in frames:
            ctx.frame_destroy(f)


MINIMUM_SIZES = [(None, (2, 2)), (None, (128, 128)), ((4, 4, 4, 4), (2, 2)), ((4, 4, 4, 4), (32, 32))]


def minimum_case(bit_depth):
    return dict(width=16, height=16, bit_depth=bit_depth, seed=7921 + bit_depth, log2_ctb=4)


def check_minimum_sizes(ctx, o, bit_depth):
    """a 16x16 4:2:0 picture to 2x2 (the resized chroma is 1x1: every clamp of both filters folds onto one sample) and to 128x128; its 4x4 rectangle
    at (4, 4) to 2x2 and to 32x32"""
    check_format_matrix(ctx, o, minimum_case(bit_depth), MINIMUM_SIZES)


# (frame size, output size): two column tiles (the runtime evens their widths out: a partial last tile is in check_odd_sizes, 257 columns, and in the
# GPU tier's 854 columns) and three runs of rows — the chroma halo rows are read across the seams at output
# rows 15 / 16 and 31 / 32, the halo column across the seam between the tiles; ratio 8, the widest source span per output column (three tiles); ratio 4
# with 16-bit samples: three tiles whose first columns must stay chroma columns; ratio 6 (two tiles)
SEAM_CASES = (((48, 8), (384, 40)), ((2400, 16), (300, 2)), ((2064, 8), (516, 2)), ((1536, 8), (256, 2)))


def seam_planes():
    """4:2:0, 10 bits, random planes -> [((w, h), out_size, planes)]"""
    rng = np.random.default_rng(7930)
    return [((w, h), out_size, [rng.integers(0, 1024, (ph, pw)).astype(np.uint16) for pw, ph in worklist.plane_dims(w, h, 1)]) for (w, h), out_size in SEAM_CASES]


def check_tile_seams(ctx):
    for (w, h), out_size, planes in seam_planes():
        frame = ctx.frame_create(w, h, 1, 10, 10)
        try:
            ctx.frame_upload(frame, planes)
            check_all(ctx, frame, planes, (1, 10, 10), [(None, out_size)], MATRIX_CONVERSIONS[:1], what="%dx%d" % (w, h))
        finally:
            ctx.frame_destroy(frame)


def check_odd_sizes(ctx):
    """output sizes that are odd (4:4:4, monochrome): a last run of one row where a pass of the kernel takes two, a last tile of one column"""
    rng = np.random.default_rng(7940)
    for cf, size, outs in ((3, (64, 32), [(33, 17), (257, 33), (9, 5)]), (0, (64, 40), [(9, 5), (63, 39)])):
        frame = ctx.frame_create(size[0], size[1], cf, 10, 10)
        try:
            planes = [rng.integers(0, 1024, (ph, pw)).astype(np.uint16) for pw, ph in worklist.plane_dims(size[0], size[1], cf) if pw]
            ctx.frame_upload(frame, planes)
            check_all(ctx, frame, planes, (cf, 10, 10), [(None, o) for o in outs], MATRIX_CONVERSIONS[:1], what="cf %d" % cf)
        finally:
            ctx.frame_destroy(frame)


VALUE_OUT = [(16, 4), (96, 20), (256, 64)]


def check_values(ctx, bd):
    """export_rgb_util.value_cases (128x32, 4:4:4) resized to three sizes under every conversion; the expected outputs of each conversion must hold
    0, M and interior values on every channel, else the clips at both ends are not exercised"""
    frame = ctx.frame_create(128, 32, 3, bd, bd)
    try:
        cases = value_cases(bd)
        for matrix, full in ALL_CONVERSIONS:
            for samples in SAMPLES:
                want = [expected_resized_rgb(planes, 3, bd, bd, capi.RGB_PLANAR, samples, matrix, full, out_size) for _, planes in cases for out_size in VALUE_OUT]
                M = 65535 if samples == capi.RGB_U16 else 255
                for c in range(3):
                    seen = np.concatenate([w[c].ravel() for w in want])
                    assert (seen == 0).any() and (seen == M).any() and ((seen > 0) & (seen < M)).any(), \
                        "channel %d of matrix %d full %d samples %d does not reach both clips and the interior" % (c, matrix, full, samples)
        for name, planes in cases:
            ctx.frame_upload(frame, planes)
            check_all(ctx, frame, planes, (3, bd, bd), [(None, s) for s in VALUE_OUT], ALL_CONVERSIONS, what="%s %d bit" % (name, bd))
    finally:
        ctx.frame_destroy(frame)


def check_gate(ctx, out_size=(80, 48), layout=capi.RGB_PACKED, samples=capi.RGB_U8, matrix=capi.MATRIX_BT709, full=0):
    """export_resized_util.check_gate_resized for the new call: behind a decode whose lists the device rejected it writes nothing, behind an accepted
    decode of the same lists it does"""
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
        tokens.append(ctx.frame_export_resized_rgb(dst, layout, samples, matrix, full, out_size))
    good, bad = [ctx.frame_export_finish(t, raw=True) for t in tokens]
    assert ctx.decode_status(serials[0]) == 0 and ctx.decode_status(serials[1]) == M355_ERR_INVALID
    with_planes = ctx.frame_download(dst)           # (the rejected decode left the accepted picture in the frame)
    assert_export(good[0], good[1], expected_resized_rgb(with_planes, 1, 8, 8, layout, samples, matrix, full, out_size), "behind the accepted decode")
    for raw in bad[1]:
        assert np.all(raw == capi.DEVICE_FILL), "a resized R'G'B' export behind a rejected decode wrote to its destination"
    ctx.wait()
    for f in handles + [dst]:
        ctx.frame_destroy(f)


def check_hazard(ctx, depth, out_size=(80, 36), layout=capi.RGB_PACKED, samples=capi.RGB_U8, matrix=capi.MATRIX_BT709, full=0):
    """export_resized_util.check_hazard_resized for the new call: four pictures decoded alternately into a pool of two frames, each exported right
    behind its decode into a buffer of its own, no host wait in between; every export must deliver what the export of the same picture decoded alone
    delivers.  (On the GPU with several pictures in flight this sees a decode that does not wait for the export of its frame's previous picture; the
    SIMT interpreter finishes every launch before the next call and checks the bookkeeping's results only.)"""
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
            tokens.append(ctx.frame_export_resized_rgb(pool[j % 2], layout, samples, matrix, full, out_size, rect))
        got = [ctx.frame_export_finish(t, raw=True) for t in tokens]
        ctx.wait()
        for j in range(4):
            ctx.decode_resident(handles[j])
            ctx.wait()
            planes = ctx.frame_download(pool[j % 2])
            alone = ctx.frame_export_finish(ctx.frame_export_resized_rgb(pool[j % 2], layout, samples, matrix, full, out_size, rect))
            assert_planes_equal(alone, expected_resized_rgb(planes, 1, 10, 10, layout, samples, matrix, full, out_size, rect), "picture %d alone" % j)
            assert_export(got[j][0], got[j][1], alone, "picture %d, depth %d" % (j, depth))
        for j in (0, 1):
            assert not np.array_equal(got[j][0][0], got[j + 2][0][0]), "the pictures that share a frame must differ for this test to see a hazard"
        for h in handles:
            ctx.release(h)
        for f in pool + [r0]:
            ctx.frame_destroy(f)
    finally:
        ctx.set_pipeline_depth(1)
