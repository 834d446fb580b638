"""Shared by the m355_frames_export_tensor_rois tests (SIMT-interpreter build and GPU): the drivers.  The call is a composition
(include/de265_mi355x.h), and every slice is held against two independent expectations:
  the restatement   export_tensor_util.expected_ints of the planes m355_frame_download returns for the slice's frame, with the slice's rectangle,
                    through export_tensor_util.expected_tensor — the columns reversed for a mirrored slice (the channels of an NHWC pixel keep their
                    order);
  the single call   m355_frames_export_tensor with n = 1 for the same frame and rectangle on the same library, reversed in the same way: the
                    composition through public calls, and the tie to code that this call does not run (another kernel instantiation).
Every comparison is bit-exact, and every byte of the destination that is no element of the tensor must still hold capi.DEVICE_FILL (assert_tensor).
Restatements and single calls are computed once per (frame, rectangle, conversion, output size, ...) and shared through a References object.

tile_w / tiles_of restate the runtime's resize_rgb_tile_w on the CPU: the tests that want slices of different unit counts in one grid assert with
them that their rectangles give the tile counts they were chosen for."""
import numpy as np

from export_tensor_util import (BATCH_CASES, DTYPES, LAYOUTS, SAMPLES, M355_ERR_INVALID, assert_tensor, decode_batch, decode_into_frame,  # noqa: F401
                                expected_ints, expected_tensor, imagenet)
from export_rgb_util import MATRIX_CONVERSIONS
from synth_util import make_case
from libde265_amd import capi, worklist

MIRROR = capi.ROI_MIRROR

# case 1 of the issue: six regions of ONE 128x64 frame — the whole frame, the two 16x8 corners (8x up at 128x64), an inset, an odd-sized inner
# rectangle on the chroma grid, the right half — at three output sizes: 8x down for the whole frame, a middle one, 8x up for the corners
COMPOSITION_ROIS = [(0, 0, 128, 64), (0, 0, 16, 8), (112, 56, 16, 8), (2, 2, 124, 60), (34, 6, 62, 34), (64, 0, 64, 64)]
COMPOSITION_SIZES = [(16, 16), (64, 32), (128, 64)]
# case 2: regions of a 1040x144 10-bit frame to 130x18 (two runs of rows) with 2, 1, 2, 1, 1, 2 tiles across
MIXED_SIZE, MIXED_OUT = (1040, 144), (130, 18)
MIXED_ROIS = [(0, 0, 1040, 144), (0, 0, 130, 18), (0, 126, 1040, 18), (910, 0, 130, 144), (454, 62, 132, 20), (0, 72, 1040, 72)]
MIXED_TILES = [2, 1, 2, 1, 1, 2]
# ... and of an 8-bit frame of the same size to 258x34 (<1, *>): two tiles across in every slice (uniform: 258 columns never fit one tile)
MIXED8_OUT = (258, 34)
MIXED8_ROIS = [(0, 0, 1040, 144), (0, 0, 258, 34), (520, 72, 520, 72), (100, 20, 600, 100)]


def max_taps(sn, dn):
    return min(16, (2 * max(sn, dn) + dn - 1) // dn)


def tile_w(sn, dn, sb, sw):
    """resize_rgb_tile_w of the runtime: the tile width for sn source columns to dn output columns, sb bytes per source sample, sw = SubWidthC"""
    S = 16 // sb
    csn, cdn = sn // sw, dn // sw

    def vectors(w, s, d):
        return ((w - 1) * s // d + 2 + max_taps(s, d) + S - 1) // S

    def fits(w):
        return 2 * vectors(w, sn, dn) <= 256 and (sw != 2 or 4 * vectors(w // 2 + 1, csn, cdn) <= 256)

    w = 256                                     # resize_tile_w: a few columns less where that saves a wavefront of the vertical pass
    nv = vectors(w, sn, dn)
    k = nv // 64
    if k >= 1 and nv % 64 != 0 and nv % 64 <= 16:
        while w > 1 and vectors(w, sn, dn) > 64 * k:
            w -= 1
    if sw == 2:
        w = w & ~1 if w > 2 else 2
    t = w
    while t > 64 and not fits(t):
        t -= sw
    if fits(t):
        w = t
    tiles = (dn + w - 1) // w
    even = (dn + tiles - 1) // tiles
    if sw == 2:
        even = (even + 1) & ~1
    return min(even, w)


def tiles_of(sn, dn, sb, sw):
    return (dn + tile_w(sn, dn, sb, sw) - 1) // tile_w(sn, dn, sb, sw)


def reverse_columns(elements, layout):
    """one slice, (3, h, w) or (h, w, 3), with its pixels in reverse order along x"""
    return elements[:, :, ::-1] if layout == capi.TENSOR_NCHW else elements[:, ::-1, :]


class References:
    """the two expectations of a slice, each computed once and left unchanged"""

    def __init__(self, ctx):
        self.ctx, self.ints, self.single = ctx, {}, {}

    def restated(self, frame, planes, geom, samples, matrix, full, out_size, rect):
        key = (frame, rect, samples, matrix, full, out_size)
        if key not in self.ints:
            self.ints[key] = expected_ints(planes, geom, samples, matrix, full, out_size, rect)
        return self.ints[key]

    def single_call(self, frame, layout, dtype, samples, matrix, full, out_size, scale, bias, rect):
        key = (frame, rect, layout, dtype, samples, matrix, full, out_size, tuple(scale), tuple(bias))
        if key not in self.single:
            got = self.ctx.tensor_export_finish(self.ctx.frames_export_tensor([frame], layout, dtype, samples, matrix, full, out_size, scale, bias, rect))
            assert np.all(got[2] == capi.DEVICE_FILL)
            self.single[key] = got[0][0]
        return self.single[key]


def normalise(rois):
    """(x0, y0, w, h) / (x0, y0, w, h, flags) / None -> (rect or None, flags) per entry"""
    out = []
    for r in rois:
        if r is None or r[2] == 0:
            out.append((None, 0 if r is None or len(r) < 5 else r[4]))
        else:
            out.append((tuple(r[:4]), r[4] if len(r) > 4 else 0))
    return out


def check_rois(ctx, refs, frames, planes, rois, geom, layout, dtype, samples, matrix, full, out_size, scale, bias, host=False, wait_frame=None, what=""):
    """one batch of regions: every slice against the restatement and against the single call; every mirrored entry must have an unmirrored twin (same
    frame, same rectangle) in the batch, and the two slices must be reversals of each other.  -> the elements"""
    what = "%s n %d to %dx%d layout %d dtype %d samples %d matrix %d full %d" % (what, len(frames), out_size[0], out_size[1], layout, dtype, samples, matrix, full)
    entries = normalise(rois)
    args = [(rect if rect is not None else (0, 0, 0, 0)) + (flags,) for rect, flags in entries]
    token = ctx.frames_export_tensor_rois(frames, args, layout, dtype, samples, matrix, full, out_size, scale, bias, host=host)
    got = ctx.tensor_export_finish(token, wait_frame=wait_frame)
    want = []
    for f, p, (rect, flags) in zip(frames, planes, entries):
        ints = refs.restated(f, p, geom, samples, matrix, full, out_size, rect)
        w = expected_tensor([ints], layout, dtype, scale, bias)[0]
        want.append(reverse_columns(w, layout) if flags & MIRROR else w)
    assert_tensor(got, np.stack(want), what)
    for i, (f, (rect, flags)) in enumerate(zip(frames, entries)):
        one = refs.single_call(f, layout, dtype, samples, matrix, full, out_size, scale, bias, rect)
        if flags & MIRROR:
            one = reverse_columns(one, layout)
        assert np.array_equal(got[0][i], one), "%s: slice %d (%s, flags %d) differs from m355_frames_export_tensor with n = 1" % (what, i, rect, flags)
        if flags & MIRROR:
            twins = [j for j, (g, (r2, f2)) in enumerate(zip(frames, entries)) if g == f and r2 == rect and not f2 & MIRROR]
            assert twins, "%s: the mirrored entry %d has no unmirrored twin in the batch" % (what, i)
            assert np.array_equal(got[0][i], reverse_columns(got[0][twins[0]], layout)), "%s: slices %d and %d are no reversals of each other" % (what, i, twins[0])
            assert not np.array_equal(got[0][i], got[0][twins[0]]), "%s: a slice that equals its reversal shows nothing" % what
    return got[0]


def rotate(k):
    """layout, dtype, samples of the k-th export of a test, rotating as export_tensor_util.check_batch does"""
    return LAYOUTS[k % 2], DTYPES[k % 3], SAMPLES[(k // 2) % 2]


def upload_random(ctx, size, cf, bd, seed):
    """a frame filled by m355_frame_upload with seeded random planes -> (frame, planes)"""
    w, h = size
    sw, sh = (2 if cf in (1, 2) else 1), (2 if cf == 1 else 1)
    rng = np.random.default_rng(seed)
    dt = np.uint8 if bd == 8 else np.uint16
    planes = [rng.integers(0, 1 << bd, (h, w)).astype(dt)]
    if cf:
        planes += [rng.integers(0, 1 << bd, (h // sh, w // sw)).astype(dt) for _ in range(2)]
    frame = ctx.frame_create(w, h, cf, bd, bd)
    ctx.frame_upload(frame, planes)
    return frame, planes


def check_composition(ctx, o, mirrored=False):
    """case 1 (mirrored: every region twice, flags alternating per slice)"""
    frame, planes, geom, destroy = decode_into_frame(ctx, o, BATCH_CASES[1])
    refs = References(ctx)
    try:
        rois = COMPOSITION_ROIS if not mirrored else [r + (fl,) for r in COMPOSITION_ROIS for fl in (0, MIRROR)]
        matrix, full = MATRIX_CONVERSIONS[0]
        for k, out_size in enumerate(COMPOSITION_SIZES):
            for layout, dtype, samples in (rotate(2 * k), rotate(2 * k + 1)):
                scale, bias = imagenet(samples)
                check_rois(ctx, refs, [frame] * len(rois), [planes] * len(rois), rois, geom, layout, dtype, samples, matrix, full, out_size, scale, bias,
                           what="composition")
    finally:
        for f in destroy:
            ctx.frame_destroy(f)


def check_mixed_units(ctx, mirrored=False):
    """case 2: slices of different unit counts in one grid, the list as it is and rotated by one (the first slice then has one tile); mirrored: the
    list with a two-tile and a one-tile slice repeated mirrored — the seam between two tiles changes sides"""
    assert [tiles_of(r[2], MIXED_OUT[0], 2, 2) for r in MIXED_ROIS] == MIXED_TILES
    frame, planes = upload_random(ctx, MIXED_SIZE, 1, 10, 8401)
    refs = References(ctx)
    try:
        matrix, full = MATRIX_CONVERSIONS[0]
        if mirrored:
            lists = [MIXED_ROIS + [MIXED_ROIS[0] + (MIRROR,), MIXED_ROIS[4] + (MIRROR,)]]
        else:
            lists = [MIXED_ROIS, MIXED_ROIS[1:] + MIXED_ROIS[:1]]
        for k, rois in enumerate(lists):
            layout, dtype, samples = rotate(k + (2 if mirrored else 0))
            scale, bias = imagenet(samples)
            check_rois(ctx, refs, [frame] * len(rois), [planes] * len(rois), rois, (1, 10, 10), layout, dtype, samples, matrix, full, MIXED_OUT, scale, bias,
                       what="mixed units")
    finally:
        ctx.frame_destroy(frame)


def check_mixed_8bit(ctx):
    """... and an 8-bit frame of the same size to 258x34: the <1, *> instantiations with regions; every slice has two tiles across"""
    assert [tiles_of(r[2], MIXED8_OUT[0], 1, 2) for r in MIXED8_ROIS] == [2] * len(MIXED8_ROIS)
    frame, planes = upload_random(ctx, MIXED_SIZE, 1, 8, 8402)
    refs = References(ctx)
    try:
        for k in range(2):
            layout, dtype, samples = LAYOUTS[k], (capi.TENSOR_F16, capi.TENSOR_F32)[k], SAMPLES[k]
            scale, bias = imagenet(samples)
            check_rois(ctx, refs, [frame] * len(MIXED8_ROIS), [planes] * len(MIXED8_ROIS), MIXED8_ROIS, (1, 8, 8), layout, dtype, samples, capi.MATRIX_BT709, 0,
                       MIXED8_OUT, scale, bias, what="8-bit")
    finally:
        ctx.frame_destroy(frame)


def check_different_sizes(ctx, o):
    """case 3: whole frames of 64x32, 128x64 and 64x32 in one tensor of 32x16 slices (the existing call rejects this)"""
    frames, planes, geom, destroy = decode_batch(ctx, o)
    refs = References(ctx)
    try:
        for k in range(2):
            layout, dtype, samples = rotate(k)
            scale, bias = imagenet(samples)
            check_rois(ctx, refs, frames, planes, [None] * 3, geom, layout, dtype, samples, capi.MATRIX_BT709, 0, (32, 16), scale, bias, what="sizes")
    finally:
        for f in destroy:
            ctx.frame_destroy(f)


def check_mirror_odd_widths(ctx, o):
    """output rows that end in half a dword: a monochrome 8-bit 64x40 frame, region (3, 1, 50, 30) to 33x17 as F16 NCHW and BF16 NHWC, and the 4:4:4
    10-bit picture of FORMATS to 33x17; every region plain and mirrored"""
    from export_tensor_util import FORMATS
    mono, mplanes = upload_random(ctx, (64, 40), 0, 8, 8403)
    frame, planes, geom, destroy = decode_into_frame(ctx, o, dict(FORMATS[3], width=64, height=32, log2_ctb=5))
    assert geom[0] == 3
    refs = References(ctx)
    try:
        scale, bias = imagenet(capi.RGB_U8)
        for layout, dtype in ((capi.TENSOR_NCHW, capi.TENSOR_F16), (capi.TENSOR_NHWC, capi.TENSOR_BF16)):
            rois = [(3, 1, 50, 30, 0), (3, 1, 50, 30, MIRROR)]
            check_rois(ctx, refs, [mono] * 2, [mplanes] * 2, rois, (0, 8, 8), layout, dtype, capi.RGB_U8, capi.MATRIX_BT709, 0, (33, 17), scale, bias, what="mono")
            rois = [(0, 0, 64, 32, MIRROR), (0, 0, 64, 32, 0), (5, 3, 41, 21, 0), (5, 3, 41, 21, MIRROR)]
            check_rois(ctx, refs, [frame] * 4, [planes] * 4, rois, geom, layout, dtype, capi.RGB_U8, capi.MATRIX_BT709, 0, (33, 17), scale, bias, what="4:4:4")
    finally:
        for f in destroy + [mono]:
            ctx.frame_destroy(f)


def full_array_rois(seed=8404):
    """32 different regions of a 128x64 4:2:0 frame that 16x16 accepts: widths 2..128, heights 2..64, all on the chroma grid"""
    rng = np.random.default_rng(seed)
    rois = set()
    while len(rois) < 32:
        w, h = 2 * int(rng.integers(1, 65)), 2 * int(rng.integers(1, 33))
        rois.add((2 * int(rng.integers(0, (128 - w) // 2 + 1)), 2 * int(rng.integers(0, (64 - h) // 2 + 1)), w, h))
    return sorted(rois)


def check_full_array(ctx, o):
    """case 5: the whole record array — 32 different regions of one frame, and 32 times the same region, which must equal m355_frames_export_tensor
    of 32 times the frame with that rectangle, byte for byte (the whole buffers)"""
    frame, planes, geom, destroy = decode_into_frame(ctx, o, BATCH_CASES[1])
    refs = References(ctx)
    try:
        scale, bias = imagenet(capi.RGB_U8)
        rois = full_array_rois()
        assert len(set(rois)) == 32
        check_rois(ctx, refs, [frame] * 32, [planes] * 32, rois, geom, capi.TENSOR_NCHW, capi.TENSOR_F16, capi.RGB_U8, capi.MATRIX_BT709, 0, (16, 16), scale, bias,
                   what="32 regions")
        rect = (34, 6, 62, 34)
        for layout, dtype in ((capi.TENSOR_NHWC, capi.TENSOR_F32), (capi.TENSOR_NCHW, capi.TENSOR_BF16)):
            args = (layout, dtype, capi.RGB_U8, capi.MATRIX_BT709, 0, (16, 16), scale, bias)
            new = ctx.tensor_export_finish(ctx.frames_export_tensor_rois([frame] * 32, [rect + (0,)] * 32, *args))
            old = ctx.tensor_export_finish(ctx.frames_export_tensor([frame] * 32, *args, rect))
            assert np.array_equal(new[1], old[1]), "32 times one region differs from m355_frames_export_tensor with that rectangle"
            assert not np.all(new[0] == new[0].flat[0])
    finally:
        for f in destroy:
            ctx.frame_destroy(f)


def check_gate(ctx, out_size=(80, 48)):
    """export_tensor_util.check_gate with regions: two regions of a frame behind a rejected decode are skipped, the regions of a frame behind an
    accepted decode and of an uploaded frame are written"""
    cfg = dict(width=128, height=64, bit_depth=8, seed=7501, intra_pct=30)
    pic, refs_ = make_case(**cfg)
    pp = pic.pp[0]
    handles = []
    for planes in refs_:
        f = ctx.frame_create_for(pp)
        ctx.frame_upload(f, planes)
        handles.append(f)
    good, bad = ctx.frame_create_for(pp), ctx.frame_create_for(pp)
    ctx.frame_fill(bad, 77, 99)
    serials = []
    for dst, corrupt in ((good, False), (bad, True)):
        p = make_case(**cfg)[0]
        p.ref_frames = [handles[i] if i < len(handles) else -1 for i in range(worklist.MAX_REF_FRAMES)]
        p.dst_frame = dst
        if corrupt:
            arr = p.ibs.copy(); arr["mode"][len(arr) // 2] = 77; p.ibs = arr
        ctx.submit_in_place(p, fill_threads=1)
        serials.append(ctx.last_serial())
    scale, bias = imagenet(capi.RGB_U8)
    batches = ((capi.TENSOR_NCHW, capi.TENSOR_F16, [(good, (0, 0, 128, 64, 0)), (bad, (0, 0, 64, 32, 0)), (handles[0], (16, 8, 96, 48, MIRROR)), (bad, (32, 16, 96, 48, MIRROR))]),
               (capi.TENSOR_NHWC, capi.TENSOR_F32, [(bad, (0, 0, 128, 64, 0)), (bad, (64, 32, 64, 32, 0)), (good, (2, 2, 120, 60, 0))]))
    for layout, dtype, batch in batches:
        token = ctx.frames_export_tensor_rois([f for f, _ in batch], [r for _, r in batch], layout, dtype, capi.RGB_U8, capi.MATRIX_BT709, 0, out_size, scale, bias)
        elements, raw, outside = ctx.tensor_export_finish(token)
        assert ctx.decode_status(serials[0]) == 0 and ctx.decode_status(serials[1]) == M355_ERR_INVALID
        assert np.all(outside == capi.DEVICE_FILL)
        fill = (capi.DEVICE_FILL * 0x01010101) & (0xFFFFFFFF if dtype == capi.TENSOR_F32 else 0xFFFF)
        for i, (f, r) in enumerate(batch):
            if f == bad:
                assert np.all(elements[i] == fill), "the slice of a frame behind a rejected decode was written"
            else:
                ints = [expected_ints(ctx.frame_download(f), (1, 8, 8), capi.RGB_U8, capi.MATRIX_BT709, 0, out_size, r[:4])]
                want = expected_tensor(ints, layout, dtype, scale, bias)[0]
                assert np.array_equal(elements[i], reverse_columns(want, layout) if r[4] else want), "slice %d beside a rejected frame" % i
    ctx.wait()
    for f in handles + [good, bad]:
        ctx.frame_destroy(f)


def check_hazard(ctx, depth, out_size=(80, 36), layout=capi.TENSOR_NCHW, dtype=capi.TENSOR_F16):
    """export_tensor_util.check_hazard with regions: behind each decode a batch of [a region of the reference frame, two regions of the frame just
    decoded, one of them mirrored], no host wait in between.  The decoded frame is not frames[0]: the next decode into it waits for the batch's one
    mark, which every frame of the batch keeps"""
    from libde265_amd import synth
    ctx.set_pipeline_depth(depth)
    try:
        cfg = dict(width=128, height=64, bit_depth=10, seed=5, n_refs=1)
        pics = [synth.picture(**dict(cfg, seed=5 + j)) for j in range(4)]
        pp = pics[0].pp[0]
        r0 = ctx.frame_create_for(pp)
        ref = synth.ref_planes(5, 128, 64, 1, 10)
        ctx.frame_upload(r0, ref)
        pool = [ctx.frame_create_for(pp) for _ in range(2)]
        rois = [(2, 2, 120, 56, 0), (0, 0, 128, 64, 0), (40, 8, 80, 40, MIRROR)]
        scale, bias = imagenet(capi.RGB_U8)
        args = (layout, dtype, capi.RGB_U8, capi.MATRIX_BT709, 0, out_size, scale, bias)
        handles, tokens = [], []
        for j, pic in enumerate(pics):
            pic.ref_frames = [r0] + [-1] * (worklist.MAX_REF_FRAMES - 1)
            pic.dst_frame = pool[j % 2]
            handles.append(ctx.upload(pic))
            ctx.decode_resident(handles[-1])
            tokens.append(ctx.frames_export_tensor_rois([r0, pool[j % 2], pool[j % 2]], rois, *args))
        got = [ctx.tensor_export_finish(t) for t in tokens]
        ctx.wait()
        for j in range(4):
            ctx.decode_resident(handles[j])
            ctx.wait()
            dec = ctx.frame_download(pool[j % 2])
            want = []
            for p, r in zip([ref, dec, dec], rois):
                w = expected_tensor([expected_ints(p, (1, 10, 10), capi.RGB_U8, capi.MATRIX_BT709, 0, out_size, r[:4])], layout, dtype, scale, bias)[0]
                want.append(reverse_columns(w, layout) if r[4] else w)
            assert_tensor(got[j], np.stack(want), "picture %d, depth %d" % (j, depth))
        for j in (0, 1):
            assert not np.array_equal(got[j][0][1], got[j + 2][0][1]), "the pictures that share a frame must differ for this test to see a hazard"
        for h in handles:
            ctx.release(h)
        for f in pool + [r0]:
            ctx.frame_destroy(f)
    finally:
        ctx.set_pipeline_depth(1)


def check_pinned_host(ctx, o):
    """a pinned-host destination, read by the host behind m355_frame_export_wait of ONE frame of the batch — the last, then the middle one"""
    frames, planes, geom, destroy = decode_batch(ctx, o)
    refs = References(ctx)
    try:
        scale, bias = imagenet(capi.RGB_U16)
        rois = [(0, 0, 64, 32, 0), (8, 4, 100, 44, 0), (8, 4, 100, 44, MIRROR), None]
        batch, bplanes = [frames[0], frames[1], frames[1], frames[2]], [planes[0], planes[1], planes[1], planes[2]]
        for wait_frame, layout, dtype in ((frames[2], capi.TENSOR_NHWC, capi.TENSOR_BF16), (frames[1], capi.TENSOR_NCHW, capi.TENSOR_F32)):
            check_rois(ctx, refs, batch, bplanes, rois, geom, layout, dtype, capi.RGB_U16, capi.MATRIX_BT709, 0, (36, 14), scale, bias, host=True,
                       wait_frame=wait_frame, what="pinned, waited for frame %d" % wait_frame)
            for f in frames:
                ctx.frame_export_wait(f)
    finally:
        for f in destroy:
            ctx.frame_destroy(f)
