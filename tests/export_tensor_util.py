"""Shared by the m355_frames_export_tensor tests (SIMT-interpreter build, GPU and glue): the restatement of what the call delivers and the drivers
that check exports against it.  The definition is a composition (include/de265_mi355x.h), and so is the restatement:
  the integers   export_resized_rgb_util.expected_resized_rgb (planar: R, G, B) of the planes m355_frame_download returns, per slice — and the drivers
                 also hold them against what the existing m355_frame_export_resized_rgb call delivers for the same frame;
  the float stage in numpy: np.float32(v) * np.float32(scale) + np.float32(bias) as two separate float32 operations (numpy does not fuse them),
                 then F32 as it is, F16 through .astype(np.float16) (round to nearest even, gradual underflow, overflow to infinity), BF16 through the
                 integer expression (bits + 0x7FFF + ((bits >> 16) & 1)) >> 16 on the uint32 view.
Every comparison is bit-exact on the uint16 / uint32 views of the elements, and every byte of the destination that is no element of the tensor — row
padding, the gaps between planes and between slices — must still hold capi.DEVICE_FILL."""
import numpy as np

from export_util import FORMATS, chroma_grid_rect, decode_into_frame, format_id  # noqa: F401
from export_resized_util import MATRIX_RECT, MATRIX_SIZES
from export_resized_rgb_util import MINIMUM_SIZES, M355_ERR_INVALID, expected_resized_rgb, minimum_case  # noqa: F401
from export_rgb_util import MATRIX_CONVERSIONS
from synth_util import make_case
from libde265_amd import capi, worklist

LAYOUTS = (capi.TENSOR_NCHW, capi.TENSOR_NHWC)
DTYPES = (capi.TENSOR_F32, capi.TENSOR_F16, capi.TENSOR_BF16)
SAMPLES = (capi.RGB_U8, capi.RGB_U16)
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


# (scale, bias) of the tests that run the float stage over every integer 0..65535: identity, 1 / 255, the three ImageNet pairs, 1 / 65535 (small v give
# binary16 subnormals) and (2, -3) (large v overflow binary16 to infinity); none makes a nonzero binary32 subnormal
ELEMENT_PAIRS = [(1.0, 0.0), (1.0 / 255.0, 0.0)] + [(1.0 / (255.0 * s), -m / s) for m, s in zip(IMAGENET_MEAN, IMAGENET_STD)] + [(1.0 / 65535.0, 0.0), (2.0, -3.0)]


def imagenet(samples):
    """(scale, bias) per channel of the usual normalisation of a 0..1 picture, for integers 0..255 or 0..65535: x / M is folded into the scale"""
    M = 65535.0 if samples == capi.RGB_U16 else 255.0
    return [1.0 / (M * s) for s in IMAGENET_STD], [-m / s for m, s in zip(IMAGENET_MEAN, IMAGENET_STD)]


def bf16_bits(r):
    """float32 array -> bfloat16 bit patterns (uint16), round to nearest even, by the integer expression of the header"""
    bits = np.ascontiguousarray(r, np.float32).view(np.uint32).astype(np.uint64)
    return ((bits + 0x7FFF + ((bits >> 16) & 1)) >> 16).astype(np.uint16)


def element_bits(v, scale, bias, dtype):
    """m355_tensor_element on an array of integers -> uint32 (F32) or uint16 bit patterns"""
    with np.errstate(over="ignore"):
        t = v.astype(np.float32) * np.float32(scale)
        r = t + np.float32(bias)
        assert t.dtype == np.float32 and r.dtype == np.float32
        if dtype == capi.TENSOR_F32:
            return r.view(np.uint32)
        if dtype == capi.TENSOR_F16:
            return r.astype(np.float16).view(np.uint16)
    return bf16_bits(r)


def expected_tensor(ints, layout, dtype, scale, bias):
    """ints: per slice the planes [R, G, B] of the integer stage -> the elements' bit patterns, (n, 3, h, w) or (n, h, w, 3)"""
    out = np.stack([np.stack([element_bits(rgb[c], scale[c], bias[c], dtype) for c in range(3)]) for rgb in ints])
    return np.ascontiguousarray(out.transpose(0, 2, 3, 1)) if layout == capi.TENSOR_NHWC else out


def expected_ints(planes, geom, samples, matrix, full_range, out_size, rect=None):
    cf, bdl, bdc = geom
    return expected_resized_rgb(planes, cf, bdl, bdc, capi.RGB_PLANAR, samples, matrix, full_range, out_size, rect)


def assert_tensor(got, want, what):
    elements, raw, outside = got
    assert elements.dtype == want.dtype and elements.shape == want.shape, "%s: %s %s, expected %s %s" % (what, elements.dtype, elements.shape, want.dtype, want.shape)
    if not np.array_equal(elements, want):
        bad = np.argwhere(elements != want)
        k = tuple(bad[0])
        raise AssertionError("%s: %d of %d elements differ, first at %s: 0x%x, expected 0x%x" % (what, len(bad), want.size, k, int(elements[k]), int(want[k])))
    assert outside.size and np.all(outside == capi.DEVICE_FILL), "%s: bytes that are no element of the tensor were written" % what


def check_tensor(ctx, frames, planes, geom, layout, dtype, samples, matrix, full_range, out_size, scale, bias, rect=None, host=False, what="", ints=None,
                 against_call=True):
    """one batch against the restatement; planes[i] = what m355_frame_download returns for frames[i].  against_call: the integers of the restatement
    are also held against the planar output of the existing m355_frame_export_resized_rgb call for each distinct frame (left unchanged: computed
    once per frame).  -> the elements"""
    what = "%s n %d to %dx%d layout %d dtype %d samples %d matrix %d full %d rect %s" % (what, len(frames), out_size[0], out_size[1], layout, dtype, samples,
                                                                                      matrix, full_range, rect)
    if ints is None:
        ints = [expected_ints(p, geom, samples, matrix, full_range, out_size, rect) for p in planes]
    if against_call:
        seen = set()
        for f, rgb in zip(frames, ints):
            if f in seen:
                continue
            seen.add(f)
            call = ctx.frame_export_finish(ctx.frame_export_resized_rgb(f, capi.RGB_PLANAR, samples, matrix, full_range, out_size, rect))
            for c in range(3):
                assert np.array_equal(call[c], rgb[c]), "%s: the restatement's integers differ from m355_frame_export_resized_rgb, channel %d" % (what, c)
    got = ctx.tensor_export_finish(ctx.frames_export_tensor(frames, layout, dtype, samples, matrix, full_range, out_size, scale, bias, rect, host=host))
    assert_tensor(got, expected_tensor(ints, layout, dtype, scale, bias), what)
    return got[0]


def check_format_matrix(ctx, o, cfg):
    """one 64x32 picture of a format, exported alone: every (rectangle, output size) of the resized exports' matrix x layout x dtype; U8 / U16 of the
    integer stage and the two conversions of the R'G'B' matrix alternate from export to export, so each layout and dtype meets both"""
    frame, planes, geom, frames = decode_into_frame(ctx, o, cfg)
    try:
        k = 0
        for rect, out_size in MATRIX_SIZES:
            r = None if rect is None else chroma_grid_rect(rect, geom[0])
            for layout in LAYOUTS:
                for dtype in DTYPES:
                    samples = SAMPLES[(k + k // 6) % 2]
                    matrix, full = MATRIX_CONVERSIONS[(k // 2) % 2]
                    scale, bias = imagenet(samples)
                    check_tensor(ctx, [frame], [planes], geom, layout, dtype, samples, matrix, full, out_size, scale, bias, r, what=format_id(cfg),
                                 against_call=(dtype == capi.TENSOR_F32))
                    k += 1
    finally:
        for f in frames:
            ctx.frame_destroy(f)


def check_composition(ctx, o, cfg):
    """through the public calls alone, no Python arithmetic but int -> float: n = 1, F32, scale 1, bias 0 delivers the bytes of
    m355_frame_export_resized_rgb converted to float"""
    frame, planes, geom, frames = decode_into_frame(ctx, o, cfg)
    try:
        for rect, out_size in MATRIX_SIZES:
            r = None if rect is None else chroma_grid_rect(rect, geom[0])
            for samples in SAMPLES:
                matrix, full = MATRIX_CONVERSIONS[samples]
                call = ctx.frame_export_finish(ctx.frame_export_resized_rgb(frame, capi.RGB_PLANAR, samples, matrix, full, out_size, r))
                packed = ctx.frame_export_finish(ctx.frame_export_resized_rgb(frame, capi.RGB_PACKED, samples, matrix, full, out_size, r))[0]
                assert not np.all(call[0] == call[0].flat[0]), "a constant picture shows nothing"
                for layout in LAYOUTS:
                    got = ctx.tensor_export_finish(ctx.frames_export_tensor([frame], layout, capi.TENSOR_F32, samples, matrix, full, out_size, (1, 1, 1), (0, 0, 0), r))
                    if layout == capi.TENSOR_NCHW:
                        want = np.stack(call).astype(np.float32)[None]
                    else:
                        want = packed.reshape(out_size[1], out_size[0], 3).astype(np.float32)[None]
                    assert_tensor(got, want.view(np.uint32), "%s rect %s to %dx%d layout %d samples %d" % (format_id(cfg), r, out_size[0], out_size[1], layout, samples))
    finally:
        for f in frames:
            ctx.frame_destroy(f)


BATCH_CASES = [dict(width=64, height=32, bit_depth=10, seed=8101, log2_ctb=5), dict(width=128, height=64, bit_depth=10, seed=8102, log2_ctb=5),
               dict(width=64, height=32, bit_depth=10, seed=8103, log2_ctb=5)]
BATCH_RECT = (0, 0, 64, 32)
# one workgroup per slice; two tiles across (the runtime evens them out: the seam lies at an odd multiple of 2) and three runs of rows per slice
BATCH_SIZES = [(16, 16), (258, 34)]


def decode_batch(ctx, o, cases=BATCH_CASES):
    """-> (frames, planes, geom, frames to destroy): one decoded picture per case, of different content (and here of different sizes, so of different
    pitches)"""
    frames, planes, destroy, geom = [], [], [], None
    for cfg in cases:
        f, p, g, fs = decode_into_frame(ctx, o, cfg)
        assert geom is None or g == geom
        geom = g
        frames.append(f); planes.append(p); destroy += fs
    return frames, planes, geom, destroy


def crop(planes, rect, cf):
    sw, sh = (2 if cf in (1, 2) else 1), (2 if cf == 1 else 1)
    x0, y0, w, h = rect
    return [p[(y0 // (sh if c else 1)):((y0 + h) // (sh if c else 1)), (x0 // (sw if c else 1)):((x0 + w) // (sw if c else 1))] for c, p in enumerate(planes)]


def check_batch(ctx, o):
    """three distinct frames of different content, the second one larger than the others (another pitch), the rectangle (0, 0, 64, 32) of each: every
    slice is its own frame's picture; n = 1 and n = 3 at both sizes of BATCH_SIZES, so that the split of the grid index into slice and tile is
    exercised where a slice is one workgroup and where it is several"""
    frames, planes, geom, destroy = decode_batch(ctx, o)
    try:
        assert not np.array_equal(crop(planes[0], BATCH_RECT, 1)[0], crop(planes[1], BATCH_RECT, 1)[0]) and not np.array_equal(planes[0][0], planes[2][0])
        k = 0
        for out_size in BATCH_SIZES:
            matrix, full = MATRIX_CONVERSIONS[0]
            for samples in SAMPLES:
                ints = [expected_ints(p, geom, samples, matrix, full, out_size, BATCH_RECT) for p in planes]
                scale, bias = imagenet(samples)
                for layout in LAYOUTS:
                    dtype = DTYPES[k % 3]
                    k += 1
                    check_tensor(ctx, frames, planes, geom, layout, dtype, samples, matrix, full, out_size, scale, bias, BATCH_RECT, what="batch", ints=ints,
                                 against_call=(layout == capi.TENSOR_NCHW))
                    check_tensor(ctx, frames[1:2], planes[1:2], geom, layout, dtype, samples, matrix, full, out_size, scale, bias, BATCH_RECT, what="single",
                                 ints=ints[1:2], against_call=False)
    finally:
        for f in destroy:
            ctx.frame_destroy(f)


def check_same_frame_twice(ctx, o):
    frame, planes, geom, destroy = decode_into_frame(ctx, o, BATCH_CASES[0])
    try:
        scale, bias = imagenet(capi.RGB_U8)
        for layout, dtype in ((capi.TENSOR_NCHW, capi.TENSOR_F16), (capi.TENSOR_NHWC, capi.TENSOR_F32)):
            got = check_tensor(ctx, [frame, frame], [planes, planes], geom, layout, dtype, capi.RGB_U8, capi.MATRIX_BT709, 0, (40, 18), scale, bias, what="twice")
            assert np.array_equal(got[0], got[1])
    finally:
        for f in destroy:
            ctx.frame_destroy(f)


def check_minimum_sizes(ctx, o, bit_depth):
    """export_resized_rgb_util.MINIMUM_SIZES as a batch of two (the frame and a second one of other content): 2x2 outputs, whose rows are shorter
    than a dword for 2-byte elements in NCHW"""
    cases = [minimum_case(bit_depth), dict(minimum_case(bit_depth), seed=8200 + bit_depth)]
    frames, planes, geom, destroy = decode_batch(ctx, o, cases)
    try:
        k = 0
        for rect, out_size in MINIMUM_SIZES:
            for layout in LAYOUTS:
                for dtype in DTYPES:
                    samples = SAMPLES[k % 2]
                    k += 1
                    scale, bias = imagenet(samples)
                    check_tensor(ctx, frames, planes, geom, layout, dtype, samples, capi.MATRIX_BT709, 0, out_size, scale, bias, rect, what="minimum",
                                 against_call=(dtype == capi.TENSOR_F32))
    finally:
        for f in destroy:
            ctx.frame_destroy(f)


def check_gate(ctx, out_size=(80, 48)):
    """a batch of three frames: one behind an accepted decode, one behind a decode whose lists the device rejected, one that no decode wrote (an
    uploaded reference).  The rejected frame's slice is untouched, the other two are what the restatement says"""
    cfg = dict(width=128, height=64, bit_depth=8, seed=7501, intra_pct=30)
    pic, refs = make_case(**cfg)
    pp = pic.pp[0]
    handles = []
    for planes in refs:
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
    for layout, dtype, batch in ((capi.TENSOR_NCHW, capi.TENSOR_F16, [good, bad, handles[0]]), (capi.TENSOR_NHWC, capi.TENSOR_F32, [bad, handles[0], good])):
        token = ctx.frames_export_tensor(batch, layout, dtype, capi.RGB_U8, capi.MATRIX_BT709, 0, out_size, scale, bias)
        elements, raw, outside = ctx.tensor_export_finish(token)
        assert ctx.decode_status(serials[0]) == 0 and ctx.decode_status(serials[1]) == M355_ERR_INVALID
        assert np.all(outside == capi.DEVICE_FILL)
        fill = (capi.DEVICE_FILL * 0x01010101) & (0xFFFFFFFF if dtype == capi.TENSOR_F32 else 0xFFFF)
        for i, f in enumerate(batch):
            if f == bad:
                assert np.all(elements[i] == fill), "the slice of a frame behind a rejected decode was written"
            else:
                ints = [expected_ints(ctx.frame_download(f), (1, 8, 8), capi.RGB_U8, capi.MATRIX_BT709, 0, out_size)]
                want = expected_tensor(ints, layout, dtype, scale, bias)[0]
                assert np.array_equal(elements[i], want), "slice %d beside a rejected frame" % i
    ctx.wait()
    for f in handles + [good, bad]:
        ctx.frame_destroy(f)


def check_hazard(ctx, depth, out_size=(80, 36), layout=capi.TENSOR_NCHW, dtype=capi.TENSOR_F16):
    """export_resized_rgb_util.check_hazard for batches: four pictures decoded alternately into a pool of two frames, and right behind each decode a
    batch of [the reference frame, the frame just decoded] into a buffer of its own, no host wait in between.  The decoded frame is NOT frames[0]:
    what makes the next decode into it wait is the batch's one mark, which every frame of the batch keeps.  Every batch must deliver what a batch of
    the same pictures, decoded alone, delivers.  (On the GPU with several pictures in flight this sees a decode that does not wait for the batch that
    reads its frame; the SIMT interpreter finishes every launch before the next call and checks the bookkeeping's results only.)"""
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
        rect = (2, 2, 120, 56)
        scale, bias = imagenet(capi.RGB_U8)
        args = (layout, dtype, capi.RGB_U8, capi.MATRIX_BT709, 0, out_size, scale, bias, rect)
        handles, tokens = [], []
        for j, pic in enumerate(pics):
            pic.ref_frames = [r0] + [-1] * (worklist.MAX_REF_FRAMES - 1)
            pic.dst_frame = pool[j % 2]
            handles.append(ctx.upload(pic))
            ctx.decode_resident(handles[-1])
            tokens.append(ctx.frames_export_tensor([r0, pool[j % 2]], *args))
        got = [ctx.tensor_export_finish(t) for t in tokens]
        ctx.wait()
        for j in range(4):
            ctx.decode_resident(handles[j])
            ctx.wait()
            planes = [ref, ctx.frame_download(pool[j % 2])]
            ints = [expected_ints(p, (1, 10, 10), capi.RGB_U8, capi.MATRIX_BT709, 0, out_size, rect) for p in planes]
            assert_tensor(got[j], expected_tensor(ints, layout, dtype, scale, bias), "picture %d, depth %d" % (j, depth))
        for j in (0, 1):
            assert not np.array_equal(got[j][0][1], got[j + 2][0][1]), "the pictures that share a frame must differ for this test to see a hazard"
        for h in handles:
            ctx.release(h)
        for f in pool + [r0]:
            ctx.frame_destroy(f)
    finally:
        ctx.set_pipeline_depth(1)


def check_pinned_host(ctx, o):
    """a pinned-host destination, read by the host behind m355_frame_export_wait alone — of the batch's LAST frame, then (a second batch) of its middle
    one: every frame of the batch holds the one mark behind the launch"""
    frames, planes, geom, destroy = decode_batch(ctx, o)
    try:
        scale, bias = imagenet(capi.RGB_U16)
        ints = [expected_ints(p, geom, capi.RGB_U16, capi.MATRIX_BT709, 0, (36, 14), BATCH_RECT) for p in planes]
        for wait_frame, layout, dtype in ((frames[2], capi.TENSOR_NHWC, capi.TENSOR_BF16), (frames[1], capi.TENSOR_NCHW, capi.TENSOR_F32)):
            token = ctx.frames_export_tensor(frames, layout, dtype, capi.RGB_U16, capi.MATRIX_BT709, 0, (36, 14), scale, bias, BATCH_RECT, host=True)
            got = ctx.tensor_export_finish(token, wait_frame=wait_frame)
            assert_tensor(got, expected_tensor(ints, layout, dtype, scale, bias), "pinned, waited for frame %d" % wait_frame)
            for f in frames:
                ctx.frame_export_wait(f)          # (each frame of the batch has the mark, or none: either way this returns)
    finally:
        for f in destroy:
            ctx.frame_destroy(f)


def check_every_integer(ctx):
    """the DEVICE's float stage over every integer 0..65535 (the host function has tests/test_tensor_element.py): a 256x256 monochrome 16-bit frame
    whose sample at (x, y) is 256 y + x, exported at its own size (the resize is the identity), full range to U16, where the matrix has cy = 1 << F
    and R = G = B = the sample — so the integers of the tensor are 0..65535, each once per channel, which the restatement confirms before anything is
    compared.  ELEMENT_PAIRS go three at a time into the three channels, under every dtype and both layouts (alternating)."""
    planes = [np.arange(65536, dtype=np.uint16).reshape(256, 256)]
    frame = ctx.frame_create(256, 256, 0, 16, 16)
    try:
        ctx.frame_upload(frame, planes)
        ints = [expected_ints(planes, (0, 16, 16), capi.RGB_U16, capi.MATRIX_BT709, 1, (256, 256))]
        for c in range(3):
            assert np.array_equal(ints[0][c], planes[0]), "the integer stage is not the identity here"
        k = 0
        for first in range(0, len(ELEMENT_PAIRS), 3):
            pairs = (ELEMENT_PAIRS[first:first + 3] + ELEMENT_PAIRS[:2])[:3]
            scale, bias = [p[0] for p in pairs], [p[1] for p in pairs]
            for dtype in DTYPES:
                check_tensor(ctx, [frame], [planes], (0, 16, 16), LAYOUTS[k % 2], dtype, capi.RGB_U16, capi.MATRIX_BT709, 1, (256, 256), scale, bias,
                             what="every integer, pairs from %d" % first, ints=ints, against_call=(k == 0))
                k += 1
    finally:
        ctx.frame_destroy(frame)
