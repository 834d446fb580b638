"""Shared by the tone-object tests (SIMT-interpreter build, GPU and glue): TONE OBJECTS of include/de265_mi355x.h restated in Python integers / numpy
int64 — the pixel function with its step 2b, the preset builder in doubles — on top of export_colour_util.py (imported, not copied: steps 1, 2, the
index and the composed exports' U16 integers are its).  A SET is the tables of export_colour_util plus a "tone" entry (norm, weights, gain); a set
without one is a plain object.  Three sets: RANDOM (seeded, NORM_LUMA), EXTREME (gain entries 0 and GAIN_ONE only, weights +-65535, NORM_LUMA) and the
PRESET PQ / BT.2020 -> gamma 2.4 / BT.709, BT.2390, maxRGB, 203 / 1000 nits.  Every comparison of pixels is exact, destination padding included."""
import math

import numpy as np

import export_colour_util as cu
from export_colour_util import (BIAS, FULL, KERNEL_CASES, KERNEL_LOCS, MATRIX, ONE, OUT_KNOTS, SCALE, TENSOR_FORMATS, U8, U16, census_planes, ints16, knot,
                                out_index, random_planes, upload)
from export_rgb_util import M355_ERR_INVALID, shape_rgb  # noqa: F401
from export_siting_util import TENSOR_ROIS, assert_same_bytes, finish
from export_tensor_util import assert_tensor, expected_tensor
from export_tensor_rois_util import reverse_columns
from export_util import assert_export
from synth_util import make_case
from libde265_amd import capi, worklist

GAIN_ONE, MAXRGB, LUMA = capi.TONE_GAIN_ONE, capi.NORM_MAXRGB, capi.NORM_LUMA
WIDE = ((320, 48), (272, 40))        # two column tiles, three row tiles


# ---- the pixel function ------------------------------------------------------------------------------------------------------------------------------

def stage_values(S, rgb16):
    """steps 1, 2 and 2b -> dict(P = the three clipped matrix outputs, s = the norm's sum before its clip (LUMA), n, idx, fr, g, Pt = the three P')"""
    P = [np.clip(s, 0, ONE) for s in cu.linear_and_sums(S, rgb16)[1]]
    q = S["tone"]
    w = [int(x) for x in q["weights"]]
    s = (w[0] * P[0] + w[1] * P[1] + w[2] * P[2] + (1 << 13)) >> 14
    n = np.clip(s, 0, ONE) if q["norm"] == LUMA else np.maximum(np.maximum(P[0], P[1]), P[2])
    idx, fr = out_index(n)
    gain = q["gain"].astype(np.int64)
    g = (gain[idx] * (256 - fr) + gain[np.minimum(idx + 1, OUT_KNOTS - 1)] * fr + 128) >> 8
    return dict(P=P, s=s, n=n, idx=idx, fr=fr, g=g, Pt=[(p * g + (1 << 23)) >> 24 for p in P])


def pixels(S, rgb16, samples):
    """m355_colour_pixel_tone over arrays (a set without a tone: m355_colour_pixel): three int64 arrays of 0..65535 -> three int64 arrays"""
    if "tone" not in S:
        return cu.colour_pixels(S, rgb16, samples)
    lo = S["lut_out"].astype(np.int64)
    out = []
    for P in stage_values(S, rgb16)["Pt"]:
        idx, fr = out_index(P)
        o = (lo[idx] * (256 - fr) + lo[np.minimum(idx + 1, OUT_KNOTS - 1)] * fr + 128) >> 8
        out.append(o if samples == U16 else (2 * o + 257) // 514)
    return out


def tone_ctypes(S, reserved=(0, 0, 0)):
    q = S["tone"]
    return capi.colour_tone(q["norm"], q["weights"], q["gain"], reserved)


def create(ctx, S):
    """the set as an object of the context: a tone object, or a plain one for a set without a tone"""
    if "tone" not in S:
        return ctx.colour_create(cu.to_ctypes(S))
    return ctx.colour_create_tone(cu.to_ctypes(S), tone_ctypes(S))


def from_ctypes(t, q):
    return dict(cu.from_ctypes(t), tone=dict(norm=int(q.norm), weights=np.array(q.weights[:], np.int64), gain=np.array(q.gain[:], np.int64)))


# ---- the tone preset in doubles --------------------------------------------------------------------------------------------------------------------------

def pq_inverse(nits):
    m1, m2, c1, c2, c3 = 2610 / 16384, 2523 / 4096 * 128, 3424 / 4096, 2413 / 4096 * 32, 2392 / 4096 * 32
    p = (max(nits, 0.0) / 10000.0) ** m1
    return ((c1 + c2 * p) / (1 + c3 * p)) ** m2


def tone_curve(tone, x, white, peak):
    """y(x) of the preset's tone: x and y in units of white"""
    if tone == capi.TONE_REINHARD:
        w = max(1.0, peak / white)
        return min(1.0, x * (1 + x / (w * w)) / (1 + x))
    if tone == capi.TONE_BT2390:
        lw = pq_inverse(peak)
        max_lum = pq_inverse(white) / lw
        if max_lum < 1.0:
            ks = 1.5 * max_lum - 0.5
            assert ks >= 0
            e1 = min(1.0, pq_inverse(x * white) / lw)
            if e1 > ks:
                t = (e1 - ks) / (1 - ks)
                e2 = (2 * t ** 3 - 3 * t ** 2 + 1) * ks + (t ** 3 - 2 * t ** 2 + t) * (1 - ks) + (-2 * t ** 3 + 3 * t ** 2) * max_lum
                return min(1.0, cu.eotf(16, min(max(e2, 0.0), 1.0) * lw, white) / white)
    return min(1.0, x)


def preset_tone(in_transfer, in_primaries, out_transfer, out_primaries, tone, norm, white_nits=0, peak_nits=0):
    """m355_colour_preset_tone in Python doubles -> the set"""
    S = cu.preset_tables(in_transfer, in_primaries, out_transfer, out_primaries, capi.TONE_CLIP, white_nits, peak_nits)
    white = float(white_nits) if white_nits else 203.0
    top = cu.eotf(cu._transfer(in_transfer), 1.0, white)
    peak = float(peak_nits) if peak_nits else top
    weights = [0, 0, 0]
    if norm == LUMA:
        row = cu.rgb_to_xyz(1 if out_primaries == 2 else out_primaries)[1]
        weights = [int(math.floor(v * 16384 + 0.5)) for v in row]
        weights[max(range(3), key=lambda c: (weights[c], -c))] += 16384 - sum(weights)
    gain = [GAIN_ONE]
    for i in range(1, OUT_KNOTS):
        x = knot(i) / ONE * top / white
        gain.append(int(math.floor(min(1.0, tone_curve(tone, x, white, peak) / x) * GAIN_ONE + 0.5)))
    S["tone"] = dict(norm=norm, weights=np.array(weights, np.int64), gain=np.array(gain, np.int64))
    return S


# ---- the three sets ------------------------------------------------------------------------------------------------------------------------------------------

def _random_set(seed=20250):
    rng = np.random.default_rng(seed)
    return dict(cu.RANDOM, tone=dict(norm=LUMA, weights=rng.integers(-20000, 40000, 3), gain=rng.integers(0, GAIN_ONE + 1, OUT_KNOTS)))


def _extreme_set(seed=20251):
    """matrix rows of +-65535 bring P to both ends of its clip, weights of +-65535 (one negative) the norm; the gain entries are 0 and GAIN_ONE only"""
    rng = np.random.default_rng(seed)
    return dict(lut_in=cu.RANDOM["lut_in"], matrix=np.array([65535, -65535, 65535, -65535, 65535, 16384, 16384, 0, 0], np.int64), lut_out=cu.RANDOM["lut_out"],
                tone=dict(norm=LUMA, weights=np.array([65535, -65535, 65535], np.int64), gain=rng.integers(0, 2, OUT_KNOTS) * GAIN_ONE))


RANDOM = _random_set()
EXTREME = _extreme_set()
PRESET_ARGS = (16, 9, 1, 1, capi.TONE_BT2390, MAXRGB, 203, 1000)
PRESET = preset_tone(*PRESET_ARGS)
SETS = {"random": RANDOM, "extreme": EXTREME, "preset": PRESET}
UNIT = dict(cu.RANDOM, tone=dict(norm=MAXRGB, weights=np.zeros(3, np.int64), gain=np.full(OUT_KNOTS, GAIN_ONE, np.int64)))   # every gain = 1: the plain object


# ---- the census of the picture inputs -------------------------------------------------------------------------------------------------------------------------

def conditions_reached(S, rgb16):
    v = stage_values(S, rgb16)
    P, n, fr, idx, g = v["P"], v["n"], v["fr"], v["idx"], v["g"]
    got = set()
    if np.any(n < 64): got.add("n<64")
    if np.any((n >= 64) & (fr != 0)): got.add("n>=64, fr!=0")
    if np.any((idx == OUT_KNOTS - 1) & (n == ONE)): got.add("idx=1216")
    if np.any(g == 0): got.add("g=0")
    if np.any(g == GAIN_ONE): got.add("g=ONE")
    if np.any((g == GAIN_ONE) & ((P[0] == ONE) | (P[1] == ONE) | (P[2] == ONE))): got.add("P=ONE, g=ONE")
    if S["tone"]["norm"] == LUMA:
        if np.any(v["s"] < 0): got.add("luma clip low")
        if np.any(v["s"] > ONE): got.add("luma clip high")
    else:
        for c, name in enumerate("RGB"):
            a, b = P[(c + 1) % 3], P[(c + 2) % 3]
            if np.any((P[c] > a) & (P[c] > b)): got.add("max " + name)
        if np.any(((P[0] == n) & (P[1] == n)) | ((P[1] == n) & (P[2] == n)) | ((P[0] == n) & (P[2] == n))): got.add("tie")
    return got


WANT = {"random": {"n<64", "n>=64, fr!=0", "idx=1216", "luma clip low", "luma clip high"},
        "preset": {"n>=64, fr!=0", "idx=1216", "g=ONE", "max R", "max G", "max B", "tie"},
        "extreme": {"n<64", "idx=1216", "g=0", "g=ONE", "P=ONE, g=ONE", "luma clip low", "luma clip high"}}


def check_census():
    """from the restatement alone: what the picture inputs of the kernel cases reach under each set"""
    for name, S in SETS.items():
        got = set()
        for bd in (8, 10):
            for planes, out_size, loc, rect, filt in cu.kernel_case_inputs(bd):
                got |= conditions_reached(S, ints16(planes, bd, out_size, loc, rect, filt, "census"))
        assert WANT[name] <= got, "set %s misses %s" % (name, sorted(WANT[name] - got))


def check_differs_from_plain(bd=10):
    """the expectations themselves: a tone object's are not those of the plain object of the same tables"""
    rgb = ints16(census_planes(bd), bd, (48, 24), 0, None, cu.TRIANGLE, "census")
    for S in SETS.values():
        assert any(not np.array_equal(a, b) for a, b in zip(pixels(S, rgb, U16), cu.colour_pixels(S, rgb, U16)))


# ---- the composed exports with a tone object -------------------------------------------------------------------------------------------------------------------

def expected_ints(S, planes, bd, samples, out_size, loc=0, rect=None, filt=cu.TRIANGLE, key=None):
    return pixels(S, ints16(planes, bd, out_size, loc, rect, filt, key), samples)


def expected_rgb(S, planes, bd, layout, samples, out_size, loc=0, rect=None, filt=cu.TRIANGLE, key=None):
    return shape_rgb(expected_ints(S, planes, bd, samples, out_size, loc, rect, filt, key), layout, samples)


def check_kernel_cases(ctx, bd, S, name):
    """the 64x32 cases of one bit depth under one set: packed and planar, U8 and U16, chroma_loc 0 and 2, both filters"""
    planes = census_planes(bd)
    frame, handle = upload(ctx, planes, bd), create(ctx, S)
    try:
        for rect, out_size, filters in KERNEL_CASES:
            for filt in filters:
                for loc in KERNEL_LOCS:
                    for layout in (capi.RGB_PACKED, capi.RGB_PLANAR):
                        for samples in (U8, U16):
                            what = "%s %d bit rect %s to %dx%d filter %d type %d layout %d samples %d" % (name, bd, rect, out_size[0], out_size[1], filt, loc, layout, samples)
                            want = expected_rgb(S, planes, bd, layout, samples, out_size, loc, rect, filt, "census")
                            got, raws = finish(ctx, ctx.frame_export_resized_rgb(frame, layout, samples, MATRIX, FULL, out_size, rect, filter=filt, chroma_loc=loc, colour=handle))
                            assert_export(got, raws, want, what)
    finally:
        ctx.frame_destroy(frame)
        ctx.colour_destroy(handle)


def check_wide(ctx, S, name, bd=10):
    size, out_size = WIDE
    planes = random_planes(bd, 9930, size)
    frame, handle = upload(ctx, planes, bd), create(ctx, S)
    try:
        got, raws = finish(ctx, ctx.frame_export_resized_rgb(frame, capi.RGB_PACKED, U8, MATRIX, FULL, out_size, chroma_loc=2, colour=handle))
        assert_export(got, raws, expected_rgb(S, planes, bd, capi.RGB_PACKED, U8, out_size, 2, key="tone wide"), "wide, " + name)
    finally:
        ctx.frame_destroy(frame)
        ctx.colour_destroy(handle)


def tensor_calls(ctx, frames, handle, layout, dtype, samples, out_size, loc):
    """the batch of the three frames and the three regions of frame 0 through one object -> the two finished tensors"""
    return (ctx.tensor_export_finish(ctx.frames_export_tensor(frames, layout, dtype, samples, MATRIX, FULL, out_size, SCALE, BIAS, chroma_loc=loc, colour=handle)),
            ctx.tensor_export_finish(ctx.frames_export_tensor_rois([frames[0]] * 3, TENSOR_ROIS, layout, dtype, samples, MATRIX, FULL, out_size, SCALE, BIAS,
                                                                   chroma_loc=loc, colour=handle)))


def check_tensors(ctx, S, name, bd=10, out_size=(48, 24), loc=2):
    """3 frames as one tensor, and 3 regions (one mirrored) as one tensor"""
    planes = [random_planes(bd, 9920 + k) for k in range(3)]
    frames, handle = [upload(ctx, p, bd) for p in planes], create(ctx, S)
    try:
        for layout, dtype, samples in TENSOR_FORMATS:
            what = "%s layout %d dtype %d samples %d" % (name, layout, dtype, samples)
            ints = [expected_ints(S, p, bd, samples, out_size, loc, key="tensor%d" % k) for k, p in enumerate(planes)]
            want = []
            for x0, y0, w, h, flags in TENSOR_ROIS:
                one = expected_tensor([expected_ints(S, planes[0], bd, samples, out_size, loc, (x0, y0, w, h), key="roi")], layout, dtype, SCALE, BIAS)[0]
                want.append(reverse_columns(one, layout) if flags & capi.ROI_MIRROR else one)
            batch, rois = tensor_calls(ctx, frames, handle, layout, dtype, samples, out_size, loc)
            assert_tensor(batch, expected_tensor(ints, layout, dtype, SCALE, BIAS), "tensor, " + what)
            assert_tensor(rois, np.stack(want), "rois, " + what)
    finally:
        for f in frames:
            ctx.frame_destroy(f)
        ctx.colour_destroy(handle)


def check_extreme(ctx, bd=10):
    planes = census_planes(bd)
    frame, handle = upload(ctx, planes, bd), create(ctx, EXTREME)
    try:
        for samples in (U8, U16):
            got, raws = finish(ctx, ctx.frame_export_resized_rgb(frame, capi.RGB_PLANAR, samples, MATRIX, FULL, (48, 24), colour=handle))
            assert_export(got, raws, expected_rgb(EXTREME, planes, bd, capi.RGB_PLANAR, samples, (48, 24), key="census"), "extreme")
    finally:
        ctx.frame_destroy(frame)
        ctx.colour_destroy(handle)


def check_unit_gain_is_plain(ctx, bd=10):
    """a tone object whose every gain is GAIN_ONE delivers what m355_colour_create with the same tables delivers, byte for byte, in the three exports"""
    planes = [random_planes(bd, 9920 + k) for k in range(3)]
    frames = [upload(ctx, p, bd) for p in planes]
    tone, plain = create(ctx, UNIT), create(ctx, cu.RANDOM)
    try:
        for samples in (U8, U16):
            rr = (frames[0], capi.RGB_PACKED, samples, MATRIX, FULL, (48, 24), (2, 2, 44, 26))
            assert_same_bytes(finish(ctx, ctx.frame_export_resized_rgb(*rr, chroma_loc=2, colour=tone)),
                              finish(ctx, ctx.frame_export_resized_rgb(*rr, chroma_loc=2, colour=plain)), "resized rgb, samples %d" % samples)
        for layout, dtype, samples in TENSOR_FORMATS:
            for a, b in zip(tensor_calls(ctx, frames, tone, layout, dtype, samples, (48, 24), 2), tensor_calls(ctx, frames, plain, layout, dtype, samples, (48, 24), 2)):
                assert np.array_equal(a[1], b[1]), "tensor bytes, layout %d dtype %d" % (layout, dtype)
    finally:
        for f in frames:
            ctx.frame_destroy(f)
        ctx.colour_destroy(tone)
        ctx.colour_destroy(plain)


def check_destroy_after_export(ctx, bd=10):
    """m355_colour_destroy of a tone object directly behind an export: it waits for the context's work, the export's bytes are exact"""
    planes = census_planes(bd)
    frame, handle = upload(ctx, planes, bd), create(ctx, RANDOM)
    try:
        token = ctx.frame_export_resized_rgb(frame, capi.RGB_PACKED, U16, MATRIX, FULL, (128, 64), colour=handle)
        ctx.colour_destroy(handle)
        got, raws = finish(ctx, token)
        assert_export(got, raws, expected_rgb(RANDOM, planes, bd, capi.RGB_PACKED, U16, (128, 64), key="census"), "destroy behind the export")
    finally:
        ctx.frame_destroy(frame)


def check_gate(ctx, S=RANDOM, layout=capi.RGB_PACKED, samples=U8, out_size=(96, 48)):
    """export_colour_util.check_gate_colour's scenario with a tone object: behind a decode whose lists the device rejected the export writes nothing,
    behind an accepted decode of the same lists it does"""
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
    colour = create(ctx, S)
    tokens, serials = [], []
    for corrupt in (False, True):
        p = make_case(**cfg)[0]
        p.ref_frames = [handles[i] if i < len(handles) else -1 for i in range(worklist.MAX_REF_FRAMES)]
        p.dst_frame = dst
        if corrupt:
            arr = p.ibs.copy(); arr["mode"][len(arr) // 2] = 77; p.ibs = arr
        ctx.submit_in_place(p, fill_threads=1)
        serials.append(ctx.last_serial())
        tokens.append(ctx.frame_export_resized_rgb(dst, layout, samples, MATRIX, FULL, out_size, chroma_loc=2, colour=colour))
    good, bad = [ctx.frame_export_finish(t, raw=True) for t in tokens]
    assert ctx.decode_status(serials[0]) == 0 and ctx.decode_status(serials[1]) == M355_ERR_INVALID
    with_planes = ctx.frame_download(dst)
    assert_export(good[0], good[1], expected_rgb(S, with_planes, 8, layout, samples, out_size, 2), "behind the accepted decode")
    for raw in bad[1]:
        assert np.all(raw == capi.DEVICE_FILL), "a tone export behind a rejected decode wrote to its destination"
    ctx.wait()
    ctx.colour_destroy(colour)
    for f in handles + [dst]:
        ctx.frame_destroy(f)


def check_hazard(ctx, depth, S=RANDOM, layout=capi.RGB_PACKED, samples=U8, out_size=(96, 48)):
    """export_colour_util.check_hazard_colour's scenario with a tone object: four pictures decoded alternately into a pool of two frames, each exported
    right behind its decode, no host wait in between; every export delivers what the export of the same picture decoded alone does"""
    from libde265_amd import synth
    from synth_util import assert_planes_equal
    ctx.set_pipeline_depth(depth)
    try:
        cfg = dict(width=128, height=64, bit_depth=10, seed=5, n_refs=1)
        pics = [synth.picture(**dict(cfg, seed=5 + j)) for j in range(4)]
        pp = pics[0].pp[0]
        r0 = ctx.frame_create_for(pp)
        ctx.frame_upload(r0, synth.ref_planes(5, 128, 64, 1, 10))
        pool = [ctx.frame_create_for(pp) for _ in range(2)]
        colour = create(ctx, S)
        rect = (2, 2, 122, 58)
        handles, tokens = [], []
        for j, pic in enumerate(pics):
            pic.ref_frames = [r0] + [-1] * (worklist.MAX_REF_FRAMES - 1)
            pic.dst_frame = pool[j % 2]
            handles.append(ctx.upload(pic))
            ctx.decode_resident(handles[-1])
            tokens.append(ctx.frame_export_resized_rgb(pool[j % 2], layout, samples, MATRIX, FULL, out_size, rect, chroma_loc=2, colour=colour))
        got = [ctx.frame_export_finish(t, raw=True) for t in tokens]
        ctx.wait()
        for j in range(4):
            ctx.decode_resident(handles[j])
            ctx.wait()
            planes = ctx.frame_download(pool[j % 2])
            alone = ctx.frame_export_finish(ctx.frame_export_resized_rgb(pool[j % 2], layout, samples, MATRIX, FULL, out_size, rect, chroma_loc=2, colour=colour))
            assert_planes_equal(alone, expected_rgb(S, planes, 10, layout, samples, out_size, 2, rect), "picture %d alone" % j)
            assert_export(got[j][0], got[j][1], alone, "picture %d, depth %d" % (j, depth))
        for j in (0, 1):
            assert not np.array_equal(got[j][0][0], got[j + 2][0][0]), "the pictures that share a frame must differ for this test to see a hazard"
        for h in handles:
            ctx.release(h)
        ctx.colour_destroy(colour)
        for f in pool + [r0]:
            ctx.frame_destroy(f)
    finally:
        ctx.set_pipeline_depth(1)
