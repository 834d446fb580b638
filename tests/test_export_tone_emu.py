"""Tone objects of the composed exports (TONE OBJECTS in include/de265_mi355x.h) on the SIMT-interpreter build: m355_colour_pixel_tone against the
restatement of export_tone_util.py, the census of what the picture inputs reach, the tone presets against a restatement in doubles, that hue is kept
where a per-channel curve does not keep it, the kernels in their three modes under the three sets, and the edges of the contract.  Every comparison of
pixels is exact, destination padding included."""
import ctypes

import numpy as np
import pytest

from test_emu_picture import emu_lib  # noqa: F401  (fixture)
import export_colour_util as cu
import export_tone_util as tu
from export_tone_util import GAIN_ONE, LUMA, M355_ERR_INVALID, MAXRGB, ONE, PRESET_ARGS, RANDOM, SETS, U8, U16
from libde265_amd import capi

M355_ERR_BUSY = 6


@pytest.fixture()
def ctx(emu_lib):  # noqa: F811
    c = capi.Context(emu_lib, 0)
    yield c
    c.close()


@pytest.mark.parametrize("samples", [U8, U16])
@pytest.mark.parametrize("name", ["random", "extreme", "preset"])
def test_pixel_function_is_the_restatement(emu_lib, name, samples):  # noqa: F811
    S = SETS[name]
    t, q = cu.to_ctypes(S), tu.tone_ctypes(S)
    rng = np.random.default_rng(41 + samples)
    vals = [0, 63, 64, 65535]
    triples = np.concatenate([rng.integers(0, 65536, (20000, 3)), np.array([(a, b, c) for a in vals for b in vals for c in vals])])
    want = np.stack(tu.pixels(S, [triples[:, 0], triples[:, 1], triples[:, 2]], samples), axis=1)
    for k, v in enumerate(triples):
        assert emu_lib.colour_pixel_tone(t, q, v, samples) == tuple(int(x) for x in want[k]), (name, tuple(v))


@pytest.mark.parametrize("norm", [MAXRGB, LUMA])
def test_pixel_function_at_the_corners_of_n(emu_lib, norm):  # noqa: F811
    """tables under which P is what the test sets (lut_in[k] = k, knots 1022 .. 1024 = ONE - 1, ONE, ONE, the identity matrix) and a luma row that is the
    red channel: n runs over 0, 63, 64, 127, 128, ONE - 1, ONE — the first and the last knot of the gain table and both sides of the index's switch"""
    lut_in = np.arange(cu.IN_KNOTS, dtype=np.int64)
    lut_in[1022], lut_in[1023], lut_in[1024] = ONE - 1, ONE, ONE
    S = dict(lut_in=lut_in, matrix=np.array([16384, 0, 0, 0, 16384, 0, 0, 0, 16384]), lut_out=cu.RANDOM["lut_out"],
             tone=dict(norm=norm, weights=np.array([16384, 0, 0] if norm == LUMA else [0, 0, 0]), gain=RANDOM["tone"]["gain"]))
    t, q = cu.to_ctypes(S), tu.tone_ctypes(S)
    vs = [0, 63 * 64, 64 * 64, 127 * 64, 128 * 64, 1022 * 64, 1023 * 64]
    rgb = [np.array(vs), np.array(vs) // 2, np.array(vs) // 3]
    v = tu.stage_values(S, rgb)
    assert [int(x) for x in v["n"]] == [0, 63, 64, 127, 128, ONE - 1, ONE] and list(v["idx"]) == [0, 63, 64, 127, 128, 1215, 1216] and v["fr"][-2] == 255
    for samples in (U8, U16):
        want = np.stack(tu.pixels(S, rgb, samples), axis=1)
        for k in range(len(vs)):
            assert emu_lib.colour_pixel_tone(t, q, (rgb[0][k], rgb[1][k], rgb[2][k]), samples) == tuple(int(x) for x in want[k])


def test_census_of_the_picture_inputs():
    tu.check_census()
    tu.check_differs_from_plain()


PRESETS = [PRESET_ARGS, (18, 9, 13, 1, capi.TONE_CLIP, LUMA, 0, 0), (16, 9, 1, 1, capi.TONE_REINHARD, LUMA, 203, 4000), (16, 9, 13, 9, capi.TONE_BT2390, LUMA, 100, 0),
           (1, 1, 1, 1, capi.TONE_BT2390, MAXRGB, 0, 0), (16, 9, 1, 1, capi.TONE_CLIP, MAXRGB, 0, 0)]


def library_preset(lib, args):
    return lib.colour_preset_tone(*args[:4], tone=args[4], norm=args[5], white_nits=args[6], peak_nits=args[7])


@pytest.mark.parametrize("args", PRESETS)
def test_tone_presets_against_doubles(emu_lib, args):  # noqa: F811
    """Mapped light gain[i] * knot(i) must not decrease.  A gain is a real number rounded to Q24, off by at most 1 / 2 of its unit, so the mapped light
    of knot i is known to knot(i) / 2 of its units (2^-24 of a unit of P) and no closer: where the curve is flat — a clip, the EETF above the peak — the
    exact products are equal and the rounded ones scatter by that much.  The assertion allows exactly this, and nothing for the curve itself."""
    t, q = library_preset(emu_lib, args)
    got, want = tu.from_ctypes(t, q), tu.preset_tone(*args)
    for k in ("lut_in", "matrix", "lut_out"):
        assert np.abs(got[k] - want[k]).max() <= 1, k
    assert np.abs(got["tone"]["gain"] - want["tone"]["gain"]).max() <= 1 and np.abs(got["tone"]["weights"] - want["tone"]["weights"]).max() <= 1
    assert got["tone"]["norm"] == args[5] and list(q.reserved[:]) == [0, 0, 0]
    in_t, in_p, out_t, out_p, tone, norm, white, peak = args
    plain = emu_lib.colour_preset(in_t, in_p, out_t, out_p, min(tone, capi.TONE_REINHARD), white, peak)
    clip = emu_lib.colour_preset(in_t, in_p, out_t, out_p, capi.TONE_CLIP, white, peak)
    assert bytes(t.lut_in) == bytes(plain.lut_in) and bytes(t.matrix) == bytes(plain.matrix) and bytes(t.lut_out) == bytes(clip.lut_out) and t.pad == 0
    gain = got["tone"]["gain"]
    assert gain[0] == GAIN_ONE and gain.max() <= GAIN_ONE and np.all(np.diff(gain) <= 0)
    knots = [cu.knot(i) for i in range(cu.OUT_KNOTS)]
    light = [int(g) * k for g, k in zip(gain, knots)]
    for i in range(cu.OUT_KNOTS - 1):
        assert 2 * (light[i + 1] - light[i]) >= -(knots[i] + knots[i + 1]), i
    w = got["tone"]["weights"]
    assert (int(w.sum()) == 16384 and w.min() > 0) if norm == LUMA else not w.any()
    if args[0] == 1:
        assert np.all(gain == GAIN_ONE)                       # SDR in: the peak is white, maxLum = 1, the identity


def test_hue_is_kept(emu_lib):  # noqa: F811
    """P' = (P g + 2^23) >> 24 with one g for the three channels: P'_c = P_c g / 2^24 + e_c with |e_c| <= 1 / 2, so P'_a P_b - P'_b P_a = e_a P_b - e_b P_a,
    at most (P_a + P_b) / 2 in magnitude.  The per-channel Reinhard preset maps the same pixels' channels each by its own factor: taking its curve in
    the same units (P' = y(x) ONE white / S, in doubles, rounded), the same quantity exceeds the bound — by orders of magnitude in the highlights."""
    in_t, in_p, out_t, out_p = PRESET_ARGS[:4]
    rng = np.random.default_rng(77)
    rgb = [rng.integers(0, 65536, 50000) for _ in range(3)]
    worst = 0
    for tone, norm in ((capi.TONE_BT2390, MAXRGB), (capi.TONE_REINHARD, LUMA), (capi.TONE_CLIP, MAXRGB)):
        S = tu.from_ctypes(*emu_lib.colour_preset_tone(in_t, in_p, out_t, out_p, tone=tone, norm=norm, white_nits=203, peak_nits=1000))
        v = tu.stage_values(S, rgb)
        assert np.any(v["g"] < GAIN_ONE // 2)                   # (the pixels reach the highlights, where the gain acts)
        for a, b in ((0, 1), (1, 2), (0, 2)):
            assert np.all(2 * np.abs(v["Pt"][a] * v["P"][b] - v["Pt"][b] * v["P"][a]) <= v["P"][a] + v["P"][b]), (tone, a, b)
    S = tu.from_ctypes(*emu_lib.colour_preset_tone(in_t, in_p, out_t, out_p, tone=capi.TONE_REINHARD, norm=MAXRGB, white_nits=203, peak_nits=1000))
    P = tu.stage_values(S, rgb)["P"]
    scale, w2 = 10000.0 / 203.0, (1000.0 / 203.0) ** 2
    per_channel = []
    for p in P:
        x = p.astype(np.float64) / ONE * scale
        per_channel.append(np.floor(np.minimum(1.0, x * (1 + x / w2) / (1 + x)) / scale * ONE + 0.5).astype(np.int64))
    for a, b in ((0, 1), (1, 2), (0, 2)):
        excess = 2 * np.abs(per_channel[a] * P[b] - per_channel[b] * P[a]) - (P[a] + P[b])
        worst = max(worst, int(excess.max()))
    assert worst > 0, "the per-channel curve keeps the ratios too: the test shows nothing"


def test_unit_gain_is_the_plain_object(ctx):
    tu.check_unit_gain_is_plain(ctx)


@pytest.mark.parametrize("name", ["random", "preset"])
@pytest.mark.parametrize("bit_depth", [8, 10])
def test_kernel_cases(ctx, bit_depth, name):
    tu.check_kernel_cases(ctx, bit_depth, SETS[name], name)


@pytest.mark.parametrize("name", ["random", "preset"])
def test_wider_than_a_tile(ctx, name):
    tu.check_wide(ctx, SETS[name], name)


@pytest.mark.parametrize("name", ["random", "preset"])
def test_tensor_and_rois(ctx, name):
    tu.check_tensors(ctx, SETS[name], name)


def test_extreme_set(ctx):
    tu.check_extreme(ctx)


def test_rejections_of_create(ctx):
    lib = ctx.L.lib
    t, q, h = cu.to_ctypes(RANDOM), tu.tone_ctypes(RANDOM), ctypes.c_int(0)
    ref = ctypes.byref
    assert lib.m355_colour_create_tone(ctx.h, ref(t), None, ref(h)) == M355_ERR_INVALID
    assert lib.m355_colour_create_tone(ctx.h, None, ref(q), ref(h)) == M355_ERR_INVALID
    assert lib.m355_colour_create_tone(ctx.h, ref(t), ref(q), None) == M355_ERR_INVALID
    assert lib.m355_colour_create_tone(None, ref(t), ref(q), ref(h)) == M355_ERR_INVALID
    for field, k, v in (("lut_in", 0, ONE + 1), ("matrix", 8, -65536), ("pad", None, 1)):                       # whatever m355_colour_create rejects
        bad = cu.to_ctypes(RANDOM)
        if k is None:
            setattr(bad, field, v)
        else:
            getattr(bad, field)[k] = v
        assert lib.m355_colour_create_tone(ctx.h, ref(bad), ref(q), ref(h)) == M355_ERR_INVALID, field
    maxrgb = dict(RANDOM, tone=dict(RANDOM["tone"], norm=MAXRGB, weights=[0, 0, 0]))
    for S, field, k, v in ((RANDOM, "norm", None, 2), (RANDOM, "norm", None, -1), (RANDOM, "gain", 0, GAIN_ONE + 1), (RANDOM, "gain", 1216, 0xFFFFFFFF),
                           (RANDOM, "weights", 0, 65536), (RANDOM, "weights", 2, -65536), (maxrgb, "weights", 1, 1), (maxrgb, "weights", 2, -1),
                           (RANDOM, "reserved", 0, 1), (RANDOM, "reserved", 2, 1)):
        bad = tu.tone_ctypes(S)
        if k is None:
            setattr(bad, field, v)
        else:
            getattr(bad, field)[k] = v
        assert lib.m355_colour_create_tone(ctx.h, ref(t), ref(bad), ref(h)) == M355_ERR_INVALID, (field, k, v)
    # nothing was allocated: the sixteen slots are all free; the edges of the bounds are inside them
    edge = tu.tone_ctypes(dict(RANDOM, tone=dict(norm=LUMA, weights=[65535, -65535, 0], gain=np.full(cu.OUT_KNOTS, GAIN_ONE))))
    handles = [ctx.colour_create_tone(t, edge) for _ in range(capi.COLOUR_OBJECTS)]
    for x in handles:
        ctx.colour_destroy(x)


def test_rejections_of_preset_and_pixel(emu_lib):  # noqa: F811
    ok = dict(in_transfer=16, in_primaries=9, out_transfer=1, out_primaries=1, tone=capi.TONE_BT2390, norm=MAXRGB, white_nits=203, peak_nits=1000, reserved=0)
    emu_lib.colour_preset_tone(**ok)
    bad = [dict(in_transfer=3), dict(out_transfer=16), dict(in_primaries=4), dict(out_primaries=8), dict(tone=3), dict(tone=-1), dict(norm=2), dict(norm=-1),
           dict(reserved=1), dict(white_nits=-1), dict(peak_nits=100), dict(white_nits=5, peak_nits=10000)]          # (the last: KS < 0)
    for b in bad:
        with pytest.raises(capi.M355Error) as e:
            emu_lib.colour_preset_tone(**dict(ok, **b))
        assert e.value.code == M355_ERR_INVALID, b
    emu_lib.colour_preset_tone(**dict(ok, tone=capi.TONE_CLIP, white_nits=5, peak_nits=10000))                      # KS is BT.2390's alone
    with pytest.raises(capi.M355Error) as e:                                                                       # the plain preset keeps refusing tone 2
        emu_lib.colour_preset(16, 9, 1, 1, capi.TONE_BT2390, 203, 1000)
    assert e.value.code == M355_ERR_INVALID
    d, t, q = capi.ColourPresetDesc(16, 9, 1, 1, 2, 0, 0, 0), capi.ColourTables(), capi.ColourTone()
    ref, lib = ctypes.byref, emu_lib.lib
    assert lib.m355_colour_preset_tone(None, 0, ref(t), ref(q)) == M355_ERR_INVALID
    assert lib.m355_colour_preset_tone(ref(d), 0, None, ref(q)) == M355_ERR_INVALID
    assert lib.m355_colour_preset_tone(ref(d), 0, ref(t), None) == M355_ERR_INVALID
    assert lib.m355_colour_preset_tone(ref(d), 0, ref(t), ref(q)) == 0
    rgb, out = (ctypes.c_uint32 * 3)(1, 2, 3), (ctypes.c_uint32 * 3)()
    assert lib.m355_colour_pixel_tone(ref(t), ref(q), rgb, U16, out) == 0
    assert lib.m355_colour_pixel_tone(None, ref(q), rgb, U16, out) == M355_ERR_INVALID
    assert lib.m355_colour_pixel_tone(ref(t), None, rgb, U16, out) == M355_ERR_INVALID
    assert lib.m355_colour_pixel_tone(ref(t), ref(q), None, U16, out) == M355_ERR_INVALID
    assert lib.m355_colour_pixel_tone(ref(t), ref(q), rgb, U16, None) == M355_ERR_INVALID
    assert lib.m355_colour_pixel_tone(ref(t), ref(q), rgb, 2, out) == M355_ERR_INVALID
    q.gain[7] = GAIN_ONE + 1
    assert lib.m355_colour_pixel_tone(ref(t), ref(q), rgb, U16, out) == M355_ERR_INVALID
    q.gain[7] = 0
    t.pad = 1
    assert lib.m355_colour_pixel_tone(ref(t), ref(q), rgb, U16, out) == M355_ERR_INVALID


def test_sixteen_objects_of_mixed_kinds(ctx):
    """one handle space and one limit for both kinds; m355_colour_destroy destroys either; a handle keeps its kind's arithmetic"""
    lib = ctx.L.lib
    t, q, h = cu.to_ctypes(RANDOM), tu.tone_ctypes(RANDOM), ctypes.c_int(0)
    handles = [ctx.colour_create_tone(t, q) if k % 2 else ctx.colour_create(t) for k in range(capi.COLOUR_OBJECTS)]
    assert len(set(handles)) == capi.COLOUR_OBJECTS and min(handles) >= 0x100
    assert lib.m355_colour_create_tone(ctx.h, ctypes.byref(t), ctypes.byref(q), ctypes.byref(h)) == M355_ERR_BUSY
    assert lib.m355_colour_create(ctx.h, ctypes.byref(t), ctypes.byref(h)) == M355_ERR_BUSY
    planes = cu.census_planes(10)
    frame = cu.upload(ctx, planes, 10)
    for k in (0, 1, capi.COLOUR_OBJECTS - 1):
        got, raws = tu.finish(ctx, ctx.frame_export_resized_rgb(frame, capi.RGB_PACKED, U16, cu.MATRIX, cu.FULL, (48, 24), colour=handles[k]))
        S = RANDOM if k % 2 else cu.RANDOM
        tu.assert_export(got, raws, tu.expected_rgb(S, planes, 10, capi.RGB_PACKED, U16, (48, 24), key="census"), "object %d" % k)
    ctx.colour_destroy(handles.pop(1))                          # a tone object's slot goes to a plain object and back
    handles.append(ctx.colour_create(t))
    ctx.colour_destroy(handles.pop())
    handles.append(ctx.colour_create_tone(t, q))
    assert len(set(handles)) == capi.COLOUR_OBJECTS
    got, raws = tu.finish(ctx, ctx.frame_export_resized_rgb(frame, capi.RGB_PACKED, U16, cu.MATRIX, cu.FULL, (48, 24), colour=handles[-1]))
    tu.assert_export(got, raws, tu.expected_rgb(RANDOM, planes, 10, capi.RGB_PACKED, U16, (48, 24), key="census"), "the recycled slot")
    for x in handles:
        ctx.colour_destroy(x)
    assert lib.m355_colour_destroy(ctx.h, handles[0]) == M355_ERR_INVALID
    ctx.frame_destroy(frame)


def test_plain_calls_still_reject_a_tone_handle(ctx):
    """m355_frame_export_rgb_opts and m355_frame_export_resized_opts have no colour stage: a tone object's handle is rejected like any other"""
    lib = ctx.L.lib
    buf = ctx.device_alloc(1 << 16)
    frame, live = ctx.frame_create(64, 32, 1, 8, 8), tu.create(ctx, RANDOM)
    o = capi.ExportOpts()
    o.reserved[0] = live
    rgb = capi.RgbDesc(layout=capi.RGB_PACKED, samples=U8, matrix=capi.MATRIX_BT709, full_range=0)
    rgb.dst[0] = buf; rgb.pitch[0] = 400
    rs = capi.ResizeDesc(layout=capi.EXPORT_PLANAR, samples=capi.EXPORT_NATIVE, out_width=32, out_height=16)
    for k in range(3):
        rs.dst[k] = buf + 8192 * k; rs.pitch[k] = 128
    assert lib.m355_frame_export_rgb_opts(ctx.h, frame, ctypes.byref(rgb), ctypes.byref(o)) == M355_ERR_INVALID
    assert lib.m355_frame_export_resized_opts(ctx.h, frame, ctypes.byref(rs), ctypes.byref(o)) == M355_ERR_INVALID
    ctx.wait()
    assert np.all(ctx.device_read(buf, 1 << 16) == capi.DEVICE_FILL), "a rejected export wrote to its destination"
    ctx.colour_destroy(live)
    ctx.device_free(buf)
    ctx.frame_destroy(frame)


def test_destroy_directly_after_an_export(ctx):
    tu.check_destroy_after_export(ctx)


def test_gate_and_recycled_frames(ctx):
    """(the interpreter runs every launch to its end at once: this walks the bookkeeping, the GPU tier sees a missing wait)"""
    tu.check_gate(ctx)
    tu.check_hazard(ctx, 1)
    tu.check_hazard(ctx, 3)
