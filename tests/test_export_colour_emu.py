"""The colour transform stage of the composed exports (COLOUR TRANSFORM in include/de265_mi355x.h) on the SIMT-interpreter build: m355_colour_pixel
against the restatement of export_colour_util.py, the census of what the picture inputs reach, the presets against a restatement in doubles, the
kernels in their three modes under the table sets (a), (b) and (c), and the edges of the contract.  Every comparison of pixels is exact, destination
padding included."""
import ctypes

import numpy as np
import pytest

from test_emu_picture import emu_lib  # noqa: F401  (fixture)
import export_colour_util as cu
from export_colour_util import M355_ERR_INVALID, ONE, PRESET, PRESET_ARGS, RANDOM, TABLE_SETS, U8, U16
from libde265_amd import capi

M355_ERR_BUSY = 6


@pytest.fixture()
def ctx(emu_lib):  # noqa: F811
    c = capi.Context(emu_lib, 0)
    yield c
    c.close()


def corner_triples(T):
    """v = 0, 63, 64 and 65535 in every channel, in every combination"""
    vals = [0, 63, 64, 65535]
    return [(a, b, c) for a in vals for b in vals for c in vals]


@pytest.mark.parametrize("samples", [U8, U16])
@pytest.mark.parametrize("name", ["random", "extreme", "preset"])
def test_pixel_function_is_the_restatement(emu_lib, name, samples):  # noqa: F811
    T = TABLE_SETS[name]
    t = cu.to_ctypes(T)
    rng = np.random.default_rng(31 + samples)
    triples = np.concatenate([rng.integers(0, 65536, (20000, 3)), np.array(corner_triples(T))])
    want = np.stack(cu.colour_pixels(T, [triples[:, 0], triples[:, 1], triples[:, 2]], samples), axis=1)
    for k, v in enumerate(triples):
        assert emu_lib.colour_pixel(t, v, samples) == tuple(int(x) for x in want[k]), (name, tuple(v))


@pytest.mark.parametrize("samples", [U8, U16])
def test_pixel_function_at_the_corners_of_P(emu_lib, samples):  # noqa: F811
    """tables under which P is what the test sets: lut_in[k] = k (so v = 64 k gives L = k), knot 1023 and 1024 = ONE - 1 and ONE, the identity matrix,
    and a random output table"""
    lut_in = np.arange(cu.IN_KNOTS, dtype=np.int64)
    lut_in[1022], lut_in[1023], lut_in[1024] = ONE - 1, ONE, ONE
    T = dict(lut_in=lut_in, matrix=np.array([16384, 0, 0, 0, 16384, 0, 0, 0, 16384]), lut_out=RANDOM["lut_out"])
    t = cu.to_ctypes(T)
    want_P = [0, 63, 64, 127, 128, ONE - 1, ONE]
    vs = [0, 63 * 64, 64 * 64, 127 * 64, 128 * 64, 1022 * 64, 1023 * 64]
    rgb = [np.array(vs), np.array(vs[::-1]), np.array(vs)]
    assert [int(x) for x in np.clip(cu.linear_and_sums(T, rgb)[1][0], 0, ONE)] == want_P
    want = np.stack(cu.colour_pixels(T, rgb, samples), axis=1)
    for k in range(len(vs)):
        assert emu_lib.colour_pixel(t, (rgb[0][k], rgb[1][k], rgb[2][k]), samples) == tuple(int(x) for x in want[k])
    idx, fr = cu.out_index(np.array(want_P))
    assert list(idx) == [0, 63, 64, 127, 128, 1215, 1216] and fr[-1] == 0 and fr[-2] == 255


def test_u8_delivery_over_every_value(emu_lib):  # noqa: F811
    """lut_out[i] and an identity path deliver every o: (2 o + 257) / 514 is o / 257 rounded, and the library's is that"""
    o = np.arange(65536, dtype=np.int64)
    assert np.array_equal((2 * o + 257) // 514, np.floor(o / 257 + 0.5).astype(np.int64))
    # P < 64 reads lut_out[P] with fr = 0: 64 values of o per table, 1024 tables cover all of them
    lut_in = np.zeros(cu.IN_KNOTS, np.int64)
    lut_in[1:] = np.minimum(np.arange(1, cu.IN_KNOTS), 63)
    got = np.zeros(65536, np.int64)
    for base in range(0, 65536, 64):
        lut_out = np.zeros(cu.OUT_KNOTS, np.int64)
        lut_out[:64] = np.arange(base, base + 64)
        t = capi.colour_tables(lut_in, [16384, 0, 0, 0, 16384, 0, 0, 0, 16384], lut_out)
        for p in range(0, 64, 3):
            r = emu_lib.colour_pixel(t, (64 * p, 64 * min(p + 1, 63), 64 * min(p + 2, 63)), U8)
            got[base + p], got[base + min(p + 1, 63)], got[base + min(p + 2, 63)] = r
    assert np.array_equal(got, (2 * o + 257) // 514)


def test_census_of_the_picture_inputs():
    cu.check_census()
    cu.check_differs_from_plain()


def test_knots_bracket_every_P():
    """the indexing is continuous at 64 and every P lies between its knot and the next"""
    rng = np.random.default_rng(5)
    P = np.concatenate([np.arange(0, 4096), rng.integers(0, ONE + 1, 200000), np.array([ONE - 1, ONE])])
    idx, fr = cu.out_index(P)
    knots = np.array([cu.knot(i) for i in range(cu.OUT_KNOTS)] + [cu.knot(cu.OUT_KNOTS - 1)], dtype=np.int64)
    assert np.all(knots[idx] <= P) and np.all((P < knots[idx + 1]) | (idx == cu.OUT_KNOTS - 1))
    assert np.all(np.diff(knots[:cu.OUT_KNOTS]) > 0)


PRESETS = [PRESET_ARGS, (18, 9, 13, 1, capi.TONE_CLIP, 0, 0), (1, 1, 1, 1, capi.TONE_REINHARD, 0, 0)]


@pytest.mark.parametrize("args", PRESETS)
def test_presets_against_doubles(emu_lib, args):  # noqa: F811
    got = cu.from_ctypes(emu_lib.colour_preset(*args))
    want = cu.preset_tables(*args)
    for k in ("lut_in", "matrix", "lut_out"):
        assert np.abs(got[k] - want[k]).max() <= 1, k
    assert np.all(np.diff(got["lut_in"]) >= 0) and np.all(np.diff(got["lut_out"]) >= 0)
    assert got["lut_in"][0] == 0 and got["lut_in"][1024] == ONE and got["lut_out"][0] == 0 and got["lut_out"][1216] == 65535
    assert [int(got["matrix"][3 * r:3 * r + 3].sum()) for r in range(3)] == [16384] * 3
    if args[1] == args[3]:
        assert list(got["matrix"]) == [16384, 0, 0, 0, 16384, 0, 0, 0, 16384]


def test_preset_identity_and_rejections(emu_lib):  # noqa: F811
    for p in (1, 2, 5, 6, 9):
        assert list(emu_lib.colour_preset(1, p, 1, p).matrix[:]) == [16384, 0, 0, 0, 16384, 0, 0, 0, 16384]
    assert list(emu_lib.colour_preset(1, 2, 1, 1).matrix[:]) == [16384, 0, 0, 0, 16384, 0, 0, 0, 16384]        # unspecified counts as BT.709
    for a, b in ((1, 9), (9, 1), (5, 6), (6, 9)):
        m = emu_lib.colour_preset(1, a, 1, b).matrix[:]
        assert [sum(m[3 * r:3 * r + 3]) for r in range(3)] == [16384] * 3 and m[1] != 0
    ok = dict(in_transfer=16, in_primaries=9, out_transfer=1, out_primaries=1, tone=capi.TONE_REINHARD, white_nits=203, peak_nits=1000, reserved=0)
    emu_lib.colour_preset(**ok)
    bad = [dict(in_transfer=3), dict(in_transfer=0), dict(in_transfer=17), dict(out_transfer=16), dict(out_transfer=18), dict(out_transfer=4), dict(in_primaries=4),
           dict(in_primaries=0), dict(out_primaries=8), dict(out_primaries=12), dict(tone=2), dict(tone=-1), dict(reserved=1), dict(white_nits=-1),
           dict(peak_nits=-5), dict(peak_nits=100), dict(white_nits=0, peak_nits=202)]
    for b in bad:
        with pytest.raises(capi.M355Error) as e:
            emu_lib.colour_preset(**dict(ok, **b))
        assert e.value.code == M355_ERR_INVALID, b
    d, t = capi.ColourPresetDesc(16, 9, 1, 1, 0, 0, 0, 0), capi.ColourTables()
    assert emu_lib.lib.m355_colour_preset(None, ctypes.byref(t)) == M355_ERR_INVALID
    assert emu_lib.lib.m355_colour_preset(ctypes.byref(d), None) == M355_ERR_INVALID
    emu_lib.colour_preset(16, 9, 1, 1, white_nits=203, peak_nits=203)                                            # peak == white is given and allowed


@pytest.mark.parametrize("name", ["random", "preset"])
@pytest.mark.parametrize("bit_depth", [8, 10])
def test_kernel_cases(ctx, bit_depth, name):
    cu.check_kernel_cases(ctx, bit_depth, TABLE_SETS[name], name)


@pytest.mark.parametrize("name", ["random", "preset"])
def test_wider_than_a_tile(ctx, name):
    cu.check_wide(ctx, TABLE_SETS[name], name)


@pytest.mark.parametrize("name", ["random", "preset"])
def test_tensor_and_rois(ctx, name):
    cu.check_tensors(ctx, TABLE_SETS[name], name)


def test_extreme_tables_and_neutral_grey(ctx):
    cu.check_extreme(ctx)
    cu.check_grey(ctx)


def test_handle_zero_is_the_plain_call(ctx):
    cu.check_handle_zero_is_plain(ctx)


def test_handles_and_rejections(emu_lib, ctx):  # noqa: F811
    lib = ctx.L.lib
    other = capi.Context(emu_lib, 0)
    nbytes = 1 << 16
    buf = ctx.device_alloc(nbytes)
    frame = ctx.frame_create(64, 32, 1, 8, 8)
    live, dead, foreign = ctx.colour_create(cu.to_ctypes(RANDOM)), ctx.colour_create(cu.to_ctypes(PRESET)), other.colour_create(cu.to_ctypes(RANDOM))
    ctx.colour_destroy(dead)
    assert live >= 0x100 and dead >= 0x100 and foreign >= 0x100 and len({live, dead, foreign}) == 3

    def opts(colour):
        o = capi.ExportOpts()
        o.reserved[0] = colour
        return ctypes.byref(o)

    rgb = capi.RgbDesc(layout=capi.RGB_PACKED, samples=U8, matrix=capi.MATRIX_BT709, full_range=0)
    rgb.dst[0] = buf; rgb.pitch[0] = 400
    rs = capi.ResizeDesc(layout=capi.EXPORT_PLANAR, samples=capi.EXPORT_NATIVE, out_width=32, out_height=16)
    rr = capi.ResizeRgbDesc(layout=capi.RGB_PACKED, samples=U8, matrix=capi.MATRIX_BT709, full_range=0, out_width=32, out_height=16)
    rr.dst[0] = buf; rr.pitch[0] = 400
    for k in range(3):
        rs.dst[k] = buf + 8192 * k; rs.pitch[k] = 128
    td = capi.TensorDesc(layout=capi.TENSOR_NHWC, dtype=capi.TENSOR_F32, samples=U8, matrix=capi.MATRIX_BT709, full_range=0, out_width=32, out_height=16,
                         stride_n=32768, stride_c=0, stride_h=512)
    td.scale = (ctypes.c_float * 3)(1, 1, 1)
    td.dst = buf
    roi = (capi.TensorRoi * 1)(capi.TensorRoi(0, 0, 64, 32, 0))
    one = (ctypes.c_int * 1)(frame)

    def composed(o):
        return [("resized rgb", lib.m355_frame_export_resized_rgb_opts(ctx.h, frame, ctypes.byref(rr), o)),
                ("tensor", lib.m355_frames_export_tensor_opts(ctx.h, one, 1, ctypes.byref(td), o)),
                ("rois", lib.m355_frames_export_tensor_rois_opts(ctx.h, one, roi, 1, ctypes.byref(td), o))]

    for what, h in (("destroyed", dead), ("another context's", foreign), ("the value 1", 1), ("negative", -live), ("255", 0xFF)):
        for name, rc in composed(opts(h)):
            assert rc == M355_ERR_INVALID, "%s accepts %s handle" % (name, what)
    assert lib.m355_frame_export_rgb_opts(ctx.h, frame, ctypes.byref(rgb), opts(live)) == M355_ERR_INVALID
    assert lib.m355_frame_export_resized_opts(ctx.h, frame, ctypes.byref(rs), opts(live)) == M355_ERR_INVALID
    ctx.wait()
    assert np.all(ctx.device_read(buf, nbytes) == capi.DEVICE_FILL), "a rejected export wrote to its destination"
    for name, rc in composed(opts(live)):
        assert rc == 0, (name, ctx.L.error())
    assert lib.m355_colour_destroy(ctx.h, dead) == M355_ERR_INVALID and lib.m355_colour_destroy(ctx.h, foreign) == M355_ERR_INVALID
    assert lib.m355_colour_destroy(ctx.h, 0) == M355_ERR_INVALID and lib.m355_colour_destroy(None, live) == M355_ERR_INVALID
    ctx.colour_destroy(live)
    other.colour_destroy(foreign)
    ctx.device_free(buf)
    ctx.frame_destroy(frame)
    other.close()


def test_sixteen_objects_and_the_checks_of_create(ctx):
    lib = ctx.L.lib
    t = cu.to_ctypes(RANDOM)
    handles = [ctx.colour_create(t) for _ in range(capi.COLOUR_OBJECTS)]
    assert len(set(handles)) == capi.COLOUR_OBJECTS and min(handles) >= 0x100
    h = ctypes.c_int(0)
    assert lib.m355_colour_create(ctx.h, ctypes.byref(t), ctypes.byref(h)) == M355_ERR_BUSY
    ctx.colour_destroy(handles.pop())
    handles.append(ctx.colour_create(t))
    assert len(set(handles)) == capi.COLOUR_OBJECTS
    for x in handles:
        ctx.colour_destroy(x)
    assert lib.m355_colour_create(ctx.h, None, ctypes.byref(h)) == M355_ERR_INVALID
    assert lib.m355_colour_create(ctx.h, ctypes.byref(t), None) == M355_ERR_INVALID
    assert lib.m355_colour_create(None, ctypes.byref(t), ctypes.byref(h)) == M355_ERR_INVALID
    for field, k, v in (("lut_in", 0, ONE + 1), ("lut_in", 1024, 0xFFFFFFFF), ("matrix", 0, 65536), ("matrix", 8, -65536), ("pad", None, 1)):
        bad = cu.to_ctypes(RANDOM)
        if k is None:
            setattr(bad, field, v)
        else:
            getattr(bad, field)[k] = v
        assert lib.m355_colour_create(ctx.h, ctypes.byref(bad), ctypes.byref(h)) == M355_ERR_INVALID, (field, k)
    edge = cu.to_ctypes(dict(RANDOM, matrix=np.array([65535, -65535] * 4 + [0])))
    edge.lut_in[5] = ONE
    ctx.colour_destroy(ctx.colour_create(edge))


def test_destroy_directly_after_an_export(ctx):
    cu.check_destroy_after_export(ctx)


def test_gate_and_recycled_frames(ctx):
    """(the interpreter runs every launch to its end at once: this walks the bookkeeping, the GPU tier sees a missing wait)"""
    cu.check_gate_colour(ctx)
    cu.check_hazard_colour(ctx, 1)
    cu.check_hazard_colour(ctx, 3)
