"""What the exports answer to malformed calls, pinned word for word: the return code, the text of m355_last_error() and — where two arguments are wrong —
which of the two is reported.  The table below is run against the SIMT-interpreter build (and once, marked gpu, against the product library) and held
against tests/golden/export_rejections.json, which was recorded from the same table with the build BEFORE the exports' host side was folded into
runtime_export.hip: a refactor of the checks must leave every entry as it is.  No case launches a kernel: every call is rejected.

A case is (name, kind, call).  kind "cross": two faults that different stages of the entry point check (plan, options, resize check, descriptor check);
kind "within": two faults of one stage; the earlier check must win in both.  Frames: 64x32 4:2:0 8-bit, 64x32 4:0:0 8-bit, 64x32 4:2:2 10-bit and a second
4:2:0 frame of 48x24 for the batch checks, created in this order in a fresh context (messages name frame handles).

M355_RECORD_EXPORT_REJECTIONS=1 writes the JSON instead of comparing (only ever against a build whose answers are the reference)."""
import ctypes
import json
import os

import pytest

from test_emu_picture import emu_lib  # noqa: F401  (fixture)
from libde265_amd import capi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "export_rejections.json")
PLANAR, SEMI, NATIVE, MSB16, U8 = capi.EXPORT_PLANAR, capi.EXPORT_SEMIPLANAR, capi.EXPORT_NATIVE, capi.EXPORT_MSB16, capi.EXPORT_U8
GHOST = 0x7FFF0000                 # a colour handle no context ever gives out in a test run (handles count up from 0x100)
CROSS, WITHIN = "cross", "within"


def build_cases(ctx):
    """-> [(name, kind, call)]; every call returns the entry point's return code"""
    lib = ctx.L.lib
    f420 = ctx.frame_create(64, 32, 1, 8, 8)
    mono = ctx.frame_create(64, 32, 0, 8, 8)
    f422 = ctx.frame_create(64, 32, 2, 10, 10)
    other = ctx.frame_create(48, 24, 1, 8, 8)
    buf = ctx.device_alloc(1 << 16)
    inf, nan = float("inf"), float("nan")
    ref = ctypes.byref
    D3 = (0, 16384, 32768)                                            # three planes inside buf

    def planes(d, dst, pitch):
        for k in range(3):
            d.dst[k] = None if dst[k] is None else buf + dst[k]
            d.pitch[k] = pitch[k]
        return d

    def rect_of(d, rect):
        d.x0, d.y0, d.width, d.height = rect
        return d

    def ed(layout=PLANAR, samples=NATIVE, rect=(0, 0, 0, 0), dst=D3, pitch=(128, 128, 128)):
        return planes(rect_of(capi.ExportDesc(layout=layout, samples=samples), rect), dst, pitch)

    def rd(layout=capi.RGB_PACKED, samples=capi.RGB_U8, matrix=capi.MATRIX_BT709, full=0, rect=(0, 0, 0, 0), dst=D3, pitch=(512, 512, 512)):
        return planes(rect_of(capi.RgbDesc(layout=layout, samples=samples, matrix=matrix, full_range=full), rect), dst, pitch)

    def zd(layout=PLANAR, samples=NATIVE, out=(32, 16), rect=(0, 0, 0, 0), dst=D3, pitch=(128, 128, 128)):
        return planes(rect_of(capi.ResizeDesc(layout=layout, samples=samples, out_width=out[0], out_height=out[1]), rect), dst, pitch)

    def zrd(layout=capi.RGB_PACKED, samples=capi.RGB_U8, matrix=capi.MATRIX_BT709, full=0, out=(32, 16), rect=(0, 0, 0, 0), dst=D3, pitch=(512, 512, 512)):
        d = capi.ResizeRgbDesc(layout=layout, samples=samples, matrix=matrix, full_range=full, out_width=out[0], out_height=out[1])
        return planes(rect_of(d, rect), dst, pitch)

    def td(out=(32, 16), layout=capi.TENSOR_NCHW, dtype=capi.TENSOR_F16, samples=capi.RGB_U8, matrix=capi.MATRIX_BT709, full=0, rect=(0, 0, 0, 0),
           scale=(1, 1, 1), bias=(0, 0, 0), dst=0, sn=4096, sc=1200, sh=72):
        d = capi.TensorDesc(layout=layout, dtype=dtype, samples=samples, matrix=matrix, full_range=full, out_width=out[0], out_height=out[1],
                            stride_n=sn, stride_c=sc, stride_h=sh)
        rect_of(d, rect)
        d.scale = (ctypes.c_float * 3)(*scale)
        d.bias = (ctypes.c_float * 3)(*bias)
        d.dst = None if dst is None else buf + dst
        return d

    def opts(filter=0, chroma_loc=0, colour=0, reserved=None):
        o = capi.ExportOpts(filter=filter, chroma_loc=chroma_loc)
        o.reserved[0] = colour
        for k, v in (reserved or {}).items():
            o.reserved[k] = v
        return o

    def export(f, d):
        return lambda: lib.m355_frame_export(ctx.h, f, ref(d) if d is not None else None)

    def scaled(f, d, k):
        return lambda: lib.m355_frame_export_scaled(ctx.h, f, ref(d) if d is not None else None, k)

    def with_opts(entry):
        def bound(f, d, o=None):
            return lambda: entry(ctx.h, f, ref(d) if d is not None else None, ref(o) if o is not None else None)
        return bound

    rgb, resized, resized_rgb = (with_opts(lib.m355_frame_export_rgb_opts), with_opts(lib.m355_frame_export_resized_opts),
                                 with_opts(lib.m355_frame_export_resized_rgb_opts))

    def ints(frames):
        return (ctypes.c_int * max(1, len(frames)))(*frames) if frames is not None else None

    def tensor(frames, d, o=None, n=None, c=ctx.h):
        return lambda: lib.m355_frames_export_tensor_opts(c, ints(frames), len(frames) if n is None else n, ref(d) if d is not None else None,
                                                          ref(o) if o is not None else None)

    def rois(frames, rr, d, o=None, n=None, c=ctx.h):
        ra = (capi.TensorRoi * max(1, len(rr)))(*[capi.TensorRoi(*r) for r in rr]) if rr is not None else None
        return lambda: lib.m355_frames_export_tensor_rois_opts(c, ints(frames), ra, len(frames) if n is None else n, ref(d) if d is not None else None,
                                                               ref(o) if o is not None else None)

    def coeffs(matrix, full, bdl, bdc, samples, out=True):
        k = capi.RgbCoeffs()
        return lambda: lib.m355_rgb_coefficients(matrix, full, bdl, bdc, samples, ref(k) if out else None)

    def tables(lut_in0=0, matrix0=0, pad=0):
        t = capi.ColourTables(pad=pad)
        t.lut_in[0], t.matrix[0] = lut_in0, matrix0
        return t

    def colour_create(t, c=ctx.h, handle=True):
        h = ctypes.c_int(0)
        return lambda: lib.m355_colour_create(c, ref(t) if t is not None else None, ref(h) if handle else None)

    def colour_create_when_full():
        made, h = [], ctypes.c_int(0)
        t = tables()
        for _ in range(capi.COLOUR_OBJECTS):
            assert lib.m355_colour_create(ctx.h, ref(t), ref(h)) == 0, ctx.L.error()
            made.append(h.value)
        rc, text = lib.m355_colour_create(ctx.h, ref(t), ref(h)), ctx.L.error()
        for m in made:
            assert lib.m355_colour_destroy(ctx.h, m) == 0
        return rc, text

    def colour_pixel(t, rgb=True, samples=capi.RGB_U8, out=True):
        a, b = (ctypes.c_uint32 * 3)(), (ctypes.c_uint32 * 3)()
        return lambda: lib.m355_colour_pixel(ref(t) if t is not None else None, a if rgb else None, samples, b if out else None)

    def preset(d, out=True):
        t = capi.ColourTables()
        return lambda: lib.m355_colour_preset(ref(d) if d is not None else None, ref(t) if out else None)

    def element(scale, bias, dtype, out=True):
        bits = ctypes.c_uint32(0)
        return lambda: lib.m355_tensor_element(100, scale, bias, dtype, ref(bits) if out else None)

    W = (0, 0, 0, 0, 0)
    two = [f420, f420]
    return [
        # ---- m355_frame_export: one stage, the plan ----
        ("export: bad handle", None, export(99, ed())),
        ("export: negative handle", None, export(-1, ed())),
        ("export: null descriptor", None, export(f420, None)),
        ("export: unknown layout", None, export(f420, ed(layout=2))),
        ("export: unknown samples", None, export(f420, ed(samples=3))),
        ("export: rectangle leaves the frame", None, export(f420, ed(rect=(32, 0, 48, 16)))),
        ("export: rectangle of a negative width", None, export(f420, ed(rect=(0, 0, -4, 16)))),
        ("export: rectangle off the chroma grid", None, export(f420, ed(rect=(1, 0, 16, 16)))),
        ("export: rectangle off the 4:2:2 chroma grid", None, export(f422, ed(rect=(1, 1, 16, 15), pitch=(256, 256, 256)))),
        ("export: no destination for plane 1", None, export(f420, ed(dst=(0, None, 32768)))),
        ("export: no destination for the monochrome plane", None, export(mono, ed(dst=(None, None, None)))),
        ("export: pitch below the row of plane 0", None, export(f420, ed(pitch=(63, 128, 128)))),
        ("export: pitch below the interleaved row", None, export(f420, ed(layout=SEMI, pitch=(64, 63, 0)))),
        ("export: pitch below the 16-bit row of 4:2:2 chroma", None, export(f422, ed(pitch=(128, 63, 64)))),
        ("export: pitch below the MSB16 row", None, export(f420, ed(samples=MSB16, pitch=(127, 128, 128)))),
        ("export: bad handle and null descriptor", WITHIN, export(99, None)),
        ("export: unknown layout and unknown samples", WITHIN, export(f420, ed(layout=2, samples=3))),
        ("export: unknown samples and rectangle off the frame", WITHIN, export(f420, ed(samples=3, rect=(0, 0, 128, 32)))),
        ("export: rectangle off the frame and off the grid", WITHIN, export(f420, ed(rect=(1, 0, 64, 32)))),
        ("export: no destination and a short pitch of plane 0", WITHIN, export(f420, ed(dst=(None, 16384, 32768), pitch=(1, 128, 128)))),
        ("export: short pitch of plane 1 and no destination for plane 2", WITHIN, export(f420, ed(dst=(0, 16384, None), pitch=(128, 31, 128)))),
        ("export: unknown layout and no destination", CROSS, export(f420, ed(layout=2, dst=(None, None, None)))),
        ("export: rectangle off the grid and a short pitch", CROSS, export(f420, ed(rect=(0, 1, 16, 16), pitch=(1, 1, 1)))),
        # ---- m355_frame_export_scaled: the scale, then the plan ----
        ("scaled: log2_scale 4", None, scaled(f420, ed(), 4)),
        ("scaled: log2_scale negative", None, scaled(f420, ed(), -1)),
        ("scaled: log2_scale 0 is the plain export", None, scaled(f420, ed(layout=2), 0)),
        ("scaled: width no multiple of the blocks", None, scaled(f420, ed(rect=(0, 0, 62, 32)), 1)),
        ("scaled: 4:2:2 height no multiple of the blocks", None, scaled(f422, ed(rect=(0, 0, 64, 30), pitch=(256, 256, 256)), 2)),
        ("scaled: whole 48x24 frame no multiple of the blocks", None, scaled(other, ed(), 3)),
        ("scaled: pitch below the scaled row", None, scaled(f420, ed(pitch=(31, 128, 128)), 1)),
        ("scaled: no destination for plane 2", None, scaled(f420, ed(dst=(0, 16384, None)), 1)),
        ("scaled: unknown samples", None, scaled(f420, ed(samples=-1), 2)),
        ("scaled: log2_scale 4 and a bad handle", CROSS, scaled(99, ed(), 4)),
        ("scaled: log2_scale 5 and a null descriptor", CROSS, scaled(f420, None, 5)),
        ("scaled: no multiple and no destination", CROSS, scaled(f420, ed(rect=(0, 0, 62, 32), dst=(None, None, None)), 1)),
        ("scaled: rectangle off the grid and no multiple", WITHIN, scaled(f420, ed(rect=(1, 0, 62, 32)), 1)),
        # ---- m355_frame_export_rgb_opts: plan, options, descriptor ----
        ("rgb: bad handle", None, rgb(99, rd())),
        ("rgb: null descriptor", None, rgb(f420, None)),
        ("rgb: rectangle leaves the frame", None, rgb(f420, rd(rect=(0, 16, 64, 32)))),
        ("rgb: rectangle off the chroma grid", None, rgb(f420, rd(rect=(0, 0, 16, 15)))),
        ("rgb: no destination for plane 0", None, rgb(f420, rd(dst=(None, 16384, 32768)))),
        ("rgb: reserved[3] set", None, rgb(f420, rd(), opts(reserved={3: 7}))),
        ("rgb: a colour transform", None, rgb(f420, rd(), opts(colour=GHOST))),
        ("rgb: a filter", None, rgb(f420, rd(), opts(filter=1))),
        ("rgb: chroma_loc 4", None, rgb(f420, rd(), opts(chroma_loc=4))),
        ("rgb: chroma_loc negative", None, rgb(f420, rd(), opts(chroma_loc=-1))),
        ("rgb: chroma_loc 1 for 4:2:2", None, rgb(f422, rd(), opts(chroma_loc=1))),
        ("rgb: chroma_loc 2 for 4:0:0", None, rgb(mono, rd(), opts(chroma_loc=2))),
        ("rgb: unknown layout", None, rgb(f420, rd(layout=2))),
        ("rgb: unknown matrix", None, rgb(f420, rd(matrix=3))),
        ("rgb: unknown samples", None, rgb(f420, rd(samples=2))),
        ("rgb: full_range 2, null options", None, rgb(f420, rd(full=2), None)),
        ("rgb: no destination for plane 2", None, rgb(f420, rd(layout=capi.RGB_PLANAR, dst=(0, 16384, None)))),
        ("rgb: packed pitch below the row", None, rgb(f420, rd(pitch=(191, 0, 0)))),
        ("rgb: planar pitch of plane 1 below the row", None, rgb(f420, rd(layout=capi.RGB_PLANAR, pitch=(64, 63, 64)))),
        ("rgb: 16-bit plane at an odd address", None, rgb(f420, rd(samples=capi.RGB_U16, dst=(1, 16384, 32768)))),
        ("rgb: 16-bit plane with an odd pitch", None, rgb(f420, rd(samples=capi.RGB_U16, pitch=(385, 512, 512)))),
        ("rgb: no destination for plane 0 and reserved set", CROSS, rgb(f420, rd(dst=(None, None, None)), opts(reserved={1: 1}))),
        ("rgb: rectangle off the frame and chroma_loc 4", CROSS, rgb(f420, rd(rect=(0, 0, 66, 32)), opts(chroma_loc=4))),
        ("rgb: reserved set and unknown layout", CROSS, rgb(f420, rd(layout=2), opts(reserved={5: -1}))),
        ("rgb: a filter and an unknown matrix", CROSS, rgb(f420, rd(matrix=3), opts(filter=1))),
        ("rgb: chroma_loc for 4:2:2 and a short pitch", CROSS, rgb(f422, rd(pitch=(10, 0, 0)), opts(chroma_loc=3))),
        ("rgb: reserved set and chroma_loc 9", WITHIN, rgb(f420, rd(), opts(chroma_loc=9, reserved={2: 2}))),
        ("rgb: a colour transform and a filter", WITHIN, rgb(f420, rd(), opts(filter=1, colour=GHOST))),
        ("rgb: a filter and chroma_loc 4", WITHIN, rgb(f420, rd(), opts(filter=2, chroma_loc=4))),
        ("rgb: unknown layout and unknown matrix", WITHIN, rgb(f420, rd(layout=-1, matrix=3))),
        ("rgb: unknown matrix and no destination for plane 1", WITHIN, rgb(f420, rd(layout=capi.RGB_PLANAR, matrix=-1, dst=(0, None, 32768)))),
        ("rgb: 16-bit pitch short and odd", WITHIN, rgb(f420, rd(samples=capi.RGB_U16, pitch=(383, 0, 0)))),
        ("rgb: plane 1 at an odd address and no destination for plane 2", WITHIN,
         rgb(f420, rd(layout=capi.RGB_PLANAR, samples=capi.RGB_U16, dst=(0, 16385, None)))),
        # ---- m355_frame_export_resized_opts: plan, options, resize check, destinations ----
        ("resized: bad handle", None, resized(99, zd())),
        ("resized: null descriptor", None, resized(f420, None)),
        ("resized: unknown layout", None, resized(f420, zd(layout=2))),
        ("resized: unknown samples", None, resized(f420, zd(samples=3))),
        ("resized: rectangle leaves the frame", None, resized(f420, zd(rect=(60, 0, 8, 8)))),
        ("resized: reserved[1] set", None, resized(f420, zd(), opts(reserved={1: 1}))),
        ("resized: a colour transform", None, resized(f420, zd(), opts(colour=GHOST))),
        ("resized: chroma_loc 1 for 4:0:0", None, resized(mono, zd(), opts(chroma_loc=1))),
        ("resized: unknown filter", None, resized(f420, zd(), opts(filter=2))),
        ("resized: out_width 0", None, resized(f420, zd(out=(0, 16)))),
        ("resized: out_height negative", None, resized(f420, zd(out=(32, -16)))),
        ("resized: out_width odd, 4:2:0", None, resized(f420, zd(out=(33, 16)))),
        ("resized: out_height odd, 4:2:0", None, resized(f420, zd(out=(32, 15)))),
        ("resized: out_width odd, 4:2:2", None, resized(f422, zd(out=(33, 15), pitch=(256, 256, 256)))),
        ("resized: more than 8x down", None, resized(f420, zd(out=(6, 16)))),
        ("resized: more than 8x up", None, resized(f420, zd(rect=(0, 0, 2, 2), out=(32, 16)))),
        ("resized: cubic, more than 4x down", None, resized(f420, zd(out=(14, 16)), opts(filter=1))),
        ("resized: no destination for plane 1", None, resized(f420, zd(dst=(0, None, 32768)))),
        ("resized: pitch below the output row", None, resized(f420, zd(pitch=(31, 128, 128)))),
        ("resized: pitch below the interleaved output row", None, resized(f420, zd(layout=SEMI, pitch=(32, 31, 0)))),
        ("resized: pitch below the 16-bit output row", None, resized(f422, zd(pitch=(64, 31, 32)))),
        ("resized: no destination for the monochrome plane", None, resized(mono, zd(dst=(None, None, None)))),
        ("resized: unknown layout and no destination", CROSS, resized(f420, zd(layout=2, dst=(None, None, None)))),
        ("resized: rectangle off the frame and an odd output size", CROSS, resized(f420, zd(rect=(0, 0, 64, 34), out=(33, 17)))),
        ("resized: reserved set and more than 8x down", CROSS, resized(f420, zd(out=(6, 16)), opts(reserved={4: 1}))),
        ("resized: chroma_loc 5 and an unknown filter", CROSS, resized(f420, zd(), opts(filter=2, chroma_loc=5))),
        ("resized: more than 8x down and no destination", CROSS, resized(f420, zd(out=(6, 16), dst=(None, None, None)))),
        ("resized: unknown samples and a colour transform", CROSS, resized(f420, zd(samples=3), opts(colour=GHOST))),
        ("resized: unknown filter and out_width 0", WITHIN, resized(f420, zd(out=(0, 16)), opts(filter=2))),
        ("resized: odd output size and more than 8x down", WITHIN, resized(f420, zd(out=(7, 16)))),
        ("resized: no destination and a short pitch of plane 1", WITHIN, resized(f420, zd(dst=(0, None, 32768), pitch=(32, 1, 16)))),
        # ---- m355_frame_export_resized_rgb_opts: plan, options (with the colour transform), resize check, descriptor ----
        ("resized rgb: bad handle", None, resized_rgb(99, zrd())),
        ("resized rgb: null descriptor", None, resized_rgb(f420, None)),
        ("resized rgb: rectangle off the chroma grid", None, resized_rgb(f420, zrd(rect=(2, 1, 16, 16)))),
        ("resized rgb: unknown colour transform", None, resized_rgb(f420, zrd(), opts(colour=GHOST))),
        ("resized rgb: chroma_loc 3 for 4:2:2", None, resized_rgb(f422, zrd(), opts(chroma_loc=3))),
        ("resized rgb: unknown filter", None, resized_rgb(f420, zrd(), opts(filter=-1))),
        ("resized rgb: out_width odd", None, resized_rgb(f420, zrd(out=(31, 16)))),
        ("resized rgb: cubic, more than 4x down", None, resized_rgb(f420, zrd(out=(32, 6)), opts(filter=1))),
        ("resized rgb: more than 8x down", None, resized_rgb(f420, zrd(out=(32, 2)))),
        ("resized rgb: unknown layout", None, resized_rgb(f420, zrd(layout=2))),
        ("resized rgb: unknown matrix", None, resized_rgb(f420, zrd(matrix=3))),
        ("resized rgb: no destination for plane 0", None, resized_rgb(f420, zrd(dst=(None, 16384, 32768)))),
        ("resized rgb: pitch below the output row", None, resized_rgb(f420, zrd(pitch=(95, 0, 0)))),
        ("resized rgb: 16-bit planar plane 2 at an odd address", None,
         resized_rgb(f420, zrd(layout=capi.RGB_PLANAR, samples=capi.RGB_U16, dst=(0, 16384, 32769)))),
        ("resized rgb: unknown colour transform and more than 8x down", CROSS, resized_rgb(f420, zrd(out=(6, 16)), opts(colour=GHOST))),
        ("resized rgb: an odd output size and an unknown layout", CROSS, resized_rgb(f420, zrd(layout=2, out=(33, 16)))),
        ("resized rgb: cubic ratio and an unknown matrix", CROSS, resized_rgb(f420, zrd(matrix=3, out=(14, 16)), opts(filter=1))),
        ("resized rgb: bad handle and reserved set", CROSS, resized_rgb(-5, zrd(), opts(reserved={1: 3}))),
        ("resized rgb: unknown filter and no destination", CROSS, resized_rgb(f420, zrd(dst=(None, None, None)), opts(filter=7))),
        ("resized rgb: unknown samples and a short pitch", WITHIN, resized_rgb(f420, zrd(samples=2, pitch=(1, 1, 1)))),
        # ---- m355_frames_export_tensor_opts: the batch, plan per frame, options, resize check, descriptor ----
        ("tensor: n 0", None, tensor([f420], td(), n=0)),
        ("tensor: n 33", None, tensor([f420] * 33, td())),
        ("tensor: null frames", None, tensor(None, td(), n=1)),
        ("tensor: null descriptor", None, tensor([f420], None)),
        ("tensor: null context", None, tensor([f420], td(), c=None)),
        ("tensor: bad handle in entry 1", None, tensor([f420, 99], td())),
        ("tensor: another chroma format in entry 1", None, tensor([f420, f422], td())),
        ("tensor: monochrome beside 4:2:0", None, tensor([mono, f420], td())),
        ("tensor: whole frames of different sizes", None, tensor([f420, other], td())),
        ("tensor: a rectangle the second frame does not hold", None, tensor([f420, other], td(rect=(0, 0, 64, 32)))),
        ("tensor: reserved[5] set", None, tensor(two, td(), opts(reserved={5: 1}))),
        ("tensor: unknown colour transform", None, tensor(two, td(), opts(colour=GHOST))),
        ("tensor: unknown filter", None, tensor(two, td(), opts(filter=2))),
        ("tensor: out_height odd", None, tensor(two, td(out=(32, 17)))),
        ("tensor: more than 8x down", None, tensor(two, td(out=(6, 16)))),
        ("tensor: cubic, more than 4x down", None, tensor(two, td(out=(14, 16)), opts(filter=1))),
        ("tensor: unknown layout", None, tensor(two, td(layout=2))),
        ("tensor: unknown dtype", None, tensor(two, td(dtype=3))),
        ("tensor: unknown matrix", None, tensor(two, td(matrix=3))),
        ("tensor: scale infinite", None, tensor(two, td(scale=(1, inf, 1)))),
        ("tensor: bias NaN", None, tensor(two, td(bias=(0, 0, nan)))),
        ("tensor: no destination", None, tensor(two, td(dst=None))),
        ("tensor: F16 destination at an odd address", None, tensor(two, td(dst=1))),
        ("tensor: F32 stride_c off a multiple of 4", None, tensor(two, td(dtype=capi.TENSOR_F32, sh=128, sc=2050, sn=8192))),
        ("tensor: stride_h below the row", None, tensor(two, td(sh=62))),
        ("tensor: stride_c lets the planes overlap", None, tensor(two, td(sc=15 * 72 + 62, sn=8192))),
        ("tensor: stride_n lets the slices overlap", None, tensor(two, td(sc=15 * 72 + 64, sn=3 * (15 * 72 + 64) - 2))),
        ("tensor: NHWC stride_n lets the slices overlap", None, tensor(two, td(layout=capi.TENSOR_NHWC, sh=200, sn=15 * 200 + 190))),
        ("tensor: unknown colour transform and unknown dtype", CROSS, tensor(two, td(dtype=3), opts(colour=GHOST))),
        ("tensor: another chroma format and reserved set", CROSS, tensor([f420, f422], td(), opts(reserved={2: 1}))),
        ("tensor: an odd output size and scale infinite", CROSS, tensor(two, td(out=(33, 16), scale=(inf, 1, 1)))),
        ("tensor: bad handle in entry 1 and unknown layout", CROSS, tensor([f420, -1], td(layout=2))),
        ("tensor: chroma_loc 4 and more than 8x down", CROSS, tensor(two, td(out=(6, 16)), opts(chroma_loc=4))),
        ("tensor: n 0 and a null descriptor", WITHIN, tensor([f420], None, n=0)),
        ("tensor: rectangle off entry 0 and a bad handle in entry 1", WITHIN, tensor([f420, 99], td(rect=(0, 0, 65, 32)))),
        ("tensor: unknown layout and unknown dtype", WITHIN, tensor(two, td(layout=2, dtype=3))),
        ("tensor: unknown dtype and unknown matrix", WITHIN, tensor(two, td(dtype=-1, matrix=3))),
        ("tensor: no destination and stride_h below the row", WITHIN, tensor(two, td(dst=None, sh=2))),
        ("tensor: an odd stride_h below the row", WITHIN, tensor(two, td(sh=61))),
        # ---- m355_frames_export_tensor_rois_opts: the batch, flags and plan per entry, options, resize check per entry, descriptor ----
        ("rois: n 0", None, rois([f420], [W], td(), n=0)),
        ("rois: n 33", None, rois([f420] * 33, [W] * 33, td())),
        ("rois: null rois", None, rois([f420], None, td())),
        ("rois: null descriptor", None, rois([f420], [W], None)),
        ("rois: null context", None, rois([f420], [W], td(), c=None)),
        ("rois: a descriptor rectangle", None, rois(two, [W, W], td(rect=(0, 0, 64, 32)))),
        ("rois: an unknown flag in entry 1", None, rois(two, [W, (0, 0, 64, 32, 2)], td())),
        ("rois: bad handle in entry 1", None, rois([f420, 99], [W, W], td())),
        ("rois: an entry that leaves its smaller frame", None, rois([f420, other], [W, (0, 0, 64, 32, 0)], td())),
        ("rois: an entry off the chroma grid", None, rois(two, [W, (1, 0, 16, 16, 0)], td())),
        ("rois: another chroma format in entry 1", None, rois([f420, f422], [W, W], td())),
        ("rois: reserved[1] set", None, rois(two, [W, W], td(), opts(reserved={1: 9}))),
        ("rois: unknown colour transform", None, rois(two, [W, W], td(), opts(colour=GHOST))),
        ("rois: out_width 0", None, rois(two, [W, W], td(out=(0, 16)))),
        ("rois: more than 8x up in entry 1", None, rois(two, [W, (0, 0, 2, 2, 0)], td())),
        ("rois: more than 8x down in entry 0", None, rois([f420, other], [W, W], td(out=(6, 16)))),
        ("rois: cubic, more than 4x down in entry 1", None, rois(two, [(0, 0, 32, 16, 0), W], td(out=(14, 16)), opts(filter=1))),
        ("rois: unknown dtype", None, rois(two, [W, W], td(dtype=3))),
        ("rois: no destination", None, rois(two, [W, W], td(dst=None))),
        ("rois: stride_n lets the slices overlap", None, rois(two, [W, W], td(sn=2 * 1200 + 15 * 72 + 62))),
        ("rois: an unknown flag in entry 1 and a bad rectangle in entry 0", CROSS, rois(two, [(0, 0, 66, 32, 0), (0, 0, 64, 32, 4)], td())),
        ("rois: a ratio in entry 1 and stride_n overlapping", CROSS, rois(two, [W, (0, 0, 2, 2, 0)], td(sn=64))),
        ("rois: unknown colour transform and a cubic ratio", CROSS, rois(two, [W, W], td(out=(14, 16)), opts(filter=1, colour=GHOST))),
        ("rois: a descriptor rectangle and an unknown flag", WITHIN, rois(two, [(0, 0, 64, 32, 8), W], td(rect=(0, 0, 0, 8)))),
        ("rois: an entry off its frame and unknown matrix", CROSS, rois([other, f420], [(0, 0, 64, 32, 0), W], td(matrix=3))),
        ("rois: n 0 and a descriptor rectangle", WITHIN, rois([f420], [W], td(rect=(0, 0, 64, 32)), n=0)),
        ("rois: an unknown flag and a bad rectangle in entry 0", WITHIN, rois(two, [(0, 0, 66, 32, 2), W], td())),
        # ---- the host-only calls and the colour objects ----
        ("coefficients: null result", None, coeffs(1, 0, 8, 8, 0, out=False)),
        ("coefficients: unknown matrix", None, coeffs(3, 0, 8, 8, 0)),
        ("coefficients: full_range 2", None, coeffs(1, 2, 8, 8, 0)),
        ("coefficients: unknown samples", None, coeffs(1, 0, 8, 8, 2)),
        ("coefficients: luma depth 7", None, coeffs(1, 0, 7, 8, 0)),
        ("coefficients: chroma depth 17", None, coeffs(1, 0, 8, 17, 1)),
        ("coefficients: null result and unknown matrix", WITHIN, coeffs(3, 0, 8, 8, 0, out=False)),
        ("coefficients: unknown matrix and luma depth 7", WITHIN, coeffs(-1, 0, 7, 8, 0)),
        ("colour create: null context", None, colour_create(tables(), c=None)),
        ("colour create: null tables", None, colour_create(None)),
        ("colour create: null handle", None, colour_create(tables(), handle=False)),
        ("colour create: lut_in above one", None, colour_create(tables(lut_in0=capi.COLOUR_ONE + 1))),
        ("colour create: matrix entry outside", None, colour_create(tables(matrix0=-65536))),
        ("colour create: pad set", None, colour_create(tables(pad=1))),
        ("colour create: lut_in above one and pad set", WITHIN, colour_create(tables(lut_in0=capi.COLOUR_ONE + 1, pad=1))),
        ("colour create: every object live", None, colour_create_when_full),
        ("colour destroy: null context", None, lambda: lib.m355_colour_destroy(None, GHOST)),
        ("colour destroy: handle 0", None, lambda: lib.m355_colour_destroy(ctx.h, 0)),
        ("colour destroy: unknown handle", None, lambda: lib.m355_colour_destroy(ctx.h, GHOST)),
        ("colour preset: null descriptor", None, preset(None)),
        ("colour preset: null tables", None, preset(capi.ColourPresetDesc(1, 1, 1, 1, 0, 0, 0, 0), out=False)),
        ("colour preset: unknown transfer", None, preset(capi.ColourPresetDesc(3, 1, 1, 1, 0, 0, 0, 0))),
        ("colour pixel: null tables", None, colour_pixel(None)),
        ("colour pixel: null input", None, colour_pixel(tables(), rgb=False)),
        ("colour pixel: null output", None, colour_pixel(tables(), out=False)),
        ("colour pixel: unknown samples", None, colour_pixel(tables(), samples=2)),
        ("colour pixel: tables outside their bounds", None, colour_pixel(tables(pad=5))),
        ("tensor element: null result", None, element(1.0, 0.0, capi.TENSOR_F16, out=False)),
        ("tensor element: unknown dtype", None, element(1.0, 0.0, 3)),
        ("tensor element: scale infinite", None, element(inf, 0.0, capi.TENSOR_F32)),
        ("tensor element: bias NaN", None, element(1.0, nan, capi.TENSOR_BF16)),
        ("export wait: bad handle", None, lambda: lib.m355_frame_export_wait(ctx.h, 99)),
        ("export order: bad handle", None, lambda: lib.m355_frame_export_order(ctx.h, -1, None)),
    ]


def run(ctx):
    """-> {name: [return code, m355_last_error()]} and the kinds' counts"""
    got, kinds = {}, {CROSS: 0, WITHIN: 0}
    for name, kind, call in build_cases(ctx):
        assert name not in got, name
        r = call()
        rc, text = r if isinstance(r, tuple) else (r, ctx.L.error())
        assert rc != 0, "%s: accepted (the table holds rejected calls only: none may launch)" % name
        got[name] = [rc, text]
        if kind:
            kinds[kind] += 1
    return got, kinds


def check(lib):
    ctx = capi.Context(lib, 0)
    try:
        got, kinds = run(ctx)
    finally:
        ctx.close()
    assert kinds[CROSS] >= 12 and kinds[WITHIN] >= 4, kinds
    if os.environ.get("M355_RECORD_EXPORT_REJECTIONS"):
        with open(GOLDEN, "w") as f:
            json.dump(got, f, indent=1, sort_keys=True)
            f.write("\n")
        return
    with open(GOLDEN) as f:
        want = json.load(f)
    assert sorted(got) == sorted(want), "the table and the recording hold different cases"
    wrong = {n: (got[n], want[n]) for n in got if got[n] != want[n]}
    assert not wrong, "\n".join("%s: got %r, recorded %r" % (n, g, w) for n, (g, w) in sorted(wrong.items()))


def test_export_rejections_match_the_recording(emu_lib):  # noqa: F811
    check(emu_lib)


@pytest.mark.gpu
def test_export_rejections_match_the_recording_on_the_gpu():
    lib = capi.Library()
    assert lib.device_count() >= 1
    check(lib)
