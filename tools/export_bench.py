#!/usr/bin/env python3
"""What m355_frame_export costs at the C5 frame geometry (7680x4320, 10-bit, 4:2:0), timed with events on the context's stream in one process:

  (a) three hipMemcpy2DAsync device-to-device plane copies on that stream, between buffers with the frame's pitch — what an application
      could do today if it had the plane pointers
  (b) m355_frame_export NATIVE planar, whole frame
  (c) MSB16 semi-planar, the frame minus an 8-sample border (x0 = y0 = 8: misaligned source rows)
  (d) U8 semi-planar, whole frame
  (e), (f) what separates (c) from (b): MSB16 semi-planar uncropped, NATIVE planar cropped
  (g), (h), (i) m355_frame_export_scaled NATIVE planar, whole frame, downscaled 2x, 4x, 8x
  (j) U8 semi-planar downscaled 4x: the 8K to 1080p NV12 proxy
  (k), (l) m355_frame_export_rgb, whole frame, BT.709 limited range: U8 packed and U16 planar.  (k) reads the frame's 99.5 MB and writes
      7680 * 4320 * 3 = 99.5 MB — exactly the bytes of (b), which is therefore its traffic floor; the result line has (k) / (b)
  (m), (n) m355_frame_export_resized to 1920x1080, NATIVE planar and U8 semi-planar: the output sizes of (h) and (j); the result line has (m) / (h)
      and (n) / (j), the cost of the triangle over the box at the same traffic
  (o), (p) m355_frame_export_resized NATIVE planar to 2560x1440 (ratio 3) and to 1280x720 (ratio 6)
  (q), (r), (s) m355_frame_export_resized_rgb, BT.709 limited range: U8 packed and U16 planar to 1920x1080, U8 planar (CHW) to 1280x720
  (t), (u), (v) m355_frame_export_rgb of a frame of the resized size — the second half of the chain that (q), (r), (s) replace: U8 packed and U16
      planar of the 1920x1080 window of a 1920x1088 10-bit frame, U8 planar of a 1280x720 frame.  One launch must not lose to the two it fuses:
      the bars are (q) <= (m) + (t), (r) <= (m) + (u), (s) <= (p) + (v), each + the spread of (b)
  (w), (x) m355_frames_export_tensor of the one frame, F16 NHWC to 1920x1080, and m355_frame_export_resized_rgb U16 packed of the same geometry: the
      same bytes written, only the epilogue differs; the bar is (w) <= (x) + the spread of (b).  (r) is the planar row beside (x)
  (y8), (z8), (y32), (z32) a 224x224 export of the 1080x1080 window (420, 0) of N = 8 / 32 frames of 1920x1088: (y) N consecutive
      m355_frame_export_resized_rgb U8 planar launches, one per frame; (z) ONE m355_frames_export_tensor batch of the same N frames, F16 NCHW.  A
      slice is 14 workgroups, so a single launch leaves most of the chip empty; the bars are (z) <= (y) + the spread of (b)
  (R8), (R32) m355_frames_export_tensor_rois with 8 / 32 regions all equal to the window of (z8), (z32), of the same frames: the new call where the old
      one can do the same; the bars are (R) <= (z) + the spread (max - min) of that (z) row's own rounds
  (S32), (T32) 32 DIFFERENT regions of one 1920x1088 frame to 224x224, F16 NCHW — a seeded list (ROI_SEED) that holds both ratio limits (28x28: 8x up,
      1792 columns: 8x down) and regions of two tiles across, printed in the result line: (S32) 32 m355_frames_export_tensor launches with n = 1,
      one per region; (T32) ONE m355_frames_export_tensor_rois of the list, every fourth region mirrored.  The bar is (T32) <= (S32) + the spread of (b)
  (Q8), (Q32) m355_frames_export_tensor_rois with 8 / 32 regions of 896x896 at (512, 96) of the frames of (z8), (z32) to 224x224, F16 NCHW: ratio
      exactly 4, the most M355_FILTER_CUBIC takes
  --filter cubic adds, beside (m), (n), (q), (w), (Q8), (Q32), the same calls through the _filtered entry points with M355_FILTER_CUBIC as (Cm), (Cn),
      (Cq), (Cw), (CQ8), (CQ32) — 8K to 1080p is ratio exactly 4 — and their ratios to the triangle's rows in the result line; no bar is set for them
  --chroma-loc N (1, 2 or 3; may repeat) adds, beside (k), (l), (m), (n), (q), (w), (Q8), (Q32), the same calls through the _opts entry points with
      chroma sample location type N as (LNk), (LNl), (LNm), (LNn), (LNq), (LNw), (LNQ8), (LNQ32), and their ratios to the type-0 rows; no bar is set
  --colour adds, beside (q), (w), (z8), (z32), (T32), (Q8), (Q32), the same calls through the _opts entry points with a colour transform (the preset PQ /
      BT.2020 -> gamma 2.4 / BT.709, Reinhard, 203 / 1000 nits) as (Kq), (Kw), (Kz8), (Kz32), (KT32), (KQ8), (KQ32), on frames of seeded RANDOM samples — the
      stage gathers from its tables by the pixel's value, so a constant frame would show its best case —, the colour-off calls on those frames as (K0q),
      (K0z32), and the ratios in the result line; no bar is set for them
  --tone (implies --colour) adds, beside the seven K rows, the same calls with a tone object (m355_colour_create_tone: the preset PQ / BT.2020 -> gamma
      2.4 / BT.709, BT.2390, maxRGB, 203 / 1000 nits) as (Gq), (Gw), (Gz8), (Gz32), (GT32), (GQ8), (GQ32), and their ratios to the K rows; no bar is set
  --pixels adds the pixel formats (m355_frame_export_pixels, m355_frame_export_resized_pixels) and, beside them, the packed R'G'B' rows of the same frame
      and size they are held against — a pixel is 4 bytes, between the 3 of U8 packed and the 6 of U16 packed, and the destination is the larger side of
      the traffic: (Pk16) m355_frame_export_rgb U16 packed of the whole frame, beside (k); (Xk8), (Xk10) BGRA8 and A2R10G10B10 of the whole frame;
      (Pq8), (Pq16) m355_frame_export_resized_rgb U8 / U16 packed to 3840x2160 of a frame of seeded RANDOM samples, (Xq8), (Xq10) the two pixel formats of
      the same call, and (PG8), (PG16), (XG8), (XG10) the four with the tone object of --tone.  A library without the pixel entry points (a parent build
      loaded through M355_LIB) runs the P rows only.  No bar is set; the result line says whether each X row lies between its two P rows

and, beside them, m355_measure_copy_rate for the frame's byte count.  Every figure is the median of --iters launches; (b) is measured in
--rounds separate rounds spread over the run, and the spread of their medians is the margin (c), (d), (g)-(j) and (m)-(p) are held against: a scaled or resized export reads exactly (b)'s source bytes and writes at most a
quarter of (b)'s destination bytes, so it should not be slower than (b).  Beside each scaled row: its source bytes / time.  The HIP calls
of (a) and the events go to the runtime the library itself has loaded (no second runtime in the process).

  python tools/export_bench.py [--out profiles/export_bench.txt]
"""
import argparse
import ctypes
import json
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from libde265_amd import capi  # noqa: E402

W, H, BD = 7680, 4320, 10
D2D = 3   # hipMemcpyDeviceToDevice
ROI_SEED = 8500


def hip_runtime():
    """the HIP runtime the product library is linked against, as already mapped into this process"""
    with open("/proc/self/maps") as f:
        for line in f:
            if "libamdhip64" in line:
                return ctypes.CDLL(line.split()[-1])
    raise RuntimeError("the product library has not loaded a HIP runtime")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="append the result lines to this file")
    ap.add_argument("--filter", choices=("triangle", "cubic"), default="triangle", help="cubic: also measure the cubic filter's rows beside the triangle's")
    ap.add_argument("--chroma-loc", type=int, choices=(1, 2, 3), action="append", default=[],
                    help="also measure this chroma sample location type's rows beside the type-0 rows (may repeat)")
    ap.add_argument("--colour", action="store_true", help="also measure the composed exports with a colour transform, on frames of random samples")
    ap.add_argument("--tone", action="store_true", help="also measure the colour rows with a tone object (one gain per pixel: BT.2390, maxRGB); implies --colour")
    ap.add_argument("--pixels", action="store_true", help="also measure the pixel-format exports beside the packed R'G'B' rows of the same frame and size")
    args = ap.parse_args()
    args.colour = args.colour or args.tone

    lib = capi.Library()
    ctx = capi.Context(lib, 0)
    hip = hip_runtime()
    vp = ctypes.c_void_p
    hip.hipEventCreate.argtypes = [ctypes.POINTER(vp)]
    hip.hipEventRecord.argtypes = [vp, vp]
    hip.hipEventSynchronize.argtypes = [vp]
    hip.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), vp, vp]
    hip.hipMemcpy2DAsync.argtypes = [vp, ctypes.c_size_t, vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int, vp]
    e0, e1 = vp(), vp()
    assert hip.hipEventCreate(ctypes.byref(e0)) == 0 and hip.hipEventCreate(ctypes.byref(e1)) == 0

    frame = ctx.frame_create(W, H, 1, BD, BD)
    ctx.frame_fill(frame, 600, 500)
    stream = ctx.stream()          # the frame was written by no decode: its exports run on the active lane's stream
    planes = [(W, H), (W // 2, H // 2), (W // 2, H // 2)]
    frame_bytes = sum(w * h * 2 for w, h in planes)
    pitch = [(w * 2 + 127) // 128 * 128 for w, h in planes]
    src = [ctx.device_alloc(p * h + 256, fill=0x5A) for p, (w, h) in zip(pitch, planes)]
    # one set of destinations, large enough for every variant
    dst = [ctx.device_alloc(n, fill=None) for n in (W * 2 * H, W * 2 * (H // 2), W * (H // 2))]

    def timed(fn):
        ms = []
        for k in range(-3, args.iters):
            hip.hipEventRecord(e0, stream)
            fn()
            hip.hipEventRecord(e1, stream)
            assert hip.hipEventSynchronize(e1) == 0
            t = ctypes.c_float()
            assert hip.hipEventElapsedTime(ctypes.byref(t), e0, e1) == 0
            if k >= 0:
                ms.append(t.value)
        return statistics.median(ms)

    def copies():
        for k, (w, h) in enumerate(planes):
            assert hip.hipMemcpy2DAsync(dst[k], w * 2, src[k], pitch[k], w * 2, h, D2D, stream) == 0

    def export(layout, samples, rect, elem, log2_scale=0):
        d = capi.ExportDesc(layout=layout, samples=samples)
        if rect:
            d.x0, d.y0, d.width, d.height = rect
        w = (rect[2] if rect else W) >> log2_scale
        rows = [w * elem, w * elem if layout else w // 2 * elem, w // 2 * elem]
        for k in range(3):
            d.dst[k] = dst[k]; d.pitch[k] = rows[k]
        if log2_scale:
            return lambda: lib.check(lib.lib.m355_frame_export_scaled(ctx.h, frame, ctypes.byref(d), log2_scale))
        return lambda: lib.check(lib.lib.m355_frame_export(ctx.h, frame, ctypes.byref(d)))

    def opts_of(filter, loc, colour=0):
        o = capi.ExportOpts(filter=filter, chroma_loc=loc)
        o.reserved[0] = colour
        return o

    def export_resized(layout, samples, out_size, elem, filter=0, loc=0):
        d = capi.ResizeDesc(layout=layout, samples=samples, out_width=out_size[0], out_height=out_size[1])
        w = out_size[0]
        rows = [w * elem, w * elem if layout else w // 2 * elem, w // 2 * elem]
        for k in range(3):
            d.dst[k] = dst[k]; d.pitch[k] = rows[k]
        if loc:
            o = opts_of(filter, loc)
            return lambda: lib.check(lib.lib.m355_frame_export_resized_opts(ctx.h, frame, ctypes.byref(d), ctypes.byref(o)))
        if filter:
            return lambda: lib.check(lib.lib.m355_frame_export_resized_filtered(ctx.h, frame, ctypes.byref(d), filter))
        return lambda: lib.check(lib.lib.m355_frame_export_resized(ctx.h, frame, ctypes.byref(d)))

    rgb_dst = [ctx.device_alloc(n, fill=None) for n in (W * 3 * H, W * 2 * H, W * 2 * H)]

    def export_rgb(layout, samples, elem, loc=0):
        d = capi.RgbDesc(layout=layout, samples=samples, matrix=capi.MATRIX_BT709, full_range=0)
        for k in range(3):
            d.dst[k] = rgb_dst[k]; d.pitch[k] = W * elem * (1 if layout == capi.RGB_PLANAR else 3)
        if loc:
            o = opts_of(0, loc)
            return lambda: lib.check(lib.lib.m355_frame_export_rgb_opts(ctx.h, frame, ctypes.byref(d), ctypes.byref(o)))
        return lambda: lib.check(lib.lib.m355_frame_export_rgb(ctx.h, frame, ctypes.byref(d)))

    def export_resized_rgb(layout, samples, out_size, elem, filter=0, loc=0, colour=0, frame=frame):
        d = capi.ResizeRgbDesc(layout=layout, samples=samples, matrix=capi.MATRIX_BT709, full_range=0, out_width=out_size[0], out_height=out_size[1])
        for k in range(3):
            d.dst[k] = rgb_dst[k]; d.pitch[k] = out_size[0] * elem * (1 if layout == capi.RGB_PLANAR else 3)
        if loc or colour:
            o = opts_of(filter, loc, colour)
            return lambda: lib.check(lib.lib.m355_frame_export_resized_rgb_opts(ctx.h, frame, ctypes.byref(d), ctypes.byref(o)))
        if filter:
            return lambda: lib.check(lib.lib.m355_frame_export_resized_rgb_filtered(ctx.h, frame, ctypes.byref(d), filter))
        return lambda: lib.check(lib.lib.m355_frame_export_resized_rgb(ctx.h, frame, ctypes.byref(d)))

    # frames of the resized sizes, for the R'G'B' export that the chain ends with (a frame's height is a multiple of 8: 1088 rows, of which 1080)
    small = {(1920, 1080): ctx.frame_create(1920, 1088, 1, BD, BD), (1280, 720): ctx.frame_create(1280, 720, 1, BD, BD)}
    for f in small.values():
        ctx.frame_fill(f, 600, 500)

    def export_rgb_small(layout, samples, size, elem):
        d = capi.RgbDesc(layout=layout, samples=samples, matrix=capi.MATRIX_BT709, full_range=0)
        d.x0, d.y0, d.width, d.height = 0, 0, size[0], size[1]
        for k in range(3):
            d.dst[k] = rgb_dst[k]; d.pitch[k] = size[0] * elem * (1 if layout == capi.RGB_PLANAR else 3)
        return lambda: lib.check(lib.lib.m355_frame_export_rgb(ctx.h, small[size], ctypes.byref(d)))

    def export_tensor(frames, layout, dtype, samples, out_size, rect=None, filter=0, loc=0, colour=0):
        eb = 4 if dtype == capi.TENSOR_F32 else 2
        ow, oh = out_size
        row = ow * eb * (3 if layout == capi.TENSOR_NHWC else 1)
        sc = oh * row if layout == capi.TENSOR_NCHW else 0
        d = capi.TensorDesc(layout=layout, dtype=dtype, samples=samples, matrix=capi.MATRIX_BT709, full_range=0, out_width=ow, out_height=oh,
                            stride_n=3 * ow * oh * eb, stride_c=sc, stride_h=row)
        M = 65535.0 if samples == capi.RGB_U16 else 255.0
        d.scale = (ctypes.c_float * 3)(*[1.0 / (M * x) for x in (0.229, 0.224, 0.225)])
        d.bias = (ctypes.c_float * 3)(*[-m / x for m, x in zip((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))])
        if rect:
            d.x0, d.y0, d.width, d.height = rect
        assert len(frames) * 3 * ow * oh * eb <= W * 3 * H
        d.dst = rgb_dst[0]
        arr = (ctypes.c_int * len(frames))(*frames)
        if loc or colour:
            o = opts_of(filter, loc, colour)
            return lambda: lib.check(lib.lib.m355_frames_export_tensor_opts(ctx.h, arr, len(frames), ctypes.byref(d), ctypes.byref(o)))
        if filter:
            return lambda: lib.check(lib.lib.m355_frames_export_tensor_filtered(ctx.h, arr, len(frames), ctypes.byref(d), filter))
        return lambda: lib.check(lib.lib.m355_frames_export_tensor(ctx.h, arr, len(frames), ctypes.byref(d)))

    def export_tensor_rois(frames, rois, layout, dtype, samples, out_size, filter=0, loc=0, colour=0):
        eb = 4 if dtype == capi.TENSOR_F32 else 2
        ow, oh = out_size
        row = ow * eb * (3 if layout == capi.TENSOR_NHWC else 1)
        sc = oh * row if layout == capi.TENSOR_NCHW else 0
        d = capi.TensorDesc(layout=layout, dtype=dtype, samples=samples, matrix=capi.MATRIX_BT709, full_range=0, out_width=ow, out_height=oh,
                            stride_n=3 * ow * oh * eb, stride_c=sc, stride_h=row)
        M = 65535.0 if samples == capi.RGB_U16 else 255.0
        d.scale = (ctypes.c_float * 3)(*[1.0 / (M * x) for x in (0.229, 0.224, 0.225)])
        d.bias = (ctypes.c_float * 3)(*[-m / x for m, x in zip((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))])
        assert len(frames) == len(rois) and len(frames) * 3 * ow * oh * eb <= W * 3 * H
        d.dst = rgb_dst[0]
        arr = (ctypes.c_int * len(frames))(*frames)
        ra = (capi.TensorRoi * len(rois))(*[capi.TensorRoi(*r) for r in rois])
        if loc or colour:
            o = opts_of(filter, loc, colour)
            return lambda: lib.check(lib.lib.m355_frames_export_tensor_rois_opts(ctx.h, arr, ra, len(frames), ctypes.byref(d), ctypes.byref(o)))
        if filter:
            return lambda: lib.check(lib.lib.m355_frames_export_tensor_rois_filtered(ctx.h, arr, ra, len(frames), ctypes.byref(d), filter))
        return lambda: lib.check(lib.lib.m355_frames_export_tensor_rois(ctx.h, arr, ra, len(frames), ctypes.byref(d)))

    # the frames of the batch rows: 32 frames of 1920x1088, of which the centre square goes to a model's 224x224
    batch = [ctx.frame_create(1920, 1088, 1, BD, BD) for _ in range(32)]
    for k, f in enumerate(batch):
        ctx.frame_fill(f, 300 + 20 * k, 400 + 10 * k)
    SQUARE = (420, 0, 1080, 1080)
    SQUARE4 = (512, 96, 896, 896)      # to 224x224: ratio exactly 4

    def singles(n):
        descs = []
        for k in range(n):
            d = capi.ResizeRgbDesc(layout=capi.RGB_PLANAR, samples=capi.RGB_U8, matrix=capi.MATRIX_BT709, full_range=0, out_width=224, out_height=224)
            d.x0, d.y0, d.width, d.height = SQUARE
            for c in range(3):
                d.dst[c] = rgb_dst[0] + (3 * k + c) * 224 * 224; d.pitch[c] = 224
            descs.append(d)

        def run():
            for k in range(n):
                lib.check(lib.lib.m355_frame_export_resized_rgb(ctx.h, batch[k], ctypes.byref(descs[k])))
        return run

    # 32 different regions of batch[0] that 224x224 accepts (28..1792 columns, 28..1088 rows, on the chroma grid): the two ratio limits first, then
    # seeded ones, of which those of 510 columns and more have two tiles across
    rng = random.Random(ROI_SEED)
    roi_list = [(946, 530, 28, 28), (64, 0, 1792, 1088), (288, 4, 1344, 1080)]
    while len(roi_list) < 32:
        w, h = 2 * rng.randint(14, 896), 2 * rng.randint(14, 544)
        r = (2 * rng.randint(0, (1920 - w) // 2), 2 * rng.randint(0, (1088 - h) // 2), w, h)
        if r not in roi_list:
            roi_list.append(r)

    def single_rois():
        calls = []
        for k, r in enumerate(roi_list):
            d = capi.TensorDesc(layout=capi.TENSOR_NCHW, dtype=capi.TENSOR_F16, samples=capi.RGB_U8, matrix=capi.MATRIX_BT709, full_range=0, out_width=224,
                                out_height=224, stride_n=3 * 224 * 224 * 2, stride_c=224 * 224 * 2, stride_h=224 * 2)
            d.scale = (ctypes.c_float * 3)(*[1.0 / (255.0 * x) for x in (0.229, 0.224, 0.225)])
            d.bias = (ctypes.c_float * 3)(*[-m / x for m, x in zip((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))])
            d.x0, d.y0, d.width, d.height = r
            d.dst = rgb_dst[0] + k * 3 * 224 * 224 * 2
            calls.append((d, (ctypes.c_int * 1)(batch[0])))

        def run():
            for d, arr in calls:
                lib.check(lib.lib.m355_frames_export_tensor(ctx.h, arr, 1, ctypes.byref(d)))
        return run

    variants = {
        "a_memcpy2d_x3": copies,
        "b_native_planar": export(capi.EXPORT_PLANAR, capi.EXPORT_NATIVE, None, 2),
        "c_msb16_semiplanar_crop8": export(capi.EXPORT_SEMIPLANAR, capi.EXPORT_MSB16, (8, 8, W - 16, H - 16), 2),
        "d_u8_semiplanar": export(capi.EXPORT_SEMIPLANAR, capi.EXPORT_U8, None, 1),
        # beside the four: (c) without its crop (aligned source rows, interleaved stores) and (b) with it (misaligned rows, plain stores)
        "e_msb16_semiplanar": export(capi.EXPORT_SEMIPLANAR, capi.EXPORT_MSB16, None, 2),
        "f_native_planar_crop8": export(capi.EXPORT_PLANAR, capi.EXPORT_NATIVE, (8, 8, W - 16, H - 16), 2),
        "g_native_planar_2x": export(capi.EXPORT_PLANAR, capi.EXPORT_NATIVE, None, 2, 1),
        "h_native_planar_4x": export(capi.EXPORT_PLANAR, capi.EXPORT_NATIVE, None, 2, 2),
        "i_native_planar_8x": export(capi.EXPORT_PLANAR, capi.EXPORT_NATIVE, None, 2, 3),
        "j_u8_semiplanar_4x": export(capi.EXPORT_SEMIPLANAR, capi.EXPORT_U8, None, 1, 2),
        "k_rgb_u8_packed": export_rgb(capi.RGB_PACKED, capi.RGB_U8, 1),
        "l_rgb_u16_planar": export_rgb(capi.RGB_PLANAR, capi.RGB_U16, 2),
        "m_resized_native_planar_1080p": export_resized(capi.EXPORT_PLANAR, capi.EXPORT_NATIVE, (1920, 1080), 2),
        "n_resized_u8_semiplanar_1080p": export_resized(capi.EXPORT_SEMIPLANAR, capi.EXPORT_U8, (1920, 1080), 1),
        "o_resized_native_planar_1440p": export_resized(capi.EXPORT_PLANAR, capi.EXPORT_NATIVE, (2560, 1440), 2),
        "p_resized_native_planar_720p": export_resized(capi.EXPORT_PLANAR, capi.EXPORT_NATIVE, (1280, 720), 2),
        "q_resized_rgb_u8_packed_1080p": export_resized_rgb(capi.RGB_PACKED, capi.RGB_U8, (1920, 1080), 1),
        "r_resized_rgb_u16_planar_1080p": export_resized_rgb(capi.RGB_PLANAR, capi.RGB_U16, (1920, 1080), 2),
        "s_resized_rgb_u8_planar_720p": export_resized_rgb(capi.RGB_PLANAR, capi.RGB_U8, (1280, 720), 1),
        "t_rgb_u8_packed_of_1080p": export_rgb_small(capi.RGB_PACKED, capi.RGB_U8, (1920, 1080), 1),
        "u_rgb_u16_planar_of_1080p": export_rgb_small(capi.RGB_PLANAR, capi.RGB_U16, (1920, 1080), 2),
        "v_rgb_u8_planar_of_720p": export_rgb_small(capi.RGB_PLANAR, capi.RGB_U8, (1280, 720), 1),
        "w_tensor_f16_nhwc_1080p": export_tensor([frame], capi.TENSOR_NHWC, capi.TENSOR_F16, capi.RGB_U16, (1920, 1080)),
        "x_resized_rgb_u16_packed_1080p": export_resized_rgb(capi.RGB_PACKED, capi.RGB_U16, (1920, 1080), 2),
        "y8_resized_rgb_u8_planar_224_x8": singles(8),
        "z8_tensor_f16_nchw_224_batch8": export_tensor(batch[:8], capi.TENSOR_NCHW, capi.TENSOR_F16, capi.RGB_U8, (224, 224), SQUARE),
        "y32_resized_rgb_u8_planar_224_x32": singles(32),
        "z32_tensor_f16_nchw_224_batch32": export_tensor(batch, capi.TENSOR_NCHW, capi.TENSOR_F16, capi.RGB_U8, (224, 224), SQUARE),
        "R8_tensor_rois_f16_nchw_224_batch8": export_tensor_rois(batch[:8], [SQUARE + (0,)] * 8, capi.TENSOR_NCHW, capi.TENSOR_F16, capi.RGB_U8, (224, 224)),
        "R32_tensor_rois_f16_nchw_224_batch32": export_tensor_rois(batch, [SQUARE + (0,)] * 32, capi.TENSOR_NCHW, capi.TENSOR_F16, capi.RGB_U8, (224, 224)),
        "S32_tensor_f16_nchw_224_x32_regions": single_rois(),
        "T32_tensor_rois_f16_nchw_224_32_regions": export_tensor_rois([batch[0]] * 32, [r + (capi.ROI_MIRROR if k % 4 == 3 else 0,) for k, r in enumerate(roi_list)],
                                                                      capi.TENSOR_NCHW, capi.TENSOR_F16, capi.RGB_U8, (224, 224)),
    }
    def region_rows(prefix, filter, loc=0):
        return {"%sQ%d_tensor_rois_f16_nchw_224_of_896_batch%d" % (prefix, n, n):
                export_tensor_rois(batch[:n], [SQUARE4 + (0,)] * n, capi.TENSOR_NCHW, capi.TENSOR_F16, capi.RGB_U8, (224, 224), filter, loc) for n in (8, 32)}

    variants.update(region_rows("", 0))
    cubic_of = {}                      # a cubic row -> the triangle's row of the same call
    if args.filter == "cubic":
        C = capi.FILTER_CUBIC
        variants.update({
            "Cm_cubic_resized_native_planar_1080p": export_resized(capi.EXPORT_PLANAR, capi.EXPORT_NATIVE, (1920, 1080), 2, C),
            "Cn_cubic_resized_u8_semiplanar_1080p": export_resized(capi.EXPORT_SEMIPLANAR, capi.EXPORT_U8, (1920, 1080), 1, C),
            "Cq_cubic_resized_rgb_u8_packed_1080p": export_resized_rgb(capi.RGB_PACKED, capi.RGB_U8, (1920, 1080), 1, C),
            "Cw_cubic_tensor_f16_nhwc_1080p": export_tensor([frame], capi.TENSOR_NHWC, capi.TENSOR_F16, capi.RGB_U16, (1920, 1080), None, C),
        })
        variants.update(region_rows("C", C))
        for n in variants:
            if n[0] == "C":
                key = n[1:].split("_")[0] + "_"
                cubic_of[n] = [t for t in variants if t.startswith(key)][0]
    sited_of = {}                      # a row of another chroma sample location type -> the type-0 row of the same call
    for loc in sorted(set(args.chroma_loc)):
        L = "L%d" % loc
        rows = {
            L + "k_sited_rgb_u8_packed": export_rgb(capi.RGB_PACKED, capi.RGB_U8, 1, loc),
            L + "l_sited_rgb_u16_planar": export_rgb(capi.RGB_PLANAR, capi.RGB_U16, 2, loc),
            L + "m_sited_resized_native_planar_1080p": export_resized(capi.EXPORT_PLANAR, capi.EXPORT_NATIVE, (1920, 1080), 2, 0, loc),
            L + "n_sited_resized_u8_semiplanar_1080p": export_resized(capi.EXPORT_SEMIPLANAR, capi.EXPORT_U8, (1920, 1080), 1, 0, loc),
            L + "q_sited_resized_rgb_u8_packed_1080p": export_resized_rgb(capi.RGB_PACKED, capi.RGB_U8, (1920, 1080), 1, 0, loc),
            L + "w_sited_tensor_f16_nhwc_1080p": export_tensor([frame], capi.TENSOR_NHWC, capi.TENSOR_F16, capi.RGB_U16, (1920, 1080), None, 0, loc),
        }
        rows.update(region_rows(L, 0, loc))
        for n in rows:
            key = n[2:].split("_")[0] + "_"
            sited_of[n] = [t for t in variants if t.startswith(key)][0]
        variants.update(rows)
    colour_of, made = {}, []           # a row with a colour transform -> the colour-off row of the same call
    tone_of = {}                       # a row with a tone object -> the row of the same call with the plain colour transform
    if args.colour:
        import numpy as np
        rng_c = np.random.default_rng(ROI_SEED)

        def random_frame(w, h):
            f = ctx.frame_create(w, h, 1, BD, BD)
            ctx.frame_upload(f, [rng_c.integers(0, 1 << BD, (ph, pw)).astype(np.uint16) for pw, ph in ((w, h), (w // 2, h // 2), (w // 2, h // 2))])
            made.append(f)
            return f

        cframe, cbatch = random_frame(W, H), [random_frame(1920, 1088) for _ in range(32)]
        K = ctx.colour_create(lib.colour_preset(16, 9, 1, 1, capi.TONE_REINHARD, 203, 1000))
        rois32 = [r + (capi.ROI_MIRROR if k % 4 == 3 else 0,) for k, r in enumerate(roi_list)]
        rows = {
            "K0q_random_resized_rgb_u8_packed_1080p": export_resized_rgb(capi.RGB_PACKED, capi.RGB_U8, (1920, 1080), 1, frame=cframe),
            "K0z32_random_tensor_f16_nchw_224_batch32": export_tensor(cbatch, capi.TENSOR_NCHW, capi.TENSOR_F16, capi.RGB_U8, (224, 224), SQUARE),
            "Kq_colour_resized_rgb_u8_packed_1080p": export_resized_rgb(capi.RGB_PACKED, capi.RGB_U8, (1920, 1080), 1, colour=K, frame=cframe),
            "Kw_colour_tensor_f16_nhwc_1080p": export_tensor([cframe], capi.TENSOR_NHWC, capi.TENSOR_F16, capi.RGB_U16, (1920, 1080), colour=K),
            "Kz8_colour_tensor_f16_nchw_224_batch8": export_tensor(cbatch[:8], capi.TENSOR_NCHW, capi.TENSOR_F16, capi.RGB_U8, (224, 224), SQUARE, colour=K),
            "Kz32_colour_tensor_f16_nchw_224_batch32": export_tensor(cbatch, capi.TENSOR_NCHW, capi.TENSOR_F16, capi.RGB_U8, (224, 224), SQUARE, colour=K),
            "KT32_colour_tensor_rois_f16_nchw_224_32_regions": export_tensor_rois([cbatch[0]] * 32, rois32, capi.TENSOR_NCHW, capi.TENSOR_F16, capi.RGB_U8, (224, 224), colour=K),
        }
        rows.update({"KQ%d_colour_tensor_rois_f16_nchw_224_of_896_batch%d" % (n, n):
                     export_tensor_rois(cbatch[:n], [SQUARE4 + (0,)] * n, capi.TENSOR_NCHW, capi.TENSOR_F16, capi.RGB_U8, (224, 224), colour=K) for n in (8, 32)})
        for n in rows:
            key = n[2 if n[1] == "0" else 1:].split("_")[0] + "_"
            colour_of[n] = [t for t in variants if t.startswith(key)][0]
        variants.update(rows)
        if args.tone:
            G = ctx.colour_create_tone(*lib.colour_preset_tone(16, 9, 1, 1, tone=capi.TONE_BT2390, norm=capi.NORM_MAXRGB, white_nits=203, peak_nits=1000))
            gains = {
                "Gq_tone_resized_rgb_u8_packed_1080p": export_resized_rgb(capi.RGB_PACKED, capi.RGB_U8, (1920, 1080), 1, colour=G, frame=cframe),
                "Gw_tone_tensor_f16_nhwc_1080p": export_tensor([cframe], capi.TENSOR_NHWC, capi.TENSOR_F16, capi.RGB_U16, (1920, 1080), colour=G),
                "Gz8_tone_tensor_f16_nchw_224_batch8": export_tensor(cbatch[:8], capi.TENSOR_NCHW, capi.TENSOR_F16, capi.RGB_U8, (224, 224), SQUARE, colour=G),
                "Gz32_tone_tensor_f16_nchw_224_batch32": export_tensor(cbatch, capi.TENSOR_NCHW, capi.TENSOR_F16, capi.RGB_U8, (224, 224), SQUARE, colour=G),
                "GT32_tone_tensor_rois_f16_nchw_224_32_regions": export_tensor_rois([cbatch[0]] * 32, rois32, capi.TENSOR_NCHW, capi.TENSOR_F16, capi.RGB_U8, (224, 224), colour=G),
            }
            gains.update({"GQ%d_tone_tensor_rois_f16_nchw_224_of_896_batch%d" % (n, n):
                          export_tensor_rois(cbatch[:n], [SQUARE4 + (0,)] * n, capi.TENSOR_NCHW, capi.TENSOR_F16, capi.RGB_U8, (224, 224), colour=G) for n in (8, 32)})
            for n in gains:
                tone_of[n] = [t for t in rows if t.startswith("K" + n[1:].split("_")[0] + "_")][0]
            variants.update(gains)
    pixel_of = {}                      # a pixel-format row -> (the U8 packed row, the U16 packed row) of the same frame and size
    if args.pixels:
        import numpy as np
        rng_p = np.random.default_rng(ROI_SEED + 1)
        pframe = ctx.frame_create(W, H, 1, BD, BD)
        ctx.frame_upload(pframe, [rng_p.integers(0, 1 << BD, (ph, pw)).astype(np.uint16) for pw, ph in planes])
        made.append(pframe)
        px_dst = ctx.device_alloc(W * 6 * H, fill=None)
        PG = ctx.colour_create_tone(*lib.colour_preset_tone(16, 9, 1, 1, tone=capi.TONE_BT2390, norm=capi.NORM_MAXRGB, white_nits=203, peak_nits=1000))
        UHD = (3840, 2160)

        def packed(samples, elem, out_size=None, colour=0):
            """the packed R'G'B' row: m355_frame_export_rgb of the whole frame, or m355_frame_export_resized_rgb_opts of the random frame to out_size"""
            if out_size is None:
                d = capi.RgbDesc(layout=capi.RGB_PACKED, samples=samples, matrix=capi.MATRIX_BT709, full_range=0)
                d.dst[0] = px_dst; d.pitch[0] = W * elem * 3
                return lambda: lib.check(lib.lib.m355_frame_export_rgb(ctx.h, frame, ctypes.byref(d)))
            d = capi.ResizeRgbDesc(layout=capi.RGB_PACKED, samples=samples, matrix=capi.MATRIX_BT709, full_range=0, out_width=out_size[0], out_height=out_size[1])
            d.dst[0] = px_dst; d.pitch[0] = out_size[0] * elem * 3
            o = opts_of(0, 0, colour)
            return lambda: lib.check(lib.lib.m355_frame_export_resized_rgb_opts(ctx.h, pframe, ctypes.byref(d), ctypes.byref(o)))

        def pixels(format, out_size=None, colour=0):
            d = capi.PixelDesc(format=format, alpha=3, matrix=capi.MATRIX_BT709, full_range=0)
            d.dst = px_dst
            if out_size is None:
                d.pitch = W * 4
                return lambda: lib.check(lib.lib.m355_frame_export_pixels(ctx.h, frame, ctypes.byref(d), None))
            d.out_width, d.out_height = out_size
            d.pitch = out_size[0] * 4
            o = opts_of(0, 0, colour)
            return lambda: lib.check(lib.lib.m355_frame_export_resized_pixels(ctx.h, pframe, ctypes.byref(d), ctypes.byref(o)))

        variants.update({
            "Pk16_rgb_u16_packed": packed(capi.RGB_U16, 2),
            "Pq8_random_resized_rgb_u8_packed_2160p": packed(capi.RGB_U8, 1, UHD),
            "Pq16_random_resized_rgb_u16_packed_2160p": packed(capi.RGB_U16, 2, UHD),
            "PG8_tone_resized_rgb_u8_packed_2160p": packed(capi.RGB_U8, 1, UHD, PG),
            "PG16_tone_resized_rgb_u16_packed_2160p": packed(capi.RGB_U16, 2, UHD, PG),
        })
        if hasattr(lib.lib, "m355_frame_export_pixels"):
            rows = {
                "Xk8_pixels_bgra8": (pixels(capi.PIXEL_BGRA8), "k_rgb_u8_packed", "Pk16_rgb_u16_packed"),
                "Xk10_pixels_a2r10g10b10": (pixels(capi.PIXEL_A2R10G10B10), "k_rgb_u8_packed", "Pk16_rgb_u16_packed"),
                "Xq8_random_resized_pixels_bgra8_2160p": (pixels(capi.PIXEL_BGRA8, UHD), "Pq8_random_resized_rgb_u8_packed_2160p", "Pq16_random_resized_rgb_u16_packed_2160p"),
                "Xq10_random_resized_pixels_a2r10g10b10_2160p": (pixels(capi.PIXEL_A2R10G10B10, UHD), "Pq8_random_resized_rgb_u8_packed_2160p",
                                                                 "Pq16_random_resized_rgb_u16_packed_2160p"),
                "XG8_tone_resized_pixels_bgra8_2160p": (pixels(capi.PIXEL_BGRA8, UHD, PG), "PG8_tone_resized_rgb_u8_packed_2160p", "PG16_tone_resized_rgb_u16_packed_2160p"),
                "XG10_tone_resized_pixels_a2r10g10b10_2160p": (pixels(capi.PIXEL_A2R10G10B10, UHD, PG), "PG8_tone_resized_rgb_u8_packed_2160p",
                                                               "PG16_tone_resized_rgb_u16_packed_2160p"),
            }
            for n, (fn, u8, u16) in rows.items():
                variants[n] = fn
                pixel_of[n] = (u8, u16)
    scaled = [n for n in variants if n[0] in "ghijmnop"]
    ms = {n: [] for n in variants}
    for _ in range(args.rounds):
        for n, fn in variants.items():
            ms[n].append(timed(fn))
    ctx.wait()
    res = {n: statistics.median(v) for n, v in ms.items()}
    b = ms["b_native_planar"]
    spread = max(b) - min(b)
    out = {
        "geometry": "%dx%d %d-bit 4:2:0, %d bytes per frame" % (W, H, BD, frame_bytes),
        "iters": args.iters, "rounds": args.rounds,
        "ms_median": res, "ms_rounds": ms, "b_spread_ms": spread,
        "GBps_read_plus_written": {"a_memcpy2d_x3": 2 * frame_bytes / res["a_memcpy2d_x3"] / 1e6, "b_native_planar": 2 * frame_bytes / res["b_native_planar"] / 1e6},
        "scaled_GBps_source_read": {n: frame_bytes / res[n] / 1e6 for n in scaled},
        "rgb": {"k_over_b": res["k_rgb_u8_packed"] / res["b_native_planar"], "l_over_b": res["l_rgb_u16_planar"] / res["b_native_planar"],
                "k_bytes_read_plus_written": frame_bytes + W * H * 3, "l_bytes_read_plus_written": frame_bytes + W * H * 6},
        "resized": {"m_over_h": res["m_resized_native_planar_1080p"] / res["h_native_planar_4x"],
                    "n_over_j": res["n_resized_u8_semiplanar_1080p"] / res["j_u8_semiplanar_4x"]},
        "resized_rgb": {"q_over_m_plus_t": res["q_resized_rgb_u8_packed_1080p"] / (res["m_resized_native_planar_1080p"] + res["t_rgb_u8_packed_of_1080p"]),
                        "r_over_m_plus_u": res["r_resized_rgb_u16_planar_1080p"] / (res["m_resized_native_planar_1080p"] + res["u_rgb_u16_planar_of_1080p"]),
                        "s_over_p_plus_v": res["s_resized_rgb_u8_planar_720p"] / (res["p_resized_native_planar_720p"] + res["v_rgb_u8_planar_of_720p"])},
        "tensor": {"w_over_x": res["w_tensor_f16_nhwc_1080p"] / res["x_resized_rgb_u16_packed_1080p"],
                   "z8_over_y8": res["z8_tensor_f16_nchw_224_batch8"] / res["y8_resized_rgb_u8_planar_224_x8"],
                   "z32_over_y32": res["z32_tensor_f16_nchw_224_batch32"] / res["y32_resized_rgb_u8_planar_224_x32"],
                   "us_per_frame": {n: 1e3 * res[n] / k for n, k in (("y8_resized_rgb_u8_planar_224_x8", 8), ("z8_tensor_f16_nchw_224_batch8", 8),
                                                                    ("y32_resized_rgb_u8_planar_224_x32", 32), ("z32_tensor_f16_nchw_224_batch32", 32))}},
        "tensor_rois": {"roi_seed": ROI_SEED, "rois": roi_list,
                        "z8_spread_ms": max(ms["z8_tensor_f16_nchw_224_batch8"]) - min(ms["z8_tensor_f16_nchw_224_batch8"]),
                        "z32_spread_ms": max(ms["z32_tensor_f16_nchw_224_batch32"]) - min(ms["z32_tensor_f16_nchw_224_batch32"]),
                        "R8_over_z8": res["R8_tensor_rois_f16_nchw_224_batch8"] / res["z8_tensor_f16_nchw_224_batch8"],
                        "R32_over_z32": res["R32_tensor_rois_f16_nchw_224_batch32"] / res["z32_tensor_f16_nchw_224_batch32"],
                        "T32_over_S32": res["T32_tensor_rois_f16_nchw_224_32_regions"] / res["S32_tensor_f16_nchw_224_x32_regions"],
                        "us_per_region": {n: 1e3 * res[n] / 32 for n in ("S32_tensor_f16_nchw_224_x32_regions", "T32_tensor_rois_f16_nchw_224_32_regions")}},
        "cubic_over_triangle": {n: res[n] / res[t] for n, t in cubic_of.items()},
        "sited_over_type_0": {n: res[n] / res[t] for n, t in sited_of.items()},
        "colour_over_colour_off": {n: res[n] / res[t] for n, t in colour_of.items()},
        "colour_rounds_ms": {n: ms[n] for n in colour_of},
        "tone_over_colour": {n: res[n] / res[t] for n, t in tone_of.items()},
        "tone_rounds_ms": {n: ms[n] for n in tone_of},
        "pixels": {n: {"ms": res[n], "u8_packed_ms": res[a], "u16_packed_ms": res[b_], "at_most_u16_packed": res[n] <= res[b_]} for n, (a, b_) in pixel_of.items()},
        "pixels_rounds_ms": {n: ms[n] for n in variants if n[0] in "PX"},
        "copy_rate_GBps_same_bytes": ctx.measure_copy_rate(frame_bytes, 9),
        "bars": {"b_le_a": res["b_native_planar"] <= res["a_memcpy2d_x3"],
                 "c_le_b_plus_spread": res["c_msb16_semiplanar_crop8"] <= res["b_native_planar"] + spread,
                 "d_le_b_plus_spread": res["d_u8_semiplanar"] <= res["b_native_planar"] + spread,
                 **{n[0] + "_le_b_plus_spread": res[n] <= res["b_native_planar"] + spread for n in scaled},
                 "q_le_m_plus_t_plus_spread": res["q_resized_rgb_u8_packed_1080p"] <= res["m_resized_native_planar_1080p"] + res["t_rgb_u8_packed_of_1080p"] + spread,
                 "r_le_m_plus_u_plus_spread": res["r_resized_rgb_u16_planar_1080p"] <= res["m_resized_native_planar_1080p"] + res["u_rgb_u16_planar_of_1080p"] + spread,
                 "s_le_p_plus_v_plus_spread": res["s_resized_rgb_u8_planar_720p"] <= res["p_resized_native_planar_720p"] + res["v_rgb_u8_planar_of_720p"] + spread,
                 "w_le_x_plus_spread": res["w_tensor_f16_nhwc_1080p"] <= res["x_resized_rgb_u16_packed_1080p"] + spread,
                 "z8_le_y8_plus_spread": res["z8_tensor_f16_nchw_224_batch8"] <= res["y8_resized_rgb_u8_planar_224_x8"] + spread,
                 "z32_le_y32_plus_spread": res["z32_tensor_f16_nchw_224_batch32"] <= res["y32_resized_rgb_u8_planar_224_x32"] + spread,
                 "R8_le_z8_plus_z8_spread": res["R8_tensor_rois_f16_nchw_224_batch8"] <= res["z8_tensor_f16_nchw_224_batch8"]
                 + max(ms["z8_tensor_f16_nchw_224_batch8"]) - min(ms["z8_tensor_f16_nchw_224_batch8"]),
                 "R32_le_z32_plus_z32_spread": res["R32_tensor_rois_f16_nchw_224_batch32"] <= res["z32_tensor_f16_nchw_224_batch32"]
                 + max(ms["z32_tensor_f16_nchw_224_batch32"]) - min(ms["z32_tensor_f16_nchw_224_batch32"]),
                 "T32_le_S32_plus_spread": res["T32_tensor_rois_f16_nchw_224_32_regions"] <= res["S32_tensor_f16_nchw_224_x32_regions"] + spread},
    }
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")
    for p in src + dst + rgb_dst + ([px_dst] if args.pixels else []):
        ctx.device_free(p)
    for f in list(small.values()) + batch + made:
        ctx.frame_destroy(f)
    ctx.close()


if __name__ == "__main__":
    main()
