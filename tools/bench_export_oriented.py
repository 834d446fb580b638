#!/usr/bin/env python3
"""What an oriented export (m355_frame_export_oriented, m355_frame_export_pixels_oriented) costs on this box beside the plain export of the same frame
and layout (m355_frame_export, m355_frame_export_pixels), all in one run of one process.

For a 1920x1080 8-bit 4:2:0 frame and a 7680x4320 10-bit 4:2:0 frame (noise), for planar NATIVE, semi-planar MSB16 (NV12-shaped / P010) and BGRA8:
  plain        the un-oriented call
  1, 3, 5      mirror, rotation by 180 degrees, rotation by 90 degrees clockwise (the transposing kernel)
Sixteen exports enqueued back to back and waited for with m355_frame_export_wait, host clock around the batch / 16 = the time PER EXPORT: the kernel with
its launch gap.  The C ABI has no hook for device events on the library's own streams, so this counts the launch gap AGAINST the export, as
tools/bench_ssim.py does.  Median of `--batches` batches after a warm-up batch.  bytes = source bytes read once + destination bytes written once.

What a user does without these calls is the plain export plus a second pass over the same bytes, which even at copy speed costs the plain export's time
again.  THE CONDITION: an oriented export takes less than twice its plain counterpart — the tool exits 1 if one does not.

  python tools/bench_export_oriented.py [--batches 13] [--out profiles/export_oriented_bench.txt]
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BATCH = 16
CASES = [("1080p 8-bit 4:2:0", 1920, 1080, 8), ("8K 10-bit 4:2:0", 7680, 4320, 10)]
ORIENTATIONS = (1, 3, 5)


def per_export(ctx, frame, call, batches):
    out = []
    for k in range(batches + 1):
        t0 = time.perf_counter()
        for _ in range(BATCH):
            ctx.L.check(call())
        ctx.frame_export_wait(frame)
        if k:                                       # (the first batch warms up: the code object)
            out.append(1e3 * (time.perf_counter() - t0) / BATCH)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=13)
    ap.add_argument("--out", default=None, help="write the table to this file as well")
    ap.add_argument("--size", action="append", default=None, help="WxHxBITS instead of the two frames above (repeatable)")
    args = ap.parse_args()
    cases = CASES if not args.size else [(s, *[int(v) for v in s.split("x")]) for s in args.size]

    from libde265_amd import capi
    lib = capi.Library()
    ctx = capi.Context(lib, 0)
    L = lib.lib
    lines = ["# tools/bench_export_oriented.py: per export = host clock around %d exports back to back + m355_frame_export_wait / %d, median [min..max] of %d batches;" % (
        BATCH, BATCH, args.batches),
             "# one process, nothing else in flight; ratio = oriented / plain of the same frame and layout"]
    ok = True
    for name, w, h, bd in cases:
        fh = (h + 7) & ~7                           # (1080 rows lie in a frame of 1088 and leave through a rectangle)
        rng = np.random.default_rng(w + bd)
        dt = np.uint8 if bd <= 8 else np.uint16
        planes = [rng.integers(0, 1 << bd, (ph, pw)).astype(dt) for pw, ph in ((w, fh), (w // 2, fh // 2), (w // 2, fh // 2))]
        frame = ctx.frame_create(w, fh, 1, bd, bd)
        ctx.frame_upload(frame, planes)
        ctx.wait()
        sb = 1 if bd <= 8 else 2
        src_bytes = w * h * 3 // 2 * sb
        lines.append("%s (%dx%d, %.1f MB per frame)" % (name, w, h, src_bytes / 1e6))
        kinds = [("planar NATIVE", capi.EXPORT_PLANAR, capi.EXPORT_NATIVE, sb), ("semi-planar MSB16", capi.EXPORT_SEMIPLANAR, capi.EXPORT_MSB16, 2), ("BGRA8", None, None, 4)]
        for kind, layout, samples, db in kinds:
            dst_bytes = w * h * 4 if layout is None else w * h * 3 // 2 * db
            # one destination per plane; the pitch is the row, so a plane's bytes are the same in every orientation
            semi = layout == capi.EXPORT_SEMIPLANAR
            sizes = [w * h * 4] if layout is None else [w * h * db] + [(w // 2) * (h // 2) * db * (2 if semi else 1)] * (1 if semi else 2)
            bufs = [ctx.device_alloc(n, fill=None) for n in sizes]

            def desc_for(o):
                tr = bool((o or 0) & capi.ORIENT_TRANSPOSE)
                if layout is None:
                    d = capi.PixelDesc(format=capi.PIXEL_BGRA8, alpha=255, matrix=capi.MATRIX_BT709, full_range=0)
                    d.dst, d.pitch = bufs[0], (h if tr else w) * 4
                else:
                    d = capi.ExportDesc(layout=layout, samples=samples)
                    for k, b in enumerate(bufs):
                        pw, ph = (w, h) if k == 0 else (w // 2, h // 2)
                        d.dst[k] = b
                        d.pitch[k] = (ph if tr else pw) * db * (2 if semi and k else 1)
                d.x0, d.y0, d.width, d.height = 0, 0, w, h
                return d

            def call_for(o):
                d = desc_for(o)
                if layout is None:
                    if o is None:
                        return lambda: L.m355_frame_export_pixels(ctx.h, frame, ctypes.byref(d), None)
                    return lambda: L.m355_frame_export_pixels_oriented(ctx.h, frame, ctypes.byref(d), None, o)
                if o is None:
                    return lambda: L.m355_frame_export(ctx.h, frame, ctypes.byref(d))
                return lambda: L.m355_frame_export_oriented(ctx.h, frame, ctypes.byref(d), o)

            t_plain = per_export(ctx, frame, call_for(None), args.batches)
            m_plain = statistics.median(t_plain)
            lines.append("  %-18s plain          %.4f [%.4f..%.4f] ms   %5.0f GB/s (%.1f MB read + %.1f MB written)" % (
                kind, m_plain, min(t_plain), max(t_plain), (src_bytes + dst_bytes) / (m_plain * 1e-3) / 1e9, src_bytes / 1e6, dst_bytes / 1e6))
            for o in ORIENTATIONS:
                t = per_export(ctx, frame, call_for(o), args.batches)
                m = statistics.median(t)
                held = m < 2 * m_plain
                ok = ok and held
                lines.append("  %-18s orientation %d  %.4f [%.4f..%.4f] ms   %5.0f GB/s   ratio %.2f   %s" % (
                    kind, o, m, min(t), max(t), (src_bytes + dst_bytes) / (m * 1e-3) / 1e9, m / m_plain, "below 2x" if held else "MISSES 2x"))
            for b in bufs:
                ctx.device_free(b)
        ctx.frame_destroy(frame)
    ctx.close()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
