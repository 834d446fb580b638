#!/usr/bin/env python3
"""What an SSIM request (m355_frame_ssim_async) costs on this box, beside the path it replaces — getting the frame to the host — and beside the
comparison request (m355_frame_measure_async) on the same pair of frames, all in one run.

For a 1920x1080 8-bit 4:2:0 frame and a 7680x4320 10-bit 4:2:0 frame (noise against a perturbed copy, both in frames of one context):
  ssim      all planes, and luma only        measure   m355_frame_measure_async on the same pair
            sixteen requests (M355_*_REQUESTS) enqueued back to back behind one another and collected, host clock around the batch / 16 = the
            time PER REQUEST: the kernel with its launch gap, the event record and the collection.  The C ABI has no hook for device events on
            the library's own streams, so this is what tools/measure_rate.py measures too; it counts the launch gap AGAINST the request.
            Median of `--batches` batches after a warm-up batch: at least 200 requests per figure.
  download  m355_frame_download of the three planes of the one frame into touched host arrays, host clock, median of `--downloads` calls;
            and m355_frame_download_async + wait into pinned planes, the fastest way to the host this library has.
  bytes     the algorithmic bytes of the SSIM kernel: every sample of both pictures read once, nothing written = 2 x the frame's bytes, over the
            request's time.

THE CONDITION: the SSIM request with all planes takes less time than m355_frame_download of that one frame, at both sizes — the tool exits 1 if not.

  python tools/bench_ssim.py [--batches 13] [--downloads 15] [--out profiles/ssim_bench.txt]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BATCH = 16          # M355_SSIM_REQUESTS = M355_MEASURE_REQUESTS
CASES = [("1080p 8-bit 4:2:0", 1920, 1080, 8), ("8K 10-bit 4:2:0", 7680, 4320, 10)]


def planes_for(w, h, bd, seed):
    rng = np.random.default_rng(seed)
    dt = np.uint8 if bd <= 8 else np.uint16
    peak = (1 << bd) - 1
    a = [rng.integers(0, peak + 1, (ph, pw), dtype=np.int64) for pw, ph in ((w, h), (w // 2, h // 2), (w // 2, h // 2))]
    b = [np.clip(p + rng.integers(-(peak // 16), peak // 16 + 1, p.shape), 0, peak) for p in a]
    return [p.astype(dt) for p in a], [p.astype(dt) for p in b]


def per_request(enqueue, collect, batches):
    out = []
    for k in range(batches + 1):
        t0 = time.perf_counter()
        tickets = [enqueue() for _ in range(BATCH)]
        results = [collect(tk) for tk in tickets]
        if k:                                       # (the first batch warms up: code object, pinned records)
            out.append(1e3 * (time.perf_counter() - t0) / BATCH)
        assert all(r == results[0] for r in results)
    return out, results[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=13)
    ap.add_argument("--downloads", type=int, default=15)
    ap.add_argument("--out", default=None, help="write the table to this file as well")
    ap.add_argument("--size", action="append", default=None, help="WxHxBITS instead of the two frames above (repeatable; the condition is still checked)")
    args = ap.parse_args()
    cases = CASES if not args.size else [(s, *[int(v) for v in s.split("x")]) for s in args.size]

    from libde265_amd import capi
    lib = capi.Library()
    ctx = capi.Context(lib, 0)
    lines = ["# tools/bench_ssim.py: per request = host clock around %d requests back to back + collected / %d, median [min..max] of %d batches (%d requests);" % (BATCH, BATCH, args.batches, BATCH * args.batches),
             "# download = host clock, median [min..max] of %d calls; frame against frame, one process, nothing else in flight" % args.downloads]
    ok = True
    for name, w, h, bd in cases:
        # (the frame's height is a multiple of 8: 1080 rows lie in a frame of 1088, measured and downloaded through a rectangle / as a whole)
        fh = (h + 7) & ~7
        a, b = planes_for(w, fh, bd, seed=w + bd)
        geom = (w, fh, 1, bd, bd)
        fa, fb = ctx.frame_create(*geom), ctx.frame_create(*geom)
        ctx.frame_upload(fa, a)
        ctx.frame_upload(fb, b)
        ctx.wait()
        rect = (0, 0, w, h)
        frame_bytes = (w * h * 3 // 2) * (1 if bd <= 8 else 2)

        def cell(v):
            return "%.4f [%.4f..%.4f] ms" % (statistics.median(v), min(v), max(v))

        t_all, r_all = per_request(lambda: ctx.frame_ssim_async(fa, ref_frame=fb, rect=rect), ctx.frame_ssim_result, args.batches)
        t_luma, r_luma = per_request(lambda: ctx.frame_ssim_async(fa, ref_frame=fb, rect=rect, planes=1), ctx.frame_ssim_result, args.batches)
        t_meas, _ = per_request(lambda: ctx.frame_measure_async(fa, ref_frame=fb, rect=rect), ctx.frame_measure_result, args.batches)
        assert r_all[0] == r_luma[0] and r_luma[1]["n"] == 0 and r_all[1]["n"] == (w // 2 - 10) * (h // 2 - 10)

        dst = [np.ones_like(p) for p in a]
        t_down = []
        for k in range(args.downloads + 1):
            t0 = time.perf_counter()
            for c in range(3):
                lib.check(lib.lib.m355_frame_download(ctx.h, fa, c, dst[c].ctypes.data, dst[c].shape[1]))
            if k:
                t_down.append(1e3 * (time.perf_counter() - t0))
        assert all((d == p).all() for d, p in zip(dst, a))
        pinned = ctx.pinned_planes(fa)
        t_pin = []
        for k in range(args.downloads + 1):
            t0 = time.perf_counter()
            ctx.frame_download_start(fa, pinned)
            ctx.frame_download_wait(fa)
            if k:
                t_pin.append(1e3 * (time.perf_counter() - t0))
        ctx.pinned_free(pinned)
        ctx.frame_destroy(fa)
        ctx.frame_destroy(fb)

        m_all, m_luma, m_meas, m_down, m_pin = [statistics.median(v) for v in (t_all, t_luma, t_meas, t_down, t_pin)]
        held = m_all < m_down
        ok = ok and held
        lines += ["%s (%dx%d, %.1f MB per frame; ssim of the planes %s)" % (name, w, h, frame_bytes / 1e6, ", ".join("%.6f" % r["ssim"] for r in r_all)),
                  "  ssim request, all planes                    %s   %.0f GB/s algorithmic (2 x %.1f MB read)" % (cell(t_all), 2 * frame_bytes / (m_all * 1e-3) / 1e9, frame_bytes / 1e6),
                  "  ssim request, luma only                     %s" % cell(t_luma),
                  "  measure request (SSD / SAD / MSE)           %s   ssim all planes / measure = %.1f" % (cell(t_meas), m_all / m_meas),
                  "  m355_frame_download, the one frame          %s   (frame of %d rows)" % (cell(t_down), fh),
                  "  m355_frame_download_async + wait, pinned    %s" % cell(t_pin),
                  "  condition: ssim all planes < m355_frame_download: %s (%.4f ms against %.4f ms, %.1f times; against the pinned download %.1f times)" % (
                      "HOLDS" if held else "DOES NOT HOLD", m_all, m_down, m_down / m_all, m_pin / m_all)]
    ctx.close()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
