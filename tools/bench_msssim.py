#!/usr/bin/env python3
"""What an MS-SSIM request (m355_frame_msssim_async, five levels) costs on this box, beside the SSIM request (m355_frame_ssim_async) on the same pair
of frames and beside what a caller without it has to pay first — bringing both pictures to the host —, all in one run.

For a 1920x1080 8-bit 4:2:0 frame and a 7680x4320 10-bit 4:2:0 frame (noise against a perturbed copy, both in frames of one context):
  msssim    levels = 5, all planes and luma only; and levels = 1, all planes: the first launch alone, without the pyramid's stores (the split of the
            request's time: the C ABI has no hook for device events on the library's own streams)
  ssim      m355_frame_ssim_async of the same planes
            FOUR requests (M355_MSSSIM_REQUESTS; the same batch for the SSIM rows) enqueued back to back and collected, host clock around the batch
            / 4 = the time PER REQUEST: the kernels with their launch gaps, the event record and the collection.  Median of `--batches` batches after
            a warm-up batch, which also allocates the four slots' scratch.
  download  m355_frame_download_async + wait of the three planes of the one frame into pinned planes, host clock, median of `--downloads` calls.
  bytes     the algorithmic bytes of the request: both pictures read once, a third of that written and read once more = 2 x (1 + 2/3) x the frame.

THE CONDITION: at 8K the request with all planes takes less time than TWO pinned downloads — the tool exits 1 if not.  The 1080p figures are recorded
without a condition: launch overhead dominates there.

  python tools/bench_msssim.py [--batches 50] [--downloads 15] [--out profiles/msssim_bench.txt]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BATCH = 4           # M355_MSSSIM_REQUESTS
CASES = [("1080p 8-bit 4:2:0", 1920, 1080, 8, False), ("8K 10-bit 4:2:0", 7680, 4320, 10, True)]


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
        if k:                                       # (the first batch warms up: code object, pinned records, the slots' scratch)
            out.append(1e3 * (time.perf_counter() - t0) / BATCH)
        assert all(r == results[0] for r in results)
    return out, results[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=50)
    ap.add_argument("--downloads", type=int, default=15)
    ap.add_argument("--out", default=None, help="write the table to this file as well")
    ap.add_argument("--size", action="append", default=None, help="WxHxBITS instead of the two frames above (repeatable; the condition is checked on each)")
    args = ap.parse_args()
    cases = CASES if not args.size else [(s, *[int(v) for v in s.split("x")], True) for s in args.size]

    from libde265_amd import capi
    lib = capi.Library()
    ctx = capi.Context(lib, 0)
    lines = ["# tools/bench_msssim.py: per request = host clock around %d requests back to back + collected / %d, median [min..max] of %d batches (%d requests);" % (BATCH, BATCH, args.batches, BATCH * args.batches),
             "# download = host clock, median [min..max] of %d calls; frame against frame, levels = 5, one process, nothing else in flight" % args.downloads]
    ok = True
    for name, w, h, bd, conditional in cases:
        fh = (h + 7) & ~7                           # (1080 rows lie in a frame of 1088, measured through a rectangle)
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

        def ms(levels, planes=0):
            return per_request(lambda: ctx.frame_msssim_async(fa, ref_frame=fb, rect=rect, planes=planes, levels=levels), ctx.frame_msssim_result, args.batches)

        def ss(planes=0):
            return per_request(lambda: ctx.frame_ssim_async(fa, ref_frame=fb, rect=rect, planes=planes), ctx.frame_ssim_result, args.batches)

        t_all, r_all = ms(5)
        t_luma, r_luma = ms(5, planes=1)
        t_one, r_one = ms(1)
        t_sall, s_all = ss()
        t_sluma, _ = ss(planes=1)
        assert r_all[0] == r_luma[0] and r_luma[1]["n"][0] == 0 and r_all[1]["n"][4] == ((w // 2 >> 4) - 10) * ((h // 2 >> 4) - 10)
        assert all(r_all[c]["sum_q"][0] == r_one[c]["sum_q"][0] == s_all[c]["sum_q"] for c in range(3)), "level 0 is the SSIM request's sum"

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

        m_all, m_luma, m_one, m_sall, m_sluma, m_pin = [statistics.median(v) for v in (t_all, t_luma, t_one, t_sall, t_sluma, t_pin)]
        held = m_all < 2 * m_pin
        traffic = 2 * frame_bytes * 5 / 3
        lines += ["%s (%dx%d, %.1f MB per frame; msssim of the planes %s)" % (name, w, h, frame_bytes / 1e6, ", ".join("%.6f" % r["msssim"] for r in r_all)),
                  "  msssim request, 5 levels, all planes        %s   %.0f GB/s algorithmic (%.1f MB)" % (cell(t_all), traffic / (m_all * 1e-3) / 1e9, traffic / 1e6),
                  "  msssim request, 5 levels, luma only         %s" % cell(t_luma),
                  "  msssim request, 1 level, all planes         %s   (launch 1 without the pyramid; 5 levels - 1 level = %.4f ms for the pyramid's stores and launch 2)" % (cell(t_one), m_all - m_one),
                  "  ssim request, all planes                    %s   msssim / ssim = %.2f (the work model: somewhat above 1.33)" % (cell(t_sall), m_all / m_sall),
                  "  ssim request, luma only                     %s   msssim / ssim = %.2f" % (cell(t_sluma), m_luma / m_sluma),
                  "  m355_frame_download_async + wait, pinned    %s   (the one frame; a caller without the request pays two)" % cell(t_pin)]
        if conditional:
            ok = ok and held
            lines.append("  condition: msssim all planes < two pinned downloads: %s (%.4f ms against %.4f ms, %.2f times)" % ("HOLDS" if held else "DOES NOT HOLD", m_all, 2 * m_pin, 2 * m_pin / m_all))
        else:
            lines.append("  (no condition at this size: %.4f ms against two pinned downloads %.4f ms)" % (m_all, 2 * m_pin))
    ctx.close()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
