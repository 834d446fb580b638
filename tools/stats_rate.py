#!/usr/bin/env python3
"""What a statistics request (m355_frame_stats_async) costs on this box, beside the existing calls that read the same frame, from the same run.

  One process, one context, an 8K 10-bit 4:2:0 frame (7680x4320, 99.5 MB) holding (a) seeded random samples, (b) one constant per plane, (c) a
  smooth gradient; each measured with planes only and with light = 1 (BT.2020, limited range, chroma sample location type 2).
  Per figure: sixteen requests enqueued back to back on one stream and collected, host clock around the batch / 16 = the time PER REQUEST — the
  kernel with its launch gap, the event records and the collection; not the kernel's time alone, which only a trace gives.  Median and min..max
  over `--batches` batches behind one warm-up batch.
  Beside them, timed the same way: m355_frame_measure_async of the random frame against the gradient frame (it reads both: twice the bytes),
  m355_frame_export_rgb of the random frame as packed U16 with the same conversion and siting (the light pass's reads and arithmetic plus 6 bytes
  per pixel of stores), and m355_measure_copy_rate.
  The yardsticks are those calls, never the new code against itself: planes only <= the comparison; light <= the export; the constant frame within
  the min..max the random frame shows.

  python tools/stats_rate.py [--batches 9] [--out profiles/stats_rate.txt]
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

W, H, BD = 7680, 4320, 10
BATCH = 16          # M355_STATS_REQUESTS = M355_MEASURE_REQUESTS


def contents():
    rng = np.random.default_rng(8010)
    shapes = [(H, W), (H // 2, W // 2), (H // 2, W // 2)]
    yield "random", [rng.integers(0, 1 << BD, s, dtype=np.uint16) for s in shapes]
    yield "constant", [np.full(s, v, np.uint16) for s, v in zip(shapes, (64, 512, 512))]
    yield "gradient", [((np.arange(s[1], dtype=np.int64)[None, :] * 700 // s[1]) + (np.arange(s[0], dtype=np.int64)[:, None] * 300 // s[0]) + 16).astype(np.uint16)
                       for s in shapes]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=9)
    ap.add_argument("--out", default=None, help="write the table to this file as well")
    args = ap.parse_args()

    from libde265_amd import capi
    lib = capi.Library()
    assert lib.device_count() >= 1, "no HIP device visible"
    ctx = capi.Context(lib, 0)
    frames = {}
    for name, planes in contents():
        frames[name] = ctx.frame_create(W, H, 1, BD, BD)
        ctx.frame_upload(frames[name], planes)
    frame_bytes = (W * H + 2 * (W // 2) * (H // 2)) * 2
    light = dict(light=True, matrix=capi.MATRIX_BT2020, full_range=0, chroma_loc=2)

    def timed(enqueue, collect):
        """per-request seconds of `--batches` batches of BATCH requests, behind one warm-up batch"""
        out = []
        for b in range(args.batches + 1):
            t0 = time.perf_counter()
            tickets = [enqueue() for _ in range(BATCH)]
            results = collect(tickets)
            if b:
                out.append((time.perf_counter() - t0) / BATCH)
        return out, results

    rows, first = {}, {}
    for name in frames:
        for mode, kw in (("planes", {}), ("light", light)):
            f = frames[name]
            t, results = timed(lambda: ctx.frame_stats_async(f, black=64, **kw), lambda tk: [ctx.frame_stats_result(x) for x in tk])
            assert all(r == results[0] for r in results)
            rows[(name, mode)], first[(name, mode)] = t, results[0]
    assert first[("constant", "planes")]["planes"][0]["hist"][64 >> 2] == W * H and first[("constant", "planes")]["box"] is None
    assert sum(first[("random", "light")]["light"]["hist"]) == W * H

    t_measure, results = timed(lambda: ctx.frame_measure_async(frames["random"], ref_frame=frames["gradient"]), lambda tk: [ctx.frame_measure_result(x) for x in tk])
    assert results[0][0]["n_diff"] > 0

    pitch = 6 * W
    dst = ctx.device_alloc(pitch * H, fill=None)
    desc = capi.RgbDesc(layout=capi.RGB_PACKED, samples=capi.RGB_U16, matrix=capi.MATRIX_BT2020, full_range=0)
    desc.dst[0], desc.pitch[0] = dst, pitch
    opts = capi.ExportOpts(filter=0, chroma_loc=2)

    def export():
        lib.check(lib.lib.m355_frame_export_rgb_opts(ctx.h, frames["random"], ctypes.byref(desc), ctypes.byref(opts)))

    t_export, _ = timed(export, lambda tk: ctx.frame_export_wait(frames["random"]))
    copy_gbps = ctx.measure_copy_rate()
    ctx.device_free(dst)
    ctx.close()

    def cell(v):
        return "%.3f ms [%.3f..%.3f]" % (1e3 * statistics.median(v), 1e3 * min(v), 1e3 * max(v))

    med = lambda v: statistics.median(v)  # noqa: E731
    lines = ["# tools/stats_rate.py: %dx%d, %d bit, 4:2:0 (%.1f MB per frame), one process; per request = host clock around %d enqueued back to back + collected, / %d;"
             % (W, H, BD, frame_bytes / 1e6, BATCH, BATCH),
             "# median [min..max] of %d batches" % args.batches,
             "copy rate of this box (m355_measure_copy_rate, read + written)          %.0f GB/s" % copy_gbps]
    for name in frames:
        for mode in ("planes", "light"):
            t = rows[(name, mode)]
            lines.append("stats, %-8s frame, %-6s                                        %s   %.0f GB/s of frame bytes" % (name, mode, cell(t), frame_bytes / med(t) / 1e9))
    lines += ["m355_frame_measure_async, random against gradient frame (2 x the bytes)  %s" % cell(t_measure),
              "m355_frame_export_rgb_opts, random frame, packed U16, BT.2020, type 2     %s" % cell(t_export),
              "yardsticks (the existing calls of this run):"]

    def verdict(what, a, b):
        lines.append("  %-68s %s (%.3f against %.3f ms)" % (what, "met" if med(a) <= med(b) else "MISSED", 1e3 * med(a), 1e3 * med(b)))

    for name in frames:
        verdict("planes only, %s <= the comparison" % name, rows[(name, "planes")], t_measure)
        verdict("light, %s <= the R'G'B' export" % name, rows[(name, "light")], t_export)
    for mode in ("planes", "light"):
        r, c = rows[("random", mode)], rows[("constant", mode)]
        lines.append("  %-68s %s (%.3f ms against [%.3f..%.3f])" % ("constant frame, %s, within the random frame's min..max" % mode,
                                                                   "met" if med(c) <= max(r) else "MISSED", 1e3 * med(c), 1e3 * min(r), 1e3 * max(r)))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
