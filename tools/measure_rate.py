#!/usr/bin/env python3
"""What a frame-against-frame comparison (m355_frame_measure_async) costs on this box, beside the box's own copy rate from the same run.

  request  a C5-size (8K 10-bit 4:2:0) frame against a second frame: sixteen requests enqueued back to back on one stream and collected,
           host clock around the batch / 16 = the time PER REQUEST — the kernel with its launch gap, the event records and the host's row
           sums at collection; not the kernel's time alone, which only a trace gives.  The median over `--batches` batches.
           The kernel reads both frames once (2 x 99.5 MB) and writes 8 bytes per row (69 KB):
           bytes / time is set beside m355_measure_copy_rate (read + written bytes / time of a float4 copy), the ceiling of this box.
  stream   a resident C5 picture decoded `--steps` times at pipeline depth 3, the decodes going round three destination frames:
           with every picture compared against a fixed frame behind its decode (collected two pictures later, blocking on that request
           only) and with no comparison; rounds alternate between the two, per arm the median and min..max of the rounds.

  python tools/measure_rate.py [--steps 200] [--rounds 3] [--out profiles/measure_rate.txt]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOAD = "c5_8k10_8tiles"
DEPTH = 3
BATCH = 16          # M355_MEASURE_REQUESTS


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batches", type=int, default=9)
    ap.add_argument("--out", default=None, help="write the table to this file as well")
    args = ap.parse_args()

    from libde265_amd import capi, synth, worklist
    lib = capi.Library()
    ctx = capi.Context(lib, 0)
    cfg = dict(synth.CONFIGS[WORKLOAD])
    pic = synth.picture(**cfg)
    pp = pic.pp[0]
    w, h, cf, bd = int(pp["width"]), int(pp["height"]), int(pp["chroma_format_idc"]), int(pp["bit_depth_luma"])
    refs = []
    for i in range(cfg["n_refs"]):
        f = ctx.frame_create_for(pp)
        ctx.frame_upload(f, synth.ref_planes(cfg["seed"] + 17 * i, w, h, cf, bd))
        refs.append(f)
    pic.ref_frames = [refs[i] if i < len(refs) else -1 for i in range(worklist.MAX_REF_FRAMES)]
    handles, dsts = [], []
    for _ in range(DEPTH):
        pic.dst_frame = ctx.frame_create_for(pp)
        dsts.append(pic.dst_frame)
        handles.append(ctx.upload(pic))
    ctx.set_pipeline_depth(DEPTH)
    dims = worklist.plane_dims(w, h, cf)
    frame_bytes = sum(pw * ph for pw, ph in dims) * (1 if bd <= 8 else 2)
    moved = 2 * frame_bytes + 8 * sum(ph for pw, ph in dims if pw)

    copy_gbps = ctx.measure_copy_rate()

    # ---- per request: a decoded frame against a reference frame of the picture, requests back to back
    ctx.decode_resident(handles[0])
    ctx.wait()
    per_request = []
    for b in range(args.batches + 1):
        t0 = time.perf_counter()
        tickets = [ctx.frame_measure_async(dsts[0], ref_frame=refs[0]) for _ in range(BATCH)]
        results = [ctx.frame_measure_result(tk) for tk in tickets]
        if b:                                       # (the first batch warms up: code object, pinned row arrays)
            per_request.append((time.perf_counter() - t0) / BATCH)
    assert all(r == results[0] for r in results) and results[0][0]["n_diff"] > 0
    request_ms = 1e3 * statistics.median(per_request)
    request_gbps = moved / (request_ms * 1e-3) / 1e9

    # ---- stream: every picture compared, three in flight
    def run(n, measured):
        pending = []
        for i in range(n):
            ctx.decode_resident(handles[i % DEPTH])
            if measured:
                pending.append(ctx.frame_measure_async(dsts[i % DEPTH], ref_frame=refs[0]))
                if len(pending) > 2:
                    ctx.frame_measure_result(pending.pop(0))
        for tk in pending:
            ctx.frame_measure_result(tk)
        ctx.wait()

    ms = {True: [], False: []}
    for rnd in range(args.rounds):
        for measured in ((True, False) if rnd % 2 == 0 else (False, True)):
            run(args.warmup, measured)
            t0 = time.perf_counter()
            run(args.steps, measured)
            ms[measured].append(1e3 * (time.perf_counter() - t0) / args.steps)
    ctx.close()

    def cell(v):
        return "%.3f [%.3f..%.3f] ms = %.0f pictures/s" % (statistics.median(v), min(v), max(v), 1e3 / statistics.median(v))

    lines = ["# tools/measure_rate.py: %s (%dx%d, %d bit, %.1f MB per frame), frame against frame, one process" % (WORKLOAD, w, h, bd, frame_bytes / 1e6),
             "copy rate of this box (m355_measure_copy_rate, read + written)   %.0f GB/s" % copy_gbps,
             "per request: %d enqueued back to back + collected, host clock / %d, median of %d batches   %.3f ms [%.3f..%.3f]" % (BATCH, BATCH, args.batches, request_ms, 1e3 * min(per_request), 1e3 * max(per_request)),
             "        %.1f MB read + written per request                       %.0f GB/s = %.2f of the copy rate" % (moved / 1e6, request_gbps, request_gbps / copy_gbps),
             "stream, depth %d, %d steps, %d rounds alternating: median [min..max]" % (DEPTH, args.steps, args.rounds),
             "        every picture compared (collected 2 later)               %s" % cell(ms[True]),
             "        no comparison                                            %s" % cell(ms[False])]
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
