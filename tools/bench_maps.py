#!/usr/bin/env python3
"""What a side-map request (m355_picture_maps_async) costs on this box, beside a device-to-device copy of the bytes it writes and beside the decode
it rides along with — all in one run, for the synthetic pictures c5_8k10_8tiles and c3_4k_inter (libde265_amd/synth.py) at 4x4 units.

  request   all seven maps, and MAP_MV + MAP_REF only: `--requests` (64) requests enqueued back to back into destinations allocated once, with up
            to sixteen (M355_MAPS_REQUESTS) outstanding — when every slot is taken the OLDEST ticket is collected, so the stream always has fifteen
            requests queued behind the one that runs and the host's collections hide behind the device's work —, then the rest is collected; host
            clock around the whole run, which ends in the last request's completion, / 64 = the time PER REQUEST: zero fill, both kernels and the
            gaps between three launches.  The requests run on a stream of the library's own, which the C ABI does not hand out, so there is no place
            for a pair of device events around them; a host clock around work that ends in a device synchronisation is the other form
            the measuring guide allows.  Median of `--batches` runs behind a warm-up run: 832 requests per figure.
  rate      the bytes the request WRITES into the caller's memory over that time, beside m355_measure_copy_rate for a copy of the same byte count
            (which reports read + written bytes: a copy that writes N bytes moves 2 N).  ratio = request time / time of that copy.
  decode    m355_decode_resident of the picture round three handles and three frames at depth 3, host clock around `--decodes` decodes ending in
            m355_wait, without and with an all-maps request behind every decode (collected eight decodes later), alternating, median of 5 rounds.

  python tools/bench_maps.py [--batches 13] [--decodes 60] [--configs c5_8k10_8tiles,c3_4k_inter] [--out profiles/side_maps_bench.txt]
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SLOTS = 16          # M355_MAPS_REQUESTS
LOG2_UNIT = 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=13)
    ap.add_argument("--requests", type=int, default=64, help="requests back to back per timed run")
    ap.add_argument("--decodes", type=int, default=60)
    ap.add_argument("--configs", default="c5_8k10_8tiles,c3_4k_inter")
    ap.add_argument("--out", default=None, help="write the table to this file as well")
    args = ap.parse_args()

    from libde265_amd import capi, synth, worklist
    lib = capi.Library()
    L = lib.lib
    ctx = capi.Context(lib, 0)
    lines = ["# tools/bench_maps.py: per request = host clock around %d requests back to back (up to %d outstanding, the oldest collected first) / %d, median [min..max] of %d runs (%d requests);" % (
                 args.requests, SLOTS, args.requests, args.batches, args.requests * args.batches),
             "# units of 4x4 samples; one process, nothing else in flight but what the line says"]

    def cell(v, unit="ms"):
        return "%.4f [%.4f..%.4f] %s" % (statistics.median(v), min(v), max(v), unit)

    for name in args.configs.split(","):
        cfg = synth.CONFIGS[name]
        pic = synth.picture(**cfg)
        pp = pic.pp[0]
        w, h = int(pp["width"]), int(pp["height"])
        uw, uh = (w + 3) >> 2, (h + 3) >> 2
        refs = [synth.ref_planes(cfg["seed"] + 17 * i, w, h, int(pp["chroma_format_idc"]), int(pp["bit_depth_luma"]), int(pp["bit_depth_chroma"]))
                for i in range(cfg["n_refs"])]
        rf = []
        for planes in refs:
            rf.append(ctx.frame_create_for(pp))
            ctx.frame_upload(rf[-1], planes)
        pic.ref_frames = [rf[i] if i < len(rf) else -1 for i in range(worklist.MAX_REF_FRAMES)]
        dsts = [ctx.frame_create_for(pp) for _ in range(3)]
        handles = []
        for d in dsts:
            pic.dst_frame = d
            handles.append(ctx.upload(pic))
        ctx.set_pipeline_depth(3)
        bufs = [ctx.device_alloc(uw * uh * capi.MAP_ELEM_BYTES[m], fill=None) for m in range(capi.N_MAPS)]

        def desc_for(maps):
            d = capi.MapsDesc(log2_unit=LOG2_UNIT)
            for m in maps:
                d.dst[m] = bufs[m]; d.pitch[m] = uw * capi.MAP_ELEM_BYTES[m]
            return d

        tk, info = ctypes.c_ulonglong(0), capi.MapsInfo()

        def enqueue(d, handle):
            lib.check(L.m355_picture_maps_async(ctx.h, handle, ctypes.byref(d), ctypes.byref(tk)))
            return tk.value

        def collect(t):
            lib.check(L.m355_picture_maps_result(ctx.h, t, 1, ctypes.byref(info)))

        def per_request(maps):
            d, out = desc_for(maps), []
            for k in range(args.batches + 1):
                pending = []
                t0 = time.perf_counter()
                for _ in range(args.requests):
                    if len(pending) == SLOTS:
                        collect(pending.pop(0))
                    pending.append(enqueue(d, handles[0]))
                for t in pending:
                    collect(t)
                if k:                                   # (the first run warms up: code objects, the scratch allocation)
                    out.append(1e3 * (time.perf_counter() - t0) / args.requests)
            return out

        lines.append("%s (%dx%d: %d x %d units; %d CUs, %d TUs, %d PBs, %d intra blocks)" % (name, w, h, uw, uh, len(pic.cus), len(pic.tus), len(pic.pbs), len(pic.ibs)))
        for what, maps in (("all seven maps", tuple(range(capi.N_MAPS))), ("MAP_MV + MAP_REF", (capi.MAP_MV, capi.MAP_REF))):
            t = per_request(maps)
            out_bytes = uw * uh * sum(capi.MAP_ELEM_BYTES[m] for m in maps)
            copy_gbs = ctx.measure_copy_rate(max(out_bytes, 1 << 20), 9)   # read + written bytes / time (the call takes 1 MiB at least)
            copy_ms = 2 * out_bytes / (copy_gbs * 1e9) * 1e3
            med = statistics.median(t)
            assert capi.MAP_CU not in maps or info.covered == uw * uh, "the synthetic picture's coding units cover it"
            lines += ["  request, %-18s %s   writes %.1f MB: %.0f GB/s written" % (what + ":", cell(t), out_bytes / 1e6, out_bytes / (med * 1e-3) / 1e9),
                      "    a device copy of %.1f MB: %.4f ms (m355_measure_copy_rate %.0f GB/s read + written); request / copy = %.1f" % (
                          out_bytes / 1e6, copy_ms, copy_gbs, med / copy_ms)]

        d_all = desc_for(tuple(range(capi.N_MAPS)))

        def decode_round(with_maps):
            pending = []
            t0 = time.perf_counter()
            for k in range(args.decodes):
                ctx.decode_resident(handles[k % 3])
                if with_maps:
                    pending.append(enqueue(d_all, handles[k % 3]))
                    if len(pending) > 8:
                        collect(pending.pop(0))
            for t in pending:
                collect(t)
            ctx.wait()
            return 1e3 * (time.perf_counter() - t0) / args.decodes

        decode_round(False); decode_round(True)                     # warm-up
        plain, mapped = [], []
        for _ in range(5):
            plain.append(decode_round(False))
            mapped.append(decode_round(True))
        lines += ["  m355_decode_resident, depth 3, per picture: %s   with an all-maps request behind every picture: %s   (+%.4f ms)" % (
            cell(plain), cell(mapped), statistics.median(mapped) - statistics.median(plain))]
        for b in bufs:
            ctx.device_free(b)
        for hd in handles:
            ctx.release(hd)
        for f in dsts + rf:
            ctx.frame_destroy(f)
        ctx.set_pipeline_depth(1)
    ctx.close()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
