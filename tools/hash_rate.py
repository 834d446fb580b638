#!/usr/bin/env python3
"""Pictures per second when EVERY picture is hashed, three pictures in flight: what m355_frame_hash_async is for.

A resident picture (C3: 4K 8-bit, C5: 8K 10-bit — synth.CONFIGS, the shapes of bench.py) is decoded N times at pipeline depth 3, the
decodes going round three destination frames, each decode followed by a hash of its destination:

  sync   m355_frame_hash right behind every decode: it waits for every picture in flight (the only path before the request form)
  async  m355_frame_hash_async behind every decode, collected two pictures later (blocking on that request only)
  none   no hash at all: what the decodes alone cost

for CRC, checksum and MD5.  Every (picture, hash type, arm) runs in a PROCESS OF ITS OWN (this script calls itself); the rounds go through
the arms in alternating order, so that a drift of the machine falls on all of them; a figure is the host time around `--steps` decodes that
ends in m355_wait, after `--warmup` untimed ones.  Per cell: the median over the rounds and min..max.  The async arm checks, outside the
timed window, that a request's value equals m355_frame_hash's.

  python tools/hash_rate.py [--steps 300] [--rounds 3] [--out profiles/hash_async_rate.txt]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = {"C3": "c3_4k_inter", "C5": "c5_8k10_8tiles"}
TYPES = {"crc": 1, "checksum": 2, "md5": 0}
ARMS = ("sync", "async", "none")
DEPTH = 3


def worker(args):
    from libde265_amd import capi, synth, worklist
    lib = capi.Library()
    ctx = capi.Context(lib, 0)
    cfg = dict(synth.CONFIGS[WORKLOADS[args.workload]])
    pic = synth.picture(**cfg)
    pp = pic.pp[0]
    refs = []
    for i in range(cfg["n_refs"]):
        f = ctx.frame_create_for(pp)
        ctx.frame_upload(f, synth.ref_planes(cfg["seed"] + 17 * i, int(pp["width"]), int(pp["height"]), int(pp["chroma_format_idc"]), int(pp["bit_depth_luma"])))
        refs.append(f)
    pic.ref_frames = [refs[i] if i < len(refs) else -1 for i in range(worklist.MAX_REF_FRAMES)]
    handles, dsts = [], []
    for _ in range(DEPTH):
        pic.dst_frame = ctx.frame_create_for(pp)
        dsts.append(pic.dst_frame)
        handles.append(ctx.upload(pic))
    ctx.set_pipeline_depth(DEPTH)
    t = TYPES[args.type]

    def run(n):
        pending = []
        for i in range(n):
            ctx.decode_resident(handles[i % DEPTH])
            if args.arm == "sync":
                ctx.frame_hash(dsts[i % DEPTH], t)
            elif args.arm == "async":
                pending.append(ctx.frame_hash_async(dsts[i % DEPTH], t))
                if len(pending) > 2:
                    ctx.frame_hash_result(pending.pop(0))
        for tk in pending:
            ctx.frame_hash_result(tk)
        ctx.wait()

    run(args.warmup)
    t0 = time.perf_counter()
    run(args.steps)
    dt = time.perf_counter() - t0
    if args.arm == "async":                     # same value as the synchronous call (outside the timed window)
        assert ctx.frame_hash_result(ctx.frame_hash_async(dsts[0], t)) == ctx.frame_hash(dsts[0], t)
    ctx.close()
    print(json.dumps({"workload": args.workload, "type": args.type, "arm": args.arm, "steps": args.steps, "ms_per_picture": 1e3 * dt / args.steps}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--md5-steps", type=int, default=60, help="steps of the MD5 cells (a host-bound hash: tens of milliseconds per picture)")
    ap.add_argument("--out", default=None, help="write the table to this file as well")
    ap.add_argument("--workload", choices=sorted(WORKLOADS))
    ap.add_argument("--type", choices=sorted(TYPES))
    ap.add_argument("--arm", choices=ARMS, help="run ONE cell in this process (what the driver starts)")
    args = ap.parse_args()
    if args.arm:
        return worker(args)

    ms = {}
    for rnd in range(args.rounds):
        for wl in WORKLOADS:
            for ty in TYPES:
                for arm in (ARMS if rnd % 2 == 0 else ARMS[::-1]):
                    if arm == "none" and ty != "crc":
                        continue                # (no hash: one column serves the three types)
                    steps = args.md5_steps if ty == "md5" and arm != "none" else args.steps
                    cmd = [sys.executable, os.path.abspath(__file__), "--workload", wl, "--type", ty, "--arm", arm, "--steps", str(steps), "--warmup", str(max(6, steps // 10))]
                    out = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, timeout=600).stdout.decode()
                    ms.setdefault((wl, ty, arm), []).append(json.loads(out.strip().splitlines()[-1])["ms_per_picture"])
    lines = ["# tools/hash_rate.py: ms per picture (host clock around the decodes + hashes, ending in m355_wait), depth %d, resident picture," % DEPTH,
             "# every cell a process of its own, %d rounds in alternating order: median [min..max]; steps %d (MD5 cells %d)" % (args.rounds, args.steps, args.md5_steps),
             "%-4s %-9s %-26s %-26s %-26s %s" % ("pic", "hash", "sync (m355_frame_hash)", "async (collected 2 later)", "none", "sync/async")]
    for wl in WORKLOADS:
        for ty in TYPES:
            def cell(arm):
                v = ms[(wl, "crc" if arm == "none" else ty, arm)]
                return "%.3f [%.3f..%.3f]" % (statistics.median(v), min(v), max(v))
            ratio = statistics.median(ms[(wl, ty, "sync")]) / statistics.median(ms[(wl, ty, "async")])
            lines.append("%-4s %-9s %-26s %-26s %-26s %.2fx" % (wl, ty, cell("sync"), cell("async"), cell("none"), ratio))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
