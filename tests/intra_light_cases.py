"""Cases and driver of the light intra path (k_intra_light.h: on inter pictures the CTBs without a cross-CTB intra dependency run as one wave per
CTB and colour component inside k_intra's launch), shared by the interpreter tier (test_emu_intra_light.py) and the GPU tier
(test_gpu_intra_light.py).  Every case is decoded with one and with three pictures in flight, different pictures following each other on a lane,
and compared bit-exactly with the oracle; the oracle's pictures are computed once per process and shared.

The pictures are the smallest that can still go wrong: one to twelve 64x64 CTBs, widths and heights that are no multiple of the CTB, so that blocks
touch all four picture borders and the unavailable-neighbour substitution is exercised on each of them."""
import ctypes

import numpy as np

from oracle_py import Oracle
from synth_util import assert_planes_equal, make_case, oracle_decode
from libde265_amd import capi, synth, worklist

IBF_PCM = 4          # m355_ib.flags (de265_mi355x.h M355_IBF_PCM)

# name -> (synthetic picture configuration, properties the lists must have: checked, not assumed)
CASES = {
    "128x128_8bit": (dict(width=128, height=128, bit_depth=8, intra_pct=14, n_refs=2, seed=4151), ()),
    # 16x16 CUs split into four 8x8 transform blocks: several dependent levels inside one wave's walk
    "128x128_10bit_split_tus": (dict(width=128, height=128, bit_depth=10, intra_pct=10, n_refs=2, seed=4139, fixed_cu_log2=4), ("split",)),
    # 32x32 CUs.  The schedule table keeps a CTB that holds a 32x32 intra block on the workgroup path (runtime_internal.h sched::intra_light_32x32): the case has
    # such CTBs beside light ones, and FORCED_32 (a process of its own, M355_INTRA_LIGHT_32=1) sends them down the light path as well
    "192x128_8bit_32x32": (dict(width=192, height=128, bit_depth=8, intra_pct=20, n_refs=2, seed=4122, fixed_cu_log2=5), ("b32",)),
    # (PCM coding units are one in ten of the intra ones: at this size only a low intra share leaves CTBs with them free of dependencies)
    "192x128_10bit_pcm": (dict(width=192, height=128, bit_depth=10, intra_pct=6, n_refs=2, seed=4129, features=synth.SYN_PCM), ("pcm",)),
    "200x136_8bit_constrained": (dict(width=200, height=136, bit_depth=8, intra_pct=10, n_refs=2, seed=4102, features=synth.SYN_CONSTRAINED_INTRA), ("borders", "mixed")),
    "200x136_10bit_tiles_slices": (dict(width=200, height=136, bit_depth=10, intra_pct=10, n_refs=2, seed=4106, tile_cols=2, tile_rows=1, n_slices=2), ("mixed",)),
    "128x128_mono": (dict(width=128, height=128, bit_depth=8, intra_pct=10, n_refs=2, seed=4104, chroma_format=4), ("mixed",)),
    # light CTBs and CTBs of dependency chains (k_intra's ticket) in the same picture
    "128x128_10bit_mixed_a": (dict(width=128, height=128, bit_depth=10, intra_pct=10, n_refs=2, seed=4142, fixed_cu_log2=4), ("mixed",)),
    "200x136_8bit_mixed_b": (dict(width=200, height=136, bit_depth=8, intra_pct=10, n_refs=2, seed=4102), ("mixed", "borders")),
    "192x128_8bit_mixed_c_32x32": (dict(width=192, height=128, bit_depth=8, intra_pct=20, n_refs=2, seed=4133, fixed_cu_log2=5), ("mixed", "b32")),
}
FORCED_32 = ["192x128_8bit_32x32", "192x128_8bit_mixed_c_32x32"]
SEED_STEP = 1000      # the pictures of a case: its configuration with seed, seed + SEED_STEP, seed + 2 * SEED_STEP

_pictures = {}        # (case, k) -> (picture, the oracle's planes); the reference frames are those of the case's first picture
_refs = {}


def intra_counts(ctx):
    """(work items, of which claimed through the ticket, of which run by a workgroup each, light items) of the decode prepared last — the library's
    internal accessor"""
    out = (ctypes.c_int * 4)()
    fn = ctx.L.lib.m355_debug_intra_counts
    fn.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
    fn.restype = None
    fn(ctx.h, out)
    return tuple(out)


def case_pictures(oracle_cdll, name):
    cfg, _ = CASES[name]
    if (name, 0) not in _pictures:
        o = Oracle(oracle_cdll)
        for k in range(3):
            pic, refs = make_case(**dict(cfg, seed=cfg["seed"] + k * SEED_STEP))
            if k == 0:
                _refs[name] = refs
            _pictures[(name, k)] = (pic, oracle_decode(o, pic, _refs[name]))
    return [_pictures[(name, k)] for k in range(3)], _refs[name]


def check_properties(name, pic):
    """what the case is there for must be IN its lists"""
    _, props = CASES[name]
    ibs, pp = pic.ibs, pic.pp[0]
    luma = ibs[ibs["cidx"] == 0]
    n = 1 << luma["log2_size"].astype(np.int64)
    if "b32" in props:
        assert np.any((ibs["log2_size"] == 5) & ((ibs["flags"] & IBF_PCM) == 0)), "no 32x32 intra block"
    if "pcm" in props:
        assert np.any((ibs["flags"] & IBF_PCM) != 0), "no PCM block"
    if "split" in props:      # (the case's CUs are 16x16)
        assert np.any(luma["log2_size"] == 3), "no CU split into four transform blocks"
    if "borders" in props:
        assert np.any(luma["x"] == 0) and np.any(luma["y"] == 0), "no intra block on the left / top border"
        assert np.any(luma["x"] + n == int(pp["width"])) and np.any(luma["y"] + n == int(pp["height"])), "no intra block on the right / bottom border"


def run_case(lib, oracle_cdll, name, depth, forced_32=False):
    """depth 1: the case's pictures one after the other; depth 3: six decodes in flight three at a time, so that every lane decodes two DIFFERENT
    pictures in a row.  forced_32: the process runs with M355_INTRA_LIGHT_32=1.  Returns the (work, ticket, workgroup, light) counts of the decodes."""
    pics, refs = case_pictures(oracle_cdll, name)
    _, props = CASES[name]
    check_properties(name, pics[0][0])
    order = [0, 1, 2] if depth == 1 else [0, 1, 2, 1, 2, 0]
    ctx = capi.Context(lib, 0)
    try:
        ctx.set_pipeline_depth(depth)
        pp = pics[0][0].pp[0]
        handles = []
        for planes in refs:
            f = ctx.frame_create_for(pp)
            ctx.frame_upload(f, planes)
            handles.append(f)
        dsts, counts = [], []
        for k in order:
            pic = pics[k][0]
            dst = ctx.frame_create_for(pp)
            pic.dst_frame = dst
            pic.ref_frames = [handles[i] if i < len(handles) else -1 for i in range(worklist.MAX_REF_FRAMES)]
            ctx.submit(pic)
            counts.append(intra_counts(ctx))
            dsts.append(dst)
            if depth == 1:
                ctx.wait()
        ctx.wait()
        for i, k in enumerate(order):
            assert_planes_equal(ctx.frame_download(dsts[i]), pics[k][1], "%s, %d in flight, decode %d (picture %d)" % (name, depth, i, k))
    finally:
        ctx.close()
    # the path taken: every picture has light items, a mixed case's first picture also CTBs of a dependency chain
    for i, (work, ticket, wg, light) in enumerate(counts):
        assert light >= 1, "%s decode %d: no light item (work %d, ticket %d)" % (name, i, work, ticket)
        assert ticket <= wg < work
        if forced_32:
            assert wg == ticket, "%s decode %d: a CTB without dependencies stayed a workgroup" % (name, i)
    if "mixed" in props:
        assert counts[0][1] >= 1, "%s: no CTB of a dependency chain beside the light ones" % name
    if "b32" in props and not forced_32:
        assert counts[0][2] > counts[0][1], "%s: no CTB kept as a workgroup for its 32x32 block" % name
    return counts


def run_forced_32(lib_path, oracle_path):
    """the cases with 32x32 blocks in a process that sends their CTBs down the light path (the setting the schedule table did NOT choose)"""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys, ctypes; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "from intra_light_cases import FORCED_32, run_case\n"
            "from libde265_amd import capi\n"
            "lib = capi.Library(%r); o = ctypes.CDLL(%r)\n"
            "for name in FORCED_32:\n"
            "    for depth in (1, 3):\n"
            "        run_case(lib, o, name, depth, forced_32=True)\n"
            "print('forced 32x32 ok')\n") % (here, os.path.dirname(here), lib_path, oracle_path)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, M355_INTRA_LIGHT_32="1"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "forced 32x32 ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
