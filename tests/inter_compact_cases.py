"""Cases and driver of the compact workgroups of k_inter_jobs (k_inter.hip: a workgroup takes 256 consecutive jobs of the MAIN range — the prediction
blocks of one list, of two lists and with explicit weights together, in PB order — and sorts them by kind itself; waves of one kind take the
wave-uniform path, mixed waves the per-lane one), shared by the interpreter tier (test_emu_inter_compact.py) and the GPU tier
(test_gpu_inter_compact.py).  Every case is decoded with one and with three pictures in flight, different pictures following each other on a lane,
and compared bit-exactly with the oracle; the oracle's pictures are computed once per process and shared.

Each case asserts from its own lists that it holds what it is there for: kind and job count per PB are recomputed here as the device computes them
(m355_pb_is_edge in k_common.h, d_pb_jobs in k_meta.hip, d_job_class in k_inter.hip), the MAIN list and its 256-job windows are built from them."""
import numpy as np

from oracle_py import Oracle
from synth_util import assert_planes_equal, make_case, oracle_decode
from libde265_amd import capi, worklist

BLOCK = 256           # jobs of a workgroup (M355_INTER_BLOCK)
BI, ONE, WEIGHTED, EDGE = 0, 1, 2, 3      # kinds, in the order a workgroup runs them (d_job_class); EDGE is a range of its own

# name -> (synthetic picture configuration, MAIN jobs, EDGE jobs (None: not pinned), properties the lists must have: checked, not assumed).
# The job counts are those of the device's predicate: a job is 8 rows high whatever its PB's height, so a window's vertical span is that of the
# height rounded up to 8 (counted with the PB's own height, one 8x4 PB of each of the first, second and fourth case would be MAIN instead of EDGE)
CASES = {
    # one partial workgroup holding all three kinds: MAIN is smaller than a workgroup, three waves are partly idle
    "128x96_10bit_one_partial": (dict(width=128, height=96, bit_depth=10, intra_pct=0, bipred_pct=50, weighted_pct=30, oob_mv_pct=0, n_refs=2, seed=7001),
                                 176, 236, ("partial", "all3")),
    # MAIN is under two waves
    "64x64_10bit_two_waves": (dict(width=64, height=64, bit_depth=10, intra_pct=0, bipred_pct=50, weighted_pct=30, oob_mv_pct=0, n_refs=2, seed=7005),
                              81, 71, ("under_two_waves",)),
    # four windows, three of them with all three kinds, PB sizes 4x16 .. 64x64; two PBs split between two workgroups
    "256x192_8bit_four_windows": (dict(width=256, height=192, bit_depth=8, intra_pct=5, bipred_pct=50, weighted_pct=20, oob_mv_pct=5, n_refs=2, seed=7002),
                                  800, 688, ("all3_x3", "straddle_x2", "sizes_4x16_64x64")),
    # 8x8, 8x4 and 4x8 PBs only, every window has all three kinds; the sizes are no multiple of the CTB
    "200x136_10bit_small_pbs": (dict(width=200, height=136, bit_depth=10, fixed_cu_log2=3, intra_pct=10, bipred_pct=40, weighted_pct=20, oob_mv_pct=3,
                                     n_refs=2, seed=7003), 654, 222, ("small_only", "all3_everywhere")),
    # 64x64, 64x32 and 32x64 PBs; a window of one kind (the wave-uniform paths) beside mixed windows
    "320x192_8bit_large_pbs": (dict(width=320, height=192, bit_depth=8, fixed_cu_log2=6, bipred_pct=50, weighted_pct=10, oob_mv_pct=0, n_refs=2, seed=7004),
                               576, 1344, ("large_only", "uniform_window", "mixed_window")),
    # only the two unweighted kinds, mixed; one PB split between two workgroups
    "256x192_10bit_unweighted": (dict(width=256, height=192, bit_depth=10, fixed_cu_log2=4, intra_pct=0, weighted_pct=0, bipred_pct=50, oob_mv_pct=0, n_refs=2, seed=7006),
                                 1256, 296, ("no_weighted", "mixed_window", "straddle_x1")),
    "128x96_12bit": (dict(width=128, height=96, bit_depth=12, intra_pct=0, bipred_pct=50, weighted_pct=30, oob_mv_pct=0, n_refs=2, seed=7007),
                     None, None, ("all3",)),
    "128x96_8bit_mono": (dict(width=128, height=96, bit_depth=8, intra_pct=0, bipred_pct=50, weighted_pct=30, oob_mv_pct=0, n_refs=2, seed=7008, chroma_format=4),
                         None, None, ("mono", "all3")),
    "128x96_10bit_all_weighted": (dict(width=128, height=96, bit_depth=10, intra_pct=0, bipred_pct=50, weighted_pct=100, oob_mv_pct=0, n_refs=2, seed=7009),
                                  None, None, ("all_weighted",)),
}
SEED_STEP = 1000      # the pictures of a case: its configuration with seed, seed + SEED_STEP, seed + 2 * SEED_STEP

_pictures = {}        # (case, k) -> (picture, the oracle's planes); the reference frames are those of the case's first picture
_refs = {}


def pb_is_edge(pb, width, height, cf):
    """m355_pb_is_edge (k_common.h)"""
    x, y, w, h, flags = int(pb["x"]), int(pb["y"]), int(pb["w"]), int(pb["h"]), int(pb["flags"])
    h8 = (h + 7) & ~7
    for l in range(2):
        if not flags & (worklist.PBF_MC_L0 << l) or flags & (worklist.PBF_FILL_L0 << l):
            continue
        mvx, mvy = int(pb["mv"][l][0]), int(pb["mv"][l][1])
        xl, yl = x + (mvx >> 2), y + (mvy >> 2)
        if xl - 3 < 0 or xl + w + 3 > width - 1 or yl - 3 < 0 or yl + h8 + 3 > height - 1:
            return True
        if cf == 1:
            xc, yc = (x >> 1) + (mvx >> 3), (y >> 1) + (mvy >> 3)
            if xc - 1 < 0 or xc + (w >> 1) + 1 > (width >> 1) - 1 or yc - 1 < 0 or yc + (h8 >> 1) + 1 > (height >> 1) - 1:
                return True
    return False


def pb_kind(pb, width, height, cf):
    if pb_is_edge(pb, width, height, cf):
        return EDGE
    flags = int(pb["flags"])
    if flags & worklist.PBF_WEIGHTED:
        return WEIGHTED
    return BI if (flags & worklist.PBF_MC_L0) and (flags & worklist.PBF_MC_L1) else ONE


def pb_jobs(pb):
    """d_pb_jobs (k_meta.hip): jobs of 4 columns x 8 rows"""
    return (int(pb["w"]) >> 2) * ((int(pb["h"]) + 7) >> 3)


def job_lists(pic):
    """(kind of every MAIN job in list order, PB of every MAIN job, number of EDGE jobs)"""
    pp = pic.pp[0]
    width, height, cf = int(pp["width"]), int(pp["height"]), int(pp["chroma_format_idc"])
    kinds, owners, n_edge = [], [], 0
    for i, pb in enumerate(pic.pbs):
        k, n = pb_kind(pb, width, height, cf), pb_jobs(pb)
        if k == EDGE:
            n_edge += n
        else:
            kinds += [k] * n
            owners += [i] * n
    return np.array(kinds, np.int64), np.array(owners, np.int64), n_edge


def check_properties(name, pic):
    """what the case is there for must be IN its lists"""
    _, want_main, want_edge, props = CASES[name]
    kinds, owners, n_edge = job_lists(pic)
    n_main = len(kinds)
    if want_main is not None:
        assert (n_main, n_edge) == (want_main, want_edge), "%s: %d MAIN and %d EDGE jobs" % (name, n_main, n_edge)
    windows = [set(kinds[o:o + BLOCK].tolist()) for o in range(0, n_main, BLOCK)]
    all3 = sum(w == {BI, ONE, WEIGHTED} for w in windows)
    straddle = len({int(owners[o]) for o in range(BLOCK, n_main, BLOCK) if owners[o] == owners[o - 1]})
    sizes = {(int(pb["w"]), int(pb["h"])) for pb in pic.pbs}
    for prop in props:
        if prop == "partial":
            assert 3 * 64 > n_main > 64 and len(windows) == 1
        elif prop == "under_two_waves":
            assert 64 < n_main < 128
        elif prop == "all3":
            assert all3 >= 1
        elif prop == "all3_x3":
            assert len(windows) == 4 and all3 == 3
        elif prop == "all3_everywhere":
            assert len(windows) >= 2 and all3 == len(windows)
        elif prop == "straddle_x2":
            assert straddle == 2
        elif prop == "straddle_x1":
            assert straddle == 1
        elif prop == "sizes_4x16_64x64":
            assert (4, 16) in sizes and (64, 64) in sizes
        elif prop == "small_only":
            assert sizes == {(8, 8), (8, 4), (4, 8)}, sizes
        elif prop == "large_only":
            assert sizes == {(64, 64), (64, 32), (32, 64)}, sizes
        elif prop == "uniform_window":
            assert any(len(w) == 1 for w in windows)
        elif prop == "mixed_window":
            assert any(len(w) >= 2 for w in windows)
        elif prop == "no_weighted":
            assert WEIGHTED not in set(kinds.tolist()) and {BI, ONE} in windows
        elif prop == "mono":
            assert int(pic.pp[0]["chroma_format_idc"]) == 0
        elif prop == "all_weighted":
            assert n_main > 64 and set(kinds.tolist()) == {WEIGHTED}
        else:
            raise AssertionError("unknown property " + prop)


def case_pictures(oracle_cdll, name):
    cfg = CASES[name][0]
    if (name, 0) not in _pictures:
        o = Oracle(oracle_cdll)
        for k in range(3):
            pic, refs = make_case(**dict(cfg, seed=cfg["seed"] + k * SEED_STEP))
            if k == 0:
                _refs[name] = refs
            _pictures[(name, k)] = (pic, oracle_decode(o, pic, _refs[name]))
    return [_pictures[(name, k)] for k in range(3)], _refs[name]


def run_case(lib, oracle_cdll, name, depth):
    """depth 1: the case's pictures one after the other; depth 3: six decodes in flight three at a time, so that every lane decodes two DIFFERENT
    pictures in a row."""
    pics, refs = case_pictures(oracle_cdll, name)
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
        dsts = []
        for k in order:
            pic = pics[k][0]
            dst = ctx.frame_create_for(pp)
            pic.dst_frame = dst
            pic.ref_frames = [handles[i] if i < len(handles) else -1 for i in range(worklist.MAX_REF_FRAMES)]
            ctx.submit(pic)
            dsts.append(dst)
            if depth == 1:
                ctx.wait()
        ctx.wait()
        for i, k in enumerate(order):
            assert_planes_equal(ctx.frame_download(dsts[i]), pics[k][1], "%s, %d in flight, decode %d (picture %d)" % (name, depth, i, k))
    finally:
        ctx.close()
