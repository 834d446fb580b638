"""Strong intra smoothing (d_intra_big_filter of k_intra_block.h, shared by k_intra.hip and k_intra_light.h; intrapred.h:216-234) on borders with a
SLOPE.  The bilinear interpolation B(0) + ((i * (B(+-64) - B(0)) + 32) >> 6) replaces the [1 2 1] filter of a 32x32 luma block when both borders
pass a flatness test.  On the generator's own pictures the test passes on flat borders almost only, |B(+-64) - B(0)| below the threshold 1 << (bd - 5):
there the interpolation moves a sample by less than the threshold, and swapped ends, a wrong weight or a wrong rounding change little or nothing.

The cases: CUs of 32x32 in CTBs of 32 and of 64, a third of them intra, few residuals, every motion vector zero, the references a ramp along
one axis (residual_content.axis_ramp_refs: along x for a sloped border above, along y for one to the left), levels attenuated.  A border gathered
from such a prediction is a straight line with a few steps from residuals: it passes the flatness test WITH a slope, fails it narrowly, or passes
on one side only.

Every depth asserts FROM THE ORACLE'S PLANES ALONE (residual_content.strong_census), summed over its cases:
  >= 4 strong blocks with |B(64) - B(0)| >= threshold;  >= 2 with |B(-64) - B(0)| >= threshold;  >= 4 blocks that pass one test only;
  >= 2 that fail with both sums below twice the threshold;  >= 4 filtered 32x32 luma blocks that take [1 2 1]
and the census itself is checked against the oracle first: decoded with PF_STRONG_INTRA_SMOOTHING cleared, the picture changes in blocks the
census calls strong and in blocks that predict from those, nowhere else, and never in chroma (check_strong_against_oracle) — the 4:4:4 case
has filtered 32x32 chroma blocks, which keep [1 2 1].

Both executors: the schedule keeps a CTB with a 32x32 intra block on k_intra's workgroup path (no light item in such a picture: asserted for the
"planner" cases), so the "light" cases — inter pictures with an intra share low enough to leave CTBs without an intra neighbour — also run in a
process with M355_INTRA_LIGHT_32=1, where every dependency-free CTB is a light item of k_intra_light.h; the lists must hold sloped strong
blocks in such CTBs.

Census of the seeds in this file — candidates (filtered 32x32 luma blocks), strong, sloped above / left, one test only, near misses, [1 2 1];
with the flag cleared the oracle changes n blocks, m of them strong, and leaves k strong blocks as they were (both filters give the same border):
  8bit_x_ctb32         11  5  4 / 0   6  2   6   2, 1, 4        10bit_x_ctb32        11  5  4 / 0   6  2   6   2, 1, 4
  8bit_x_ctb32_light   16 11 11 / 0   3  1   5   5, 5, 6        10bit_x_ctb32_light  16 11 11 / 0   3  2   5   5, 5, 6
  8bit_x_ctb64         12  5  4 / 0   3  2   7   1, 1, 4        10bit_x_ctb64        12  5  4 / 0   3  2   7   2, 2, 3
  8bit_y_ctb64         11  3  0 / 2   4  2   8   5, 3, 0        10bit_y_ctb64        14  4  0 / 2   7  2  10   3, 1, 3
  12bit_x_ctb32        11  5  4 / 0   6  3   6   2, 1, 4        10bit_444_y_ctb64    13  2  0 / 2   7  3  11   4, 1, 1
  12bit_x_ctb64        12  5  4 / 0   3  2   7   3, 3, 2        12bit_y_ctb64        11  4  0 / 2   4  2   7   3, 3, 1
(a border that is an exact ramp is a fixed point of both filters up to rounding: many strong blocks do not change when the flag is cleared —
the kernels are compared with the oracle on all of them all the same.)  On the generator's own content (120 pictures of 256x192 at 8 / 10 / 12
bits with 32x32 CUs, 35 % intra, its noise references and its levels) 117 of 1182 candidates take the strong filter and 11 / 4 of them have a
slope above / to the left: one sloped block in eight pictures.

CPU tier: oracle == the reference's scalar and SSE functions (oracle/_ref replay) == the kernels under the SIMT interpreter, pipeline depths 1 and 3.
GPU tier: the HIP kernels == oracle at depths 1 and 3."""
import os
import subprocess
import sys

import numpy as np
import pytest

from intra_light_cases import intra_counts
from oracle_py import Oracle
from residual_content import SHIFT, attenuate_levels, axis_ramp_refs, check_strong_against_oracle, free_ctbs, strong_census
from synth_util import assert_planes_equal, device_decode, make_case, oracle_decode
from test_emu_picture import EMU_SO, emu_lib  # noqa: F401  (fixture)
from libde265_amd import capi, worklist as W

ST_INTRA = W.STAGE_INTER | W.STAGE_RESIDUAL | W.STAGE_INTRA
HERE = os.path.dirname(os.path.abspath(__file__))
BASE = dict(width=256, height=192, fixed_cu_log2=5, intra_pct=35, cbf_pct=10, weighted_pct=0, oob_mv_pct=0)
LIGHT = dict(BASE, width=512, height=384, log2_ctb=5, intra_pct=12)       # 192 CTBs of 32, one in eight intra: some without an intra neighbour
SUMS = dict(sloped_above=4, sloped_left=2, one_only=4, near_miss=2, filtered_121=4)


def _case(bd, axis, ctb, seed, path="planner", cf=1, **kw):
    cid = "%dbit%s_%s_ctb%d%s" % (bd, "_444" if cf == 3 else "", axis, 1 << ctb, "_light" if path == "light" else "")
    return cid, (bd, axis, path, dict(LIGHT if path == "light" else BASE, bit_depth=bd, chroma_format=cf, log2_ctb=ctb, seed=seed, **kw))


# seeds chosen with the census (x ramps give sloped borders above; y ramps a sloped left border only where below-left exists: CTBs of 64)
CASES = dict([
    _case(8, "x", 5, 9503), _case(8, "x", 6, 9511), _case(8, "y", 6, 9512), _case(8, "x", 5, 9502, "light"),
    _case(10, "x", 5, 9503), _case(10, "x", 6, 9511), _case(10, "y", 6, 9519), _case(10, "x", 5, 9502, "light"), _case(10, "y", 6, 9536, cf=3),
    _case(12, "x", 5, 9503), _case(12, "x", 6, 9511), _case(12, "y", 6, 9504),
])
IDS = sorted(CASES)
LIGHT_IDS = [i for i in IDS if CASES[i][2] == "light"]
DEPTHS = sorted(set(c[0] for c in CASES.values()))


def make_strong_case(axis, **cfg):
    pic, refs = make_case(**cfg)
    pic = attenuate_levels(pic, SHIFT[cfg["bit_depth"]])
    pic.pbs["mv"][:] = 0
    pp = pic.pp[0]
    return pic, axis_ramp_refs(refs, int(pp["bit_depth_luma"]), int(pp["bit_depth_chroma"]), axis)


def light_strong(pic, cen):
    """the census' strong blocks that lie in a CTB without an intra neighbour (a CTB of 32 is the block)"""
    cs, cw = pic.ctb_size, pic.pic_w_ctbs
    free = set(free_ctbs(pic))
    return [(x, y) for (x, y) in cen["blocks"] if (y // cs) * cw + x // cs in free]


_cache = {}


def prepared(oracle_lib, cid):
    """(picture, references, the oracle's planes {stages: planes}, census) of a case; made once, never modified.  The census has been checked
    against the oracle (module header)"""
    if cid not in _cache:
        bd, axis, path, cfg = CASES[cid]
        o = Oracle(oracle_lib)
        pic, refs = make_strong_case(axis, **cfg)
        want = dict((st, oracle_decode(o, pic, refs, st)) for st in (ST_INTRA, W.STAGE_ALL))
        cen = strong_census(want[ST_INTRA], pic)
        plain = pic.copy()
        plain.pp["flags"] &= ~np.uint32(W.PF_STRONG_INTRA_SMOOTHING)
        cen["oracle"] = check_strong_against_oracle(want[ST_INTRA], oracle_decode(o, plain, refs, ST_INTRA), pic, cen)
        _cache[cid] = (pic, refs, want, cen)
    return _cache[cid]


@pytest.mark.parametrize("bd", DEPTHS)
def test_strong_census_of_a_depth(oracle, bd):
    tot = dict((k, 0) for k in SUMS)
    for cid in IDS:
        if CASES[cid][0] != bd:
            continue
        pic, _, _, cen = prepared(oracle, cid)
        print("%-24s candidates %2d strong %2d sloped above %d left %d, one test only %2d, near miss %d, [1 2 1] %2d; flag cleared: %d blocks change, %d of them strong, %d strong unchanged"
              % ((cid, cen["candidates"], cen["strong"], cen["sloped_above"], cen["sloped_left"], cen["one_only"], cen["near_miss"], cen["filtered_121"]) + cen["oracle"]))
        assert cen["oracle"][1] >= 1, "%s: the oracle shows no strong block at work" % cid
        for k in tot:
            tot[k] += cen[k]
        if CASES[cid][2] == "light":
            ls = light_strong(pic, cen)
            assert len(ls) >= 2, "%s: only %d strong blocks in CTBs without an intra neighbour" % (cid, len(ls))
        if int(pic.pp[0]["chroma_format_idc"]) == 3:
            ibs = pic.ibs
            n = int(((ibs["cidx"] > 0) & (ibs["log2_size"] == 5) & ((ibs["flags"] & W.IBF_PCM) == 0) & ~np.isin(ibs["mode"], (1, 10, 26))).sum())
            assert n >= 4, "%s: only %d filtered 32x32 chroma blocks" % (cid, n)
    for k, need in SUMS.items():
        assert tot[k] >= need, "%d bits: %s is %d over all cases, need %d" % (bd, k, tot[k], need)


@pytest.mark.parametrize("cid", IDS)
def test_strong_oracle_equals_reference_replay(oracle, ref, cid):
    from ref_replay_py import ref_replay
    pic, refs, want, _ = prepared(oracle, cid)
    for st in (ST_INTRA, W.STAGE_ALL):
        assert_planes_equal(want[st], ref_replay(ref, pic, refs, st, accel=0), "oracle vs scalar reference, stages %d" % st)
    assert_planes_equal(want[ST_INTRA], ref_replay(ref, pic, refs, ST_INTRA, accel=1), "oracle vs SSE reference")


def run_case(lib, oracle_lib, cid, forced_32=False):
    """the case at pipeline depths 1 and 3 against the oracle, and the path it took: no light item in a "planner" case; in a process with
    M355_INTRA_LIGHT_32=1 light items, and the picture's CTBs without an intra neighbour among them"""
    pic, refs, want, cen = prepared(oracle_lib, cid)
    ctx = capi.Context(lib, 0)
    try:
        ctx.set_pipeline_depth(1)
        assert_planes_equal(device_decode(ctx, pic, refs, ST_INTRA), want[ST_INTRA], "%s: kernels vs oracle, no loop filters, depth 1" % cid)
        work, ticket, wg, light = intra_counts(ctx)
        assert_planes_equal(device_decode(ctx, pic, refs), want[W.STAGE_ALL], "%s: kernels vs oracle, all stages, depth 1" % cid)
        ctx.set_pipeline_depth(3)
        assert_planes_equal(device_decode(ctx, pic, refs, ST_INTRA, resident=True, repeat=4), want[ST_INTRA], "%s: kernels vs oracle, no loop filters, depth 3" % cid)
    finally:
        ctx.close()
    if forced_32:
        assert light >= len(free_ctbs(pic)) >= 1, "%s: %d light items, %d CTBs without an intra neighbour" % (cid, light, len(free_ctbs(pic)))
    elif CASES[cid][2] == "planner":
        assert light == 0 and wg == work, "%s: %d light items of %d: a CTB with a 32x32 intra block left the workgroup path" % (cid, light, work)


def run_forced_32(lib_path, oracle_path):
    """the light cases in a process that sends CTBs with 32x32 blocks down the light path (the runtime reads the setting once per process)"""
    code = ("import sys, ctypes; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "from test_intra_strong import LIGHT_IDS, run_case\n"
            "from libde265_amd import capi\n"
            "lib = capi.Library(%r); o = ctypes.CDLL(%r)\n"
            "for cid in LIGHT_IDS:\n"
            "    run_case(lib, o, cid, forced_32=True)\n"
            "print('forced 32x32 ok')\n") % (HERE, os.path.dirname(HERE), lib_path, oracle_path)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, M355_INTRA_LIGHT_32="1"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "forced 32x32 ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


@pytest.mark.parametrize("cid", IDS)
def test_strong_emulated(emu_lib, oracle, cid):  # noqa: F811
    run_case(emu_lib, oracle, cid)


def test_strong_light_path_emulated(emu_lib, oracle):  # noqa: F811
    run_forced_32(EMU_SO, oracle._name)


@pytest.fixture(scope="module")
def gpu_lib():
    lib = capi.Library()
    assert lib.device_count() >= 1
    return lib


@pytest.mark.gpu
@pytest.mark.parametrize("cid", IDS)
def test_strong_gpu(gpu_lib, oracle, cid):
    run_case(gpu_lib, oracle, cid)


@pytest.mark.gpu
def test_strong_light_path_gpu(gpu_lib, oracle):
    run_forced_32(gpu_lib.path, oracle._name)
