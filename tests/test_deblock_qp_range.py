"""Deblocking over the WHOLE QP range (tests/deblock_qp_content.py): pictures whose QpY field, picture chroma offsets and slice offsets walk every
entry of c_tab_beta, c_tab_tc and c_qpc_420, both Clip3 bounds of both indices and the min(qP_i, 51) of the formats other than 4:2:0
(csrc/k_deblock.hip, k_deblock_dev.h; deblock.cc:517-531 and :698-721), on samples the test dictates so that the table entry decides the result.
The generator's own QPs and offsets reach the lower two thirds of the tables; the rest hangs on a few `qp_wide` seeds.

A case is a set of five pictures of one configuration (the picture offsets are one pair per picture).  test_qp_census first checks the
restatement (deblock_qp_content.restate: plain Python over the lists, following the reference) against the oracle's planes with deblocking off
(the canvas) and with SAO off, then asserts FROM THE RESTATEMENT ALONE, before any kernel runs — conditions on the input, so that a change of
the generator cannot empty the test.  `sensitive to X`: filtering the segment again with the one-step change X (the content module's header)
changes its result on lines the other pass cannot write.
  * every beta index 16..51 in >= 2 luma segments sensitive to beta- / beta+, every tc index 18..53 in >= 2 sensitive to tc- / tc+, per direction
  * >= 8 segments sensitive to beta whose filter is on (d = beta - 1) and >= 8 whose filter is off (d = beta)
  * beta index 0..15: >= 8 segments, tc index 0..17: >= 8 segments, all silent (each carries the step of tc' = 1)
  * the unclipped sums: beta below 0 in >= 2 segments, tc below 0 in >= 2; beta above 51 in >= 2 segments sensitive to the bound 51 -> 50,
    tc above 53 in >= 2 sensitive to 53 -> 52
  * >= 8 segments at edges where QP_Q + QP_P is odd are sensitive to the `+ 1` of the average; >= 8 sensitive segments at even sums
  * above 8 bits: >= 8 segments whose QP average is negative (silent: their indices stay below 14)
  * 4:2:0, per chroma plane: each qP_i of 30..42 in >= 2 segments sensitive to QP_C +- 1; qP_i >= 43 in >= 4, of them >= 2 at 43; qP_i < 30 in >= 4,
    of them >= 2 at 29; a negative qP_i in >= 2 segments, all silent
  * 4:2:2 and 4:4:4, per chroma plane: qP_i 52..63 in >= 4 segments sensitive to the min; qP_i 51 and 50 in >= 2 each sensitive to QP_C +- 1
  * pictures whose Cb and Cr offsets have opposite signs and different magnitudes hold >= 8 chroma segments in which the filter adds another
    amount to Cb than to Cr (the planes' canvases are equal); >= 8 chroma segments at odd sums are sensitive to the `+ 1`
A class the issue of this test named that legal values cannot reach: a NEGATIVE qP_i cannot be sensitive, its tc index is at most
-1 + 2 + 12 = 13 and tc' is 0 below 18; it is asked to be present and silent instead.  (tc index 53 is reached: a QP average of 41..51 beside a
PCM unit with a slice offset of 0..12.)  The monochrome case has the luma conditions only; all-intra pictures have bS 2 everywhere.

CPU tier: oracle == the reference's own apply_deblocking_filter on the same lists (oracle/_ref replay: scalar, and SSE where both depths are 8):
          on this content the oracle's deblocking restates the kernel's formulas, the replay is what makes the comparison independent;
          kernels under the SIMT interpreter == oracle at pipeline depth 1 and 3, with SAO off and with all stages; a set's five pictures in
          flight at depth 3 (a lane never meets the previous picture's offsets again); the all-intra set through m355_decode_batch
          (k_deblock_batch); the 2x2-tile set through two ranks in lockstep (k_shard.hip injects the units across the tile borders).
GPU tier: the HIP kernels == oracle, the same.

CENSUS of the sets below (deblock_qp_content.census_line): the LEAST number of sensitive segments over the beta indices 16..51 in vertical /
horizontal edges, the same for the tc indices 18..53 | segments with beta index <= 15, tc index <= 17 | unclipped beta, tc sum below 0 | beta sum above
51: sensitive to the bound / all, the same for tc above 53 | sensitive segments at odd sums (of them sensitive to the + 1), at even sums |
sensitive to beta with the filter on, off | segments with bS 1, bS 2 | with a negative QP average | per chroma plane: the least over qP_i 30..42,
qP_i >= 43 (at 43), < 30 (at 29), negative; or: sensitive to the min, at qP_i 51, 50 | Cb and Cr differ, chroma at odd sums sensitive to the + 1
  8bit           beta 2/2 tc 2/2 | low 228, 300 | <0 88, 64 | over 21/52, 41/108 | odd 560 (391), even 134 | on 493 off 167 | bS 1: 516, 2: 1124 | QP < 0 0 | Cb tab 4, >=43 132 (43: 18), <30 68 (29: 8), <0 26 | Cr tab 4, >=43 28 (43: 6), <30 74 (29: 6), <0 2 | Cb != Cr 284, odd 216
  10bit          beta 2/2 tc 2/2 | low 272, 332 | <0 88, 120 | over 43/116, 13/32 | odd 549 (395), even 127 | on 481 off 163 | bS 1: 516, 2: 1124 | QP < 0 48 | Cb tab 2, >=43 140 (43: 14), <30 68 (29: 8), <0 30 | Cr tab 2, >=43 66 (43: 10), <30 58 (29: 6), <0 2 | Cb != Cr 192, odd 214
  12bit          beta 2/2 tc 2/2 | low 372, 352 | <0 176, 212 | over 50/132, 35/92 | odd 570 (393), even 64 | on 464 off 160 | bS 1: 516, 2: 1124 | QP < 0 144 | Cb tab 2, >=43 134 (43: 14), <30 64 (29: 6), <0 62 | Cr tab 2, >=43 40 (43: 8), <30 66 (29: 4), <0 28 | Cb != Cr 192, odd 216
  16bit          beta 2/2 tc 2/2 | low 380, 388 | <0 108, 96 | over 36/92, 28/72 | odd 454 (295), even 164 | on 438 off 144 | bS 1: 0, 2: 1640 | QP < 0 52 | Cb tab 6, >=43 44 (43: 6), <30 142 (29: 4), <0 100 | Cr tab 10, >=43 100 (43: 14), <30 118 (29: 12), <0 20 | Cb != Cr 264, odd 218
  mixed_10_12    beta 2/2 tc 2/2 | low 272, 332 | <0 88, 120 | over 43/116, 13/32 | odd 549 (395), even 127 | on 481 off 163 | bS 1: 516, 2: 1124 | QP < 0 48 | Cb tab 2, >=43 140 (43: 14), <30 68 (29: 8), <0 30 | Cr tab 2, >=43 66 (43: 10), <30 58 (29: 6), <0 2 | Cb != Cr 192, odd 214
  10bit_422      beta 2/2 tc 2/2 | low 344, 416 | <0 148, 156 | over 62/164, 6/16 | odd 517 (363), even 117 | on 444 off 148 | bS 1: 516, 2: 1124 | QP < 0 88 | Cb min 18, 51: 2, 50: 4 | Cr min 36, 51: 4, 50: 4 | Cb != Cr 472, odd 364
  10bit_444      beta 2/2 tc 2/2 | low 344, 416 | <0 148, 156 | over 62/164, 6/16 | odd 517 (363), even 117 | on 444 off 148 | bS 1: 516, 2: 1124 | QP < 0 88 | Cb min 20, 51: 4, 50: 4 | Cr min 44, 51: 4, 50: 4 | Cb != Cr 608, odd 444
  8bit_mono      beta 2/2 tc 2/2 | low 228, 300 | <0 88, 64 | over 21/52, 41/108 | odd 560 (391), even 134 | on 493 off 167 | bS 1: 516, 2: 1124 | QP < 0 0
  10bit_tiles2x2 beta 2/2 tc 2/2 | low 300, 392 | <0 64, 104 | over 57/152, 45/120 | odd 594 (378), even 62 | on 455 off 153 | bS 1: 516, 2: 1124 | QP < 0 52 | Cb tab 8, >=43 52 (43: 8), <30 82 (29: 10), <0 44 | Cr tab 4, >=43 56 (43: 8), <30 68 (29: 6), <0 20 | Cb != Cr 186, odd 212
  8bit_intra     beta 2/4 tc 2/2 | low 528, 496 | <0 76, 84 | over 43/112, 8/20 | odd 343 (228), even 201 | on 382 off 128 | bS 1: 0, 2: 1640 | QP < 0 0 | Cb tab 4, >=43 64 (43: 6), <30 116 (29: 6), <0 74 | Cr tab 4, >=43 138 (43: 14), <30 66 (29: 14), <0 4 | Cb != Cr 676, odd 176"""
import numpy as np
import pytest

import deblock_qp_content as D
from batch_util import check_batches
from oracle_py import Oracle
from shard_util import local_sharded_decode
from synth_util import assert_planes_equal, device_decode, oracle_decode
from test_emu_picture import emu_lib  # noqa: F401  (fixture)
from libde265_amd import capi, synth, worklist as W

NO_DEBLOCK = W.STAGE_INTER | W.STAGE_RESIDUAL | W.STAGE_INTRA
NO_SAO = W.STAGE_ALL & ~W.STAGE_SAO


def _spec(a, sy, cb, cr, pcm_mod, pcm_phase, slices):
    return dict(a=a, sy=sy, cb=cb, cr=cr, pcm_mod=pcm_mod, pcm_phase=pcm_phase, slices=slices)


# QP at unit (0, 0), QP step per unit row (per unit column: 1), pic_cb / pic_cr_qp_offset, every pcm_mod-th unit is PCM (phase), and per slice
# (beta_offset, tc_offset).  The second picture of every set carries the extreme slice offsets in three slices; the reference reads them from
# the slice of the Q side.
EXTREME = _spec(0, 7, -12, 5, 3, 1, [(-12, -12), (0, 2), (12, 12)])
SETS = {
    "8bit": [
        _spec(4, 8, 12, -7, 3, 0, [(0, 0), (0, 0), (0, 0)]),
        EXTREME,
        _spec(31, 3, 3, 10, 3, 2, [(12, 12), (6, 8), (2, 4)]),
        _spec(20, 5, -3, -12, 2, 0, [(8, 0), (4, 2), (-12, 0)]),
        _spec(24, 10, 7, -2, 3, 0, [(4, 8), (-6, 6), (8, -8)]),
    ],
    "10bit": [
        _spec(4, 8, 12, -7, 3, 0, [(0, 0), (0, 0), (0, 0)]),
        EXTREME,
        _spec(30, 3, 3, 9, 3, 2, [(12, 12), (6, 8), (6, 2)]),
        _spec(20, 5, -3, -12, 2, 0, [(8, 0), (4, 2), (-12, 0)]),
        _spec(8, 10, 7, 12, 3, 0, [(2, -4), (-6, 6), (8, -8)]),
    ],
    "12bit": [
        _spec(4, 8, 12, -7, 3, 0, [(0, 0), (0, 0), (0, 0)]),
        EXTREME,
        _spec(32, 3, 3, 9, 3, 2, [(12, 12), (6, 8), (6, 2)]),
        _spec(20, 5, -3, -12, 2, 0, [(8, 0), (4, 2), (-12, 0)]),
        _spec(24, 9, 7, 12, 3, 0, [(2, -4), (-6, 6), (8, -8)]),
    ],
    # (16 bits: every unit PCM.  Motion compensation keeps 14 bits between its steps, there is no exact copy of a 16-bit sample)
    "16bit": [
        _spec(4, 8, -1, -1, 1, 0, [(12, -8), (-10, -10), (-8, -12)]),
        dict(EXTREME, pcm_mod=1),
        _spec(8, 8, 2, 10, 1, 1, [(6, 4), (10, -2), (6, 2)]),
        _spec(20, 5, -11, -12, 1, 0, [(10, 12), (8, -8), (6, 6)]),
        _spec(0, 10, -11, 12, 1, 0, [(4, 8), (-10, 8), (4, 2)]),
    ],
    "mixed_10_12": [
        _spec(4, 8, 12, -7, 3, 0, [(0, 0), (0, 0), (0, 0)]),
        EXTREME,
        _spec(30, 3, 3, 9, 3, 2, [(12, 12), (6, 8), (6, 2)]),
        _spec(20, 5, -3, -12, 2, 0, [(8, 0), (4, 2), (-12, 0)]),
        _spec(8, 10, 7, 12, 3, 0, [(2, -4), (-6, 6), (8, -8)]),
    ],
    "10bit_422": [
        _spec(4, 9, -11, -7, 3, 0, [(0, 0), (6, 0), (0, 0)]),
        EXTREME,
        _spec(30, 3, 3, -7, 3, 2, [(-10, -8), (10, -2), (6, 2)]),
        _spec(20, 6, -6, 4, 2, 0, [(8, 0), (4, 2), (-12, 0)]),
        _spec(36, 10, 7, 12, 3, 0, [(8, -8), (2, -2), (8, -8)]),
    ],
    "10bit_444": [
        _spec(4, 9, -11, -7, 3, 0, [(0, 0), (6, 0), (0, 0)]),
        EXTREME,
        _spec(30, 3, 3, -7, 3, 2, [(-10, -8), (10, -2), (6, 2)]),
        _spec(20, 6, -6, 4, 2, 0, [(8, 0), (4, 2), (-12, 0)]),
        _spec(36, 10, 7, 12, 3, 0, [(8, -8), (2, -2), (8, -8)]),
    ],
    "8bit_mono": [
        _spec(4, 8, 12, -7, 3, 0, [(0, 0), (0, 0), (0, 0)]),
        EXTREME,
        _spec(31, 3, 3, 10, 3, 2, [(12, 12), (6, 8), (2, 4)]),
        _spec(20, 5, -3, -12, 2, 0, [(8, 0), (4, 2), (-12, 0)]),
        _spec(24, 10, 7, -2, 3, 0, [(4, 8), (-6, 6), (8, -8)]),
    ],
    "10bit_tiles2x2": [
        _spec(4, 8, 6, -6, 3, 0, [(-8, -10), (6, 0), (0, 0)]),
        EXTREME,
        _spec(30, 3, -8, 7, 3, 2, [(6, 4), (4, 6), (6, 10)]),
        _spec(20, 5, 0, -8, 2, 2, [(-4, -2), (4, 2), (10, 12)]),
        _spec(12, 9, -11, -5, 3, 0, [(8, -8), (-8, 2), (8, -8)]),
    ],
    "8bit_intra": [
        _spec(4, 8, 12, -7, 3, 2, [(0, 0), (-10, -10), (-8, -12)]),
        EXTREME,
        _spec(16, 6, -7, 10, 3, 2, [(-2, 0), (10, -2), (6, 2)]),
        _spec(47, 5, -5, 4, 2, 0, [(8, 0), (4, -6), (-12, 0)]),
        _spec(12, 8, -7, 12, 3, 2, [(2, -4), (-6, 6), (8, -8)]),
    ],
}
# id -> generator configuration over deblock_qp_content.BASE (128x96, CTB 32, 16x16 units); picture k of a set has seed + k
CASES = {
    "8bit": dict(bit_depth=8, seed=7100),
    "10bit": dict(bit_depth=10, seed=7200),
    "12bit": dict(bit_depth=12, seed=7300),
    "16bit": dict(bit_depth=16, seed=7400),                                     # QpBdOffset 48: the negative half of the range is widest
    "mixed_10_12": dict(bit_depth=10, bit_depth_chroma=12, seed=7500),          # the chroma tc scales by the chroma depth
    "10bit_422": dict(bit_depth=10, chroma_format=2, seed=7600),
    "10bit_444": dict(bit_depth=10, chroma_format=3, seed=7700),
    "8bit_mono": dict(bit_depth=8, chroma_format=4, seed=7800),
    "10bit_tiles2x2": dict(bit_depth=10, tile_cols=2, tile_rows=2, seed=7900),  # a slice per tile: four slices
    "8bit_intra": dict(bit_depth=8, n_refs=0, intra_pct=100, seed=8000),        # every unit PCM; through m355_decode_batch too
}
IDS = list(CASES)
IN_FLIGHT, BATCHED, SHARDED = "10bit", "8bit_intra", "10bit_tiles2x2"
ALL_PCM = ("16bit", "8bit_intra")

_cache = {}


def prepared(oracle_lib, cid):
    """(list of dict(pic, refs, canvas, restated, want = {stages: oracle planes}, luma, chroma), census); made once, never modified"""
    if cid not in _cache:
        o = Oracle(oracle_lib)
        made = []
        for k, spec in enumerate(SETS[cid]):
            pic, refs, planes, luma, chroma = D.qp_picture(spec, **dict(CASES[cid], seed=CASES[cid]["seed"] + k))
            restated = D.restate(pic, planes, luma, chroma)
            want = dict((st, oracle_decode(o, pic, refs, st)) for st in (NO_DEBLOCK, NO_SAO, W.STAGE_ALL))
            made.append(dict(pic=pic, refs=refs, canvas=planes, restated=restated, want=want, luma=luma, chroma=chroma))
        _cache[cid] = (made, D.census([(m["pic"], m["luma"], m["chroma"]) for m in made]))
    return _cache[cid]


def check_conditions(cid, made, cen):
    """the conditions of the module's header"""
    pp = made[0]["pic"].pp[0]
    cf, bd = int(pp["chroma_format_idc"]), int(pp["bit_depth_luma"])
    print(D.census_line(cid, cen, cf))
    for k, m in enumerate(made):
        assert_planes_equal(m["want"][NO_DEBLOCK], m["canvas"], "%s picture %d: oracle before the filter vs the canvas" % (cid, k))
        assert_planes_equal(m["want"][NO_SAO], m["restated"], "%s picture %d: oracle vs the restatement, SAO off" % (cid, k))
        loud = [s for s in m["luma"] if (s["beta_idx"] <= 15 or s["tc_idx"] <= 17) and s["live"]]
        assert not loud, "%s picture %d: %d segments with beta' or tc' 0 changed" % (cid, k, len(loud))
    bad = D.census_failures(cen, cf, bd)
    assert not bad, "%s: %s" % (cid, "; ".join(bad))
    offs = [(int(m["pic"].pp[0]["pic_cb_qp_offset"]), int(m["pic"].pp[0]["pic_cr_qp_offset"])) for m in made]
    assert len(set(offs)) == len(offs), "%s: two pictures share their chroma offsets" % cid
    assert any(cb * cr < 0 and abs(cb) != abs(cr) for cb, cr in offs)
    assert all(len(m["pic"].slices) >= 3 for m in made)
    if cid in ALL_PCM:
        assert all(all(m["pic"].cus["flags"] == W.CUF_PCM) for m in made) and cen["bs"][1] == 0
    else:
        assert cen["bs"][1] >= 100 and cen["bs"][2] >= 100, "%s: bS 1 in %d segments, bS 2 in %d" % (cid, cen["bs"][1], cen["bs"][2])
    if bd > 8:
        assert any(int(m["pic"].cus["qp_y"].min()) < 0 for m in made)


def test_rewritten_lists_stay_legal():
    """qp_picture writes only what a bitstream can carry (QpY in -QpBdOffsetY..51, picture chroma offsets in -12..12, slice offsets even and
    in -12..12, PCM samples within their depth, pcm_loop_filter_disable off), and of the generated units it keeps positions, sizes,
    partitions and, in the inter units, the transform trees and the prediction blocks' geometry"""
    for cid in ("8bit", "16bit", "mixed_10_12", "10bit_422", "10bit_tiles2x2", "8bit_intra"):
        for k, spec in enumerate(SETS[cid]):
            cfg = dict(D.BASE, **dict(CASES[cid], seed=CASES[cid]["seed"] + k))
            pic = D.qp_picture(spec, **cfg)[0]
            gen = synth.picture(**cfg)
            D.check_legal(pic)
            qmin = -6 * (cfg["bit_depth"] - 8)
            assert int(pic.cus["qp_y"].min()) >= qmin and int(pic.cus["qp_y"].max()) <= 51
            for name in ("x", "y", "log2_size"):
                assert np.array_equal(pic.cus[name], gen.cus[name])
            inter = pic.cus["pred_mode"] != 0
            assert np.array_equal(pic.cus["part_mode"][inter], gen.cus["part_mode"][inter]) and np.array_equal(pic.cus["pred_mode"][inter], gen.cus["pred_mode"][inter])
            assert all(pic.cus["flags"][~inter] == W.CUF_PCM) and int((~inter).sum()) >= len(pic.cus) // 4
            boxes = set((int(p["x"]), int(p["y"]), int(p["w"]), int(p["h"])) for p in pic.pbs)
            assert boxes <= set((int(p["x"]), int(p["y"]), int(p["w"]), int(p["h"])) for p in gen.pbs)
            assert sum(int(p["w"]) * int(p["h"]) for p in pic.pbs) == 256 * int(inter.sum())
            assert sum(1 << (2 * int(t["log2_size"])) for t in pic.tus) == cfg["width"] * cfg["height"]
            assert len(pic.rbs) == 0 and len(pic.coeffs) == 0 and len(pic.wts) == 0
            assert np.array_equal(pic.ctbs["sao_type"], gen.ctbs["sao_type"]) and np.array_equal(pic.ctbs["sao_offset"], gen.ctbs["sao_offset"])


@pytest.mark.parametrize("cid", IDS)
def test_qp_census(oracle, cid):
    check_conditions(cid, *prepared(oracle, cid))


@pytest.mark.parametrize("cid", IDS)
def test_qp_oracle_equals_reference_replay(oracle, ref, cid):
    from ref_replay_py import ref_replay
    for k, m in enumerate(prepared(oracle, cid)[0]):
        pic, refs, want = m["pic"], m["refs"], m["want"]
        for st in (NO_DEBLOCK, NO_SAO, W.STAGE_ALL):
            assert_planes_equal(want[st], ref_replay(ref, pic, refs, st, accel=0), "picture %d: oracle vs scalar reference, stages %d" % (k, st))
        if int(pic.pp[0]["bit_depth_luma"]) == 8 and int(pic.pp[0]["bit_depth_chroma"]) == 8:
            assert_planes_equal(want[NO_SAO], ref_replay(ref, pic, refs, NO_SAO, accel=1), "picture %d: oracle vs SSE reference, SAO off" % k)


def check_kernels(ctx, made, what):
    for k, m in enumerate(made):
        pic, refs, want = m["pic"], m["refs"], m["want"]
        ctx.set_pipeline_depth(1)
        assert_planes_equal(device_decode(ctx, pic, refs, NO_SAO), want[NO_SAO], "%s picture %d: kernels vs oracle, SAO off" % (what, k))
        assert_planes_equal(device_decode(ctx, pic, refs), want[W.STAGE_ALL], "%s picture %d: kernels vs oracle, all stages" % (what, k))
        ctx.set_pipeline_depth(3)
        try:
            assert_planes_equal(device_decode(ctx, pic, refs, NO_SAO, resident=True, repeat=3), want[NO_SAO], "%s picture %d: depth 3, SAO off" % (what, k))
            assert_planes_equal(device_decode(ctx, pic, refs, resident=True, repeat=3), want[W.STAGE_ALL], "%s picture %d: depth 3, all stages" % (what, k))
        finally:
            ctx.set_pipeline_depth(1)


def run_in_flight(lib, made):
    """the set's pictures follow each other on three lanes, twice: a lane decodes pictures with different offsets in a row"""
    order = [0, 1, 2, 3, 4, 2, 0, 4, 1, 3]
    ctx = capi.Context(lib, 0)
    try:
        ctx.set_pipeline_depth(3)
        pp = made[0]["pic"].pp[0]
        dsts = []
        for k in order:
            m = made[k]
            frames = []                                     # (every picture's references hold its own canvas: a pair of frames per decode)
            for planes in m["refs"]:
                f = ctx.frame_create_for(pp)
                ctx.frame_upload(f, planes)
                frames.append(f)
            pic = m["pic"].copy()
            pic.dst_frame = ctx.frame_create_for(pp)
            pic.ref_frames = [frames[i] if i < len(frames) else -1 for i in range(W.MAX_REF_FRAMES)]
            ctx.submit(pic)
            dsts.append(pic.dst_frame)
        ctx.wait()
        for i, k in enumerate(order):
            assert_planes_equal(ctx.frame_download(dsts[i]), made[k]["want"][W.STAGE_ALL], "3 in flight, decode %d (picture %d)" % (i, k))
    finally:
        ctx.close()


def run_batched(lib, oracle_lib, made):
    pics = [m["pic"].copy() for m in made]
    ctx, _, _, _, want = check_batches(lib, Oracle(oracle_lib), None, 3, [[0, 1, 2], [3, 4], [2, 0, 4]], pics=pics)
    ctx.close()
    for k, m in enumerate(made):
        assert_planes_equal(want[k], m["want"][W.STAGE_ALL], "the batch's own expectation, picture %d" % k)


def run_sharded(lib, made, **kw):
    for k, m in enumerate(made):
        for r, got in enumerate(local_sharded_decode(lib, m["pic"], m["refs"], 2, **kw)):
            assert_planes_equal(got, m["want"][kw.get("stages", W.STAGE_ALL)], "picture %d: lockstep rank %d" % (k, r))


@pytest.mark.parametrize("cid", IDS)
def test_qp_emulated(emu_lib, oracle, cid):  # noqa: F811
    made, cen = prepared(oracle, cid)
    check_conditions(cid, made, cen)
    ctx = capi.Context(emu_lib, 0)
    try:
        check_kernels(ctx, made, cid)
    finally:
        ctx.close()


def test_qp_in_flight_emulated(emu_lib, oracle):  # noqa: F811
    run_in_flight(emu_lib, prepared(oracle, IN_FLIGHT)[0])


def test_qp_batched_emulated(emu_lib, oracle):  # noqa: F811
    run_batched(emu_lib, oracle, prepared(oracle, BATCHED)[0])


def test_qp_sharded_emulated(emu_lib, oracle):  # noqa: F811
    """two ranks, two tiles each: the units across a tile border between them are records that k_shard.hip injected, with their QpY"""
    run_sharded(emu_lib, prepared(oracle, SHARDED)[0], stages=NO_SAO)


@pytest.fixture(scope="module")
def gpu_ctx():
    lib = capi.Library()
    assert lib.device_count() >= 1
    c = capi.Context(lib, 0)
    yield c
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cid", IDS)
def test_qp_gpu(gpu_ctx, oracle, cid):
    made, cen = prepared(oracle, cid)
    check_conditions(cid, made, cen)
    check_kernels(gpu_ctx, made, cid)


@pytest.mark.gpu
def test_qp_in_flight_gpu(oracle):
    run_in_flight(capi.Library(), prepared(oracle, IN_FLIGHT)[0])


@pytest.mark.gpu
def test_qp_batched_gpu(oracle):
    run_batched(capi.Library(), oracle, prepared(oracle, BATCHED)[0])


@pytest.mark.gpu
def test_qp_sharded_gpu(oracle):
    run_sharded(capi.Library(), prepared(oracle, SHARDED)[0], device="cuda:0")
