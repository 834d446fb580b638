"""Explicit weighted prediction on weights whose results stay IN RANGE (tests/wpred_content.py).  With the generator's weights
(w = 2^denom + U[-128, 127] at every denominator) most samples of a weighted block are 0 or maxv, and at denominators 0..3 practically all of
them: the write-back of k_inter_jobs (one v_dot2 per sample for all four reference formulas, offset and rounding term merged into one
constant), of k_inter_generic and of the oracle is then compared on the final clip alone.

Every case first asserts FROM THE ORACLE'S PLANES ALONE (weighted_census / corner_census on the STAGE_INTER picture; conditions on the input, so
that a change of the generator cannot empty the test):
  in-range cases   per plane: unclipped samples (0 < v < maxv) >= 60 % of the samples of weighted PBs; PBs without a clipped sample >= 50 %
                   luma, per (lists, denominator) class present: >= 2 PBs and >= 50 % unclipped
                   all eight denominators present for one list in every 4:2:0 case of 128x96 and larger (not 8bit_cu64: its 8 CUs hold 11
                   weighted PBs, which inrange_weights spreads over two or three denominators per kind, two PBs each)
                   PBs with a negative weight >= 20 % of the weighted PBs, their samples >= 50 % unclipped
  corner cases     every kind of wpred_content.CORNER_KINDS: >= 2 PBs in which no sample of any plane is clipped and not all samples are equal
  the file         clipped samples >= 3 % of all weighted samples over the cases (test_clip_stays_exercised)
  and what a case is named after is IN its lists (check_features).

Census of the seeds in this file (oracle planes, STAGE_INTER): unclipped share and PBs without a clipped sample / weighted PBs per plane; PBs
with a negative weight and their unclipped share; the same with the generator's own weights beside it (corner cases: on the same dimmed
references).  SEED_STEP names the cases whose first seed fell short of a condition:
  case               Y, Cb, Cr: unclipped, PBs without a clipped sample / weighted PBs | PBs with a negative weight, their unclipped share || the generator's weights
  8bit_420            92 %  92/110   93 %  93/110   93 %  94/110 | negative  50, 100 % || 20 %  19/110   29 %  22/110   33 %  20/110 | negative  88,  22 %
  10bit_420           94 %  89/107   95 %  92/107   95 %  93/107 | negative  55,  99 % || 37 %  21/107   27 %  21/107   20 %  24/107 | negative  81,  34 %
  12bit_420           97 %  46/53    98 %  46/53    98 %  46/53  | negative  26, 100 % || 25 %  13/53     8 %  11/53     7 %  10/53  | negative  40,  18 %
  mixed_9_12          93 %  95/115   94 %  98/115   93 %  98/115 | negative  59,  99 % || 34 %  25/115   34 %  27/115   30 %  29/115 | negative  83,  33 %
  8bit_mono           91 % 168/197 | negative  45, 100 % || 32 %  40/197 | negative  90,  14 %
  10bit_cu8           92 % 212/251   92 % 216/251   92 % 214/251 | negative 124, 100 % || 26 %  48/251   23 %  48/251   21 %  48/251 | negative 196,  21 %
  8bit_cu64           96 %   9/11    96 %   9/11    95 %  10/11  | negative   6,  99 % || 26 %   3/11    44 %   3/11    30 %   1/11  | negative   8,  23 %
  10bit_weighted40    90 %  26/31    88 %  26/31    93 %  27/31  | negative  20, 100 % || 12 %   7/31    37 %   8/31    48 %   7/31  | negative  25,  18 %
  8bit_oob40          92 %  86/102   92 %  89/102   91 %  90/102 | negative  59,  99 % || 27 %  20/102   33 %  28/102   28 %  31/102 | negative  83,  24 %
  8bit_missing_ref    96 %  60/66    94 %  59/66    95 %  59/66  | negative  33, 100 % || 9 %   9/66     7 %   8/66     5 %   6/66  | negative  55,   7 %
  10bit_422           95 %  96/115   94 %  97/115   93 %  95/115 | negative  49,  99 % || 39 %  24/115   26 %  27/115   27 %  22/115 | negative  95,  32 %
  10bit_444           93 %  72/86    93 %  72/86    92 %  71/86  | negative  50,  99 % || 6 %  14/86     8 %  16/86    43 %  17/86  | negative  72,  10 %
  14bit_420           89 %  47/59    92 %  50/59    90 %  50/59  | negative  34,  99 % || 32 %  16/59    41 %  16/59    38 %  19/59  | negative  50,  29 %
  16bit_420           95 %  45/54    95 %  45/54    94 %  45/54  | negative  27, 100 % || 22 %  17/54    40 %  27/54    31 %  27/54  | negative  44,  27 %
  10bit_16x64         98 %  10/11   100 %  11/11   100 %  11/11  | negative   8, 100 % || 24 %   3/11    35 %   2/11    62 %   4/11  | negative   7,  31 %
  corner_8bit         96 % 183/205   96 % 189/205   95 % 188/205 | negative  97,  99 % || 36 %  70/205   41 %  71/205   44 %  82/205 | negative 157,  34 %
      good / PBs per kind: w_max=63/81 w_min=52/60 w_zero_alone=29/29 w_zero_of_two=10/10 o_min=15/29 o_max=50/58 osum_min=6/10 osum_max=7/10 opposite=9/9
  corner_10bit        95 % 121/128   95 % 124/128   93 % 124/128 | negative  60,  98 % || 68 %  43/128   53 %  37/128   32 %  54/128 | negative  91,  47 %
      good / PBs per kind: w_max=46/50 w_min=31/38 w_zero_alone=19/19 w_zero_of_two=6/6 o_min=16/19 o_max=31/38 osum_min=4/5 osum_max=4/5 opposite=5/5
  corner_12bit        95 %  82/90    99 %  86/90    99 %  85/90  | negative  43,  95 % || 41 %  28/90    52 %  30/90    45 %  35/90  | negative  72,  41 %
      good / PBs per kind: w_max=28/35 w_min=23/27 w_zero_alone=13/13 w_zero_of_two=4/4 o_min=7/13 o_max=21/25 osum_min=3/4 osum_max=3/4 opposite=4/4
  clipped samples over all cases: 19921 of 356256 = 5.6 %

CPU tier: oracle == the reference's scalar functions (oracle/_ref replay; its SSE functions too where both depths are 8) == the kernels under
          the SIMT interpreter at pipeline depths 1 and 3, for STAGE_INTER and STAGE_ALL.
GPU tier: the HIP kernels == oracle at depths 1 and 3.  One case runs three different pictures in flight."""
import pytest

import inter_compact_cases as icc
from oracle_py import Oracle
from synth_util import assert_planes_equal, device_decode, make_case, oracle_decode
from test_emu_picture import emu_lib  # noqa: F401  (fixture)
from wpred_content import CORNER_KINDS, corner_census, corner_weights, dim_refs, inrange_weights, weighted_census, weighted_pbs
from libde265_amd import capi, synth, worklist as W

STAGES = (W.STAGE_INTER, W.STAGE_ALL)
BASE = dict(width=128, height=96, intra_pct=0, cbf_pct=0, bipred_pct=50, weighted_pct=100, oob_mv_pct=0, n_refs=2)
CORNER_DIM = 2        # the corner cases' references: shifted right by 2
# seeds: + 1000 * SEED_STEP where the census of that seed fell short of the conditions above
SEED_STEP = {"10bit_420": 1, "8bit_missing_ref": 1, "16bit_420": 2, "corner_8bit": 1}


def _case(cid, **cfg):
    cfg = dict(BASE, **cfg)
    cfg["seed"] = cfg["seed"] + 1000 * SEED_STEP.get(cid, 0)
    return cid, cfg


CASES = [
    # d_inter_job_lean (k_inter_jobs): every plane of 8..12 bits in 4:2:0 and monochrome
    _case("8bit_420", bit_depth=8, seed=8101),
    _case("10bit_420", bit_depth=10, seed=8102),
    _case("12bit_420", bit_depth=12, seed=8103),
    _case("mixed_9_12", bit_depth=9, bit_depth_chroma=12, seed=8104),
    _case("8bit_mono", bit_depth=8, chroma_format=4, seed=8105),
    _case("10bit_cu8", bit_depth=10, fixed_cu_log2=3, seed=8106),                          # 8x8, 8x4 and 4x8 PBs: 4-row jobs
    _case("8bit_cu64", bit_depth=8, fixed_cu_log2=6, width=256, height=128, seed=8107),
    _case("10bit_weighted40", bit_depth=10, weighted_pct=40, seed=8108),                   # weighted and unweighted lanes in one wave
    _case("8bit_oob40", bit_depth=8, oob_mv_pct=40, seed=8109),                            # weighted jobs of the EDGE range
    _case("8bit_missing_ref", bit_depth=8, features=synth.SYN_MISSING_REF, seed=8110),     # weighted PBs predicting the constant 1 << 13
    # k_inter_generic
    _case("10bit_422", bit_depth=10, chroma_format=2, seed=8111),
    _case("10bit_444", bit_depth=10, chroma_format=3, seed=8112),
    _case("14bit_420", bit_depth=14, seed=8113),
    _case("16bit_420", bit_depth=16, seed=8114),
    _case("10bit_16x64", bit_depth=10, width=16, height=64, log2_ctb=4, oob_mv_pct=50, seed=8115),
    # the ends of the legal ranges, on dimmed references
    _case("corner_8bit", bit_depth=8, seed=8121),
    _case("corner_10bit", bit_depth=10, seed=8122),
    _case("corner_12bit", bit_depth=12, seed=8123),
]
IDS = [c[0] for c in CASES]
_BY_ID = dict(CASES)
NOT_ALL_DENOMS = ("8bit_cu64",)
IN_FLIGHT = "10bit_420"     # three pictures of this configuration (seed, + 37, + 74) follow each other on the lanes


def make_wpred_case(cid, cfg=None):
    """(picture with its weights rewritten, references) of a case"""
    cfg = _BY_ID[cid] if cfg is None else cfg
    pic, refs = make_case(**cfg)
    if cid.startswith("corner"):
        return corner_weights(pic, cfg["seed"], CORNER_DIM), dim_refs(refs, CORNER_DIM)
    return inrange_weights(pic, cfg["seed"]), refs


def census_failures(cid, pic, cen):
    """the in-range conditions of the module's header -> the list of those that do not hold"""
    bad = []
    for c, e in enumerate(cen["planes"]):
        if e["unclipped"] * 100 < 60 * e["samples"]:
            bad.append("plane %d: %d of %d samples unclipped" % (c, e["unclipped"], e["samples"]))
        if e["clean"] * 100 < 50 * cen["pbs"]:
            bad.append("plane %d: %d of %d PBs without a clipped sample" % (c, e["clean"], cen["pbs"]))
    for (lists, d), e in sorted(cen["classes"].items()):
        if e["pbs"] < 2:
            bad.append("%d list(s), denominator %d: %d PB" % (lists, d, e["pbs"]))
        if e["unclipped"] * 100 < 50 * e["samples"]:
            bad.append("%d list(s), denominator %d: %d of %d samples unclipped" % (lists, d, e["unclipped"], e["samples"]))
    pp = pic.pp[0]
    if int(pp["chroma_format_idc"]) == 1 and int(pp["width"]) >= 128 and int(pp["height"]) >= 96 and cid not in NOT_ALL_DENOMS:
        missing = [d for d in range(8) if (1, d) not in cen["classes"]]
        if missing:
            bad.append("one list: no PB with denominator %s" % missing)
    n = cen["negative"]
    if n["pbs"] * 100 < 20 * cen["pbs"]:
        bad.append("%d of %d PBs carry a negative weight" % (n["pbs"], cen["pbs"]))
    if n["unclipped"] * 100 < 50 * n["samples"]:
        bad.append("PBs with a negative weight: %d of %d samples unclipped" % (n["unclipped"], n["samples"]))
    return bad


def corner_failures(kinds):
    return ["%s: %d PBs, %d unclipped and not constant" % (k, kinds[k][0], kinds[k][1]) for k in CORNER_KINDS if kinds[k][1] < 2]


def census_line(cid, cen):
    n = cen["negative"]
    return "%-18s %s | negative %3d, %3d %%" % (cid, "  ".join("%3d %% %3d/%-3d" % (100 * e["unclipped"] // e["samples"], e["clean"], cen["pbs"])
                                                                 for e in cen["planes"]), n["pbs"], 100 * n["unclipped"] // max(1, n["samples"]))


def weighted_job_counts(pic):
    """(weighted jobs in the MAIN range, in the EDGE range), by the device's predicates as inter_compact_cases restates them"""
    pp = pic.pp[0]
    width, height, cf = int(pp["width"]), int(pp["height"]), int(pp["chroma_format_idc"])
    main = edge = 0
    for i in weighted_pbs(pic):
        pb = pic.pbs[i]
        if icc.pb_is_edge(pb, width, height, cf):
            edge += icc.pb_jobs(pb)
        else:
            main += icc.pb_jobs(pb)
    return main, edge


def check_features(cid, pic):
    """what a case is named after must be in its lists"""
    kinds, _, n_edge = icc.job_lists(pic)
    sizes = {(int(pb["w"]), int(pb["h"])) for pb in pic.pbs}
    if "weighted40" in cid:
        windows = [set(kinds[o:o + icc.BLOCK].tolist()) for o in range(0, len(kinds), icc.BLOCK)]
        assert {icc.BI, icc.ONE, icc.WEIGHTED} in windows, "%s: no 256-job window holds all three kinds" % cid
    if "oob40" in cid:
        main, edge = weighted_job_counts(pic)
        assert edge <= n_edge and edge * 100 >= 25 * (main + edge), "%s: %d of %d weighted jobs in the EDGE range" % (cid, edge, main + edge)
    if "missing_ref" in cid:
        fill = [i for i in weighted_pbs(pic) if int(pic.pbs[i]["flags"]) & (W.PBF_FILL_L0 | W.PBF_FILL_L1)]
        both = [i for i in fill if (int(pic.pbs[i]["flags"]) & (W.PBF_PRED_L0 | W.PBF_PRED_L1)) == (W.PBF_PRED_L0 | W.PBF_PRED_L1)]
        assert len(fill) >= 8 and len(both) >= 2 and len(fill) - len(both) >= 2, "%s: %d weighted PBs with a missing reference" % (cid, len(fill))
    if "cu8" in cid:
        assert sizes == {(8, 8), (8, 4), (4, 8)}, sizes
    if "cu64" in cid:
        assert all(max(s) == 64 for s in sizes), sizes
    if "mono" in cid:
        assert int(pic.pp[0]["chroma_format_idc"]) == 0
    if cid in ("8bit_420", "10bit_420", "12bit_420", "mixed_9_12", "8bit_mono", "10bit_cu8", "8bit_cu64", "8bit_missing_ref") or cid.startswith("corner"):
        assert set(kinds.tolist()) == {icc.WEIGHTED}, "%s: MAIN jobs of kinds %s" % (cid, set(kinds.tolist()))


_cache = {}


def prepared(oracle_lib, cid):
    """(picture, references, oracle planes {stages: planes}, census) of a case, its conditions checked; made once, never modified"""
    if cid not in _cache:
        o = Oracle(oracle_lib)
        pic, refs = make_wpred_case(cid)
        want = dict((st, oracle_decode(o, pic, refs, st)) for st in STAGES)
        _cache[cid] = (pic, refs, want, weighted_census(pic, want[W.STAGE_INTER]))
    pic, refs, want, cen = _cache[cid]
    check_features(cid, pic)
    if cid.startswith("corner"):
        bad = corner_failures(corner_census(pic, want[W.STAGE_INTER]))
    else:
        bad = census_failures(cid, pic, cen)
    assert not bad, "%s: %s\n%s" % (cid, "; ".join(bad), census_line(cid, cen))
    return pic, refs, want


def check_clip_stays_exercised(oracle_lib):
    samples = clipped = 0
    for cid in IDS:
        prepared(oracle_lib, cid)
        for e in _cache[cid][3]["planes"]:
            samples += e["samples"]
            clipped += e["samples"] - e["unclipped"]
    assert clipped * 100 >= 3 * samples, "only %d of %d weighted samples clipped" % (clipped, samples)


def in_flight_pictures(oracle_lib):
    """three different pictures of one configuration, weights rewritten, on the references of the first; the oracle's planes beside them"""
    if "in_flight" not in _cache:
        o = Oracle(oracle_lib)
        cfg = _BY_ID[IN_FLIGHT]
        refs = make_case(**cfg)[1]
        pics = []
        for k in range(3):
            pic = make_wpred_case(IN_FLIGHT, dict(cfg, seed=cfg["seed"] + 37 * k))[0]
            want = oracle_decode(o, pic, refs)
            bad = census_failures(IN_FLIGHT, pic, weighted_census(pic, oracle_decode(o, pic, refs, W.STAGE_INTER)))
            assert not bad, "in flight, picture %d: %s" % (k, "; ".join(bad))
            pics.append((pic, want))
        _cache["in_flight"] = (pics, refs)
    return _cache["in_flight"]


def run_in_flight(lib, oracle_lib):
    """six decodes, three in flight: every lane decodes two DIFFERENT pictures in a row (as inter_compact_cases.run_case)"""
    pics, refs = in_flight_pictures(oracle_lib)
    order = [0, 1, 2, 1, 2, 0]
    ctx = capi.Context(lib, 0)
    try:
        ctx.set_pipeline_depth(3)
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
            pic.ref_frames = [handles[i] if i < len(handles) else -1 for i in range(W.MAX_REF_FRAMES)]
            ctx.submit(pic)
            dsts.append(dst)
        ctx.wait()
        for i, k in enumerate(order):
            assert_planes_equal(ctx.frame_download(dsts[i]), pics[k][1], "3 in flight, decode %d (picture %d)" % (i, k))
    finally:
        ctx.close()


def test_weights_stay_legal():
    """inrange_weights and corner_weights write only what a bitstream can carry: w - 2^d in -128..127, offsets -128..127 scaled by the
    component's own depth, both records of a PB with the same denominators; they touch nothing but the records of weighted PBs"""
    import numpy as np
    for cid in ("mixed_9_12", "10bit_weighted40", "corner_12bit", "16bit_420"):
        pic = make_wpred_case(cid)[0]
        gen = synth.picture(**_BY_ID[cid])
        bd = [int(pic.pp[0]["bit_depth_luma"])] + [int(pic.pp[0]["bit_depth_chroma"])] * 2
        assert len(weighted_pbs(pic)) >= 8
        for i in weighted_pbs(pic):
            a, b = (pic.wts[int(j)] for j in pic.pbs[i]["wt_idx"])
            assert a["log2wd_luma"] == b["log2wd_luma"] and a["log2wd_chroma"] == b["log2wd_chroma"]
            for r in (a, b):
                for k in range(3):
                    d = int(r["log2wd_chroma" if k else "log2wd_luma"]) - max(2, 14 - bd[k])
                    assert 0 <= d <= 7 and -128 <= int(r["w"][k]) - (1 << d) <= 127, (cid, i, k)
                    o = int(r["o"][k])
                    assert o % (1 << (bd[k] - 8)) == 0 and -128 <= o >> (bd[k] - 8) <= 127, (cid, i, k)
        for name in ("pbs", "cus", "tus", "rbs", "ibs", "coeffs"):
            assert np.array_equal(getattr(pic, name), getattr(gen, name)), name
        assert len(pic.wts) == len(gen.wts)


def test_clip_stays_exercised(oracle):
    check_clip_stays_exercised(oracle)


@pytest.mark.parametrize("cid", IDS)
def test_wpred_oracle_equals_reference_replay(oracle, ref, cid):
    from ref_replay_py import ref_replay
    pic, refs, want = prepared(oracle, cid)
    for st in STAGES:
        assert_planes_equal(want[st], ref_replay(ref, pic, refs, st, accel=0), "oracle vs scalar reference, stages %d" % st)
    if int(pic.pp[0]["bit_depth_luma"]) == 8 and int(pic.pp[0]["bit_depth_chroma"]) == 8:
        # (the reference has SSE motion compensation for 8-bit samples only; its weighted write-back with explicit weights stays scalar)
        for st in STAGES:
            assert_planes_equal(want[st], ref_replay(ref, pic, refs, st, accel=1), "oracle vs SSE reference, stages %d" % st)


@pytest.mark.parametrize("cid", IDS)
def test_wpred_emulated(emu_lib, oracle, cid):  # noqa: F811
    pic, refs, want = prepared(oracle, cid)
    ctx = capi.Context(emu_lib, 0)
    try:
        for depth in (1, 3):
            ctx.set_pipeline_depth(depth)
            for st in STAGES:
                assert_planes_equal(device_decode(ctx, pic, refs, st), want[st], "kernels vs oracle, stages %d, depth %d" % (st, depth))
    finally:
        ctx.close()


def test_wpred_in_flight_emulated(emu_lib, oracle):  # noqa: F811
    run_in_flight(emu_lib, oracle)


@pytest.fixture(scope="module")
def gpu_ctx():
    lib = capi.Library()
    assert lib.device_count() >= 1
    c = capi.Context(lib, 0)
    yield c
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cid", IDS)
def test_wpred_gpu(gpu_ctx, oracle, cid):
    ctx = gpu_ctx
    pic, refs, want = prepared(oracle, cid)
    try:
        for depth in (1, 3):
            ctx.set_pipeline_depth(depth)
            for st in STAGES:
                assert_planes_equal(device_decode(ctx, pic, refs, st, resident=depth == 3, repeat=depth), want[st],
                                    "HIP vs oracle, stages %d, depth %d" % (st, depth))
    finally:
        ctx.set_pipeline_depth(1)


@pytest.mark.gpu
def test_wpred_in_flight_gpu(oracle):
    run_in_flight(capi.Library(), oracle)


@pytest.mark.gpu
def test_clip_stays_exercised_gpu_tier(oracle):
    check_clip_stays_exercised(oracle)
