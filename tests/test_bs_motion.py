"""Boundary strength from MOTION (tests/bs_motion_content.py): pictures in which neighbouring prediction blocks name the same pictures —
straight, crossed, both lists one picture, both references missing — with vectors exactly 3 or exactly 4 quarter samples apart in one
component of one pair, so that every comparison of derive_boundaryStrength's motion part (deblock.cc:294-361, d_boundary_strength in
csrc/k_deblock_dev.h) decides edges alone, in smooth content where the filter changes the segment if, and only if, bS is 1.  On the
generator's own motion these lines return 1 for all but a handful of edges: of ten one-line mutants of the function
the other interpreter-tier deblocking tests let three through and catch four more in one case of one depth only.

Every case is three pictures from one configuration: the TWINS `d3` and `d4` (the deciding difference 3 / 4, everything else equal)
and `wrap` (d3 with one pair of units per region whose vectors are 65533 apart).  test_bs_census asserts, from the lists (bs_reference)
and the ORACLE'S planes before / after the stage alone, before any kernel runs:
  * a segment with bS 0 — compared motion, same PB, no edge — is silent, in all three pictures; no sample that is 3 away from the
    8-grid in both directions changed (nothing is filtered off the grid: the 4 / 12 AMP edges);
  * every compared class has >= 8 segments with outcome 1 in d4 and >= 8 with outcome 0 in d3, in each direction the plan gives it
    (band_plan: classes one unit row high have vertical edges only);
  * per class the segments of d4 that ONE test decided reach both components, both signs and both pairs, >= 2 each;
  * TWO_SAME: >= 8 segments far-and-far (1), >= 4 far / near, >= 4 near / far, >= 4 near-and-near (0, in d3);
  * >= 90 % of the compared segments with bS 1 in d4 are live, and >= 90 % of those that are 0 in d3 and 1 in d4 (>= 80 of them);
  * an internal PB edge on the grid, coded on both sides and no TU edge, occurs (>= 4 segments, bS 0); a coded one that is a TU edge too;
    >= 2 AMP units (internal edge at 4 / 12 of a 16x16 unit, off the grid, a step of S across it; at 8 / 24 of a 32x32 unit);
  * the cases with slices, tiles without filtering across them, intra / PCM / bypass units are there for what takes edges away or makes
    them bS 2: >= 8 borders of two units that are no edge (silent, with a step), >= 8 segments per direction between a PB and an intra
    unit, >= 4 beside a PCM unit, >= 20 changed samples per chroma plane; of the class conditions they keep the liveness ones;
  * wrap: >= 4 pairs' own segments (65533 decided alone), all of them live.
(16 own segments of the wrap pairs = four pairs of the five or six a plan holds: a pair is lost where one of its units is coded.
80 flips: 6 classes x 2 directions x 8 segments less the one-row bands; 90 % as the issue of this test set it.)

CPU tier: oracle == the reference's own functions on the same lists (scalar and SSE tables); kernels under the SIMT interpreter == oracle
          at pipeline depth 1 and 3, with SAO off and on; the tile-column case through two ranks (lockstep phases and the in-process
          group): there the block across the tile column is a record injected by k_shard.hip.
GPU tier: the HIP kernels == oracle, the same; the two-rank lockstep driver of test_gpu_shard.py on the tile-column case.

CENSUS of the seeds below — per class `segments with outcome 1 in d4 / with outcome 0 in d3` (both directions together), then live / all:
  case                   ONE_STR ONE_CRO TWO_STR TWO_CRO TWO_SAME FILL    | bS 1 live | flips live | wrap own | coded internal: no TU edge, TU edge
  8bit                   20/24   24/24   28/32   20/20   40/60    64/64   | 196/196   | 192/192    | 20/20    | 8, 8
  10bit                  28/40   28/28   28/40   28/28   44/84    40/56   | 196/196   | 188/188    | 16/16    | 8, 8
  12bit                  28/48   28/28   28/44   28/28   44/72    40/56   | 196/196   | 188/188    | 20/20    | 8, 8
  16bit                  20/36   24/24   28/40   28/28   32/64    52/56   | 184/184   | 180/180    | 16/16    | 8, 8
  10bit_444              20/32   28/28   28/48   28/28   44/76    44/64   | 192/192   | 184/184    | 16/16    | 8, 8
  8bit_mono              20/20   24/24   28/56   28/28   44/64    44/60   | 188/188   | 180/180    | 16/16    | 8, 8
  10bit_ctb16            28/44   28/28   28/52   16/16   44/72    52/72   | 196/196   | 188/188    | 16/16    | 8, 8
  8bit_cu32              40/56   48/48   56/112  56/56   88/168   104/152 | 392/392   | 376/376    | 24/24    | 16, 16
  tiles2x1               56/100  60/60   84/116  208/192 96/208   60/80   | 564/564   | 508/508    | 16/16    | 8, 8
  tiles2x1_no_lf_across  56/92   56/56   80/128  200/184 88/168   56/76   | 536/536   | 480/480    | 20/20    | 8, 8
  slices3                20/32   24/24   28/40   28/28   16/20    24/32   | 140/140   | 136/136    | 12/12    | 8, 8
  10bit_intra_pcm        16/20   24/24   12/20   4/4     24/40    8/12    | 88/88     | 84/84      | 12/12    | 8, 0
Every compared segment with bS 1 is live and every one with bS 0 silent, at every depth: 4 levels of step are enough for the normal
filter (tc >= 1 at QP 22..37 with the first slice's offsets) and the ramp keeps d below beta.  AMP units: 2..13 per picture."""
import pytest

import bs_motion_content as B
from oracle_py import Oracle
from shard_util import group_sharded_decode, local_sharded_decode
from synth_util import assert_planes_equal, device_decode, oracle_decode
from test_emu_picture import emu_lib  # noqa: F401  (fixture)
from libde265_amd import capi, worklist as W

NO_DEBLOCK = W.STAGE_INTER | W.STAGE_RESIDUAL | W.STAGE_INTRA
NO_SAO = W.STAGE_ALL & ~W.STAGE_SAO
VARIANTS = (("d3", 3, False), ("d4", 4, False), ("wrap", 3, True))
ACROSS = W.SF_LF_ACROSS_SLICES | W.SF_SAO_LUMA | W.SF_SAO_CHROMA

# id -> (generator configuration over bs_motion_content.BASE, plan, slice flags).  The generator's default CTB is 64: 128x96 is one
# and a half CTB rows.  cu32: 32x32 units (the AMP edges at 8 / 24 are on the grid), 256x192 to keep 8 x 6 units.
CASES = {
    "8bit": (dict(width=128, height=96, bit_depth=8, seed=10008), B.default_plan, None),
    "10bit": (dict(width=128, height=96, bit_depth=10, seed=9010), B.default_plan, None),
    "12bit": (dict(width=128, height=96, bit_depth=12, seed=9012), B.default_plan, None),
    "16bit": (dict(width=128, height=96, bit_depth=16, seed=9016), B.default_plan, None),
    "10bit_444": (dict(width=128, height=96, bit_depth=10, chroma_format=3, seed=9103), B.default_plan, None),
    "8bit_mono": (dict(width=128, height=96, bit_depth=8, chroma_format=4, seed=9104), B.default_plan, None),
    "10bit_ctb16": (dict(width=128, height=96, bit_depth=10, log2_ctb=4, seed=11204), B.default_plan, None),
    "8bit_cu32": (dict(width=256, height=192, bit_depth=8, fixed_cu_log2=5, seed=10305), B.default_plan, None),
    "tiles2x1": (dict(width=256, height=128, bit_depth=8, tile_cols=2, seed=9401), B.band_plan, None),
    "tiles2x1_no_lf_across": (dict(width=256, height=128, bit_depth=10, tile_cols=2, lf_across_tiles=0, seed=9402), B.band_plan, None),
    # three slices: the second with deblocking disabled, the third without filtering across its borders
    "slices3": (dict(width=128, height=96, bit_depth=8, log2_ctb=4, n_slices=3, seed=9503), B.default_plan,
                [ACROSS, ACROSS | W.SF_DEBLOCK_DISABLED, ACROSS & ~W.SF_LF_ACROSS_SLICES]),
    # a third of the units intra, some of them PCM, some units cu_transquant_bypass: bS 2 beside a PB, the chroma filter runs
    "10bit_intra_pcm": (dict(width=128, height=96, bit_depth=10, intra_pct=35, features=2 + 8, seed=9606), B.default_plan, None),
}
IDS = list(CASES)
SHARDED = ("tiles2x1", "tiles2x1_no_lf_across")
# cases whose slices / tiles take edges away from the plan are there for what they take away: class reach is asserted on the others
REACH = [c for c in IDS if c not in ("slices3", "10bit_intra_pcm")]
SUPPRESSED = ("slices3", "tiles2x1_no_lf_across")
BESIDE_INTRA = ("10bit_intra_pcm",)

_cache = {}


def prepared(oracle_lib, cid):
    """{variant: (picture, references, {stages: oracle planes}, segments with `live`, census counts, plan)}; made once, never modified"""
    if cid not in _cache:
        cfg, plan, slice_flags = CASES[cid]
        o = Oracle(oracle_lib)
        made = {}
        for name, delta, wrap in VARIANTS:
            pic, refs, regions = B.make_bs_case(delta, plan=plan, wrap=wrap, slice_flags=slice_flags, **cfg)
            want = dict((st, oracle_decode(o, pic, refs, st)) for st in (NO_DEBLOCK, NO_SAO, W.STAGE_ALL))
            segs, counts = B.bs_census(pic, want[NO_DEBLOCK], want[NO_SAO])
            made[name] = (pic, refs, want, segs, counts, regions)
        _cache[cid] = made
    return _cache[cid]


def _n(segs, **kw):
    return [s for s in segs if all((s[k] if k in s else (s["info"] or {}).get(k)) == v for k, v in kw.items())]


def census_line(cid, made):
    """the figures of one case as the module's header lists them"""
    d3, d4, wr = made["d3"][3], made["d4"][3], made["wrap"][3]
    cmp4 = [s for s in d4 if s["cls"] in B.COMPARED]
    flips = [b for a, b in zip(d3, d4) if a["bs"] == 0 and b["bs"] == 1]
    own = [s for s in wr if s["info"] and s["info"]["short"] != s["bs"]]
    per = " ".join("%s %d/%d" % (B.NAMES[c][:3] + B.NAMES[c][-3:], len(_n(d4, cls=c, outcome=1)), len(_n(d3, cls=c, outcome=0))) for c in B.COMPARED)
    return "%-22s %s | bS1 live %d/%d flips live %d/%d wrap own %d/%d | coded internal no-TU %d, TU %d" % (
        cid, per, sum(s["live"] for s in cmp4 if s["bs"]), sum(1 for s in cmp4 if s["bs"]), sum(s["live"] for s in flips), len(flips),
        sum(s["live"] for s in own), len(own), len([s for s in d4 if s["internal"] and s["nz"] and s["cls"] in B.COMPARED]),
        len([s for s in d4 if s["internal"] and s["cls"] == B.CODED_TU_EDGE]))


def check_conditions(cid, made):
    """the conditions of the module's header"""
    print(census_line(cid, made))
    d3, d4, wr = made["d3"][3], made["d4"][3], made["wrap"][3]
    for name in made:
        segs, want = made[name][3], made[name][2]
        loud = [s for s in segs if s["bs"] == 0 and s["live"]]
        assert not loud, "%s %s: %d segments with bS 0 changed, first %s at (%d, %d)" % (cid, name, len(loud), B.NAMES[loud[0]["cls"]], loud[0]["x"], loud[0]["y"])
        ch = want[NO_DEBLOCK][0] != want[NO_SAO][0]
        assert not ch[3::8][:, 3::8].any() and not ch[4::8][:, 4::8].any() and not ch[3::8][:, 4::8].any() and not ch[4::8][:, 3::8].any(), "%s %s: a sample off the grid changed" % (cid, name)
    if cid in SUPPRESSED:
        # borders of two units that are no edge (a slice with the filter disabled, a slice or tile border it may not cross): silent
        # (above), although the checkerboard puts a step there
        n = len([s for s in d4 if s["cls"] == B.NO_EDGE and not s["internal"]])
        assert n >= 8, "%s: only %d segments between two units are no edge" % (cid, n)
    if cid in BESIDE_INTRA:
        for vertical in (True, False):
            n = len([s for s in d4 if s["cls"] == B.INTRA and s["vertical"] == vertical and s["inter_side"]])
            assert n >= 8, "%s: only %d segments between a PB and an intra unit (vertical %s)" % (cid, n, vertical)
        n = len([s for s in d4 if s["cls"] == B.INTRA and s["inter_side"] and s["pcm_side"]])
        assert n >= 4, "%s: only %d segments between a PB and a PCM unit" % (cid, n)
        for c in (1, 2):
            n = int((made["d4"][2][NO_DEBLOCK][c] != made["d4"][2][NO_SAO][c]).sum())
            assert n >= 20, "%s: the chroma filter changed only %d samples of plane %d" % (cid, n, c)
    if cid in REACH:
        cus = made["d4"][0].cus
        amp = cus[cus["part_mode"] >= 4]
        assert len(amp) >= 2, "%s: only %d AMP units (their internal edge is off the 8-grid in a 16x16 unit, at 8 / 24 in a 32x32 one)" % (cid, len(amp))
        regions = made["d4"][5]
        cu = 1 << dict(B.BASE, **CASES[cid][0])["fixed_cu_log2"]
        for cls in B.COMPARED:
            tall = any(r[4] == cls and r[3] - r[1] >= 2 * cu for r in regions)
            for vertical in (True, False) if tall else (True,):
                n1, n0 = len(_n(d4, cls=cls, outcome=1, vertical=vertical)), len(_n(d3, cls=cls, outcome=0, vertical=vertical))
                assert n1 >= 8 and n0 >= 8, "%s: %s has %d segments with outcome 1 in d4, %d with 0 in d3 (vertical %s)" % (cid, B.NAMES[cls], n1, n0, vertical)
            sole = [s["info"]["decider"] for s in d4 if s["cls"] == cls and s["info"]["mag"] == 4 and s["bs"] == 1]
            for what, pos in (("component", 0), ("sign", 1), ("pair", 2)):
                for v in ((1, -1) if pos == 1 else (0, 1)):
                    n = sum(1 for dcd in sole if dcd[pos] == v)
                    assert n >= 2, "%s: %s: only %d segments decided alone by %s %d" % (cid, B.NAMES[cls], n, what, v)
        same = [s for s in d4 + d3 if s["cls"] == B.TWO_SAME]
        for conj, bs, least in (((True, True), 1, 8), ((True, False), 0, 4), ((False, True), 0, 4), ((False, False), 0, 4)):
            n = sum(1 for s in same if s["info"]["conj"] == conj and s["bs"] == bs)
            assert n >= least, "%s: TWO_SAME: %d segments with the conjuncts %s" % (cid, n, conj)
        assert len([s for s in d4 if s["internal"] and s["nz"] and s["cls"] in B.COMPARED and s["bs"] == 0]) >= 4, "%s: no coded internal PB edge that is no TU edge" % cid
        assert len([s for s in d4 if s["internal"] and s["cls"] == B.CODED_TU_EDGE]) >= 4, "%s: no coded internal PB edge that is a TU edge" % cid
        own = [s for s in wr if s["info"] and s["info"]["short"] != s["bs"]]
        assert len(own) >= 16 and all(s["live"] for s in own), "%s: %d segments whose outcome differences taken in 16 bits would change, %d live" % (cid, len(own), sum(s["live"] for s in own))
    ones = [s for s in d4 if s["cls"] in B.COMPARED and s["bs"] == 1]
    assert sum(s["live"] for s in ones) * 10 >= 9 * len(ones), "%s: %d of %d compared segments with bS 1 are live" % (cid, sum(s["live"] for s in ones), len(ones))
    flips = [b for a, b in zip(d3, d4) if a["bs"] == 0 and b["bs"] == 1]
    assert len(flips) >= (80 if cid in REACH else 20) and sum(s["live"] for s in flips) * 10 >= 9 * len(flips), "%s: %d segments flip between the twins, %d live" % (cid, len(flips), sum(s["live"] for s in flips))


@pytest.mark.parametrize("cid", IDS)
def test_bs_census(oracle, cid):
    check_conditions(cid, prepared(oracle, cid))


@pytest.mark.parametrize("cid", IDS)
def test_bs_oracle_equals_reference_replay(oracle, ref, cid):
    from ref_replay_py import ref_replay
    for name, (pic, refs, want, _, _, _) in prepared(oracle, cid).items():
        for st in (NO_DEBLOCK, NO_SAO):
            assert_planes_equal(want[st], ref_replay(ref, pic, refs, st, accel=0), "%s: oracle vs scalar reference, stages %d" % (name, st))
        assert_planes_equal(want[NO_SAO], ref_replay(ref, pic, refs, NO_SAO, accel=1), "%s: oracle vs SSE reference, SAO off" % name)


def check_kernels(ctx, made, what):
    for name, (pic, refs, want, _, _, _) in made.items():
        ctx.set_pipeline_depth(1)
        assert_planes_equal(device_decode(ctx, pic, refs, NO_SAO), want[NO_SAO], "%s %s: kernels vs oracle, SAO off" % (what, name))
        assert_planes_equal(device_decode(ctx, pic, refs), want[W.STAGE_ALL], "%s %s: kernels vs oracle, all stages" % (what, name))
        ctx.set_pipeline_depth(3)
        try:
            assert_planes_equal(device_decode(ctx, pic, refs, NO_SAO, resident=True, repeat=3), want[NO_SAO], "%s %s: depth 3, SAO off" % (what, name))
            assert_planes_equal(device_decode(ctx, pic, refs, resident=True, repeat=3), want[W.STAGE_ALL], "%s %s: depth 3, all stages" % (what, name))
        finally:
            ctx.set_pipeline_depth(1)


@pytest.mark.parametrize("cid", IDS)
def test_bs_emulated(emu_lib, oracle, cid):  # noqa: F811
    made = prepared(oracle, cid)
    check_conditions(cid, made)
    ctx = capi.Context(emu_lib, 0)
    try:
        check_kernels(ctx, made, cid)
    finally:
        ctx.close()


@pytest.mark.parametrize("cid", SHARDED)
def test_bs_sharded_emulated(emu_lib, oracle, cid):  # noqa: F811
    """two ranks, one tile each: P of every edge on the tile column is a record that k_shard.hip injected"""
    for name, (pic, refs, want, segs, _, _) in prepared(oracle, cid).items():
        if int(pic.pp[0]["flags"]) & W.PF_LF_ACROSS_TILES:
            col = [s for s in segs if s["vertical"] and s["x"] == int(pic.pp[0]["width"]) // 2 and s["cls"] in B.COMPARED]
            reached = set(s["cls"] for s in col if s["bs"] == (1 if name == "d4" else 0))
            assert reached == set(B.COMPARED), "%s %s: the tile column reaches only the classes %s" % (cid, name, sorted(reached))
        for r, got in enumerate(local_sharded_decode(emu_lib, pic, refs, 2, stages=NO_SAO)):
            assert_planes_equal(got, want[NO_SAO], "%s %s: lockstep rank %d, SAO off" % (cid, name, r))
        for r, got in enumerate(group_sharded_decode(emu_lib, pic, refs, 2, repeat=2)):
            assert_planes_equal(got, want[W.STAGE_ALL], "%s %s: group rank %d" % (cid, name, r))


@pytest.fixture(scope="module")
def gpu_ctx():
    lib = capi.Library()
    assert lib.device_count() >= 1
    c = capi.Context(lib, 0)
    yield c
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cid", IDS)
def test_bs_gpu(gpu_ctx, oracle, cid):
    made = prepared(oracle, cid)
    check_conditions(cid, made)
    check_kernels(gpu_ctx, made, cid)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", SHARDED)
def test_bs_sharded_gpu(oracle, cid):
    lib = capi.Library()
    for name, (pic, refs, want, _, _, _) in prepared(oracle, cid).items():
        for r, got in enumerate(local_sharded_decode(lib, pic, refs, 2, device="cuda:0", repeat=2)):
            assert_planes_equal(got, want[W.STAGE_ALL], "%s %s: lockstep rank %d" % (cid, name, r))
