"""The residual and intra stages on content that stays IN RANGE (tests/residual_content.py): the generator's levels divided down until most of
what k_residual computes reaches the picture unclipped, beside blocks that still saturate.  On the generator's own levels 76-84 % of the samples
an 8-bit residual block writes are clipped (census below): the final Clip(pred + r) hides a transform that is off by one, a dropped rounding
term, an RDPCM sum that starts late, and k_intra then predicts from borders of 0 and maxv, on which every interpolation weight gives the same
answer.

Every case first asserts FROM THE ORACLE'S PLANES ALONE (residual_census / border_census; conditions on the input, so that a change of the
generator cannot empty the test), for the residual blocks that are added to the picture (in the all-intra cases, which have none: for the intra
blocks that carry a residual):
  per block size present:  >= 8 blocks;  unclipped samples (0 < recon < maxv) >= 60 %;  blocks without a clipped sample >= 25 % and >= 4;
                           recon != pred in >= 50 % of the samples (not in the all-intra cases: an intra block's prediction never reaches a plane)
  intra blocks beside them: unclipped samples >= 60 %, all sizes together (a quarter of the CUs: too few blocks for a count per size)
  the case:                clipped samples >= 3 % of the samples of all these blocks (the clip stays exercised)
  intra blocks >= 8x8:     >= 8 of them; borders of one single value that is 0 or maxv <= 2 % of them
  and what the case is named after is IN its lists (check_features).

Census of the seeds in this file (oracle planes; "unclipped" over all block sizes of a case, blocks without a clipped sample of all blocks):
  residual blocks added to the picture   with the generator's levels          with attenuate_levels
    8-bit cases                          9-47 % unclipped,   0-28 % of blocks   76-95 % unclipped, 42-87 % of blocks
    9 / 10-bit cases, mixed 9 / 12       13-51 %,            0-23 %             74-95 %,           50-87 %
    12 bits / 16 bits                    60 % / 76 %,        22 % / 16 %        91 % / 85 %,       73 % / 46 %
  intra blocks with a residual           10-50 % (12 bits 75 %, 16 bits 85 %)   68-99 %
  recon != pred in 67-99 % of the samples of the added blocks; 4-24 % of the samples of a case still clip (the full-int16 blocks saturate at any
  shift; 20-89 % with the generator's levels).  Single-valued intra borders at 0 / maxv: 0-2 of 20-177 blocks (10 of 144 in 8bit_all_intra with
  the generator's levels).
Per case — unclipped samples and blocks without a clipped sample / blocks, for the blocks added to the picture and for the intra blocks with a
residual; recon != pred; intra borders (>= 8x8) single-valued at 0 or maxv / all:
  case                       added blocks      intra blocks      r!=p   border | the same with the generator's levels
  8bit_420                    88 %  178/247    86 %  127/220    93 %   2/101 |  14 %    3/247    18 %    1/220    97 %   2/101
  8bit_420_cu32               85 %   41/58     79 %   20/39     92 %   0/66  |  14 %    1/58     12 %    0/39     98 %   0/66
  8bit_420_cu64               95 %   50/57     95 %   20/23     87 %   0/36  |  18 %    0/57     12 %    0/23     97 %   0/36
  9bit_420                    87 %   50/70     83 %   20/34     92 %   0/54  |  17 %    1/70     20 %    0/34     94 %   3/54
  10bit_420                   87 %  209/269    90 %  175/221    91 %   0/65  |  27 %   13/269    34 %   16/221    92 %   0/65
  10bit_420_cu64              95 %   27/31     75 %   16/21     95 %   0/36  |  44 %    1/31     30 %    0/21     99 %   0/36
  12bit_420                   91 %   49/67     99 %   34/39     92 %   0/72  |  60 %   15/67     75 %    2/39     94 %   0/72
  10bit_422                   90 %   94/116    88 %   74/111    97 %   0/170 |  28 %    0/116    35 %    0/111    99 %   0/170
  10bit_444_ccp               74 %   42/84     76 %   19/51     92 %   0/69  |  30 %    1/84     39 %    0/51     95 %   0/69
  8bit_mono                   77 %   14/22     85 %   11/16     87 %   0/20  |  14 %    0/22     10 %    0/16     94 %   0/20
  16bit_420                   85 %   25/54     93 %   29/44     96 %   0/78  |  76 %    9/54     85 %   16/44     96 %   1/78
  mixed_9_12                  91 %   42/51     94 %   12/15     94 %   0/33  |  34 %   12/51     32 %    2/15     96 %   0/33
  8bit_scaling_list           76 %   15/35     86 %    8/18     99 %   0/36  |   9 %    0/35     12 %    0/18     99 %   0/36
  8bit_rdpcm_rotate_bypass    80 %  221/298    81 %  170/259    67 %   1/177 |  30 %   46/298    20 %   19/259    70 %   2/177
  8bit_dequantized            89 %   48/73     92 %   47/67     84 %   0/120 |  47 %   21/73     40 %    7/67     93 %   0/120
  8bit_qp_wide                90 %   54/67     85 %   22/32     67 %   0/57  |  39 %    2/67     46 %    1/32     96 %   0/57
  8bit_all_intra             -                  88 %   63/91      -     0/144 | -                  10 %    0/91      -    10/144
  8bit_tiles2x2_slices3       80 %   51/77     91 %   23/29     89 %   0/51  |  12 %    0/77     18 %    0/29     95 %   0/51
  10bit_scaling_list          84 %   22/35     95 %   18/24     99 %   0/36  |  13 %    0/35     16 %    0/24    100 %   0/36
  10bit_rdpcm_rotate_bypass   82 %  352/475    93 %  424/534    78 %   0/159 |  43 %   53/475    50 %   57/534    79 %   1/159
  10bit_dequantized           85 %   37/51     93 %   33/43     90 %   0/72  |  51 %   12/51     39 %    1/43     93 %   0/72
  10bit_qp_wide               86 %   37/56     84 %   35/57     82 %   0/87  |  45 %    7/56     37 %    2/57     94 %   1/87
  10bit_all_intra            -                  84 %   57/90      -     0/144 | -                  31 %    0/90      -     3/144
  10bit_tiles2x2_slices3      93 %   43/54     68 %   12/18     94 %   0/24  |  40 %    4/54     18 %    1/18     99 %   0/24
The level shift per depth is residual_content.SHIFT (7 at 8 bits, 6 at 9 and 10, 5 at 12, 2 at 16); levels that are coefficients already
(RBF_DEQUANTIZED) take PRESCALED_SHIFT.

CPU tier: oracle == the reference's scalar and SSE functions (oracle/_ref replay) == the kernels under the SIMT interpreter at pipeline
          depths 1 and 3.
GPU tier: the HIP kernels == oracle at depths 1 and 3; three all-intra configurations through m355_decode_batch; CHAIN_CASES under the forced
          chain schedules (test_gpu_chain_forced.py)."""
import pytest

from oracle_py import Oracle
from residual_content import SHIFT, attenuate_levels, border_census, residual_census
from synth_util import assert_planes_equal, device_decode, make_case, oracle_decode
from test_emu_picture import emu_lib  # noqa: F401  (fixture)
from libde265_amd import capi, synth, worklist as W

ST_PRED = W.STAGE_INTER
ST_RES = W.STAGE_INTER | W.STAGE_RESIDUAL
ST_INTRA = W.STAGE_INTER | W.STAGE_RESIDUAL | W.STAGE_INTRA
STAGES = (ST_PRED, ST_RES, ST_INTRA, W.STAGE_ALL)

RDPCM = synth.SYN_RDPCM | synth.SYN_ROTATE | synth.SYN_TRANSQUANT_BYPASS
# 256x192: 12 CTBs of 64.  "mix": the generator's own choice of CU sizes (4x4 .. 32x32 blocks); "cu32" / "cu64": CUs of one size, for 16x16 and
# 32x32 blocks in numbers (a 64x64 CU is four 32x32 transform blocks, a third of the 32x32 ones split once more)
BASE = dict(width=256, height=192, intra_pct=25, cbf_pct=60)


def _case(cid, **cfg):
    cfg = dict(BASE, **cfg)
    cfg["seed"] = cfg.get("seed", 0) + 1000 * SEED_STEP.get(cid, 0)
    return cid, cfg


# seeds: + 1000 * SEED_STEP where the census of that seed fell short of the conditions above
SEED_STEP = {"8bit_420": 1, "8bit_420_cu32": 4, "10bit_420": 3, "12bit_420": 1, "10bit_422": 5, "8bit_mono": 4, "mixed_9_12": 3, "8bit_scaling_list": 2,
             "8bit_dequantized": 2, "8bit_qp_wide": 5, "10bit_rdpcm_rotate_bypass": 1, "10bit_qp_wide": 1, "10bit_tiles2x2_slices3": 1}

CASES = [
    _case("8bit_420", bit_depth=8, chroma_format=1, seed=9101),
    _case("8bit_420_cu32", bit_depth=8, chroma_format=1, fixed_cu_log2=5, seed=9102),
    _case("8bit_420_cu64", bit_depth=8, chroma_format=1, fixed_cu_log2=6, seed=9103),
    _case("9bit_420", bit_depth=9, chroma_format=1, fixed_cu_log2=5, seed=9104),
    _case("10bit_420", bit_depth=10, chroma_format=1, seed=9105),
    _case("10bit_420_cu64", bit_depth=10, chroma_format=1, fixed_cu_log2=6, seed=9106),
    _case("12bit_420", bit_depth=12, chroma_format=1, fixed_cu_log2=5, seed=9107),
    _case("10bit_422", bit_depth=10, chroma_format=2, fixed_cu_log2=5, seed=9108),
    _case("10bit_444_ccp", bit_depth=10, chroma_format=3, features=synth.SYN_CROSS_COMPONENT, fixed_cu_log2=5, seed=9109),
    _case("8bit_mono", bit_depth=8, chroma_format=4, fixed_cu_log2=5, seed=9110),
    _case("16bit_420", bit_depth=16, chroma_format=1, fixed_cu_log2=5, seed=9111),
    _case("mixed_9_12", bit_depth=9, bit_depth_chroma=12, chroma_format=1, fixed_cu_log2=5, seed=9112),
]
for _bd in (8, 10):
    CASES += [
        _case("%dbit_scaling_list" % _bd, bit_depth=_bd, features=synth.SYN_SCALING_LIST, fixed_cu_log2=6, seed=9120 + _bd),
        _case("%dbit_rdpcm_rotate_bypass" % _bd, bit_depth=_bd, chroma_format=3, features=RDPCM, seed=9140 + _bd),
        _case("%dbit_dequantized" % _bd, bit_depth=_bd, features=synth.SYN_DEQUANTIZED, fixed_cu_log2=5, seed=9160 + _bd),
        _case("%dbit_qp_wide" % _bd, bit_depth=_bd, qp_wide=1, fixed_cu_log2=5, seed=9180 + _bd),
        _case("%dbit_all_intra" % _bd, bit_depth=_bd, intra_pct=100, n_refs=0, fixed_cu_log2=6, seed=9200 + _bd),
        _case("%dbit_tiles2x2_slices3" % _bd, bit_depth=_bd, tile_cols=2, tile_rows=2, n_slices=3, fixed_cu_log2=5, seed=9220 + _bd),
    ]
IDS = [c[0] for c in CASES]
_BY_ID = dict(CASES)
# (also run by test_gpu_chain_forced.py under the forced chain schedules, through make_inrange_case)
CHAIN_CASES = [_BY_ID[i] for i in ("8bit_420", "10bit_444_ccp", "12bit_420")]
# all-intra configurations for m355_decode_batch (three pictures each, seeds 37 apart: batch_picture)
BATCH_CFGS = [dict(width=128, height=64, bit_depth=8, chroma_format=1, seed=9301, cbf_pct=60, fixed_cu_log2=5),
              dict(width=128, height=64, bit_depth=10, chroma_format=2, seed=9302, cbf_pct=60, fixed_cu_log2=6),
              dict(width=128, height=64, bit_depth=12, chroma_format=3, seed=9303, cbf_pct=60, fixed_cu_log2=5)]
# (seed of the configuration, picture) -> seed step, as SEED_STEP
BATCH_STEP = {(9301, 0): 3, (9301, 1): 24, (9301, 2): 3, (9302, 0): 1, (9302, 1): 8, (9303, 0): 2, (9303, 1): 2}
# levels that are coefficients already (RBF_DEQUANTIZED) skip the dequantiser's gain: shifted like the others, three of four such blocks of an
# 8-bit picture would add a residual of zero (measured: 9 of 35 changed a sample with shift 7, 33 of 35 with shift 2)
PRESCALED_SHIFT = 2


def level_shift(cfg):
    """the shift of a configuration: its luma depth's"""
    return SHIFT[cfg["bit_depth"]]


def make_inrange_case(**cfg):
    """synth_util.make_case with the levels attenuated"""
    pic, refs = make_case(**cfg)
    return attenuate_levels(pic, level_shift(cfg), PRESCALED_SHIFT), refs


def census_lines(cen, brd):
    out = []
    for kind in ("inter", "intra"):
        for l2, e in sorted(cen[kind].items()):
            out.append("%s %2d: blocks %4d clip-free %4d (%3d %%)  unclipped %3d %%  changed %3d %%" % (
                kind, 1 << l2, e["blocks"], e["clip_free"], 100 * e["clip_free"] // e["blocks"], 100 * e["unclipped"] // e["samples"],
                100 * e["changed"] // e["samples"]))
    out.append("borders: %d intra blocks >= 8x8, %d single-valued, %d at 0 / maxv" % (brd["blocks"], brd["single"], brd["extreme"]))
    return out


def census_failures(cen, brd, min_blocks=8):
    """the conditions of the module's header -> the list of those that do not hold"""
    bad = []
    samples = clipped = 0
    kinds = ("inter", "intra") if not cen["inter"] else ("inter",)
    if cen["inter"] and cen["intra"]:
        n, u = (sum(e[k] for e in cen["intra"].values()) for k in ("samples", "unclipped"))
        samples, clipped = n, n - u
        if u * 100 < 60 * n:
            bad.append("intra: %d of %d samples unclipped" % (u, n))
    for kind in kinds:
        for l2, e in sorted(cen[kind].items()):
            what = "%s %dx%d" % (kind, 1 << l2, 1 << l2)
            samples += e["samples"]
            clipped += e["samples"] - e["unclipped"]
            if e["blocks"] < min_blocks:
                bad.append("%s: only %d blocks" % (what, e["blocks"]))
            if e["unclipped"] * 100 < 60 * e["samples"]:
                bad.append("%s: %d of %d samples unclipped" % (what, e["unclipped"], e["samples"]))
            if e["clip_free"] * 100 < 25 * e["blocks"] or e["clip_free"] < 4:
                bad.append("%s: %d of %d blocks without a clipped sample" % (what, e["clip_free"], e["blocks"]))
            if kind == "inter" and e["changed"] * 100 < 50 * e["samples"]:
                bad.append("%s: recon != pred in %d of %d samples" % (what, e["changed"], e["samples"]))
    if not samples:
        bad.append("no residual blocks")
    elif clipped * 100 < 3 * samples:
        bad.append("only %d of %d samples clipped" % (clipped, samples))
    if brd["blocks"] < min_blocks:
        bad.append("only %d intra blocks of 8x8 and larger" % brd["blocks"])
    if brd["extreme"] * 100 > 2 * brd["blocks"]:
        bad.append("%d of %d intra borders are single-valued at 0 / maxv" % (brd["extreme"], brd["blocks"]))
    return bad


def case_census(want, pic):
    return residual_census(want[ST_PRED], want[ST_RES], pic, want[ST_INTRA]), border_census(want[ST_INTRA], pic)


def check_features(cid, pic):
    """what a case is named after must be in its lists"""
    r = pic.rbs
    f, k = r["flags"], r["kind"]
    if "scaling_list" in cid:
        assert pic.scaling_factors is not None and int(pic.pp[0]["flags"]) & W.PF_SCALING_LIST
    if "rdpcm" in cid:
        for what, n in (("RDPCM_H", (f & W.RBF_RDPCM_H) != 0), ("RDPCM_V", (f & W.RBF_RDPCM_V) != 0), ("rotated", (f & W.RBF_ROTATE) != 0),
                        ("bypass", k == W.RK_BYPASS), ("skip 16x16 and larger", (k == W.RK_SKIP) & (r["log2_size"] >= 4))):
            assert int(n.sum()) >= 8, "%s: only %d %s blocks" % (cid, int(n.sum()), what)
    if "dequantized" in cid:
        assert int(((f & W.RBF_DEQUANTIZED) != 0).sum()) >= 8
    if "ccp" in cid:
        assert int(((r["cidx"] > 0) & ((r["matrix_id"] >> 4) != 0)).sum()) >= 8, "%s: no cross-component prediction" % cid
    if "qp_wide" in cid:
        assert int(r["qp"].min()) < 19 and int(r["qp"].max()) > 37 + 6 * (int(pic.pp[0]["bit_depth_luma"]) - 8) - 6
    if "tiles" in cid:
        assert int(pic.pp[0]["num_tile_cols"]) == 2 and int(pic.pp[0]["num_tile_rows"]) == 2 and len(pic.slices) >= 2


_cache = {}


def prepared(oracle_lib, cid):
    """(picture, references, oracle planes {stages: planes}) of a case, its census checked; made once, never modified"""
    if cid not in _cache:
        o = Oracle(oracle_lib)
        pic, refs = make_inrange_case(**_BY_ID[cid])
        _cache[cid] = (pic, refs, dict((st, oracle_decode(o, pic, refs, st)) for st in STAGES))
    pic, refs, want = _cache[cid]
    check_features(cid, pic)
    cen, brd = case_census(want, pic)
    bad = census_failures(cen, brd)
    assert not bad, "%s: %s\n%s" % (cid, "; ".join(bad), "\n".join(census_lines(cen, brd)))
    return pic, refs, want


def batch_picture(cfg, k, step=None):
    """picture k of a batch configuration: all-intra, its levels attenuated"""
    step = BATCH_STEP.get((cfg["seed"], k), 0) if step is None else step
    return attenuate_levels(synth.picture(**dict(cfg, intra_pct=100, n_refs=0, seed=cfg["seed"] + 37 * k + 1000 * step)), level_shift(cfg), PRESCALED_SHIFT)


def batch_pictures(oracle_lib, cfg, n):
    """n attenuated intra pictures of a batch configuration, each one's census checked (a picture of 128x64 has fewer blocks: >= 4 of a size)"""
    o = Oracle(oracle_lib)
    pics = [batch_picture(cfg, k) for k in range(n)]
    for k, pic in enumerate(pics):
        want = dict((st, oracle_decode(o, pic, [], st)) for st in (ST_PRED, ST_RES, ST_INTRA))
        cen, brd = case_census(want, pic)
        bad = census_failures(cen, brd, min_blocks=4)
        assert not bad, "batch picture %d: %s\n%s" % (k, "; ".join(bad), "\n".join(census_lines(cen, brd)))
    return pics


def test_attenuate_levels_rewrites_magnitudes_only():
    """positions, signs, counts and the entry width of every block stay; bypass blocks keep their levels; narrow blocks are read and written as such"""
    import numpy as np
    pic = synth.picture(width=128, height=64, bit_depth=8, seed=9401, features=synth.SYN_TRANSQUANT_BYPASS | synth.SYN_DEQUANTIZED, intra_pct=30)
    e0, n0 = W._wide_entries(pic)
    lv0 = (e0 >> 16).astype(np.uint16).view(np.int16).astype(np.int64)
    byp = np.repeat(pic.rbs["kind"] == W.RK_BYPASS, n0)
    pre = np.repeat((pic.rbs["flags"] & W.RBF_DEQUANTIZED) != 0, n0)
    assert byp.any() and pre.any() and (~byp & ~pre).any()
    want = np.where(byp, lv0, np.sign(lv0) * np.maximum(1, np.abs(lv0) >> np.where(pre, 2, 5)))
    wide = attenuate_levels(pic, 5, 2)
    packed = W.pack_narrow(wide)                                  # after the shift most blocks fit the 16-bit form
    assert ((packed.rbs["flags"] & W.RBF_NARROW) != 0).sum() >= 8 and len(packed.coeffs) < len(wide.coeffs)
    for got in (wide, packed, attenuate_levels(packed, 0)):
        e, n = W._wide_entries(got)
        assert np.array_equal(n, n0) and np.array_equal(e & 0xFFFF, e0 & 0xFFFF)
        assert np.array_equal((e >> 16).astype(np.uint16).view(np.int16).astype(np.int64), want)
    again = attenuate_levels(packed, 0)
    assert np.array_equal(again.rbs["flags"], packed.rbs["flags"]) and np.array_equal(again.coeffs, packed.coeffs)
    assert np.array_equal(pic.coeffs, synth.picture(**pic.meta["cfg"]).coeffs)            # the argument is left alone


@pytest.mark.parametrize("cid", IDS)
def test_inrange_oracle_equals_reference_replay(oracle, ref, cid):
    from ref_replay_py import ref_replay
    pic, refs, want = prepared(oracle, cid)
    for st in (ST_RES, ST_INTRA, W.STAGE_ALL):
        assert_planes_equal(want[st], ref_replay(ref, pic, refs, st, accel=0), "oracle vs scalar reference, stages %d" % st)
    # (the reference has SSE transforms and motion compensation for 8-bit samples only; at other depths its table keeps the scalar functions)
    assert_planes_equal(want[ST_INTRA], ref_replay(ref, pic, refs, ST_INTRA, accel=1), "oracle vs SSE reference")


@pytest.mark.parametrize("cid", IDS)
def test_inrange_emulated(emu_lib, oracle, cid):  # noqa: F811
    pic, refs, want = prepared(oracle, cid)
    ctx = capi.Context(emu_lib, 0)
    try:
        ctx.set_pipeline_depth(1)
        assert_planes_equal(device_decode(ctx, pic, refs, ST_RES), want[ST_RES], "kernels vs oracle, inter + residual, depth 1")
        assert_planes_equal(device_decode(ctx, pic, refs, ST_INTRA), want[ST_INTRA], "kernels vs oracle, no loop filters, depth 1")
        ctx.set_pipeline_depth(3)
        assert_planes_equal(device_decode(ctx, pic, refs, ST_INTRA, resident=True, repeat=3), want[ST_INTRA], "kernels vs oracle, no loop filters, depth 3")
        assert_planes_equal(device_decode(ctx, pic, refs), want[W.STAGE_ALL], "kernels vs oracle, all stages, depth 3")
    finally:
        ctx.close()


@pytest.mark.parametrize("cfg", BATCH_CFGS, ids=lambda c: "%dbit_cf%d" % (c["bit_depth"], c["chroma_format"]))
def test_inrange_decode_batch_emulated(emu_lib, oracle, cfg):  # noqa: F811
    from batch_util import check_batches
    pics = batch_pictures(oracle, cfg, 3)
    check_batches(emu_lib, Oracle(oracle), cfg, 3, [[0, 1, 2], [2, 0]], stages=ST_INTRA, pics=pics)[0].close()


@pytest.fixture(scope="module")
def gpu_ctx():
    lib = capi.Library()
    assert lib.device_count() >= 1
    c = capi.Context(lib, 0)
    yield c
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cid", IDS)
def test_inrange_gpu(gpu_ctx, oracle, cid):
    ctx = gpu_ctx
    pic, refs, want = prepared(oracle, cid)
    ctx.set_pipeline_depth(1)
    assert_planes_equal(device_decode(ctx, pic, refs, ST_RES), want[ST_RES], "HIP vs oracle, inter + residual, depth 1")
    assert_planes_equal(device_decode(ctx, pic, refs, ST_INTRA), want[ST_INTRA], "HIP vs oracle, no loop filters, depth 1")
    assert_planes_equal(device_decode(ctx, pic, refs), want[W.STAGE_ALL], "HIP vs oracle, all stages, depth 1")
    ctx.set_pipeline_depth(3)
    try:
        assert_planes_equal(device_decode(ctx, pic, refs, ST_INTRA, resident=True, repeat=4), want[ST_INTRA], "HIP vs oracle, no loop filters, depth 3")
        assert_planes_equal(device_decode(ctx, pic, refs, resident=True, repeat=4), want[W.STAGE_ALL], "HIP vs oracle, all stages, depth 3")
    finally:
        ctx.set_pipeline_depth(1)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", BATCH_CFGS, ids=lambda c: "%dbit_cf%d" % (c["bit_depth"], c["chroma_format"]))
def test_inrange_decode_batch_gpu(oracle, cfg):
    from batch_util import check_batches
    pics = batch_pictures(oracle, cfg, 3)
    lib = capi.Library()
    for st in (ST_INTRA, W.STAGE_ALL):
        check_batches(lib, Oracle(oracle), cfg, 3, [[0, 1, 2], [2, 0, 1], [1]], stages=st, pics=pics)[0].close()
