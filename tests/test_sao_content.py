"""Sample adaptive offset on content and parameters that reach band offsets, clipping and blocked edges (tests/sao_content.py): pictures
whose left part is small plateaus just above 0 and whose right part is plateaus just below maxv, decoded with band positions that
follow the content, offsets over the whole range of the depth and all four edge classes — so that the band arithmetic (bd - 5 shift,
& 31 wrap, min(k, 4)), both ends of the clip, all five entries of the edge table and the masked path (tile / slice borders, PCM and
bypass CUs) of k_sao's three code paths (packed 8-bit, packed 16-bit lanes up to 15 bits, one sample per operation at 16 bits) all
move samples in one picture, beside samples that are copied.

Up to 12 bits the content comes through inter prediction from sao_refs' reference planes.  From 13 bits on the reference's 16-bit
prediction intermediates halve or wrap bright samples (fractional vectors at 13 bits, every vector from 14), so there the pictures are
all-intra and the content comes from the raw samples of their PCM coding units (pcm_plateaus), carried on by intra prediction.

Every case first asserts FROM THE ORACLE'S PLANES ALONE (sao_census of the picture before / after the stage) that the stage did enough
of each kind of work (check_census; conditions on the input, so that a change of the generator cannot empty the test):
  each edge category 0, 1, 3, 4 (edgeIdx + 2):  >= 20 changed luma samples, >= 8 in each chroma plane
  band:                                         >= 200 luma, >= 50 in each chroma plane
  wrap (band index below band_pos):             >= 8 in at least one plane
  clip_lo, clip_hi, each:                       >= 20 luma, >= 8 in each chroma plane
  tiles / slices cases: held_border >= 8, held_skip >= 16 (luma)
  unchanged:                                    >= 25 % of every plane

CPU tier: kernels under the SIMT interpreter == oracle with all stages; oracle == the reference's own SAO (oracle/_ref replay, scalar);
          three all-intra batches through m355_decode_batch under the interpreter, one of them mixing 10 and 16 bits (the whole batch
          then takes the unpacked kernel).
GPU tier: the HIP kernels == oracle: one picture at a time, three in flight from resident lists; the batches.

Not covered: 8-bit luma with deeper chroma (the issue's "8 with 12").  A picture has ONE sample type, chosen by its luma depth, in the
kernels and in the generator's reference planes alike; such a picture cannot be made or decoded here at all, with or without SAO.

Census of the oracle's planes, luma (each chroma plane at least) — edge categories 0 / 1 / 3 / 4, band, wrap, clip_lo / clip_hi:
   8bit_cf1  362 152 157 368 (45)  band  504 (128)  wrap  503  clip 481 / 111 (55 / 30)
   9bit_cf1  506 213 148 537 (75)  band  713 (236)  wrap  587  clip 524 /  70 (37 / 37)
  10bit_cf1  400 215 249 397 (25)  band  446 (562)  wrap   96  clip  85 /  48 (74 / 140)
  11bit_cf1  161  52  71 133 (20)  band 2480 (503)  wrap 1131  clip 629 / 936 (253 / 8)
  12bit_cf1  865  25  45 869 (18)  band  635 (462)  wrap  144  clip 762 /  78 (36 / 68)
  13bit_cf1  178 267 275 209 (33)  band  872 (127)  wrap  808  clip 884 /  53 (27 / 83)
  15bit_cf1   60  78  61  68 (26)  band 2981 (452)  wrap 1726  clip 270 /  49 (97 / 82)
  16bit_cf1  125 181 156 151 (36)  band  863 (568)  wrap  314  clip 157 /  21 (241 / 43)
  held_border / held_skip (luma): tiles2x2_10bit 50 / 143, tiles2x2_16bit 42 / 380, slices3_8bit 11 / 17, slices3_16bit 17 / 267.

One-line mutations of k_sao.hip, interpreter tier — failing tests of this module's 45 emulated ones / of the 365 earlier emulated ones
(test_emu_*, test_batch_emu, test_deblock_smooth and the other *_emu modules):
  band shift bd - 4, packed path 35 / 176;  unpacked path 11 / 11;  `& 0x001F001F` dropped 35 / 65;  min(k, 3) 35 / 178;
  d_pk_min_u16(.., maxv2) dropped 35 / 216;  plain packed subtract 35 / 209;  t1 and t3 swapped 35 / 228;
  `bad |= d_sao_bad` dropped for class 2 17 / 177;  skipmask ignored in the packed path 2 / 63;  unpacked band `k & 3` without `k < 4` 11 / 16.
No mutation survives; none of the mutated lines is dead.  The earlier suite already saw each of them at some depth."""
import pytest

from batch_util import check_batches
from oracle_py import Oracle
from sao_content import NO_SAO, check_offsets, directed_case, sao_census
from synth_util import assert_planes_equal, device_decode, oracle_decode
from test_emu_picture import emu_lib  # noqa: F401  (fixture)
from libde265_amd import capi, worklist as W

DEPTHS = (8, 9, 10, 11, 12, 13, 15, 16)     # 9 and 11: an offset range of their own; 15: the last packed depth; 16: the unpacked path
INTER = dict(n_refs=1, intra_pct=5, cbf_pct=10)                                     # the references' content survives prediction
INTRA = dict(n_refs=0, intra_pct=100, cbf_pct=10, fixed_cu_log2=3)                  # + PCM: the content of the depths above 12
LF = 2 + 8 + 16                              # KINDS[1] of test_deblock_smooth.py: cu_transquant_bypass, PCM, pcm_loop_filter_disable
GEOM = dict(width=96, height=64, log2_ctb=5)


def _content(bd, bdc=0, features=0):
    """the generator settings that carry the content at a depth (module header)"""
    if max(bd, bdc) <= 12:
        return dict(INTER, features=features) if features else dict(INTER)
    return dict(INTRA, features=features | 8)


def _case(cid, border=False, **cfg):
    bd, bdc = cfg["bit_depth"], cfg.get("bit_depth_chroma", 0)
    cfg = dict(cfg, **_content(bd, bdc, cfg.pop("features", 0)))
    cfg["seed"] += 1000 * SEED_STEP.get(cid, 0)
    return cid, border, cfg


# seeds: + 1000 * SEED_STEP where the census of that seed fell short of the conditions above (tiles / slices cases: the 2 to 4 CTBs beside a
# border must draw the edge type AND the PCM / bypass CUs must lie in edge CTBs; (batch, picture): the pictures of BATCHES)
SEED_STEP = {"8bit_cf1": 8, "8bit_cf2": 2, "8bit_cf3": 1, "8bit_cf4": 1, "9bit_cf1": 2, "9bit_cf4": 1, "10bit_cf1": 1, "10bit_cf3": 5,
             "11bit_cf2": 2, "11bit_cf3": 2, "11bit_cf4": 2, "12bit_cf2": 3, "12bit_cf3": 3, "13bit_cf1": 10, "13bit_cf2": 2,
             "15bit_cf1": 11, "15bit_cf2": 8, "15bit_cf3": 7, "15bit_cf4": 2, "16bit_cf3": 2,
             "mixed_12_16": 12, "tiles2x2_10bit": 23, "tiles2x2_16bit": 35, "slices3_8bit": 21, "slices3_16bit": 93,
             ("8bit_cf1", 0): 10, ("8bit_cf1", 1): 2, ("8bit_cf1", 2): 1, ("16bit_cf3", 1): 1, ("16bit_cf3", 2): 5,
             ("10_16bit_cf2", 0): 1, ("10_16bit_cf2", 1): 3}

# (id, tiles / slices case?, generator configuration)
CASES = [_case("%dbit_cf%d" % (bd, cf), bit_depth=bd, chroma_format=cf, seed=100 * bd + 10 * cf, **GEOM) for bd in DEPTHS for cf in (1, 2, 3, 4)]
CASES += [
    _case("mixed_10_12", bit_depth=10, bit_depth_chroma=12, seed=2, **GEOM),
    _case("mixed_12_16", bit_depth=12, bit_depth_chroma=16, seed=3, **GEOM),       # (one launch per picture: luma takes the unpacked kernel too)
    # chroma CTBs of 8x8: a 4x4 thread block is both a left and a right, or a top and a bottom, ring block of its CTB
    _case("ctb16_10bit", bit_depth=10, width=96, height=64, log2_ctb=4, seed=4),
    _case("ctb16_16bit", bit_depth=16, width=96, height=64, log2_ctb=4, seed=5),
    # the width crosses a 256-sample block and ends in a partial 64-sample wave tile; the height is no multiple of 16
    _case("328x40_10bit", bit_depth=10, width=328, height=40, log2_ctb=5, seed=6),
    _case("328x40_16bit", bit_depth=16, width=328, height=40, log2_ctb=5, seed=7),
    _case("tiles2x2_10bit", True, bit_depth=10, tile_cols=2, tile_rows=2, lf_across_tiles=0, features=LF, seed=8, **GEOM),
    _case("tiles2x2_16bit", True, bit_depth=16, tile_cols=2, tile_rows=2, lf_across_tiles=0, features=LF, seed=9, **GEOM),
    # three slices, whose random flags switch SAO off per slice and disable filtering across slices
    _case("slices3_8bit", True, bit_depth=8, n_slices=3, features=LF, seed=10, **GEOM),
    _case("slices3_16bit", True, bit_depth=16, n_slices=3, features=LF, seed=11, **GEOM),
]
IDS = [c[0] for c in CASES]
_BY_ID = dict((c[0], c) for c in CASES)

# all-intra pictures for m355_decode_batch: (id, [generator configuration of each picture])
def _batch(bid, cf, depths, seed):
    return bid, [dict(GEOM, bit_depth=bd, chroma_format=cf, features=8, seed=seed + 37 * k + 1000 * SEED_STEP.get((bid, k), 0), **INTRA) for k, bd in enumerate(depths)]


BATCHES = [
    _batch("8bit_cf1", 1, (8, 8, 8), 21),
    _batch("16bit_cf3", 3, (16, 16, 16), 22),
    # pictures of 10 and of 16 bits in one batch: all of them through k_sao_batch<uint16_t, false>
    _batch("10_16bit_cf2", 2, (10, 16, 10), 23),
]


def check_census(cen, border, what):
    """the conditions of the module's header; cen = sao_census(...)"""
    for c, p in enumerate(cen):
        lo_edge, lo_band, lo_clip = (20, 200, 20) if c == 0 else (8, 50, 8)
        for k in (0, 1, 3, 4):
            assert p["edge_cat"][k] >= lo_edge, "%s plane %d: only %d samples changed in edge category %d" % (what, c, p["edge_cat"][k], k)
        assert p["band"] >= lo_band, "%s plane %d: only %d samples changed by a band offset" % (what, c, p["band"])
        assert p["clip_lo"] >= lo_clip, "%s plane %d: only %d results clipped at 0" % (what, c, p["clip_lo"])
        assert p["clip_hi"] >= lo_clip, "%s plane %d: only %d results clipped at the maximum" % (what, c, p["clip_hi"])
        assert 4 * p["unchanged"] >= p["samples"], "%s plane %d: only %d of %d samples unchanged" % (what, c, p["unchanged"], p["samples"])
    assert max(p["wrap"] for p in cen) >= 8, "%s: the band table wraps past band 31 for %s samples only" % (what, [p["wrap"] for p in cen])
    if border:
        assert cen[0]["held_border"] >= 8, "%s: only %d luma samples held back at tile / slice borders" % (what, cen[0]["held_border"])
        assert cen[0]["held_skip"] >= 16, "%s: only %d luma samples held back in PCM / bypass CUs" % (what, cen[0]["held_skip"])


_cache = {}


def _prepare(oracle_lib, key, cfg, border):
    """(picture, references, the oracle's planes with all stages) of one configuration, its census checked; made once, never modified"""
    if key not in _cache:
        o = Oracle(oracle_lib)
        pic, refs, pre = directed_case(o, **cfg)
        want = oracle_decode(o, pic, refs)
        _cache[key] = (pic, refs, want, sao_census(pic, pre, want))
    pic, refs, want, cen = _cache[key]
    check_offsets(pic)
    check_census(cen, border, key)
    return pic, refs, want


def prepared(oracle_lib, cid):
    _, border, cfg = _BY_ID[cid]
    return _prepare(oracle_lib, cid, cfg, border)


def batch_prepared(oracle_lib, bid, cfgs):
    """the pictures of a batch (all-intra: no references), the census of each checked"""
    return [_prepare(oracle_lib, "batch %s picture %d" % (bid, k), cfg, False)[0] for k, cfg in enumerate(cfgs)]


@pytest.mark.parametrize("cid", IDS)
def test_sao_content_emulated(emu_lib, oracle, cid):  # noqa: F811
    pic, refs, want = prepared(oracle, cid)
    ctx = capi.Context(emu_lib, 0)
    try:
        assert_planes_equal(device_decode(ctx, pic, refs), want, "kernels vs oracle, all stages")
    finally:
        ctx.close()


@pytest.mark.parametrize("cid", IDS)
def test_sao_content_oracle_equals_reference_replay(oracle, ref, cid):
    from ref_replay_py import ref_replay
    pic, refs, want = prepared(oracle, cid)
    assert_planes_equal(oracle_decode(Oracle(oracle), pic, refs, NO_SAO), ref_replay(ref, pic, refs, NO_SAO, accel=0), "oracle vs scalar reference, SAO off")
    assert_planes_equal(want, ref_replay(ref, pic, refs, W.STAGE_ALL, accel=0), "oracle vs scalar reference, all stages")


@pytest.mark.parametrize("bid,cfgs", BATCHES, ids=[b[0] for b in BATCHES])
def test_sao_content_decode_batch_emulated(emu_lib, oracle, bid, cfgs):  # noqa: F811
    pics = batch_prepared(oracle, bid, cfgs)
    check_batches(emu_lib, Oracle(oracle), None, 3, [[0, 1, 2], [2, 0]], pics=pics)[0].close()


@pytest.fixture(scope="module")
def gpu_ctx():
    lib = capi.Library()
    assert lib.device_count() >= 1
    c = capi.Context(lib, 0)
    yield c
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cid", IDS)
def test_sao_content_gpu(gpu_ctx, oracle, cid):
    ctx = gpu_ctx
    pic, refs, want = prepared(oracle, cid)
    ctx.set_pipeline_depth(1)
    assert_planes_equal(device_decode(ctx, pic, refs), want, "depth 1")
    ctx.set_pipeline_depth(3)
    try:
        assert_planes_equal(device_decode(ctx, pic, refs, resident=True, repeat=3), want, "depth 3, three in flight")
    finally:
        ctx.set_pipeline_depth(1)


@pytest.mark.gpu
@pytest.mark.parametrize("bid,cfgs", BATCHES, ids=[b[0] for b in BATCHES])
def test_sao_content_decode_batch_gpu(oracle, bid, cfgs):
    pics = batch_prepared(oracle, bid, cfgs)
    check_batches(capi.Library(), Oracle(oracle), None, 3, [[0, 1, 2], [2, 0, 1], [1]], pics=pics)[0].close()
