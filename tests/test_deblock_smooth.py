"""Deblocking on SMOOTH content (tests/deblock_content.py): pictures predicted from references that are two thirds low-slope ramp, so that
`d < beta` holds on many luma edge segments and the normal filter (p0 / q0, p1 / q1 under dEp / dEq), the strong filter (three samples a
side) and — in the kind-1 cases: PCM units with pcm_loop_filter_disable, cu_transquant_bypass CUs — the filters of ONE side only
(filterP / filterQ, deblock.cc:561-601) all run in one picture, beside edges that are not filtered at all, at every sample type and
depth scaling (beta, tc << (BitDepth - 8)).  On the generator's own noise planes hardly any luma segment passes `d < beta`: the other
synthetic suites leave k_deblock's filter arithmetic and its write-back (np / nq rows, k_deblock.hip) all but unexecuted at 9..13 bits.

Every case first asserts, FROM THE ORACLE'S PLANES ALONE (deblock_census of the picture before / after the stage, SAO off), that the
filter did enough of each kind of work — conditions on the input, so that a change of the generator cannot empty the test:
  luma: >= 4 % of the samples changed and >= 50 % unchanged; >= 50 changed at distance 1 from the 8-grid (p1 / q1); >= 16 at distance
  >= 2 (p2 / q2: the strong filter only); kind 1: >= 4 edge segments changed on one side only;
  chroma (kind 1, all-intra): >= 20 changed samples in each plane.

CPU tier: kernels under the SIMT interpreter == oracle, with all stages and with SAO off (SAO can neither mask nor make a difference);
          oracle == the reference's own apply_deblocking_filter on the same pictures and references (oracle/_ref replay).
GPU tier: the HIP kernels == oracle: one picture at a time with and without SAO, three in flight from resident lists, a chain of
          pictures each predicted from the one deblocked in place just before it; three all-intra configurations through
          m355_decode_batch (k_deblock_batch); four cases under the forced chain schedules (test_gpu_chain_forced.py, CHAIN_CASES)."""
import pytest

from batch_util import check_batches, intra_pictures
from deblock_content import deblock_census, make_smooth_case
from oracle_py import Oracle
from synth_util import assert_planes_equal, device_decode, oracle_decode
from test_emu_picture import emu_lib  # noqa: F401  (fixture)
from libde265_amd import capi, worklist as W

NO_DEBLOCK = W.STAGE_INTER | W.STAGE_RESIDUAL | W.STAGE_INTRA
NO_SAO = W.STAGE_ALL & ~W.STAGE_SAO

DEPTHS = (8, 9, 10, 12, 13, 15, 16)          # both sample types; 15: the last depth of packed 16-bit SAO; 16
# kind 0: few intra blocks, few residuals — long smooth stretches; kind 1: + cu_transquant_bypass, PCM, pcm_loop_filter_disable (one-sided filters)
KINDS = [dict(intra_pct=5, cbf_pct=10), dict(intra_pct=30, cbf_pct=40, features=2 + 8 + 16)]
INTRA = "intra"
# seeds: 7000 + 100 * depth + 10 * chroma_format + kind, + 1000 * SEED_STEP where the census of that seed fell short of the conditions above
SEED_STEP = {(8, 1, 0): 3, (8, 1, 1): 2, (8, 2, 0): 1, (8, 2, 1): 2, (8, 3, 0): 2, (8, 3, 1): 3, (8, 4, 0): 1, (8, 4, 1): 12,
             (9, 2, 1): 2, (9, 3, 1): 1, (10, 2, 1): 1, (15, 1, 1): 1, (15, 2, 0): 1, (15, 4, 0): 1, (16, 1, 0): 3}


def _matrix(bd, cf, k):
    seed = 7000 + 100 * bd + 10 * cf + k + 1000 * SEED_STEP.get((bd, cf, k), 0)
    return ("%dbit_cf%d_kind%d" % (bd, cf, k), k, dict(width=96, height=64, log2_ctb=5, bit_depth=bd, chroma_format=cf, seed=seed, **KINDS[k]))


# (id, kind, generator configuration); 96x64 with CTBs of 32: partial CTBs, two CTB rows
CASES = [_matrix(bd, cf, k) for bd in DEPTHS for cf in (1, 2, 3, 4) for k in (0, 1)]
CASES += [
    ("tiles2x2_no_lf_across", 1, dict(width=96, height=64, log2_ctb=5, bit_depth=8, seed=11901, tile_cols=2, tile_rows=2, lf_across_tiles=0, **KINDS[1])),
    ("tiles2x2_10bit", 0, dict(width=96, height=64, log2_ctb=5, bit_depth=10, seed=7902, tile_cols=2, tile_rows=2, lf_across_tiles=0, **KINDS[0])),
    # per-slice beta / tc offsets, deblocking-disable and filter-across-slices flags
    ("slices3_192x128", 1, dict(width=192, height=128, log2_ctb=5, bit_depth=10, seed=7903, n_slices=3, **KINDS[1])),
    ("mixed_10_12", 1, dict(width=96, height=64, log2_ctb=5, bit_depth=10, bit_depth_chroma=12, seed=7904, **KINDS[1])),
    ("mixed_12_13", 1, dict(width=96, height=64, log2_ctb=5, bit_depth=12, bit_depth_chroma=13, chroma_format=2, seed=7905, **KINDS[1])),
    ("qp_wide_16bit", 1, dict(width=96, height=64, log2_ctb=5, bit_depth=16, seed=8906, qp_wide=1, **KINDS[1])),
    # every edge has bS == 2: the chroma filter runs on every edge of its grid
    ("all_intra_8bit", INTRA, dict(width=96, height=64, log2_ctb=5, bit_depth=8, seed=7093, intra_pct=100, n_refs=0, cbf_pct=10, fixed_cu_log2=3)),
    ("all_intra_12bit_444", INTRA, dict(width=96, height=64, log2_ctb=5, bit_depth=12, chroma_format=3, seed=7908, intra_pct=100, n_refs=0, cbf_pct=20)),
]
IDS = [c[0] for c in CASES]
_BY_ID = dict((c[0], c) for c in CASES)
# (also run by test_gpu_chain_forced.py under the forced chain schedules, with make_smooth_case): one per chroma format
CHAIN_CASES = [_BY_ID[i][2] for i in ("10bit_cf1_kind1", "12bit_cf2_kind1", "15bit_cf3_kind1", "16bit_cf4_kind1")]
# all-intra configurations for m355_decode_batch (batch_util makes the pictures: intra only, seeds 37 apart)
BATCH_CFGS = [
    # (8-bit intra content rarely passes the strong filter's flatness test, beta >> 3 of 2..5: 192x128 to reach 16 such samples in each picture)
    dict(width=192, height=128, log2_ctb=5, bit_depth=8, chroma_format=1, seed=7216, cbf_pct=5, fixed_cu_log2=3),
    dict(width=96, height=64, log2_ctb=5, bit_depth=10, chroma_format=2, seed=7496, cbf_pct=10, fixed_cu_log2=3),
    dict(width=96, height=64, log2_ctb=5, bit_depth=16, chroma_format=3, seed=7002, cbf_pct=10, fixed_cu_log2=3),
]


def check_census(cen, kind, what):
    """the conditions of the module's header; cen = deblock_census(...)"""
    y = cen[0]
    assert y["changed"] * 100 >= 4 * y["samples"], "%s: deblocking changed only %d of %d luma samples" % (what, y["changed"], y["samples"])
    assert y["changed"] * 2 <= y["samples"], "%s: deblocking changed %d of %d luma samples: no unfiltered edges left" % (what, y["changed"], y["samples"])
    assert y["m1"] >= 50, "%s: only %d luma samples changed at p1 / q1" % (what, y["m1"])
    assert y["m2"] >= 16, "%s: only %d luma samples changed at p2 / q2 (strong filter)" % (what, y["m2"])
    if kind == 1:
        assert y["one_sided"] >= 4, "%s: only %d luma segments filtered on one side" % (what, y["one_sided"])
    if kind in (1, INTRA):
        for c in cen[1:]:
            assert c["changed"] >= 20, "%s: deblocking changed only %d chroma samples" % (what, c["changed"])


_cache = {}


def prepared(oracle_lib, cid):
    """(picture, references, oracle planes {stages: planes}) of a case, its census checked; made once, never modified"""
    if cid not in _cache:
        _, kind, cfg = _BY_ID[cid]
        o = Oracle(oracle_lib)
        pic, refs = make_smooth_case(**cfg)
        want = dict((st, oracle_decode(o, pic, refs, st)) for st in (NO_DEBLOCK, NO_SAO, W.STAGE_ALL))
        _cache[cid] = (pic, refs, want, kind)
    pic, refs, want, kind = _cache[cid]
    check_census(deblock_census(want[NO_DEBLOCK], want[NO_SAO]), kind, cid)
    return pic, refs, want


def batch_census(oracle_lib, cfg, n):
    o = Oracle(oracle_lib)
    for k, pic in enumerate(intra_pictures(n, **cfg)):
        check_census(deblock_census(oracle_decode(o, pic, [], NO_DEBLOCK), oracle_decode(o, pic, [], NO_SAO)), INTRA, "batch picture %d" % k)


def chain_oracle(o, pic, refs, n):
    """decode k of n: the picture's lists into a frame of its own, reference 0 = the frame decode k - 1 wrote (decode 0: refs[0]) -> the last frame's planes"""
    pp = pic.pp[0]
    rf = [o.frame_new(pp) for _ in refs]
    for f, planes in zip(rf, refs):
        o.frame_set_planes(f, planes)
    out = [o.frame_new(pp) for _ in range(n)]
    pic.ref_frames = [i if i < len(refs) else -1 for i in range(W.MAX_REF_FRAMES)]
    for k in range(n):
        slots = dict(enumerate(rf))
        if k and rf:
            slots[0] = out[k - 1]
        assert o.decode(pic, out[k], slots) == 0
    planes = o.frame_planes(out[-1])
    for f in rf + out:
        o.frame_free(f)
    return planes


def chain_device(ctx, pic, refs, n):
    """the same chain from resident lists, no host synchronisation between the decodes"""
    pp = pic.pp[0]
    rf = [ctx.frame_create_for(pp) for _ in refs]
    for f, planes in zip(rf, refs):
        ctx.frame_upload(f, planes)
    out = [ctx.frame_create_for(pp) for _ in range(n)]
    handles = []
    for k in range(n):
        slots = list(rf)
        if k and rf:
            slots[0] = out[k - 1]
        pic.dst_frame = out[k]
        pic.ref_frames = slots + [-1] * (W.MAX_REF_FRAMES - len(slots))
        handles.append(ctx.upload(pic))
    ctx.wait()
    for h in handles:
        ctx.decode_resident(h)
    ctx.wait()
    planes = ctx.frame_download(out[-1])
    for h in handles:
        ctx.release(h)
    for f in rf + out:
        ctx.frame_destroy(f)
    return planes


@pytest.mark.parametrize("cid", IDS)
def test_smooth_content_emulated(emu_lib, oracle, cid):  # noqa: F811
    pic, refs, want = prepared(oracle, cid)
    ctx = capi.Context(emu_lib, 0)
    try:
        assert_planes_equal(device_decode(ctx, pic, refs, NO_SAO), want[NO_SAO], "kernels vs oracle, SAO off")
        assert_planes_equal(device_decode(ctx, pic, refs), want[W.STAGE_ALL], "kernels vs oracle, all stages")
    finally:
        ctx.close()


@pytest.mark.parametrize("cid", IDS)
def test_smooth_content_oracle_equals_reference_replay(oracle, ref, cid):
    from ref_replay_py import ref_replay
    pic, refs, want = prepared(oracle, cid)
    for st in (NO_DEBLOCK, NO_SAO, W.STAGE_ALL):
        assert_planes_equal(want[st], ref_replay(ref, pic, refs, st, accel=0), "oracle vs scalar reference, stages %d" % st)
    assert_planes_equal(want[NO_SAO], ref_replay(ref, pic, refs, NO_SAO, accel=1), "oracle vs SSE reference, SAO off")


@pytest.mark.parametrize("cfg", BATCH_CFGS, ids=lambda c: "%dbit_cf%d" % (c["bit_depth"], c["chroma_format"]))
def test_smooth_content_decode_batch_emulated(emu_lib, oracle, cfg):  # noqa: F811
    batch_census(oracle, cfg, 3)
    for st in (NO_SAO, W.STAGE_ALL):
        check_batches(emu_lib, Oracle(oracle), cfg, 3, [[0, 1, 2], [2, 0]], stages=st)[0].close()


@pytest.fixture(scope="module")
def gpu_ctx():
    lib = capi.Library()
    assert lib.device_count() >= 1
    c = capi.Context(lib, 0)
    yield c
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cid", IDS)
def test_smooth_content_gpu(gpu_ctx, oracle, cid):
    ctx = gpu_ctx
    pic, refs, want = prepared(oracle, cid)
    chain_want = chain_oracle(Oracle(oracle), pic, refs, 3)
    ctx.set_pipeline_depth(1)
    assert_planes_equal(device_decode(ctx, pic, refs), want[W.STAGE_ALL], "depth 1")
    assert_planes_equal(device_decode(ctx, pic, refs, NO_SAO), want[NO_SAO], "depth 1, SAO off")
    ctx.set_pipeline_depth(3)
    try:
        assert_planes_equal(device_decode(ctx, pic, refs, resident=True, repeat=4), want[W.STAGE_ALL], "depth 3")
        # each picture predicted from the frame the picture before it has just deblocked in place
        assert_planes_equal(chain_device(ctx, pic, refs, 3), chain_want, "depth 3, chain of 3")
    finally:
        ctx.set_pipeline_depth(1)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", BATCH_CFGS, ids=lambda c: "%dbit_cf%d" % (c["bit_depth"], c["chroma_format"]))
def test_smooth_content_decode_batch_gpu(oracle, cfg):
    batch_census(oracle, cfg, 3)
    lib = capi.Library()
    for st in (NO_SAO, W.STAGE_ALL):
        check_batches(lib, Oracle(oracle), cfg, 3, [[0, 1, 2], [2, 0, 1], [1]], stages=st)[0].close()
