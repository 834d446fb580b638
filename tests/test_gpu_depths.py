"""GPU parity at every bit depth 8..16, luma and chroma apart too: the paths that bit depth selects — k_inter_jobs (deeper of the two
depths <= 12, tap tables per (luma, chroma) pair) or k_inter_generic, packed 16-bit SAO and the chain's front-part residuals (<= 15), the
int32 deferred residuals of k_residual / k_intra (16, k_common.h m355_res32) — with one picture at a time, three in flight, through
m355_decode_batch and (test_gpu_chain_forced.py, CHAIN_CASES) the forced chain schedules.  The oracle these are checked against is
pinned to the reference at these depths by test_oracle_vs_ref_replay.py."""
import pytest

from oracle_py import Oracle
from batch_util import check_batches
from synth_util import assert_planes_equal, device_decode, make_case, oracle_decode
from test_oracle_vs_ref_replay import case_id
from libde265_amd import capi, worklist

pytestmark = pytest.mark.gpu

M355_ERR_INVALID = 3   # (capi.ERRORS)


@pytest.fixture(scope="module")
def ctx():
    lib = capi.Library()
    assert lib.device_count() >= 1
    c = capi.Context(lib, 0)
    yield c
    c.close()


# every depth in every chroma format: an intra picture with residuals in every block, an inter picture with intra blocks and dense residuals
KINDS = [dict(intra_pct=100, n_refs=0, cbf_pct=100), dict(intra_pct=40, cbf_pct=100, weighted_pct=20, oob_mv_pct=10, features=2)]
CASES = [dict(width=96, height=64, bit_depth=bd, chroma_format=cf, seed=3000 + 100 * bd + 10 * cf + k, log2_ctb=5 if k else 6, **kw)
         for bd in range(8, 17) for cf in (1, 2, 3, 4) for k, kw in enumerate(KINDS)]
CASES += [
    # QpY down to -QpBdOffsetY, residual tools, PCM, cross-component prediction
    dict(width=128, height=64, bit_depth=16, seed=3901, intra_pct=60, cbf_pct=100, qp_wide=1, features=64 + 128 + 2 + 8),
    dict(width=128, height=64, bit_depth=16, seed=3902, intra_pct=40, cbf_pct=100, chroma_format=3, features=32 + 4),
    dict(width=128, height=64, bit_depth=14, seed=3903, intra_pct=100, n_refs=0, cbf_pct=100, qp_wide=1, features=31),
    # mixed depths: k_inter_jobs with unequal tables (10/12), k_inter_generic (12/13), one component at 16 bits
    dict(width=128, height=64, bit_depth=10, bit_depth_chroma=12, seed=3911, intra_pct=20, cbf_pct=100, weighted_pct=30, oob_mv_pct=10),
    dict(width=128, height=64, bit_depth=12, bit_depth_chroma=13, seed=3912, intra_pct=20, cbf_pct=100, weighted_pct=30, qp_wide=1),
    dict(width=128, height=64, bit_depth=9, bit_depth_chroma=12, seed=3913, intra_pct=30, cbf_pct=100, chroma_format=3, features=32),
    dict(width=128, height=64, bit_depth=16, bit_depth_chroma=9, seed=3914, intra_pct=50, cbf_pct=100, chroma_format=2),
    dict(width=128, height=64, bit_depth=9, bit_depth_chroma=16, seed=3915, intra_pct=100, n_refs=0, cbf_pct=100, chroma_format=3, features=32),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: case_id(c) + "_cf%d" % c.get("chroma_format", 1))
def test_depths_bit_exact(ctx, oracle, case):
    o = Oracle(oracle)
    pic, refs = make_case(**case)
    want = oracle_decode(o, pic, refs)
    ctx.set_pipeline_depth(1)
    assert_planes_equal(device_decode(ctx, pic, refs), want, "depth 1")
    st = worklist.STAGE_INTER | worklist.STAGE_RESIDUAL | worklist.STAGE_INTRA
    assert_planes_equal(device_decode(ctx, pic, refs, st), oracle_decode(o, pic, refs, st), "no loop filters")
    ctx.set_pipeline_depth(3)
    try:
        assert_planes_equal(device_decode(ctx, pic, refs, resident=True, repeat=4), want, "depth 3")
    finally:
        ctx.set_pipeline_depth(1)


# (also run by test_gpu_chain_forced.py under the chain hooks: res_front and packed SAO at 15 bits, neither at 16)
CHAIN_CASES = [
    dict(width=128, height=64, bit_depth=15, seed=3921, intra_pct=30, cbf_pct=100, weighted_pct=20),
    dict(width=128, height=64, bit_depth=16, seed=3922, intra_pct=30, cbf_pct=100, weighted_pct=20),
    dict(width=128, height=64, bit_depth=16, seed=3923, intra_pct=100, n_refs=0, cbf_pct=100, chroma_format=3, features=32 + 2),
    dict(width=128, height=64, bit_depth=10, bit_depth_chroma=16, seed=3924, intra_pct=30, cbf_pct=100, chroma_format=2),
]


@pytest.mark.parametrize("cfg", [dict(width=192, height=128, bit_depth=15, seed=3931, cbf_pct=100),
                                 dict(width=192, height=128, bit_depth=16, seed=3932, cbf_pct=100, qp_wide=1),
                                 dict(width=192, height=128, bit_depth=16, seed=3933, cbf_pct=100, chroma_format=3, features=32 + 8)],
                         ids=case_id)
def test_depths_through_decode_batch(oracle, cfg):
    """intra pictures at 15 / 16 bits through m355_decode_batch (k_residual_batch + k_intra<BATCH>)"""
    c = check_batches(capi.Library(), Oracle(oracle), cfg, 3, [[0, 1, 2], [2, 0, 1], [1]])[0]
    c.close()


def test_mixed_8bit_and_deeper_is_refused(ctx):
    """8-bit samples beside deeper ones: M355_ERR_INVALID before anything is launched, the destination untouched"""
    for bdl, bdc in ((8, 10), (10, 8), (8, 16)):
        with pytest.raises(capi.M355Error) as e:
            ctx.frame_create(64, 64, 1, bdl, bdc)
        assert e.value.code == M355_ERR_INVALID
    pic, refs = make_case(width=64, height=64, bit_depth=8, seed=7, intra_pct=100, n_refs=0)
    pic.pp["bit_depth_chroma"] = 10
    dst = ctx.frame_create(64, 64, 1, 8, 8)
    pic.dst_frame = dst
    with pytest.raises(capi.M355Error) as e:
        ctx.submit(pic)
    assert e.value.code == M355_ERR_INVALID
    ctx.wait()
    assert all(int(p.max()) == 0 for p in ctx.frame_download(dst))
    ctx.frame_destroy(dst)
