"""Kernel-logic verification (CPU tier) at bit depths 9..16, luma and chroma apart too, through the SIMT-interpreter build vs the
oracle: small pictures from the matrix test_oracle_vs_ref_replay.py pins against the reference.  At 16 bits an intra block's deferred
residual can exceed int16 (k_common.h m355_res32): k_residual / k_intra's W16 instantiations carry it as int32."""
import pytest

from oracle_py import Oracle
from synth_util import assert_planes_equal, device_decode, make_case, oracle_decode
from test_emu_picture import emu_lib  # noqa: F401  (fixture)
from test_oracle_vs_ref_replay import case_id
from libde265_amd import capi, worklist

M355_ERR_INVALID = 3   # (capi.ERRORS)

CASES = [
    dict(width=64, height=64, bit_depth=16, seed=101, intra_pct=100, n_refs=0, cbf_pct=100),
    dict(width=64, height=64, bit_depth=16, seed=105, intra_pct=50, cbf_pct=100, features=64 + 128 + 2),
    dict(width=64, height=64, bit_depth=16, seed=108, intra_pct=30, cbf_pct=100, chroma_format=3, features=32 + 2),
    dict(width=64, height=64, bit_depth=16, seed=109, intra_pct=40, cbf_pct=100, chroma_format=2, features=31, qp_wide=1),
    dict(width=64, height=64, bit_depth=16, seed=110, intra_pct=50, cbf_pct=100, chroma_format=4, fixed_cu_log2=5),
    dict(width=64, height=64, bit_depth=15, seed=111, intra_pct=100, n_refs=0, cbf_pct=100, qp_wide=1),
    dict(width=64, height=64, bit_depth=14, seed=112, intra_pct=50, cbf_pct=100, weighted_pct=30, oob_mv_pct=20),
    dict(width=64, height=64, bit_depth=13, seed=113, intra_pct=50, cbf_pct=100, features=8 + 4),
    dict(width=64, height=64, bit_depth=11, seed=114, intra_pct=50, cbf_pct=100, qp_wide=1),
    dict(width=64, height=64, bit_depth=10, bit_depth_chroma=12, seed=115, intra_pct=30, cbf_pct=100, weighted_pct=30),
    dict(width=64, height=64, bit_depth=12, bit_depth_chroma=13, seed=116, intra_pct=30, cbf_pct=100, qp_wide=1),
    dict(width=64, height=64, bit_depth=9, bit_depth_chroma=16, seed=117, intra_pct=100, n_refs=0, cbf_pct=100, chroma_format=3, features=32),
    dict(width=64, height=64, bit_depth=16, bit_depth_chroma=9, seed=118, intra_pct=50, cbf_pct=100, chroma_format=2),
]


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_emulated_kernels_match_oracle_at_depth(emu_lib, oracle, case):  # noqa: F811
    o = Oracle(oracle)
    pic, refs = make_case(**case)
    ctx = capi.Context(emu_lib, 0)
    try:
        assert_planes_equal(device_decode(ctx, pic, refs), oracle_decode(o, pic, refs), "all stages")
        st = worklist.STAGE_INTER | worklist.STAGE_RESIDUAL | worklist.STAGE_INTRA
        assert_planes_equal(device_decode(ctx, pic, refs, st), oracle_decode(o, pic, refs, st), "no loop filters")
    finally:
        ctx.close()


def test_mixed_8bit_and_deeper_is_refused(emu_lib):  # noqa: F811
    """8-bit samples beside deeper ones (runtime.hip m355_frame_create): refused with M355_ERR_INVALID, nothing decoded"""
    ctx = capi.Context(emu_lib, 0)
    try:
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
        assert all(int(p.max()) == 0 for p in ctx.frame_download(dst))
        ctx.frame_destroy(dst)
    finally:
        ctx.close()
