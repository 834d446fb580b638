"""The generator's optional knobs (bit_depth_chroma, qp_wide: csrc/synth.c) are off by default and draw nothing when off: the work
lists of every benchmark config and of a sample of the replay suite's cases stay byte-identical to those the generator made before
the knobs existed (hashes recorded from that tree) — the bench workloads and every existing seed are unchanged."""
import hashlib

import pytest

from libde265_amd import synth

RECORDED = {
    "c2_1080p_intra": "c97318f04b60ec6c", "c3_4k_inter": "c00f4ca8510eeeed", "c4_4k_4tiles": "08305d7f5fd4de2e",
    "c5_8k10_8tiles": "8d8fc90ae6224dab", "tiny_4tiles": "9fd632bff1176337", "c5x_cu64": "12e7816ac7ffb51e",
    "c5x_cu16": "e9bbdac61036c507", "c5x_plain": "9c506dbb31357c57", "c5x_uni": "627d392666405a9d", "c5x_bi": "cf8f47065518e7c4",
    "c5x_noedge": "ac7879cf2594aa05",
}
# (test_oracle_vs_ref_replay.py CASES[::4] of the tree before the knobs)
CASES = [
    (dict(width=192, height=128, bit_depth=8, seed=11), "edb3a7ac8e0022ca"),
    (dict(width=136, height=72, bit_depth=12, seed=15, log2_ctb=5, intra_pct=40), "6f85ba0762edf8c1"),
    (dict(width=640, height=368, bit_depth=10, seed=24, intra_pct=100, n_refs=0, tile_cols=2, tile_rows=2), "efaeca381f15f5d0"),
    (dict(width=72, height=24, bit_depth=9, seed=27, log2_ctb=4, intra_pct=50), "e9247ee4180be9f7"),
    (dict(width=256, height=192, bit_depth=8, seed=73, features=1, intra_pct=40), "754beb2316d751f6"),
    (dict(width=320, height=192, bit_depth=12, seed=78, features=7, n_slices=3, intra_pct=100, n_refs=0, log2_ctb=5), "b1c7acec0bb299c9"),
    (dict(width=256, height=192, bit_depth=8, seed=91, chroma_format=4), "557ce02a499530f2"),
    (dict(width=256, height=192, bit_depth=10, seed=95, chroma_format=2, features=31, n_slices=3, tile_rows=2, intra_pct=50), "94cd203fa1170842"),
    (dict(width=256, height=192, bit_depth=10, seed=112, features=64 + 2, intra_pct=50, cbf_pct=90, fixed_cu_log2=3), "279c63d65ed7421a"),
    (dict(width=256, height=192, bit_depth=8, seed=121, features=256, intra_pct=5, weighted_pct=30), "b8d7b70de4f16a68"),
    (dict(width=256, height=192, bit_depth=10, seed=132, features=512 + 64 + 128, intra_pct=50, cbf_pct=90), "e47d7d576740a093"),
]


def list_hash(p):
    h = hashlib.sha256()
    h.update(p.pp.tobytes())
    for a in (p.slices, p.ctbs, p.cus, p.tus, p.pbs, p.wts, p.rbs, p.ibs, p.coeffs, p.pcm):
        h.update(a.tobytes())
    h.update(repr((list(p.rb_count), int(p.res_len))).encode())
    if getattr(p, "scaling_factors", None) is not None:
        h.update(p.scaling_factors.tobytes())
    return h.hexdigest()[:16]


@pytest.mark.parametrize("name", sorted(RECORDED))
def test_benchmark_config_lists_unchanged(name):
    assert list_hash(synth.picture(**synth.CONFIGS[name])) == RECORDED[name]


@pytest.mark.parametrize("case,want", CASES, ids=lambda v: "seed%d" % v["seed"] if isinstance(v, dict) else None)
def test_case_lists_unchanged(case, want):
    assert list_hash(synth.picture(**case)) == want
    # the knobs at their "off" values spelled out are the same lists
    assert list_hash(synth.picture(**dict(case, bit_depth_chroma=0, qp_wide=0))) == want


def test_knobs_change_the_lists():
    base = dict(width=128, height=64, bit_depth=12, seed=5, intra_pct=50, cbf_pct=100)
    p = synth.picture(**dict(base, bit_depth_chroma=10))
    assert int(p.pp[0]["bit_depth_luma"]) == 12 and int(p.pp[0]["bit_depth_chroma"]) == 10
    q = synth.picture(**dict(base, qp_wide=1))
    assert int(q.cus["qp_y"].min()) < 0 <= int(q.cus["qp_y"].min()) + 6 * (12 - 8)
    assert int(q.rbs["qp"].max()) > 37
