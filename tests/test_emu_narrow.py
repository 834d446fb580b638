"""16-bit coefficient entries (M355_RBF_NARROW) on the CPU tier: the product kernels under the SIMT interpreter decode packed pictures —
narrow and wide blocks mixed in one wave, cross-component chroma blocks that follow their luma block's form, every size bin, counts of
one / odd / even, a block ending in the list's last word — exactly as the oracle decodes the same lists in the wide form.  Both entry
points: lists the library copies (checked on the host) and lists recorded in place (checked by k_validate).  narrow_util.py holds the
cases; test_gpu_narrow.py runs them on the device."""
import pytest

import narrow_util
from oracle_py import Oracle
from shard_util import local_sharded_decode
from synth_util import assert_planes_equal
from test_emu_picture import emu_lib  # noqa: F401  (fixture)
from libde265_amd import capi


@pytest.fixture(scope="module")
def ctx(emu_lib):  # noqa: F811
    c = capi.Context(emu_lib, 0)
    yield c
    c.close()


@pytest.mark.parametrize("in_place", [False, True], ids=["copied", "in_place"])
@pytest.mark.parametrize("name", list(narrow_util.CASES))
def test_packed_picture_matches_oracle_emulated(ctx, oracle, name, in_place):
    narrow_util.check_case(ctx, oracle, name, in_place)


@pytest.mark.parametrize("in_place", [False, True], ids=["copied", "in_place"])
def test_narrow_block_beyond_the_list_is_refused_emulated(ctx, oracle, in_place):
    narrow_util.check_rejection(ctx, oracle, in_place)


def test_sharded_cut_counts_words_emulated(emu_lib, oracle):  # noqa: F811
    """two virtual ranks through shard.shard_picture: a narrow block's share of the coefficient list is (ncoeff + 1) / 2 words"""
    wide, packed, refs, want = narrow_util.case("sharded", oracle)
    for r, got in enumerate(local_sharded_decode(emu_lib, packed, refs, 2)):
        assert_planes_equal(got, want, "rank %d of 2" % r)
