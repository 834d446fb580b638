"""16-bit coefficient entries (M355_RBF_NARROW) on the device: k_residual's narrow fetch in every instantiation (u8 / u16 samples, W16,
the prefetched first batch and the loop, the cross-component re-read), the host's and k_validate's range checks.  The cases are those of
test_emu_narrow.py (narrow_util.py); the expected picture is the oracle's decode of the same lists in the wide form."""
import pytest

import narrow_util
from libde265_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    lib = capi.Library()
    assert lib.device_count() >= 1
    c = capi.Context(lib, 0)
    yield c
    c.close()


@pytest.mark.parametrize("in_place", [False, True], ids=["copied", "in_place"])
@pytest.mark.parametrize("name", list(narrow_util.CASES))
def test_packed_picture_matches_oracle(ctx, oracle, name, in_place):
    narrow_util.check_case(ctx, oracle, name, in_place)


@pytest.mark.parametrize("in_place", [False, True], ids=["copied", "in_place"])
def test_narrow_block_beyond_the_list_is_refused(ctx, oracle, in_place):
    narrow_util.check_rejection(ctx, oracle, in_place)
