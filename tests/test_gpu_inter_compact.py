"""GPU tier of the compact workgroups of k_inter_jobs: the cases of inter_compact_cases.py on the hardware — the partition by kind through LDS, waves
of one kind beside mixed waves in one workgroup, partial workgroups and PBs split between two —, bit-exact against the oracle with one and with three
pictures in flight."""
import pytest

from inter_compact_cases import CASES, run_case
from libde265_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    lib = capi.Library()
    assert lib.device_count() >= 1
    return lib


@pytest.mark.parametrize("depth", [1, 3])
@pytest.mark.parametrize("name", sorted(CASES))
def test_compact_inter_workgroups(lib, oracle, name, depth):
    run_case(lib, oracle, name, depth)
