"""GPU tier of the light intra path (k_intra_light.h): the cases of intra_light_cases.py on the hardware — where a wave's later blocks read what its
earlier ones stored through the L2, and the light workgroups run beside the CTB workgroups of the same launch and other pictures' kernels —, bit-exact
against the oracle with one and with three pictures in flight."""
import pytest

from intra_light_cases import CASES, run_case, run_forced_32
from libde265_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    lib = capi.Library()
    assert lib.device_count() >= 1
    return lib


@pytest.mark.parametrize("depth", [1, 3])
@pytest.mark.parametrize("name", sorted(CASES))
def test_light_intra_path(lib, oracle, name, depth):
    run_case(lib, oracle, name, depth)


def test_light_intra_path_32x32_forced(lib, oracle):
    run_forced_32(lib.path, oracle._name)
