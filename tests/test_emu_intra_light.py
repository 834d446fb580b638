"""CPU tier of the light intra path (k_intra_light.h) on the SIMT interpreter: inter pictures whose CTBs without a cross-CTB intra dependency run as one
wave per CTB and colour component, bit-exact against the oracle with one and with three pictures in flight.  The cases, what each is there for and the
conditions on the path taken (every picture has light items; the mixed cases also CTBs of a dependency chain) are intra_light_cases.py's."""
import pytest

from intra_light_cases import CASES, run_case, run_forced_32
from test_emu_picture import EMU_SO, emu_lib  # noqa: F401  (fixture)


@pytest.mark.parametrize("depth", [1, 3])
@pytest.mark.parametrize("name", sorted(CASES))
def test_light_intra_path_emulated(emu_lib, oracle, name, depth):  # noqa: F811
    run_case(emu_lib, oracle, name, depth)


def test_light_intra_path_32x32_forced_emulated(emu_lib, oracle):  # noqa: F811
    run_forced_32(EMU_SO, oracle._name)
