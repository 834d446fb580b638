"""CPU tier of the compact workgroups of k_inter_jobs on the SIMT interpreter: pictures whose 256-job windows of the MAIN range mix the kinds of
prediction block (one list, two lists, explicit weights), so that the workgroup's partition by kind, its wave-uniform paths and its mixed waves all run —
bit-exact against the oracle with one and with three pictures in flight.  The cases and what each is there for are inter_compact_cases.py's."""
import pytest

from inter_compact_cases import CASES, run_case
from test_emu_picture import emu_lib  # noqa: F401  (fixture)


@pytest.mark.parametrize("depth", [1, 3])
@pytest.mark.parametrize("name", sorted(CASES))
def test_compact_inter_workgroups_emulated(emu_lib, oracle, name, depth):  # noqa: F811
    run_case(emu_lib, oracle, name, depth)
