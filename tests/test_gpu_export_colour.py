"""The colour transform stage of the composed exports on the GPU: the cases of tests/test_export_colour_emu.py through the real instantiations of
k_export_resized_rgb with the stage — its output table in LDS, its input table through the vector cache —, in the three modes, both filters and both
sitings; the gate, the frame hazard with one and three pictures in flight, and m355_colour_destroy directly behind an export.  Expected values:
export_colour_util.py; all exact."""
import pytest

import export_colour_util as cu
from export_colour_util import TABLE_SETS
from libde265_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    lib = capi.Library()
    assert lib.device_count() >= 1
    c = capi.Context(lib, 0)
    yield c
    c.close()


@pytest.mark.parametrize("name", ["random", "preset"])
@pytest.mark.parametrize("bit_depth", [8, 10])
def test_kernel_cases(ctx, bit_depth, name):
    cu.check_kernel_cases(ctx, bit_depth, TABLE_SETS[name], name)


@pytest.mark.parametrize("name", ["random", "preset"])
def test_wider_than_a_tile(ctx, name):
    cu.check_wide(ctx, TABLE_SETS[name], name)


@pytest.mark.parametrize("name", ["random", "preset"])
def test_tensor_and_rois(ctx, name):
    cu.check_tensors(ctx, TABLE_SETS[name], name)


def test_extreme_tables_and_neutral_grey(ctx):
    cu.check_extreme(ctx)
    cu.check_grey(ctx)


def test_handle_zero_is_the_plain_call(ctx):
    cu.check_handle_zero_is_plain(ctx)


def test_colour_export_behind_a_rejected_decode_writes_nothing(ctx):
    cu.check_gate_colour(ctx)


@pytest.mark.parametrize("depth", [1, 3])
def test_colour_export_is_waited_for_by_the_next_decode(ctx, depth):
    cu.check_hazard_colour(ctx, depth)


def test_destroy_directly_after_an_export(ctx):
    cu.check_destroy_after_export(ctx)
