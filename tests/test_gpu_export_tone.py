"""Tone objects of the composed exports on the GPU: the cases of tests/test_export_tone_emu.py through the real instantiations of k_export_resized_rgb
with the gain — its table read from global memory, the 64-bit multiply-adds of the device —, in the three modes, both filters and both sitings; the
gate, the frame hazard with one and three pictures in flight, and m355_colour_destroy directly behind an export.  Expected values:
export_tone_util.py; all exact."""
import pytest

import export_tone_util as tu
from export_tone_util import SETS
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
    tu.check_kernel_cases(ctx, bit_depth, SETS[name], name)


@pytest.mark.parametrize("name", ["random", "preset"])
def test_wider_than_a_tile(ctx, name):
    tu.check_wide(ctx, SETS[name], name)


@pytest.mark.parametrize("name", ["random", "preset"])
def test_tensor_and_rois(ctx, name):
    tu.check_tensors(ctx, SETS[name], name)


def test_extreme_set(ctx):
    tu.check_extreme(ctx)


def test_unit_gain_is_the_plain_object(ctx):
    tu.check_unit_gain_is_plain(ctx)


def test_tone_export_behind_a_rejected_decode_writes_nothing(ctx):
    tu.check_gate(ctx)


@pytest.mark.parametrize("depth", [1, 3])
def test_tone_export_is_waited_for_by_the_next_decode(ctx, depth):
    tu.check_hazard(ctx, depth)


def test_destroy_directly_after_an_export(ctx):
    tu.check_destroy_after_export(ctx)
