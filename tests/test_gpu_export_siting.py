"""Chroma sample location types 0..3 (m355_export_opts) on the GPU: the cases of tests/test_export_siting_emu.py through the real instantiations —
k_export_rgb<.., LOC>, k_export_resized with a vertical flag per plane, k_export_resized_rgb in its three modes and both filters —, frames just wider
than one wavefront's chunk of k_export_rgb, where the CENTRE form's left neighbour crosses a lane, a wave and a vector boundary, the gate, and the
frame hazard with one and three pictures in flight.  Expected values: export_siting_util.py; all exact."""
import pytest

from export_siting_util import (check_chroma_case, check_constant_stays_constant, check_gate_rgb_sited, check_hazard_rgb_sited, check_lane_boundaries,
                                check_resized_sited, check_tensors_sited, check_type0_is_plain, check_wide)
from libde265_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    lib = capi.Library()
    assert lib.device_count() >= 1
    c = capi.Context(lib, 0)
    yield c
    c.close()


@pytest.mark.parametrize("bit_depth", [8, 10])
def test_type_0_through_the_opts_entry_points_is_the_plain_call(ctx, bit_depth):
    check_type0_is_plain(ctx, bit_depth)


@pytest.mark.parametrize("loc", [1, 2, 3])
@pytest.mark.parametrize("bit_depth", [8, 10])
def test_rgb_types_1_to_3(ctx, bit_depth, loc):
    check_chroma_case(ctx, bit_depth, loc)


@pytest.mark.parametrize("loc", [1, 2, 3])
@pytest.mark.parametrize("bit_depth", [8, 10])
def test_resized_and_composed_types_1_to_3(ctx, bit_depth, loc):
    check_resized_sited(ctx, bit_depth, loc)
    check_constant_stays_constant(ctx, bit_depth, loc)


@pytest.mark.parametrize("loc", [1, 3])
def test_composed_export_wider_than_a_tile(ctx, loc):
    check_wide(ctx, loc)


def test_tensor_and_rois_type_2(ctx):
    check_tensors_sited(ctx, 2)


@pytest.mark.parametrize("loc", [1, 3])
@pytest.mark.parametrize("size,bit_depth", [((1056, 16), 8), ((544, 16), 10)])
def test_rgb_centre_across_lane_wave_and_vector_boundaries(ctx, size, bit_depth, loc):
    """1056 8-bit and 544 10-bit pixels: one full wavefront chunk (1024 / 512 pixels) and a second wavefront of two / four lanes"""
    check_lane_boundaries(ctx, size, bit_depth, loc)


def test_rgb_opts_export_behind_a_rejected_decode_writes_nothing(ctx):
    check_gate_rgb_sited(ctx, 2)


@pytest.mark.parametrize("depth", [1, 3])
def test_rgb_opts_export_is_waited_for_by_the_next_decode(ctx, depth):
    check_hazard_rgb_sited(ctx, depth, 2)
