"""MS-SSIM requests (m355_frame_msssim_async / m355_frame_msssim_result) on the CPU tier: the product sources under the SIMT interpreter.  What this
tier checks is the arithmetic of the two launches of k_msssim.hip (the tile grid by samples, the pyramid from LDS with its shuffles, the levels' prefix
table, both points, the reduction, the arrival count over both launches, the record left zero), the gate's verdict, the slots' scratch and the calls'
contracts; ordering between decodes is checked where launches are asynchronous (tests/test_gpu_msssim.py) — the scenarios are the same code
(tests/msssim_util.py), at the same sizes; only the plane with more than one tile at level 4 is left to the device."""
import pytest

import msssim_util as mu
import ssim_util as su
from test_emu_picture import emu_lib  # noqa: F401  (fixture)
from libde265_amd import capi


@pytest.fixture(scope="module")
def ctx(emu_lib):  # noqa: F811
    c = capi.Context(emu_lib, 0)
    yield c
    c.close()


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("levels,size", mu.PLANE_SIZES)
def test_plane_sizes_at_which_the_pyramid_can_go_wrong(ctx, levels, size, bd):
    mu.check_plane_size(ctx, levels, size[0], size[1], bd)


@pytest.mark.parametrize("cf,bdl,bdc", su.FORMATS)
def test_chroma_formats_and_bit_depths(ctx, cf, bdl, bdc):
    mu.check_format(ctx, cf, bdl, bdc, size=352)


@pytest.mark.parametrize("bd", [8, 16])
def test_extremes_and_constants(ctx, bd):
    mu.check_extremes(ctx, bd, size=176)


def test_level_0_is_the_ssim_request(ctx):
    mu.check_level_0_is_the_ssim_request(ctx)


def test_levels_are_the_scaled_export(ctx):
    mu.check_levels_are_the_scaled_export(ctx)


def test_rectangles(ctx):
    mu.check_rectangles(ctx)


def test_reference_in_pinned_host_memory(ctx):
    mu.check_pinned_reference(ctx)


def test_plane_selection(ctx):
    mu.check_plane_selection(ctx)


@pytest.mark.parametrize("as_ref_frame,with_others", [(False, False), (True, False), (False, True)])
def test_request_is_a_reader_of_its_frames(oracle, emu_lib, as_ref_frame, with_others):  # noqa: F811
    mu.check_reader_hazard(emu_lib, oracle, 3, as_ref_frame, with_others)


def test_frames_written_on_different_lanes(oracle, emu_lib):  # noqa: F811
    mu.check_two_writers(emu_lib, oracle)


def test_four_requests_in_flight(emu_lib):  # noqa: F811
    mu.check_concurrency(emu_lib)


def test_nonblocking_collection_wait_and_destroy(emu_lib):  # noqa: F811
    mu.check_nonblocking(emu_lib)


def test_slot_reused_forty_times_with_alternating_sizes(ctx):
    mu.check_slot_reuse(ctx, rounds=40)


def test_request_behind_rejected_decode(oracle, emu_lib):  # noqa: F811
    mu.check_rejected_decode(emu_lib, oracle, 1)


def test_invalid_arguments_enqueue_nothing(emu_lib):  # noqa: F811
    mu.check_invalid(emu_lib)


def test_decoded_picture(emu_lib):  # noqa: F811
    mu.check_decoded_picture(emu_lib)
