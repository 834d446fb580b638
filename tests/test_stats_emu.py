"""Statistics requests (m355_frame_stats_async / m355_frame_stats_result) on the CPU tier: the product sources under the SIMT interpreter.
What this tier checks is the arithmetic of k_stats_req (units and spans, tails, the histograms in LDS and their flush, the ranges of the sums, the
encodings whose neutral value is 0, the light level against the restatement of the R'G'B' export, the arrival count, the record left zero), the
gate's verdict, the slot / ticket bookkeeping and the calls' contracts; that a request is ordered between the decode it follows and the next decode
into the frame is checked where launches are asynchronous (tests/test_gpu_stats.py) — the scenarios are the same code (tests/stats_util.py)."""
import pytest

import stats_util as su
from test_emu_picture import emu_lib  # noqa: F401  (fixture)
from libde265_amd import capi


@pytest.fixture(scope="module")
def ctx(emu_lib):  # noqa: F811
    c = capi.Context(emu_lib, 0)
    yield c
    c.close()


@pytest.mark.parametrize("geom", su.SHAPES)
def test_values(ctx, geom):
    su.check_values(ctx, geom)


# 2056 x 8 at 16 bit: the sum of squares of one row leaves 32 bits; bin 255 alone
@pytest.mark.parametrize("w,h,bd", [(2056, 8, 16), (2056, 8, 12), (2056, 8, 8)])
def test_largest_samples(ctx, w, h, bd):
    su.check_extremes(ctx, w, h, bd)


def test_bin_shift_is_per_plane(ctx):
    su.check_plane_depths(ctx)


def test_constant_zero_ramp_and_alternating_content(ctx):
    su.check_content(ctx)


def test_rectangles(ctx):
    su.check_rectangles(ctx)


def test_active_area(ctx):
    su.check_active_area(ctx)


def test_light_matrices_and_ranges(ctx):
    su.check_light_conversions(ctx)


@pytest.mark.parametrize("geom", [(1032, 16, 1, 8, 8), (520, 16, 1, 10, 10)])
def test_light_chroma_sample_locations(ctx, geom):
    su.check_light_siting(ctx, geom)


def test_light_other_chroma_formats(ctx):
    su.check_light_formats(ctx)


def test_light_clips_at_both_ends(ctx):
    su.check_light_clips(ctx)


def test_light_is_the_devices_own_rgb_export(ctx):
    su.check_light_against_export(ctx)


@pytest.mark.parametrize("depth", [1, 3])
@pytest.mark.parametrize("with_others", [False, True])
def test_request_is_a_reader_of_its_frame(oracle, emu_lib, depth, with_others):  # noqa: F811
    su.check_reader_hazard(emu_lib, oracle, depth, with_others)


@pytest.mark.parametrize("depth", [1, 3])
def test_request_behind_rejected_decode(oracle, emu_lib, depth):  # noqa: F811
    su.check_rejected_decode(emu_lib, oracle, depth)


def test_sixteen_requests_in_flight(emu_lib):  # noqa: F811
    su.check_concurrency(emu_lib)


def test_nonblocking_collection_wait_and_destroy(emu_lib):  # noqa: F811
    su.check_nonblocking(emu_lib)


def test_slot_reused_forty_times(ctx):
    su.check_slot_reuse(ctx, rounds=40)


def test_invalid_arguments_enqueue_nothing(emu_lib):  # noqa: F811
    su.check_invalid(emu_lib)


def test_decoded_picture(oracle, emu_lib):  # noqa: F811
    su.check_decoded_picture(emu_lib, oracle)
