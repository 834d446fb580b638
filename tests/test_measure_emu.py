"""Comparison requests (m355_frame_measure_async / m355_frame_measure_result) on the CPU tier: the product sources under the SIMT interpreter.
What this tier checks is the arithmetic of k_measure_req (spans, row sums, ranges, the first difference, the arrival count, the record left
zero), the gate's verdict, the slot / ticket bookkeeping and the calls' contracts; that a request is ordered between the decodes it follows
and the next decode into either frame is checked where launches are asynchronous (tests/test_gpu_measure.py) — the scenarios are the same
code (tests/measure_util.py), and here they walk the bookkeeping."""
import pytest

import measure_util as mu
from test_emu_picture import emu_lib  # noqa: F401  (fixture)
from libde265_amd import capi


@pytest.fixture(scope="module")
def ctx(emu_lib):  # noqa: F811
    c = capi.Context(emu_lib, 0)
    yield c
    c.close()


@pytest.mark.parametrize("geom", mu.SHAPES)
def test_values_against_memory_and_against_a_frame(ctx, geom):
    mu.check_values(ctx, geom)


def test_rectangles(ctx):
    mu.check_rectangles(ctx)


def test_reference_in_pinned_host_memory(ctx):
    mu.check_pinned_reference(ctx)


# 2056 x 8 at 16 bit: rows of 4112 bytes, five steps of a lane per row — a 32-bit row sum overflows here; 64 x 12296: three rows per wavefront
@pytest.mark.parametrize("w,h,bd", [(2056, 8, 16), (64, 12296, 16), (2056, 8, 12), (2056, 8, 8)])
def test_largest_differences(ctx, w, h, bd):
    mu.check_extremes(ctx, w, h, bd)


def test_ramps_against_reversed_ramps(ctx):
    mu.check_ramps(ctx)


def test_first_difference_and_counts(ctx):
    mu.check_first_and_counts(ctx)


@pytest.mark.parametrize("depth", [1, 3])
@pytest.mark.parametrize("as_ref_frame,with_others", [(False, False), (True, False), (False, True)])
def test_request_is_a_reader_of_its_frames(oracle, emu_lib, depth, as_ref_frame, with_others):  # noqa: F811
    mu.check_reader_hazard(emu_lib, oracle, depth, as_ref_frame, with_others)


def test_frames_written_on_different_lanes(oracle, emu_lib):  # noqa: F811
    mu.check_two_writers(emu_lib, oracle)


def test_ref_frame_rejected_on_another_lane(oracle, emu_lib):  # noqa: F811
    mu.check_rejected_ref_frame_other_lane(emu_lib, oracle)


def test_sixteen_requests_in_flight(emu_lib):  # noqa: F811
    mu.check_concurrency(emu_lib)


def test_nonblocking_collection_wait_and_destroy(emu_lib):  # noqa: F811
    mu.check_nonblocking(emu_lib)


def test_slot_reused_forty_times(ctx):
    mu.check_slot_reuse(ctx, rounds=40)


@pytest.mark.parametrize("depth", [1, 3])
def test_request_behind_rejected_decode(oracle, emu_lib, depth):  # noqa: F811
    mu.check_rejected_decode(emu_lib, oracle, depth)


def test_invalid_arguments_enqueue_nothing(emu_lib):  # noqa: F811
    mu.check_invalid(emu_lib)


def test_decoded_picture(emu_lib):  # noqa: F811
    mu.check_decoded_picture(emu_lib)
