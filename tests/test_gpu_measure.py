"""Comparison requests (m355_frame_measure_async / m355_frame_measure_result) on the device: values against memory and against a frame,
the sample ranges, the first difference, the request as a reader of both frames (queued behind the decodes it follows, in front of the next
decode into either frame) with one and three pictures in flight, sixteen requests in flight, the gate's verdict behind a rejected decode,
one slot reused forty times, every refused call — the scenarios of tests/measure_util.py on the product library.  All comparisons exact."""
import pytest

import measure_util as mu
from libde265_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu_lib():
    lib = capi.Library()          # raises if the HIP library is missing — no fallback
    assert lib.device_count() >= 1, "no HIP device visible"
    return lib


@pytest.fixture(scope="module")
def ctx(gpu_lib):
    c = capi.Context(gpu_lib, 0)
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
def test_request_is_a_reader_of_its_frames(oracle, gpu_lib, depth, as_ref_frame, with_others):
    mu.check_reader_hazard(gpu_lib, oracle, depth, as_ref_frame, with_others)


def test_frames_written_on_different_lanes(oracle, gpu_lib):
    mu.check_two_writers(gpu_lib, oracle)


def test_ref_frame_rejected_on_another_lane(oracle, gpu_lib):
    mu.check_rejected_ref_frame_other_lane(gpu_lib, oracle)


def test_sixteen_requests_in_flight(gpu_lib):
    mu.check_concurrency(gpu_lib)


def test_nonblocking_collection_wait_and_destroy(gpu_lib):
    mu.check_nonblocking(gpu_lib)


def test_slot_reused_forty_times(ctx):
    mu.check_slot_reuse(ctx, rounds=40)


@pytest.mark.parametrize("depth", [1, 3])
def test_request_behind_rejected_decode(oracle, gpu_lib, depth):
    mu.check_rejected_decode(gpu_lib, oracle, depth)


def test_invalid_arguments_enqueue_nothing(gpu_lib):
    mu.check_invalid(gpu_lib)


def test_decoded_picture(gpu_lib):
    mu.check_decoded_picture(gpu_lib)
