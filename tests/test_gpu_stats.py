"""Statistics requests (m355_frame_stats_async / m355_frame_stats_result) on the device: histograms, sums and ranges per plane, the active area,
the light level against the restatement of the R'G'B' export and against the device's own export, the request as a reader of its frame (queued
behind the decode it follows, in front of the next decode into the frame) with one and three pictures in flight and with a hash and a comparison
pending beside it, sixteen requests in flight, the gate's verdict behind a rejected decode, one slot reused forty times, every refused call — the
scenarios of tests/stats_util.py on the product library.  All comparisons exact."""
import pytest

import stats_util as su
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
def test_request_is_a_reader_of_its_frame(oracle, gpu_lib, depth, with_others):
    su.check_reader_hazard(gpu_lib, oracle, depth, with_others)


@pytest.mark.parametrize("depth", [1, 3])
def test_request_behind_rejected_decode(oracle, gpu_lib, depth):
    su.check_rejected_decode(gpu_lib, oracle, depth)


def test_sixteen_requests_in_flight(gpu_lib):
    su.check_concurrency(gpu_lib)


def test_nonblocking_collection_wait_and_destroy(gpu_lib):
    su.check_nonblocking(gpu_lib)


def test_slot_reused_forty_times(ctx):
    su.check_slot_reuse(ctx, rounds=40)


def test_invalid_arguments_enqueue_nothing(gpu_lib):
    su.check_invalid(gpu_lib)


def test_decoded_picture(oracle, gpu_lib):
    su.check_decoded_picture(gpu_lib, oracle)
