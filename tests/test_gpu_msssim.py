"""MS-SSIM requests (m355_frame_msssim_async / m355_frame_msssim_result) on the device: the plane sizes at which the pyramid can go wrong (a rim
tile without a window that still owes its blocks, odd sizes, a level one column over a tile, one window at level 4, more than one tile at level 4),
level 0 against the SSIM request and levels 1..3 against the SSIM request on scaled exports, the chroma formats and bit depths at 352 x 352 with five
levels, extremes and constants, rectangles off the tile grid, references in memory, in pinned memory and in a frame, plane selection, the request as a
reader of both frames with one and three pictures in flight, four requests in flight, the gate's verdict behind a rejected decode, one slot reused
forty times with alternating sizes, every refused call — the scenarios of tests/msssim_util.py on the product library.  Integers exact, against the
numpy restatement."""
import pytest

import msssim_util as mu
import ssim_util as su
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


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("levels,size", mu.PLANE_SIZES + [(5, mu.SIZE_5_WIDE)])
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


@pytest.mark.parametrize("depth", [1, 3])
@pytest.mark.parametrize("as_ref_frame,with_others", [(False, False), (True, False), (False, True)])
def test_request_is_a_reader_of_its_frames(oracle, gpu_lib, depth, as_ref_frame, with_others):
    mu.check_reader_hazard(gpu_lib, oracle, depth, as_ref_frame, with_others)


@pytest.mark.parametrize("depth", [1, 3])
def test_frames_written_on_different_lanes(oracle, gpu_lib, depth):
    mu.check_two_writers(gpu_lib, oracle, depth)


def test_four_requests_in_flight(gpu_lib):
    mu.check_concurrency(gpu_lib)


def test_nonblocking_collection_wait_and_destroy(gpu_lib):
    mu.check_nonblocking(gpu_lib)


def test_slot_reused_forty_times_with_alternating_sizes(ctx):
    mu.check_slot_reuse(ctx, rounds=40)


@pytest.mark.parametrize("depth", [1, 3])
def test_request_behind_rejected_decode(oracle, gpu_lib, depth):
    mu.check_rejected_decode(gpu_lib, oracle, depth)


def test_invalid_arguments_enqueue_nothing(gpu_lib):
    mu.check_invalid(gpu_lib)


def test_decoded_picture(gpu_lib):
    mu.check_decoded_picture(gpu_lib)
