"""SSIM requests (m355_frame_ssim_async / m355_frame_ssim_result) on the device: every plane size at which a tile's last column or row is
short, full or over, the chroma formats and bit depths, the extremes, rectangles, references in memory, in pinned memory and in a frame, plane
selection, maps (row tails and a guard band untouched), the request as a reader of both frames with one and three pictures in flight, sixteen
requests in flight, the gate's verdict behind a rejected decode (map untouched), one slot reused forty times, every refused call — the
scenarios of tests/ssim_util.py on the product library.  All comparisons exact, against the numpy restatement of csrc/ssim_window.h."""
import pytest

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
@pytest.mark.parametrize("pw,ph", su.PLANE_SIZES)
def test_plane_sizes_around_the_tile(ctx, pw, ph, bd):
    su.check_plane_size(ctx, pw, ph, bd)


@pytest.mark.parametrize("cf,bdl,bdc", su.FORMATS)
def test_chroma_formats_and_bit_depths(ctx, cf, bdl, bdc):
    su.check_format(ctx, cf, bdl, bdc)


@pytest.mark.parametrize("bd", [8, 16])
def test_extremes(ctx, bd):
    su.check_extremes(ctx, bd)


def test_rectangles(ctx):
    su.check_rectangles(ctx)


def test_reference_in_pinned_host_memory(ctx):
    su.check_pinned_reference(ctx)


def test_plane_selection(ctx):
    su.check_plane_selection(ctx)


@pytest.mark.parametrize("depth", [1, 3])
@pytest.mark.parametrize("as_ref_frame,with_others", [(False, False), (True, False), (False, True)])
def test_request_is_a_reader_of_its_frames(oracle, gpu_lib, depth, as_ref_frame, with_others):
    su.check_reader_hazard(gpu_lib, oracle, depth, as_ref_frame, with_others)


@pytest.mark.parametrize("depth", [1, 3])
def test_frames_written_on_different_lanes(oracle, gpu_lib, depth):
    su.check_two_writers(gpu_lib, oracle, depth)


def test_sixteen_requests_in_flight(gpu_lib):
    su.check_concurrency(gpu_lib)


def test_nonblocking_collection_wait_and_destroy(gpu_lib):
    su.check_nonblocking(gpu_lib)


def test_slot_reused_forty_times(ctx):
    su.check_slot_reuse(ctx, rounds=40)


@pytest.mark.parametrize("depth", [1, 3])
def test_request_behind_rejected_decode(oracle, gpu_lib, depth):
    su.check_rejected_decode(gpu_lib, oracle, depth)


def test_invalid_arguments_enqueue_nothing(gpu_lib):
    su.check_invalid(gpu_lib)


def test_decoded_picture(gpu_lib):
    su.check_decoded_picture(gpu_lib)
