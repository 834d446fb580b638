"""SSIM requests (m355_frame_ssim_async / m355_frame_ssim_result) on the CPU tier: the product sources under the SIMT interpreter.  What this
tier checks is the arithmetic of k_ssim_req (tiles, the two passes through LDS, the point, the map, the reduction, the arrival count, the
record left zero), the gate's verdict, the slot / ticket bookkeeping and the calls' contracts; that a request is ordered between the decodes it
follows and the next decode into either frame is checked where launches are asynchronous (tests/test_gpu_ssim.py) — the scenarios are the same
code (tests/ssim_util.py), and here they walk the bookkeeping."""
import pytest

import ssim_util as su
from test_emu_picture import emu_lib  # noqa: F401  (fixture)
from libde265_amd import capi


@pytest.fixture(scope="module")
def ctx(emu_lib):  # noqa: F811
    c = capi.Context(emu_lib, 0)
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


@pytest.mark.parametrize("as_ref_frame,with_others", [(False, False), (True, False), (False, True)])
def test_request_is_a_reader_of_its_frames(oracle, emu_lib, as_ref_frame, with_others):  # noqa: F811
    su.check_reader_hazard(emu_lib, oracle, 3, as_ref_frame, with_others)


def test_frames_written_on_different_lanes(oracle, emu_lib):  # noqa: F811
    su.check_two_writers(emu_lib, oracle)


def test_sixteen_requests_in_flight(emu_lib):  # noqa: F811
    su.check_concurrency(emu_lib)


def test_nonblocking_collection_wait_and_destroy(emu_lib):  # noqa: F811
    su.check_nonblocking(emu_lib)


def test_slot_reused_forty_times(ctx):
    su.check_slot_reuse(ctx, rounds=40)


def test_request_behind_rejected_decode(oracle, emu_lib):  # noqa: F811
    su.check_rejected_decode(emu_lib, oracle, 1)


def test_invalid_arguments_enqueue_nothing(emu_lib):  # noqa: F811
    su.check_invalid(emu_lib)


def test_decoded_picture(emu_lib):  # noqa: F811
    su.check_decoded_picture(emu_lib)
