"""Side maps of a picture's lists (m355_picture_maps_async / _result / _order) on the CPU tier: the product sources under the SIMT interpreter.
What this tier checks is the arithmetic of k_maps_raster and k_maps_gather (which records count, the cells a record covers and their clipping, the
prefix sums and the owner search across a wavefront, the sampling of a unit, the store widths at row heads and tails, the summary's encodings, the
arrival count, the record left zero) — with records that NO check has seen, which makes this tier the memory-safety check in front of the device —,
the slot / ticket bookkeeping and the calls' contracts.  That a request is ordered between the upload of its lists and whatever overwrites them is
checked where launches are asynchronous (tests/test_gpu_maps.py) — the scenarios are the same code (tests/maps_util.py)."""
import pytest

import maps_util as mu
from test_emu_picture import emu_lib  # noqa: F401  (fixture)
from libde265_amd import capi


@pytest.fixture(scope="module")
def ctx(emu_lib):  # noqa: F811
    c = capi.Context(emu_lib, 0)
    yield c
    c.close()


def test_geometries_reach_their_cases():
    mu.assert_geometries_reach_their_cases()


@pytest.mark.parametrize("log2_unit", mu.UNITS)
@pytest.mark.parametrize("name", list(mu.GEOMETRIES))
def test_geometries_and_units(ctx, name, log2_unit):
    mu.check_geometry(ctx, name, log2_unit)


def test_records_clipped_by_both_edges(ctx):
    mu.check_clipped(ctx)


def test_a_unit_takes_its_top_left_value(ctx):
    mu.check_sampling(ctx)


def test_destinations_pitches_offsets_host_memory_guards(ctx):
    mu.check_destinations(ctx)


def test_uncovered_units_hold_the_none_values(ctx):
    mu.check_uncovered(ctx)


def test_skipped_records_are_counted_and_nothing_else_changes(ctx):
    mu.check_skipped(ctx)


def test_replace_behind_a_request(ctx):
    mu.check_replace_hazard(ctx)


@pytest.mark.parametrize("depth", [1, 3])
def test_six_submits_each_with_a_request_on_the_last_picture(oracle, emu_lib, depth):  # noqa: F811
    mu.check_submit_ring(emu_lib, oracle, depth)


def test_sixteen_requests_in_flight(emu_lib):  # noqa: F811
    mu.check_concurrency(emu_lib)


def test_nonblocking_collection_wait_release_and_destroy(emu_lib):  # noqa: F811
    mu.check_nonblocking(emu_lib)


def test_slot_reused_forty_times(ctx):
    mu.check_slot_reuse(ctx, rounds=40)


def test_order_onto_a_stream(ctx):
    mu.check_order(ctx, ctx.stream(), ctx.device_read)


@pytest.mark.parametrize("case", mu.rejections(), ids=lambda c: c["what"])
def test_refused_calls_enqueue_nothing(emu_lib, case):  # noqa: F811
    mu.check_rejection(emu_lib, case)


def test_refused_collections(emu_lib):  # noqa: F811
    mu.check_result_rejections(emu_lib)


def test_decodes_undisturbed(oracle, emu_lib):  # noqa: F811
    mu.check_decodes_undisturbed(emu_lib, oracle)
