"""Side maps of a picture's lists (m355_picture_maps_async / _result / _order) on the device: every map at every unit size on the geometries
of tests/maps_util.py, records that hang over the edges, the sampling of a unit, destinations (pitches, offsets, pinned host memory, guards), uncovered
units, records no check has seen, the hazards of the arenas (m355_picture_replace behind a request; six submits with a request on
M355_PICTURE_LAST each, the ring of three arenas wrapping twice, with one and three pictures in flight), sixteen requests in flight, one slot reused
forty times, m355_picture_maps_order onto a stream of the test's own, every refused call, and decodes undisturbed — the scenarios of
tests/maps_util.py on the product library.  All comparisons exact."""
import ctypes

import numpy as np
import pytest

import maps_util as mu
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
def test_six_submits_each_with_a_request_on_the_last_picture(oracle, gpu_lib, depth):
    mu.check_submit_ring(gpu_lib, oracle, depth)


def test_sixteen_requests_in_flight(gpu_lib):
    mu.check_concurrency(gpu_lib)


def test_nonblocking_collection_wait_release_and_destroy(gpu_lib):
    mu.check_nonblocking(gpu_lib)


def test_slot_reused_forty_times(ctx):
    mu.check_slot_reuse(ctx, rounds=40)


def _runtime_of(lib):
    """the HIP runtime the product library runs on, as a ctypes handle: the copy of libamdhip64 mapped into this process (the one the dynamic linker
    bound the library to; should there be two, the one that is not torch's, which the library was linked against)"""
    paths = []
    with open("/proc/self/maps") as f:
        for line in f:
            if "libamdhip64" in line and line.split()[-1] not in paths:
                paths.append(line.split()[-1])
    assert paths, "no HIP runtime is mapped"
    own = [p for p in paths if "torch" not in p]
    return ctypes.CDLL((own or paths)[0])


def test_order_onto_a_stream_of_the_tests_own(gpu_lib, ctx):
    hip = _runtime_of(gpu_lib)
    vp = ctypes.c_void_p
    hip.hipStreamCreate.argtypes = [ctypes.POINTER(vp)]
    hip.hipMemcpyAsync.argtypes = [vp, vp, ctypes.c_size_t, ctypes.c_int, vp]
    hip.hipStreamSynchronize.argtypes = [vp]
    hip.hipStreamDestroy.argtypes = [vp]
    st = vp()
    assert hip.hipStreamCreate(ctypes.byref(st)) == 0
    try:
        def read(p, nbytes):
            host = gpu_lib.lib.m355_host_alloc(nbytes)
            assert host
            try:
                assert hip.hipMemcpyAsync(host, p, nbytes, 2, st) == 0          # hipMemcpyDeviceToHost, on the consumer's stream
                assert hip.hipStreamSynchronize(st) == 0
                return np.ctypeslib.as_array(ctypes.cast(host, ctypes.POINTER(ctypes.c_uint8)), (nbytes,)).copy()
            finally:
                gpu_lib.lib.m355_host_free(host)

        mu.check_order(ctx, st, read)
    finally:
        hip.hipStreamDestroy(st)


@pytest.mark.parametrize("case", mu.rejections(), ids=lambda c: c["what"])
def test_refused_calls_enqueue_nothing(gpu_lib, case):
    mu.check_rejection(gpu_lib, case)


def test_refused_collections(gpu_lib):
    mu.check_result_rejections(gpu_lib)


def test_decodes_undisturbed(oracle, gpu_lib):
    mu.check_decodes_undisturbed(gpu_lib, oracle)
