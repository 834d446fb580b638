"""Hash requests (m355_frame_hash_async / m355_frame_hash_result) on the CPU tier: the product sources under the SIMT interpreter.
What this tier checks is the arithmetic of the request kernel (spans, arrival count, the record left zero), the gate's verdict, the
slot / ticket bookkeeping and the calls' contracts; that a request is ordered between the decode it follows and the next decode
into the frame is checked where launches are asynchronous (tests/test_gpu_hash_async.py) — the scenarios are the same code
(tests/hash_async_util.py).

One property cannot be observed from outside and is kept by reading the code: m355_frame_hash_async and what it calls
(reader_begin, reader_end, hash_planes_take, ev_wait, ev_mark, m355_launch_frame_hash_req) contain no sync_all, hipStreamSynchronize,
hipEventSynchronize or hipDeviceSynchronize."""
import pytest

import hash_async_util as hu
from hash_util import MD5, CRC, CHECKSUM
from test_emu_picture import emu_lib  # noqa: F401  (fixture)
from test_hash import GEOMS
from libde265_amd import capi


@pytest.fixture(scope="module")
def ctx(emu_lib):  # noqa: F811
    c = capi.Context(emu_lib, 0)
    yield c
    c.close()


@pytest.mark.parametrize("geom", GEOMS)
def test_async_values_match_sync_and_oracle(oracle, ctx, geom):
    hu.check_values(ctx, oracle, geom)


@pytest.mark.parametrize("types,with_export", [((MD5,), False), ((CRC,), False), ((CHECKSUM,), False), (hu.TYPES, False), (hu.TYPES, True)])
def test_hash_is_a_reader_of_the_frame(oracle, emu_lib, types, with_export):  # noqa: F811
    hu.check_reader_hazard(emu_lib, oracle, types, with_export)


def test_sixteen_requests_in_flight(oracle, emu_lib):  # noqa: F811
    hu.check_concurrency(emu_lib, oracle)


def test_nonblocking_collection_and_bad_arguments(oracle, emu_lib):  # noqa: F811
    hu.check_nonblocking(emu_lib, oracle)


@pytest.mark.parametrize("depth", [1, 3])
def test_hash_behind_rejected_decode(oracle, emu_lib, depth):  # noqa: F811
    hu.check_rejected_decode(emu_lib, oracle, depth)


def test_slot_reused(oracle, ctx):
    hu.check_slot_reuse(ctx, oracle)
