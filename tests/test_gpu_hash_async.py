"""Hash requests (m355_frame_hash_async / m355_frame_hash_result) on the device: values, the request as a reader of its frame
(queued behind the decode it follows, in front of the next decode into the frame), sixteen requests in flight, the gate's
verdict behind a rejected decode, one slot reused forty times — the scenarios of tests/hash_async_util.py on the product library.

Shapes: frame sizes are multiples of 8, so the rows are 1032 bytes (one 1 KB block + 8 bytes: no multiple of 16; chroma rows of
516) and 520 samples of 10 bit (1040 bytes: a block + one lane; chroma 520), in all four chroma formats (one plane: another
arrival count); 64 x 8 monochrome (two workgroups, the legal minimum of rows); 64 x 12296 monochrome (0.8 MB: three rows per
wavefront, the last span short); and GEOMS of tests/test_hash.py."""
import pytest

import hash_async_util as hu
from golden_io import load_gold
from hash_util import MD5, CRC, CHECKSUM
from test_hash import GEOMS
from libde265_amd import capi

pytestmark = pytest.mark.gpu

SHAPES = [(1032, 16, cf, 8, 8) for cf in range(4)] + [(520, 16, cf, 10, 10) for cf in range(4)] + [(64, 8, 0, 8, 8), (64, 12296, 0, 8, 8)]


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


@pytest.mark.parametrize("geom", SHAPES + GEOMS)
def test_async_values_match_sync_and_oracle(oracle, ctx, geom):
    hu.check_values(ctx, oracle, geom)


@pytest.mark.parametrize("types,with_export", [((MD5,), False), ((CRC,), False), ((CHECKSUM,), False), (hu.TYPES, False), (hu.TYPES, True)])
def test_hash_is_a_reader_of_the_frame(oracle, gpu_lib, types, with_export):
    hu.check_reader_hazard(gpu_lib, oracle, types, with_export)


def test_sixteen_requests_in_flight(oracle, gpu_lib):
    hu.check_concurrency(gpu_lib, oracle)


def test_nonblocking_collection_and_bad_arguments(oracle, gpu_lib):
    hu.check_nonblocking(gpu_lib, oracle)


@pytest.mark.parametrize("depth", [1, 3])
def test_hash_behind_rejected_decode(oracle, gpu_lib, depth):
    hu.check_rejected_decode(gpu_lib, oracle, depth)


def test_slot_reused_forty_times(oracle, ctx):
    hu.check_slot_reuse(ctx, oracle, rounds=40)


def test_hash_behind_decoded_picture(gpu_lib):
    """one girlshy picture hashed behind its decode, nothing waited for first: the MD5 recorded from the reference's planes"""
    hdr, pics = load_gold("girlshy_full.m355gold.gz")
    c = capi.Context(gpu_lib, 0)
    try:
        pic = pics[0]
        dst = c.frame_create_for(pic.pp[0])
        saved = pic.dst_frame
        pic.dst_frame = dst
        c.set_pipeline_depth(3)
        c.submit(pic)
        pic.dst_frame = saved
        tickets = [c.frame_hash_async(dst, t) for t in (MD5, CRC, CHECKSUM)]
        assert [m.hex() for m in c.frame_hash_result(tickets[0])] == pic.meta["md5"]
        got = [c.frame_hash_result(tk) for tk in tickets[1:]]
        assert got == [c.frame_hash(dst, t) for t in (CRC, CHECKSUM)]
    finally:
        c.close()
