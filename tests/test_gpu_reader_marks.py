"""The readers of a frame (downloads, exports, hash requests: one mark per kind, Frame::reader) on the device, where launches are
asynchronous: the scenarios of tests/reader_marks_util.py on the product library.

Shapes: 1920x1080, 8 bit — a copy of such a frame lasts long enough for a decode that did not wait for it to land inside it; the
geometry of tests/test_gpu_pipeline.py's download test (832x480, 10 bit, two tile columns) for the scenarios that decode into a frame
with readers outstanding; and the 64x64 pictures of the CPU tier."""
import pytest

import reader_marks_util as ru
from hash_async_util import PIC_A, PIC_B
from libde265_amd import capi

pytestmark = pytest.mark.gpu

PAIRS = {"64x64": (PIC_A, PIC_B), "832x480_10bit": (ru.PIPE_A, ru.PIPE_B), "1920x1080": (ru.HD_A, ru.HD_B)}


@pytest.fixture(scope="module")
def gpu_lib():
    lib = capi.Library()          # raises if the HIP library is missing — no fallback
    assert lib.device_count() >= 1, "no HIP device visible"
    return lib


@pytest.mark.parametrize("reverse", [False, True], ids=["download_export_hash", "hash_export_download"])
@pytest.mark.parametrize("depth", [1, 3])
@pytest.mark.parametrize("pair", list(PAIRS))
def test_three_kinds_of_reader_on_one_frame(oracle, gpu_lib, pair, depth, reverse):
    ru.check_all_kinds(gpu_lib, oracle, PAIRS[pair][0], PAIRS[pair][1], depth, reverse)


def test_host_waits_are_per_kind(oracle, gpu_lib):
    ru.check_waits_per_kind(gpu_lib, oracle, (1920, 1080, 1, 8, 8))


@pytest.mark.parametrize("pair", ["832x480_10bit", "1920x1080"])
def test_two_downloads_on_different_streams(oracle, gpu_lib, pair):
    ru.check_two_downloads(gpu_lib, oracle, PAIRS[pair][0])


def test_collected_hash_leaves_nothing_behind(oracle, gpu_lib):
    ru.check_collected_hash(gpu_lib, oracle, ru.HD_A, ru.HD_B)
