"""The readers of a frame (downloads, exports, hash requests: one mark per kind, Frame::reader) on the CPU tier: the scenarios of
tests/reader_marks_util.py on the product sources under the SIMT interpreter.  Every launch finishes before the next call there, so
what this tier checks is the bookkeeping — every reader is collected with the right picture, a cleared mark is not waited for, a
context with marks outstanding closes — and the ordering is checked on the device (tests/test_gpu_reader_marks.py)."""
import pytest

import reader_marks_util as ru
from hash_async_util import PIC_A, PIC_B
from test_emu_picture import emu_lib  # noqa: F401  (fixture)


@pytest.mark.parametrize("reverse", [False, True], ids=["download_export_hash", "hash_export_download"])
@pytest.mark.parametrize("depth", [1, 3])
def test_three_kinds_of_reader_on_one_frame(oracle, emu_lib, depth, reverse):  # noqa: F811
    ru.check_all_kinds(emu_lib, oracle, PIC_A, PIC_B, depth, reverse)


def test_host_waits_are_per_kind(oracle, emu_lib):  # noqa: F811
    ru.check_waits_per_kind(emu_lib, oracle, (72, 40, 1, 8, 8))


def test_two_downloads_on_different_streams(oracle, emu_lib):  # noqa: F811
    ru.check_two_downloads(emu_lib, oracle, PIC_B)


def test_collected_hash_leaves_nothing_behind(oracle, emu_lib):  # noqa: F811
    ru.check_collected_hash(emu_lib, oracle, PIC_A, PIC_B)
