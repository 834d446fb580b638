"""M355_GLUE_NARROW=1: the glue's recorder (glue/m355_glue.cc scale_coefficients) writes the blocks that allow it as 16-bit entries
(M355_RBF_NARROW).  One generated I/P stream decoded live with the switch on and with it unset: both give the reference decoder's MD5,
and only the first records narrow blocks.  Markers and skip conditions are those of test_glue_live.py / test_streams.py."""
import pytest

import de265_py
from libde265_amd import capi
from test_emu_picture import emu_lib, EMU_SO  # noqa: F401  (fixture)
from test_glue_live import glue_lib
from test_streams import make_stream

STREAM = (256, 128, 8, 1, 1, 3, 77)      # w, h, bit depth, tile cols, tile rows, frames, seed


def narrow_blocks(lib):
    import ctypes
    lib.m355_glue_narrow_blocks.restype = ctypes.c_longlong
    return lib.m355_glue_narrow_blocks()


def check(ref, tmp_path, monkeypatch, backend, stream=STREAM):
    data = make_stream(tmp_path, *stream, intra_pct=20)
    want = de265_py.decode_stream(ref, data, threads=0, scalar=True)
    assert want[1] == stream[5] and not want[2], "the reference itself rejects the generated stream: %r" % (want,)
    lib = glue_lib()
    n0 = narrow_blocks(lib)
    monkeypatch.delenv("M355_GLUE_NARROW", raising=False)
    plain = de265_py.decode_stream(lib, data, threads=0)
    assert narrow_blocks(lib) == n0, "narrow blocks recorded with the switch unset"
    monkeypatch.setenv("M355_GLUE_NARROW", "1")
    narrow = de265_py.decode_stream(lib, data, threads=0)
    assert narrow_blocks(lib) > n0, "M355_GLUE_NARROW=1 recorded no narrow block"
    assert plain[:2] == want[:2] and narrow[:2] == want[:2], "live decode differs from the reference decoder"
    assert lib.m355_glue_cpu_pixel_calls() == 0
    import os
    assert os.path.realpath(lib.m355_glue_backend_path().decode()) == os.path.realpath(backend)


def test_narrow_recording_emulated_backend(ref, emu_lib, tmp_path, monkeypatch):  # noqa: F811
    monkeypatch.setenv("M355_LIB", EMU_SO)
    check(ref, tmp_path, monkeypatch, EMU_SO)


def test_narrow_recording_across_ranks_emulated_backend(ref, emu_lib, tmp_path, monkeypatch):  # noqa: F811
    """M355_GLUE_RANKS: the glue's per-rank cut of the coefficient list copies a narrow block's (ncoeff + 1) / 2 words"""
    monkeypatch.setenv("M355_LIB", EMU_SO)
    monkeypatch.setenv("M355_GLUE_RANKS", "2")
    check(ref, tmp_path, monkeypatch, EMU_SO, stream=(256, 128, 8, 2, 1, 3, 78))


@pytest.mark.gpu
def test_narrow_recording_gpu(ref, tmp_path, monkeypatch):
    monkeypatch.delenv("M355_LIB", raising=False)
    check(ref, tmp_path, monkeypatch, capi.DEFAULT_LIB)
