"""M355_GLUE_ASYNC_HASH=1: the glue's process_sei enqueues the picture's hash behind its decode (m355_frame_hash_async) instead of
waiting for the picture, and takes the verdict when the picture leaves the decoder.  The specification is the one of the
synchronous path — tests/test_sei_hash.py's run(): every picture hashed where it lives, none downloaded, no warning on the good
stream, DE265_ERROR_CHECKSUM_MISMATCH (5) on the stream whose last picture carries a wrong hash, output identical to the
reference — plus an application that fetches nothing until the stream is flushed."""
import ctypes

import pytest

import de265_py
import sei_util
from test_emu_picture import emu_lib, EMU_SO  # noqa: F401  (fixture)
from test_glue_live import glue_lib
from test_sei_hash import run, GPU_CASES
from test_streams import make_stream


@pytest.mark.parametrize("hash_type", [sei_util.MD5, sei_util.CRC, sei_util.CHECKSUM])
def test_async_sei_hash_emulated_backend(ref, oracle, emu_lib, tmp_path, monkeypatch, hash_type):  # noqa: F811
    monkeypatch.setenv("M355_LIB", EMU_SO)
    monkeypatch.setenv("M355_GLUE_ASYNC_HASH", "1")
    run(ref, oracle, tmp_path, 192, 128, 8, 1, 1, 3, 81 + hash_type, 0, 1, hash_type, 2)


@pytest.mark.gpu
@pytest.mark.parametrize("case,hash_type", [(GPU_CASES[0], sei_util.CRC), (GPU_CASES[1], sei_util.MD5)])
def test_async_sei_hash_gpu(ref, oracle, tmp_path, monkeypatch, case, hash_type):
    monkeypatch.delenv("M355_LIB", raising=False)
    monkeypatch.setenv("M355_GLUE_ASYNC_HASH", "1")
    run(ref, oracle, tmp_path, *case, hash_type, 8)


def late_fetch(lib, data):
    """decode everything the data allows without fetching a picture, flush, then fetch -> (pictures, warnings + errors, hashed)"""
    app = de265_py.App(lib, threads=2)
    try:
        lib.de265_set_parameter_bool(app.ctx, de265_py.PARAM_BOOL_SEI_CHECK_HASH, 1)
        app.push(data)
        more = ctypes.c_int(1)
        while more.value:
            more.value = 0
            if lib.de265_decode(app.ctx, ctypes.byref(more)) != de265_py.DE265_OK:      # (13: waiting for input data)
                break
        app.flush()
        app.drain()
        warnings = []
        while True:
            wn = lib.de265_get_warning(app.ctx)
            if wn == de265_py.DE265_OK:
                break
            warnings.append(wn)
        lib.m355_glue_hashed_pictures.restype = ctypes.c_longlong
        lib.m355_glue_hashed_pictures.argtypes = [ctypes.c_void_p]
        return app.n, warnings + app.errs, lib.m355_glue_hashed_pictures(app.ctx)
    finally:
        app.close()


def test_async_verdicts_without_fetching(ref, oracle, emu_lib, tmp_path, monkeypatch):  # noqa: F811
    monkeypatch.setenv("M355_LIB", EMU_SO)
    monkeypatch.setenv("M355_GLUE_ASYNC_HASH", "1")
    frames = 3
    data = make_stream(tmp_path, 192, 128, 8, 1, 1, frames, 85, 10, 1, 1, 0, 1, 1)
    pics = []
    assert de265_py.decode_stream(ref, data, planes_out=pics)[1] == frames
    good = sei_util.add_hash_seis(data, pics, 8, sei_util.CRC, oracle)
    bad = sei_util.add_hash_seis(data, pics, 8, sei_util.CRC, oracle, corrupt_picture=frames - 1)
    lib = glue_lib()
    n, problems, hashed = late_fetch(lib, good)
    assert (n, hashed) == (frames, frames) and 5 not in problems, (n, problems, hashed)
    n, problems, hashed = late_fetch(lib, bad)
    assert n == frames and hashed == frames and 5 in problems, (n, problems, hashed)
