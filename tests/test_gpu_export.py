"""m355_frame_export on the GPU: the format matrix of tests/test_export_emu.py through the real k_export instantiations, the frame hazard
(a decode into a frame waits for the export of the frame's previous picture) with one and three pictures in flight, and the shape every
1080p stream has — coded 1920x1088, window 1920x1080 — whose rows span several workgroups.  Expected values: the planes
m355_frame_download returns (checked against the oracle's decode) through the numpy restatement in export_util.py; all exact."""
import pytest

from oracle_py import Oracle
from export_util import FORMATS, check_export, check_format_matrix, check_gate, check_hazard, decode_into_frame, format_id
from libde265_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    lib = capi.Library()
    assert lib.device_count() >= 1
    c = capi.Context(lib, 0)
    yield c
    c.close()


@pytest.mark.parametrize("fmt", FORMATS, ids=format_id)
def test_export_format_matrix(ctx, oracle, fmt):
    check_format_matrix(ctx, Oracle(oracle), dict(fmt, width=64, height=32, log2_ctb=5), [None, (2, 2, 50, 22)])


@pytest.mark.parametrize("depth", [1, 3])
def test_export_is_waited_for_by_the_next_decode(ctx, depth):
    check_hazard(ctx, depth)


def test_export_behind_a_rejected_decode_writes_nothing(ctx):
    check_gate(ctx)


def test_export_1080p_window(ctx, oracle):
    cfg = dict(width=1920, height=1088, bit_depth=10, seed=7401, n_refs=1, intra_pct=5)
    frame, planes, geom, frames = decode_into_frame(ctx, Oracle(oracle), cfg)
    try:
        for samples in (capi.EXPORT_MSB16, capi.EXPORT_U8):
            check_export(ctx, frame, planes, geom, capi.EXPORT_SEMIPLANAR, samples, (0, 0, 1920, 1080), what="1080p")
    finally:
        for f in frames:
            ctx.frame_destroy(f)
