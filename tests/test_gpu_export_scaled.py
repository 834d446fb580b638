"""m355_frame_export_scaled on the GPU: the format matrix and the value / rounding cases of tests/test_export_scaled_emu.py through the real
k_export_scaled instantiations, the frame hazard (a decode into a frame waits for the scaled export of the frame's previous picture) with one and
three pictures in flight, the gate, and a 1920x1088 picture whose rows span several wavefronts and workgroups with a partial last one.
Expected values: the planes m355_frame_download returns through the numpy restatement in export_scaled_util.py; all exact."""
import pytest

from oracle_py import Oracle
from export_scaled_util import (FORMATS, MATRIX_RECT, check_export_scaled, check_format_matrix_scaled, check_gate_scaled, check_hazard_scaled, check_values,
                                decode_into_frame, format_id)
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
def test_scaled_format_matrix(ctx, oracle, fmt):
    check_format_matrix_scaled(ctx, Oracle(oracle), dict(fmt, width=64, height=32, log2_ctb=5), [None, MATRIX_RECT])


@pytest.mark.parametrize("bit_depth", [8, 12, 16])
def test_scaled_values_and_roundings(ctx, bit_depth):
    check_values(ctx, bit_depth)


@pytest.mark.parametrize("depth", [1, 3])
def test_scaled_export_is_waited_for_by_the_next_decode(ctx, depth):
    check_hazard_scaled(ctx, depth)


def test_scaled_export_behind_a_rejected_decode_writes_nothing(ctx):
    check_gate_scaled(ctx)


def test_scaled_export_1080p_window(ctx, oracle):
    """luma rows of 3840 bytes: four wavefronts (one workgroup) per output row, the last one partial; 1080 / 8 is no integer, hence the 1072 rows at 8x"""
    cfg = dict(width=1920, height=1088, bit_depth=10, seed=7401, n_refs=1, intra_pct=5)
    frame, planes, geom, frames = decode_into_frame(ctx, Oracle(oracle), cfg)
    try:
        for samples in (capi.EXPORT_MSB16, capi.EXPORT_U8):
            for k, rect in ((1, (0, 0, 1920, 1080)), (2, (0, 0, 1920, 1080)), (3, (0, 0, 1920, 1072))):
                check_export_scaled(ctx, frame, planes, geom, capi.EXPORT_SEMIPLANAR, samples, k, rect, what="1080p")
    finally:
        for f in frames:
            ctx.frame_destroy(f)
