"""m355_frame_export_rgb on the GPU: the format matrix, the value cases and the chroma reconstruction cases of tests/test_export_rgb_emu.py through
the real k_export_rgb instantiations, the frame hazard (a decode into a frame waits for the RGB export of the frame's previous picture) with one and
three pictures in flight, the gate, and a 1920x1088 picture whose rows span several wavefronts.  Expected values: the planes m355_frame_download
returns through the Python-integer restatement in export_rgb_util.py; all exact."""
import pytest

from oracle_py import Oracle
from export_rgb_util import (FORMATS, LAYOUTS, MATRIX_RECT, SAMPLES, check_format_matrix_rgb, check_gate_rgb, check_hazard_rgb, check_rgb, check_values,
                             chroma_case, decode_into_frame, format_id)
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
def test_rgb_format_matrix(ctx, oracle, fmt):
    check_format_matrix_rgb(ctx, Oracle(oracle), dict(fmt, width=64, height=32, log2_ctb=5), [None, MATRIX_RECT])


@pytest.mark.parametrize("bit_depth", [8, 10, 12, 16])
def test_rgb_values_and_clips(ctx, bit_depth):
    check_values(ctx, bit_depth)


@pytest.mark.parametrize("cf,bit_depth", [(1, 8), (1, 10), (2, 8), (2, 10)])
def test_rgb_chroma_reconstruction(ctx, cf, bit_depth):
    """uploaded chroma with impulses in the plane corners: the frame-edge clamps of the filter, whole and as a rectangle with partial lanes"""
    planes = chroma_case(cf, bit_depth, 7700 + 10 * cf + bit_depth)
    frame = ctx.frame_create(32, 16, cf, bit_depth, bit_depth)
    try:
        ctx.frame_upload(frame, planes)
        for layout in LAYOUTS:
            for samples in SAMPLES:
                for rect in (None, (6, 6, 20, 8)):
                    check_rgb(ctx, frame, planes, (cf, bit_depth, bit_depth), layout, samples, capi.MATRIX_BT709, 1, rect, what="chroma case")
    finally:
        ctx.frame_destroy(frame)


@pytest.mark.parametrize("depth", [1, 3])
def test_rgb_export_is_waited_for_by_the_next_decode(ctx, depth):
    check_hazard_rgb(ctx, depth)


def test_rgb_export_behind_a_rejected_decode_writes_nothing(ctx):
    check_gate_rgb(ctx)


def test_rgb_export_1080p_window(ctx, oracle):
    """rows of 240 lanes: four wavefronts (one workgroup) per row, the last one partial.  (8, 8, 1904, 1064) starts 16 bytes into the row; the third
    rectangle starts off a vector boundary (12 bytes) and ends in a lane of two pixels"""
    cfg = dict(width=1920, height=1088, bit_depth=10, seed=7401, n_refs=1, intra_pct=5)
    frame, planes, geom, frames = decode_into_frame(ctx, Oracle(oracle), cfg)
    try:
        for rect in ((0, 0, 1920, 1080), (8, 8, 1904, 1064), (6, 8, 1906, 1064)):
            check_rgb(ctx, frame, planes, geom, capi.RGB_PACKED, capi.RGB_U8, capi.MATRIX_BT709, 0, rect, what="1080p")
            check_rgb(ctx, frame, planes, geom, capi.RGB_PLANAR, capi.RGB_U16, capi.MATRIX_BT709, 0, rect, what="1080p")
    finally:
        for f in frames:
            ctx.frame_destroy(f)
