"""m355_frame_export_resized on the GPU: the format matrix, the value cases, the identity and the smallest sizes of tests/test_export_resized_emu.py
through the real k_export_resized instantiations, the frame hazard (a decode into a frame waits for the resized export of the frame's previous
picture) with one and three pictures in flight, the gate, several tiles per row, and a 1920x1088 picture whose tiles span many workgroups, down to
three sizes (one with a partial last tile) and up to one.  Expected values: the planes m355_frame_download returns through the restatement in
export_resized_util.py; all exact."""
import pytest

from oracle_py import Oracle
from export_resized_util import (FORMATS, check_export_resized, check_format_matrix_resized, check_gate_resized, check_hazard_resized, check_identity,
                                 check_minimum_sizes, check_several_tiles, check_values, decode_into_frame, format_id)
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
def test_resized_format_matrix(ctx, oracle, fmt):
    check_format_matrix_resized(ctx, Oracle(oracle), dict(fmt, width=64, height=32, log2_ctb=5))


@pytest.mark.parametrize("bit_depth", [8, 12, 16])
def test_resized_values_and_roundings(ctx, bit_depth):
    check_values(ctx, bit_depth)


@pytest.mark.parametrize("bit_depth,layout", [(8, capi.EXPORT_PLANAR), (8, capi.EXPORT_SEMIPLANAR), (10, capi.EXPORT_PLANAR), (10, capi.EXPORT_SEMIPLANAR)])
def test_same_size_is_the_plain_export(ctx, oracle, bit_depth, layout):
    check_identity(ctx, Oracle(oracle), bit_depth, layout)


@pytest.mark.parametrize("depth", [1, 3])
def test_resized_export_is_waited_for_by_the_next_decode(ctx, depth):
    check_hazard_resized(ctx, depth)


def test_resized_export_behind_a_rejected_decode_writes_nothing(ctx):
    check_gate_resized(ctx)


@pytest.mark.parametrize("bit_depth", [8, 10])
def test_resized_minimum_sizes(ctx, oracle, bit_depth):
    check_minimum_sizes(ctx, Oracle(oracle), bit_depth)


def test_resized_several_tiles(ctx):
    check_several_tiles(ctx)


@pytest.fixture(scope="module")
def picture_1080p(ctx, oracle):
    """decoded once, shared by the sizes below and left unchanged"""
    cfg = dict(width=1920, height=1088, bit_depth=10, seed=7401, n_refs=1, intra_pct=5)
    frame, planes, geom, frames = decode_into_frame(ctx, Oracle(oracle), cfg)
    yield frame, planes, geom
    for f in frames:
        ctx.frame_destroy(f)


@pytest.mark.parametrize("out_size", [(1280, 720), (960, 540), (854, 480), (2560, 1440)], ids=lambda s: "%dx%d" % s)
def test_resized_export_1080p_window(ctx, picture_1080p, out_size):
    """the 1920x1080 window: 4 to 10 tiles per row of tiles (854 columns: a partial last one), 30 to 90 runs of rows, upscaling in the last"""
    frame, planes, geom = picture_1080p
    for samples in (capi.EXPORT_MSB16, capi.EXPORT_U8):
        check_export_resized(ctx, frame, planes, geom, capi.EXPORT_SEMIPLANAR, samples, out_size, (0, 0, 1920, 1080), what="1080p")
