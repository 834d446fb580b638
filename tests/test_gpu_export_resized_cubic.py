"""m355_frame_export_resized_filtered with M355_FILTER_CUBIC on the GPU: the drivers of tests/test_export_cubic_emu.py through the real cubic
instantiations of k_export_resized — the format matrix at 64x32 (8, 10, 12 and, from random planes, 16 bits; every layout and sample format), impulses
and checkerboards of 0 and the maximum at 8, 12 and 16 bits (overshoot beyond both ends, both clips, the 16-bit operand path), the identity, the
smallest sizes, several tiles per row, the frame hazard and the gate once each — and the 1920x1080 window of a 1920x1088 picture down to two sizes,
one with a partial last tile.  Expected values: the planes m355_frame_download returns through the restatement in export_cubic_util.py; all exact."""
import pytest

from oracle_py import Oracle
import export_resized_util as tri
from export_util import FORMATS, decode_into_frame, format_id
from export_cubic_util import (MATRIX_SIZES, check_16_bit_formats, check_export_resized, check_minimum_sizes, check_several_tiles, check_value_cases, cubic)
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
def test_cubic_resized_format_matrix(ctx, oracle, fmt):
    with cubic(ctx) as c:
        tri.check_format_matrix_resized(c, Oracle(oracle), dict(fmt, width=64, height=32, log2_ctb=5), MATRIX_SIZES)


def test_cubic_resized_16_bit_samples(ctx):
    check_16_bit_formats(ctx)


@pytest.mark.parametrize("bit_depth", [8, 12, 16])
def test_cubic_resized_values_and_clips(ctx, bit_depth):
    check_value_cases(ctx, bit_depth)


@pytest.mark.parametrize("bit_depth,layout", [(8, capi.EXPORT_PLANAR), (10, capi.EXPORT_SEMIPLANAR)])
def test_cubic_same_size_is_the_plain_export(ctx, oracle, bit_depth, layout):
    with cubic(ctx) as c:
        tri.check_identity(c, Oracle(oracle), bit_depth, layout)


def test_cubic_resized_minimum_sizes(ctx):
    check_minimum_sizes(ctx)


def test_cubic_resized_several_tiles(ctx):
    check_several_tiles(ctx)


def test_cubic_resized_export_is_waited_for_by_the_next_decode(ctx):
    """three pictures in flight: the depth that can see a missing wait"""
    with cubic(ctx) as c:
        tri.check_hazard_resized(c, 3)


def test_cubic_resized_export_behind_a_rejected_decode_writes_nothing(ctx):
    with cubic(ctx) as c:
        tri.check_gate_resized(c)


@pytest.fixture(scope="module")
def picture_1080p(ctx, oracle):
    """decoded once, shared by the sizes below and left unchanged"""
    cfg = dict(width=1920, height=1088, bit_depth=10, seed=7401, n_refs=1, intra_pct=5)
    frame, planes, geom, frames = decode_into_frame(ctx, Oracle(oracle), cfg)
    yield frame, planes, geom
    for f in frames:
        ctx.frame_destroy(f)


@pytest.mark.parametrize("out_size", [(1280, 720), (854, 480)], ids=lambda s: "%dx%d" % s)
def test_cubic_resized_export_1080p_window(ctx, picture_1080p, out_size):
    """the 1920x1080 window: several tiles per row of tiles (854 columns: a partial last one), 30 and 45 runs of rows"""
    frame, planes, geom = picture_1080p
    for samples in (capi.EXPORT_MSB16, capi.EXPORT_U8):
        check_export_resized(ctx, frame, planes, geom, capi.EXPORT_SEMIPLANAR, samples, out_size, (0, 0, 1920, 1080), what="1080p")
