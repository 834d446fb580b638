"""The three composed exports with M355_FILTER_CUBIC on the GPU: the drivers of tests/test_export_cubic_emu.py through the real cubic instantiations of
k_export_resized_rgb — RR_FRAME (m355_frame_export_resized_rgb_filtered): the format matrix at 64x32 (8, 10, 12 and, from random planes, 16 bits;
packed and planar, U8 and U16), impulses and checkerboards of 0 and the maximum at 8, 12 and 16 bits, the identity, the smallest sizes, several tiles
per row, the hazard and the gate once each, and the 1920x1080 window of a 1920x1088 picture to 1280x720 and to 854x480 (a partial last tile, and a
tile width at which two segments share a pass); RR_BATCH (m355_frames_export_tensor_filtered): the format matrix NCHW / NHWC x F32 / F16 / BF16 and
a batch of 3 frames; RR_ROIS (m355_frames_export_tensor_rois_filtered): 4 regions of different ratios, one mirrored.  Expected values: the
restatement in export_cubic_util.py under the existing compositions; all exact."""
import pytest

from oracle_py import Oracle
import export_resized_rgb_util as tri_rgb
import export_tensor_util as tri_tensor
from export_util import FORMATS, decode_into_frame, format_id
from export_cubic_util import (MATRIX_SIZES, check_16_bit_formats, check_minimum_sizes, check_resized_rgb, check_several_tiles, check_tensor_batch,
                               check_tensor_rois, check_value_cases, cubic)
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
def test_cubic_resized_rgb_format_matrix(ctx, oracle, fmt):
    with cubic(ctx) as c:
        tri_rgb.check_format_matrix(c, Oracle(oracle), dict(fmt, width=64, height=32, log2_ctb=5), MATRIX_SIZES)


@pytest.mark.parametrize("fmt", FORMATS[:4], ids=format_id)
def test_cubic_tensor_format_matrix(ctx, oracle, fmt):
    with cubic(ctx) as c:
        tri_tensor.check_format_matrix(c, Oracle(oracle), dict(fmt, width=64, height=32, log2_ctb=5))


def test_cubic_resized_rgb_16_bit_samples(ctx):
    check_16_bit_formats(ctx, rgb=True)


@pytest.mark.parametrize("bit_depth", [8, 12, 16])
def test_cubic_resized_rgb_values_and_clips(ctx, bit_depth):
    check_value_cases(ctx, bit_depth, rgb=True)


@pytest.mark.parametrize("bit_depth,layout", [(8, capi.RGB_PACKED), (10, capi.RGB_PLANAR)])
def test_cubic_whole_frame_at_its_own_size_is_the_rgb_export(ctx, oracle, bit_depth, layout):
    with cubic(ctx) as c:
        tri_rgb.check_identity(c, Oracle(oracle), bit_depth, layout)


def test_cubic_resized_rgb_minimum_sizes(ctx):
    check_minimum_sizes(ctx, rgb=True)


def test_cubic_resized_rgb_several_tiles(ctx):
    check_several_tiles(ctx, rgb=True)


def test_cubic_resized_rgb_export_is_waited_for_by_the_next_decode(ctx):
    """three pictures in flight: the depth that can see a missing wait"""
    with cubic(ctx) as c:
        tri_rgb.check_hazard(c, 3)


def test_cubic_resized_rgb_export_behind_a_rejected_decode_writes_nothing(ctx):
    with cubic(ctx) as c:
        tri_rgb.check_gate(c)


def test_cubic_tensor_batch_of_3_frames(ctx):
    check_tensor_batch(ctx, 3)


def test_cubic_tensor_4_regions_one_mirrored(ctx):
    check_tensor_rois(ctx)


@pytest.fixture(scope="module")
def picture_1080p(ctx, oracle):
    """decoded once, shared by the sizes below and left unchanged"""
    cfg = dict(width=1920, height=1088, bit_depth=10, seed=7401, n_refs=1, intra_pct=5)
    frame, planes, geom, frames = decode_into_frame(ctx, Oracle(oracle), cfg)
    yield frame, planes, geom
    for f in frames:
        ctx.frame_destroy(f)


@pytest.mark.parametrize("out_size", [(1280, 720), (854, 480)], ids=lambda s: "%dx%d" % s)
def test_cubic_resized_rgb_1080p_window(ctx, picture_1080p, out_size):
    """the 1920x1080 window, BT.709 limited range, as packed U8 and as planar U16"""
    frame, planes, geom = picture_1080p
    for layout, samples in ((capi.RGB_PACKED, capi.RGB_U8), (capi.RGB_PLANAR, capi.RGB_U16)):
        check_resized_rgb(ctx, frame, planes, geom, layout, samples, capi.MATRIX_BT709, 0, out_size, (0, 0, 1920, 1080), what="1080p")
