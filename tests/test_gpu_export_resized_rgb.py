"""m355_frame_export_resized_rgb on the GPU: the drivers of tests/test_export_resized_rgb_emu.py through the real k_export_resized_rgb instantiations —
the format matrix at 64x32, the composition through the public calls, the identity, the smallest sizes, the tile seams, odd sizes, the value cases, the gate
and the frame hazard (a decode into a frame waits for the export of the frame's previous picture) with one and three pictures in flight — and a
1920x1088 10-bit picture whose 1920x1080 window is exported down to two sizes and up to one.  Expected values: the planes m355_frame_download returns
through the two restatements composed (export_resized_rgb_util.py); all exact.

The build holds four instantiations, k_export_resized_rgb<source bytes, destination bytes, RR_FRAME>; layout and chroma format are run-time switches.
Which test reaches which (every test below runs packed AND planar unless it says otherwise):
  <1, 1>  test_resized_rgb_format_matrix[bd8_8_cf1], [bd8_8_cf4] (monochrome), test_resized_rgb_values_and_clips[8], test_resized_rgb_minimum_sizes[8],
          test_whole_frame_at_its_own_size_is_the_rgb_export[8-*], test_resized_rgb_export_behind_a_rejected_decode_writes_nothing (packed)
  <1, 2>  the same tests: each runs M355_RGB_U8 and M355_RGB_U16 (the gate test: U8 only)
  <2, 1>  test_resized_rgb_format_matrix[bd10_10_cf1], [bd12_12_cf2] (4:2:2), [bd10_10_cf3] (4:4:4), [bd10_9_cf1], test_resized_rgb_tile_seams, test_resized_rgb_odd_sizes,
          test_resized_rgb_values_and_clips[12], [16], test_resized_rgb_is_the_two_calls_chained, test_resized_rgb_export_is_waited_for_by_the_next_decode
          (packed), test_resized_rgb_1080p_window (packed)
  <2, 2>  the same tests with M355_RGB_U16 (the hazard test: U8 only; the 1080p window: planar)"""
import pytest

from oracle_py import Oracle
from export_resized_rgb_util import (FORMATS, COMPOSITION_FORMATS, check_composition, check_format_matrix, check_gate, check_hazard, check_identity,
                                     check_minimum_sizes, check_odd_sizes, check_resized_rgb, check_tile_seams, check_values, decode_into_frame, format_id)
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
def test_resized_rgb_format_matrix(ctx, oracle, fmt):
    check_format_matrix(ctx, Oracle(oracle), dict(fmt, width=64, height=32, log2_ctb=5))


@pytest.mark.parametrize("fmt", COMPOSITION_FORMATS, ids=format_id)
def test_resized_rgb_is_the_two_calls_chained(ctx, oracle, fmt):
    check_composition(ctx, Oracle(oracle), fmt)


@pytest.mark.parametrize("bit_depth,layout", [(8, capi.RGB_PACKED), (8, capi.RGB_PLANAR), (10, capi.RGB_PACKED), (10, capi.RGB_PLANAR)])
def test_whole_frame_at_its_own_size_is_the_rgb_export(ctx, oracle, bit_depth, layout):
    check_identity(ctx, Oracle(oracle), bit_depth, layout)


@pytest.mark.parametrize("bit_depth", [8, 10])
def test_resized_rgb_minimum_sizes(ctx, oracle, bit_depth):
    check_minimum_sizes(ctx, Oracle(oracle), bit_depth)


def test_resized_rgb_tile_seams(ctx):
    check_tile_seams(ctx)


def test_resized_rgb_odd_sizes(ctx):
    check_odd_sizes(ctx)


@pytest.mark.parametrize("bit_depth", [8, 12, 16])
def test_resized_rgb_values_and_clips(ctx, bit_depth):
    check_values(ctx, bit_depth)


def test_resized_rgb_export_behind_a_rejected_decode_writes_nothing(ctx):
    check_gate(ctx)


@pytest.mark.parametrize("depth", [1, 3])
def test_resized_rgb_export_is_waited_for_by_the_next_decode(ctx, depth):
    """depth 3 is the one that can see a missing wait"""
    check_hazard(ctx, depth)


@pytest.fixture(scope="module")
def picture_1080p(ctx, oracle):
    """decoded once, shared by the sizes below and left unchanged"""
    cfg = dict(width=1920, height=1088, bit_depth=10, seed=7401, n_refs=1, intra_pct=5)
    frame, planes, geom, frames = decode_into_frame(ctx, Oracle(oracle), cfg)
    yield frame, planes, geom
    for f in frames:
        ctx.frame_destroy(f)


@pytest.mark.parametrize("out_size", [(1280, 720), (854, 480), (2560, 1440)], ids=lambda s: "%dx%d" % s)
def test_resized_rgb_1080p_window(ctx, picture_1080p, out_size):
    """the 1920x1080 window, BT.709 limited range, as packed U8 and as planar U16: 4 to 10 tiles per row of tiles (854 columns: a partial last one),
    30 to 90 runs of rows, upscaling in the last"""
    frame, planes, geom = picture_1080p
    for layout, samples in ((capi.RGB_PACKED, capi.RGB_U8), (capi.RGB_PLANAR, capi.RGB_U16)):
        check_resized_rgb(ctx, frame, planes, geom, layout, samples, capi.MATRIX_BT709, 0, out_size, (0, 0, 1920, 1080), what="1080p")
