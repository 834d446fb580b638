"""m355_frames_export_tensor on the GPU: the drivers of tests/test_export_tensor_emu.py through the real k_export_resized_rgb<., ., RR_BATCH> instantiations — the format
matrix at 64x32, the composition through the public calls, batches of distinct frames of different pitches with one and with several workgroups per
slice, the same frame twice, the smallest outputs, the gate per slice, a pinned-host destination read behind m355_frame_export_wait of one frame of the
batch —, the frame hazard (a decode into a frame of a batch waits for the batch) with one and three pictures in flight, and one realistic case: a
1920x1088 10-bit picture, its reference frame and a second picture as a batch of 3 distinct frames, centre square to 224x224 with the ImageNet normalisation.  Expected values: the
planes m355_frame_download returns through export_tensor_util.py; all bit-exact, the bytes outside the tensor's elements included.

The build holds four instantiations, k_export_resized_rgb<source bytes, element bytes, RR_BATCH>; layout, F16 / BF16, chroma format and U8 / U16 of the integer stage
are run-time switches.  Which test reaches which (the matrix runs NCHW and NHWC, U8 and U16, with F32, F16 and BF16):
  <1, 2>, <1, 4>  test_tensor_format_matrix[bd8_8_cf1], [bd8_8_cf4] (monochrome), test_tensor_minimum_sizes[8], test_tensor_gate_is_per_slice
  <2, 2>, <2, 4>  test_tensor_format_matrix[bd10_10_cf1], [bd12_12_cf2] (4:2:2), [bd10_10_cf3] (4:4:4), [bd10_9_cf1], test_tensor_minimum_sizes[10],
                  test_single_frame_is_the_resized_rgb_export_as_float (<2, 4>), test_batch_of_distinct_frames, test_same_frame_twice,
                  test_tensor_export_is_waited_for_by_the_next_decode (<2, 2>), test_tensor_export_into_pinned_host_memory,
                  test_tensor_1080p_batch_to_224 (<2, 2>: F16 NCHW and BF16 NHWC), test_every_integer_through_the_kernel (monochrome)"""
import numpy as np
import pytest

from oracle_py import Oracle
from export_tensor_util import (FORMATS, check_batch, check_every_integer, check_composition, check_format_matrix, check_gate, check_hazard, check_minimum_sizes, check_pinned_host,
                                check_same_frame_twice, check_tensor, decode_into_frame, format_id, imagenet)
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
def test_tensor_format_matrix(ctx, oracle, fmt):
    check_format_matrix(ctx, Oracle(oracle), dict(fmt, width=64, height=32, log2_ctb=5))


def test_single_frame_is_the_resized_rgb_export_as_float(ctx, oracle):
    check_composition(ctx, Oracle(oracle), dict(width=64, height=32, bit_depth=10, seed=8001, log2_ctb=5))


def test_every_integer_through_the_kernel(ctx):
    """the device's own float stage — the multiplication kept apart from the addition, v_cvt_f16_f32, the bfloat16 expression — on every integer
    0..65535 under the (scale, bias) pairs of tests/test_tensor_element.py, bit for bit (<2, 2> and <2, 4>, monochrome)"""
    check_every_integer(ctx)


def test_batch_of_distinct_frames(ctx, oracle):
    check_batch(ctx, Oracle(oracle))


def test_same_frame_twice(ctx, oracle):
    check_same_frame_twice(ctx, Oracle(oracle))


@pytest.mark.parametrize("bit_depth", [8, 10])
def test_tensor_minimum_sizes(ctx, oracle, bit_depth):
    check_minimum_sizes(ctx, Oracle(oracle), bit_depth)


def test_tensor_gate_is_per_slice(ctx):
    check_gate(ctx)


@pytest.mark.parametrize("depth", [1, 3])
def test_tensor_export_is_waited_for_by_the_next_decode(ctx, depth):
    """depth 3 is the one that can see a missing wait"""
    check_hazard(ctx, depth)


def test_tensor_export_into_pinned_host_memory(ctx, oracle):
    check_pinned_host(ctx, Oracle(oracle))


def test_tensor_1080p_batch_to_224(ctx, oracle):
    """the 1920x1088 10-bit picture of test_gpu_export_resized_rgb.py, its reference frame and a second picture of the same geometry decoded into a
    frame of its own, as a batch of 3 distinct frames: the centre square (420, 0, 1080, 1080) to 224x224, BT.709 limited range, ImageNet scale and
    bias, as F16 NCHW and as BF16 NHWC — 14 workgroups per slice"""
    cfg = dict(width=1920, height=1088, bit_depth=10, seed=7401, n_refs=1, intra_pct=5)
    frame, planes, geom, frames = decode_into_frame(ctx, Oracle(oracle), cfg)
    second, planes2, geom2, frames2 = decode_into_frame(ctx, Oracle(oracle), dict(cfg, seed=7402))
    try:
        assert geom2 == geom and len(frames) == 2
        batch = [frames[0], frame, second]
        down = [ctx.frame_download(frames[0]), planes, planes2]
        assert not np.array_equal(down[0][0], down[1][0]) and not np.array_equal(down[1][0], down[2][0]) and not np.array_equal(down[0][0], down[2][0])
        scale, bias = imagenet(capi.RGB_U8)
        for layout, dtype in ((capi.TENSOR_NCHW, capi.TENSOR_F16), (capi.TENSOR_NHWC, capi.TENSOR_BF16)):
            check_tensor(ctx, batch, down, geom, layout, dtype, capi.RGB_U8, capi.MATRIX_BT709, 0, (224, 224), scale, bias, (420, 0, 1080, 1080),
                         what="1080p", against_call=(layout == capi.TENSOR_NCHW))
    finally:
        for f in frames + frames2:
            ctx.frame_destroy(f)
