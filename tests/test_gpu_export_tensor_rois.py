"""m355_frames_export_tensor_rois on the GPU: the drivers of tests/test_export_tensor_rois_emu.py through the real k_export_resized_rgb<., ., RR_ROIS>
instantiations — regions of one frame at both ratio limits, slices of different unit counts in one two-dimensional grid, whole frames of different
sizes, mirrored slices (the seam between two tiles, output rows that end in half a dword), the full record array, the gate per slice, a pinned-host
destination read behind m355_frame_export_wait of one frame of the batch —, the frame hazard with one and three pictures in flight, and one realistic
case: eight regions of a 1920x1088 10-bit picture and of its reference frame to 224x224 with the ImageNet normalisation.  Every slice has two
expectations (export_tensor_rois_util.py): the restatement of the planes m355_frame_download returns, and m355_frames_export_tensor with n = 1 for
the same frame and rectangle, which runs another instantiation of the kernel; all bit-exact, the bytes outside the tensor's elements included.

Which test reaches which instantiation (layout, F16 / BF16, chroma format, U8 / U16 and the mirror are run-time switches):
  <1, 2, RR_ROIS>, <1, 4, RR_ROIS>  test_regions_of_an_8bit_frame (4:2:0, two tiles across in every slice), test_mirror_at_odd_output_widths (monochrome,
                              <1, 2, RR_ROIS>), test_rois_gate_is_per_slice
  <2, 2, RR_ROIS>, <2, 4, RR_ROIS>  test_regions_of_one_frame, test_slices_of_different_unit_counts, test_whole_frames_of_different_sizes,
                              test_mirrored_regions_of_one_frame, test_mirror_across_the_seam_of_two_tiles, test_mirror_at_odd_output_widths (4:4:4,
                              <2, 2, RR_ROIS>), test_full_record_array, test_rois_export_is_waited_for_by_the_next_decode (<2, 2, RR_ROIS>),
                              test_rois_export_into_pinned_host_memory, test_rois_1080p_regions_to_224 (<2, 2, RR_ROIS>: F16 NCHW and BF16 NHWC)"""
import numpy as np
import pytest

from oracle_py import Oracle
from export_tensor_rois_util import (MIRROR, References, check_composition, check_different_sizes, check_full_array, check_gate, check_hazard,
                                     check_mirror_odd_widths, check_mixed_8bit, check_mixed_units, check_pinned_host, check_rois, decode_into_frame, imagenet,
                                     tiles_of)
from libde265_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    lib = capi.Library()
    assert lib.device_count() >= 1
    c = capi.Context(lib, 0)
    yield c
    c.close()


def test_regions_of_one_frame(ctx, oracle):
    check_composition(ctx, Oracle(oracle))


def test_slices_of_different_unit_counts(ctx):
    check_mixed_units(ctx)


def test_regions_of_an_8bit_frame(ctx):
    check_mixed_8bit(ctx)


def test_whole_frames_of_different_sizes(ctx, oracle):
    check_different_sizes(ctx, Oracle(oracle))


def test_mirrored_regions_of_one_frame(ctx, oracle):
    check_composition(ctx, Oracle(oracle), mirrored=True)


def test_mirror_across_the_seam_of_two_tiles(ctx):
    check_mixed_units(ctx, mirrored=True)


def test_mirror_at_odd_output_widths(ctx, oracle):
    check_mirror_odd_widths(ctx, Oracle(oracle))


def test_full_record_array(ctx, oracle):
    check_full_array(ctx, Oracle(oracle))


def test_rois_gate_is_per_slice(ctx):
    check_gate(ctx)


@pytest.mark.parametrize("depth", [1, 3])
def test_rois_export_is_waited_for_by_the_next_decode(ctx, depth):
    """depth 3 is the one that can see a missing wait"""
    check_hazard(ctx, depth)


def test_rois_export_into_pinned_host_memory(ctx, oracle):
    check_pinned_host(ctx, Oracle(oracle))


def test_rois_1080p_regions_to_224(ctx, oracle):
    """the 1920x1088 10-bit picture of test_tensor_1080p_batch_to_224 and its reference frame: eight regions to 224x224, BT.709 limited range, ImageNet
    scale and bias, as F16 NCHW and as BF16 NHWC — a 28x28 box (8x up), a 1792x1088 box (8x down across, two tiles), a 1344-wide box and the
    centre square (two tiles of 112 each: at this output width regions from 510 columns up have two), a 400x300 box of the picture and of the
    reference frame (one tile), and two of them mirrored beside their plain twins.  Each slice is held against the single call"""
    cfg = dict(width=1920, height=1088, bit_depth=10, seed=7401, n_refs=1, intra_pct=5)
    frame, planes, geom, frames = decode_into_frame(ctx, Oracle(oracle), cfg)
    refs = References(ctx)
    try:
        assert len(frames) == 2
        ref, ref_planes = frames[0], ctx.frame_download(frames[0])
        assert not np.array_equal(ref_planes[0], planes[0])
        rois = [(946, 530, 28, 28, 0), (64, 0, 1792, 1088, 0), (288, 4, 1344, 1080, 0), (420, 0, 1080, 1080, 0), (600, 200, 400, 300, 0),
                (64, 0, 1792, 1088, MIRROR), (946, 530, 28, 28, MIRROR), (600, 200, 400, 300, 0)]
        batch = [frame] * 7 + [ref]
        down = [planes] * 7 + [ref_planes]
        assert [tiles_of(r[2], 224, 2, 2) for r in rois] == [1, 2, 2, 2, 1, 2, 1, 1]
        scale, bias = imagenet(capi.RGB_U8)
        for layout, dtype in ((capi.TENSOR_NCHW, capi.TENSOR_F16), (capi.TENSOR_NHWC, capi.TENSOR_BF16)):
            check_rois(ctx, refs, batch, down, rois, geom, layout, dtype, capi.RGB_U8, capi.MATRIX_BT709, 0, (224, 224), scale, bias, what="1080p")
    finally:
        for f in frames:
            ctx.frame_destroy(f)
