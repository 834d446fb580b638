"""Chroma sample location types 0..3 (m355_export_opts) on the SIMT-interpreter build: the restatement of export_siting_util.py against itself, type 0
through every _opts entry point against the plain and the _filtered entry points, types 1..3 of m355_frame_export_rgb_opts with all four clamps, the
resizing and the composed exports on grids that keep the siting, the two tensor calls, the rejections and the layout of the options structure.  Every
comparison is exact, destination padding included."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from test_emu_picture import emu_lib  # noqa: F401  (fixture)
from export_siting_util import (M355_ERR_INVALID, check_chroma_case, check_constant_stays_constant, check_resized_sited, check_restatement,
                                check_tensors_sited, check_type0_is_plain, check_wide, check_gate_rgb_sited, check_hazard_rgb_sited, check_lane_boundaries)
from libde265_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def ctx(emu_lib):  # noqa: F811
    c = capi.Context(emu_lib, 0)
    yield c
    c.close()


def test_restatement_reconstructs_each_types_own_ramp():
    """independent of the kernels: a plane that samples base + 2 g X + 2 g' Y at a type's own chroma positions is reconstructed exactly by that
    type's filter wherever no tap is clamped, and by no other type's; type 0 is the existing restatement"""
    check_restatement()


@pytest.mark.parametrize("bit_depth", [8, 10])
def test_type_0_through_the_opts_entry_points_is_the_plain_call(ctx, bit_depth):
    check_type0_is_plain(ctx, bit_depth)


@pytest.mark.parametrize("loc", [1, 2, 3])
@pytest.mark.parametrize("bit_depth", [8, 10])
def test_rgb_types_1_to_3(ctx, bit_depth, loc):
    """corner impulses: all four clamps; whole frame and a rectangle, both layouts, U8 and U16; the expected output differs from type 0's"""
    check_chroma_case(ctx, bit_depth, loc)


@pytest.mark.parametrize("loc", [1, 2, 3])
@pytest.mark.parametrize("bit_depth", [8, 10])
def test_resized_and_composed_types_1_to_3(ctx, bit_depth, loc):
    check_resized_sited(ctx, bit_depth, loc)


@pytest.mark.parametrize("loc", [1, 2, 3])
def test_constant_frame_stays_constant(ctx, loc):
    check_constant_stays_constant(ctx, 8, loc)
    check_constant_stays_constant(ctx, 10, loc)


@pytest.mark.parametrize("loc", [1, 3])
def test_composed_export_wider_than_a_tile(ctx, loc):
    check_wide(ctx, loc)


@pytest.mark.parametrize("size,bit_depth", [((1056, 16), 8), ((544, 16), 10)])
def test_rgb_centre_across_lane_and_wave_boundaries(ctx, size, bit_depth):
    """rows just wider than one wavefront's chunk of k_export_rgb: the left neighbour of a lane's first pixel lies in the lane, the wave before it"""
    check_lane_boundaries(ctx, size, bit_depth, 3)


def test_tensor_and_rois_type_2(ctx):
    check_tensors_sited(ctx, 2)


def test_gate_and_recycled_frames_type_2(ctx):
    """(the interpreter runs every launch to its end at once: this walks the bookkeeping of the _opts entry point, the GPU tier sees a missing wait)"""
    check_gate_rgb_sited(ctx)
    check_hazard_rgb_sited(ctx, 3)


def test_rejections_leave_the_destination_untouched(ctx):
    lib = ctx.L.lib
    nbytes = 1 << 16
    buf = ctx.device_alloc(nbytes)
    frames = {cf: ctx.frame_create(64, 32, cf, 8, 8) for cf in (0, 1, 2, 3)}
    f420 = frames[1]

    def opts(filter=0, loc=0, reserved=None):
        o = capi.ExportOpts(filter=filter, chroma_loc=loc)
        if reserved is not None:
            o.reserved[reserved] = 1
        return ctypes.byref(o)

    rgb = capi.RgbDesc(layout=capi.RGB_PACKED, samples=capi.RGB_U8, matrix=capi.MATRIX_BT709, full_range=0)
    rgb.dst[0] = buf; rgb.pitch[0] = 400
    rs = capi.ResizeDesc(layout=capi.EXPORT_PLANAR, samples=capi.EXPORT_NATIVE, out_width=32, out_height=16)
    rr = capi.ResizeRgbDesc(layout=capi.RGB_PACKED, samples=capi.RGB_U8, matrix=capi.MATRIX_BT709, full_range=0, out_width=32, out_height=16)
    rr.dst[0] = buf; rr.pitch[0] = 400
    for k in range(3):
        rs.dst[k] = buf + 8192 * k; rs.pitch[k] = 128
    td = capi.TensorDesc(layout=capi.TENSOR_NHWC, dtype=capi.TENSOR_F32, samples=capi.RGB_U8, matrix=capi.MATRIX_BT709, full_range=0, out_width=32, out_height=16,
                         stride_n=32768, stride_c=0, stride_h=512)
    td.scale = (ctypes.c_float * 3)(1, 1, 1)
    td.dst = buf
    roi = (capi.TensorRoi * 1)(capi.TensorRoi(0, 0, 64, 32, 0))

    def calls(frame, o):
        one = (ctypes.c_int * 1)(frame)
        return [("rgb", lib.m355_frame_export_rgb_opts(ctx.h, frame, ctypes.byref(rgb), o)),
                ("resized", lib.m355_frame_export_resized_opts(ctx.h, frame, ctypes.byref(rs), o)),
                ("resized rgb", lib.m355_frame_export_resized_rgb_opts(ctx.h, frame, ctypes.byref(rr), o)),
                ("tensor", lib.m355_frames_export_tensor_opts(ctx.h, one, 1, ctypes.byref(td), o)),
                ("rois", lib.m355_frames_export_tensor_rois_opts(ctx.h, one, roi, 1, ctypes.byref(td), o))]

    for loc in (-1, 4, 5, 6):
        for name, rc in calls(f420, opts(loc=loc)):
            assert rc == M355_ERR_INVALID, "%s accepts chroma_loc %d" % (name, loc)
    for cf in (0, 2, 3):
        for loc in (1, 2, 3):
            for name, rc in calls(frames[cf], opts(loc=loc)):
                assert rc == M355_ERR_INVALID, "%s accepts chroma_loc %d for chroma format %d" % (name, loc, cf)
    for k in range(6):
        for name, rc in calls(f420, opts(reserved=k)):
            assert rc == M355_ERR_INVALID, "%s accepts a non-zero reserved[%d]" % (name, k)
    for name, rc in calls(f420, opts(filter=2)):
        assert rc == M355_ERR_INVALID, "%s accepts filter 2" % name
    assert lib.m355_frame_export_rgb_opts(ctx.h, f420, ctypes.byref(rgb), opts(filter=capi.FILTER_CUBIC)) == M355_ERR_INVALID
    ctx.wait()
    assert np.all(ctx.device_read(buf, nbytes) == capi.DEVICE_FILL), "a rejected export wrote to its destination"
    # what the limits admit: every type for 4:2:0, type 0 for every chroma format, the cubic filter where something is resized
    for loc in (0, 1, 2, 3):
        for name, rc in calls(f420, opts(loc=loc)):
            assert rc == 0, (name, loc, ctx.L.error())
    for cf in (0, 2, 3):
        for name, rc in calls(frames[cf], opts()):
            assert rc == 0, (name, cf, ctx.L.error())
    for name, rc in calls(f420, opts(filter=capi.FILTER_CUBIC, loc=3))[1:]:
        assert rc == 0, (name, ctx.L.error())
    ctx.wait()
    ctx.device_free(buf)
    for f in frames.values():
        ctx.frame_destroy(f)


def test_export_opts_layout_matches_the_header():
    """ctypes' mirror against the structure as the C compiler sees it in include/de265_mi355x.h"""
    src = ("#include <stdio.h>\n#include <stddef.h>\n#include \"de265_mi355x.h\"\nint main(){printf(\"%zu %zu %zu %zu\\n\", sizeof(m355_export_opts), "
           "offsetof(m355_export_opts, filter), offsetof(m355_export_opts, chroma_loc), offsetof(m355_export_opts, reserved)); return 0;}")
    exe = os.path.join(ROOT, ".pytest_cache", "abi_export_opts")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(ROOT, "include"), "-o", exe], input=src, text=True, check=True)
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    O = capi.ExportOpts
    assert got == [ctypes.sizeof(O), O.filter.offset, O.chroma_loc.offset, O.reserved.offset] == [32, 0, 4, 8]
    assert O.reserved.size == 24
