"""ctypes binding of the C ABI declared in include/de265_mi355x.h (the product library
libde265_mi355x.so, built by csrc/Makefile for gfx950).  There is NO fallback: if the library is
missing or no HIP device is visible, loading / context creation raises."""
import ctypes
import os

import numpy as np

from . import worklist

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(_HERE, "libde265_mi355x.so")

ERRORS = {1: "M355_ERR_NO_DEVICE", 2: "M355_ERR_HIP", 3: "M355_ERR_INVALID", 4: "M355_ERR_NOMEM", 5: "M355_ERR_TIMEOUT", 6: "M355_ERR_BUSY", 7: "M355_ERR_STALE"}


HALO_SUM_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p)
ALL_GATHER_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_void_p)


class Comm(ctypes.Structure):
    """m355_comm (include/de265_mi355x.h): the exchange callbacks of m355_decode_sharded"""
    _fields_ = [("user", ctypes.c_void_p), ("halo_sum", HALO_SUM_FN), ("all_gather", ALL_GATHER_FN)]


class M355Error(RuntimeError):
    def __init__(self, code, text):
        super().__init__("%s: %s" % (ERRORS.get(code, code), text))
        self.code = code


HASH_MD5, HASH_CRC, HASH_CHECKSUM = 0, 1, 2


class PictureHash(ctypes.Structure):
    """m355_picture_hash (include/de265_mi355x.h), the fields of sei_decoded_picture_hash (sei.h:64-69)"""
    _fields_ = [("md5", (ctypes.c_uint8 * 16) * 3), ("crc", ctypes.c_uint16 * 3), ("checksum", ctypes.c_uint32 * 3)]


EXPORT_PLANAR, EXPORT_SEMIPLANAR = 0, 1
EXPORT_NATIVE, EXPORT_MSB16, EXPORT_U8 = 0, 1, 2
DEVICE_FILL = 0xA5          # the sentinel byte this harness fills export destinations with before an export (Context.device_alloc)


class ExportDesc(ctypes.Structure):
    """m355_export_desc (include/de265_mi355x.h)"""
    _fields_ = [("layout", ctypes.c_int32), ("samples", ctypes.c_int32),
                ("x0", ctypes.c_int32), ("y0", ctypes.c_int32), ("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("dst", ctypes.c_void_p * 3), ("pitch", ctypes.c_int64 * 3)]


RESIZE_MAX_TAPS = 16


class ResizeDesc(ctypes.Structure):
    """m355_resize_desc (include/de265_mi355x.h)"""
    _fields_ = [("layout", ctypes.c_int32), ("samples", ctypes.c_int32),
                ("x0", ctypes.c_int32), ("y0", ctypes.c_int32), ("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("out_width", ctypes.c_int32), ("out_height", ctypes.c_int32),
                ("dst", ctypes.c_void_p * 3), ("pitch", ctypes.c_int64 * 3)]


RGB_PACKED, RGB_PLANAR = 0, 1
RGB_U8, RGB_U16 = 0, 1
MATRIX_BT601, MATRIX_BT709, MATRIX_BT2020 = 0, 1, 2


class RgbDesc(ctypes.Structure):
    """m355_rgb_desc (include/de265_mi355x.h)"""
    _fields_ = [("layout", ctypes.c_int32), ("samples", ctypes.c_int32), ("matrix", ctypes.c_int32), ("full_range", ctypes.c_int32),
                ("x0", ctypes.c_int32), ("y0", ctypes.c_int32), ("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("dst", ctypes.c_void_p * 3), ("pitch", ctypes.c_int64 * 3)]


class ResizeRgbDesc(ctypes.Structure):
    """m355_resize_rgb_desc (include/de265_mi355x.h)"""
    _fields_ = [("layout", ctypes.c_int32), ("samples", ctypes.c_int32), ("matrix", ctypes.c_int32), ("full_range", ctypes.c_int32),
                ("x0", ctypes.c_int32), ("y0", ctypes.c_int32), ("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("out_width", ctypes.c_int32), ("out_height", ctypes.c_int32),
                ("dst", ctypes.c_void_p * 3), ("pitch", ctypes.c_int64 * 3)]


PIXEL_RGBA8, PIXEL_BGRA8, PIXEL_BGR8, PIXEL_A2B10G10R10, PIXEL_A2R10G10B10 = 0, 1, 2, 3, 4     # M355_PIXEL_*
PIXEL_FORMATS = (PIXEL_RGBA8, PIXEL_BGRA8, PIXEL_BGR8, PIXEL_A2B10G10R10, PIXEL_A2R10G10B10)


def pixel_bytes(format):
    """bytes per pixel of a PIXEL_* format"""
    return 3 if format == PIXEL_BGR8 else 4


# M355_ORIENT_*: three bits (TRANSPOSE first, then FLIP, then MIRROR) and the four rotations
ORIENT_MIRROR, ORIENT_FLIP, ORIENT_TRANSPOSE = 1, 2, 4
ORIENT_ROTATE_0, ORIENT_ROTATE_180, ORIENT_ROTATE_90_CW, ORIENT_ROTATE_90_CCW = 0, 3, 5, 6
ORIENTATIONS = tuple(range(8))


class PixelDesc(ctypes.Structure):
    """m355_pixel_desc (include/de265_mi355x.h)"""
    _fields_ = [("format", ctypes.c_int32), ("alpha", ctypes.c_int32), ("matrix", ctypes.c_int32), ("full_range", ctypes.c_int32),
                ("x0", ctypes.c_int32), ("y0", ctypes.c_int32), ("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("out_width", ctypes.c_int32), ("out_height", ctypes.c_int32),
                ("dst", ctypes.c_void_p), ("pitch", ctypes.c_int64)]


TENSOR_MAX_FRAMES = 32
TENSOR_NCHW, TENSOR_NHWC = 0, 1
TENSOR_F32, TENSOR_F16, TENSOR_BF16 = 0, 1, 2


class TensorDesc(ctypes.Structure):
    """m355_tensor_desc (include/de265_mi355x.h)"""
    _fields_ = [("layout", ctypes.c_int32), ("dtype", ctypes.c_int32),
                ("samples", ctypes.c_int32), ("matrix", ctypes.c_int32), ("full_range", ctypes.c_int32),
                ("x0", ctypes.c_int32), ("y0", ctypes.c_int32), ("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("out_width", ctypes.c_int32), ("out_height", ctypes.c_int32),
                ("scale", ctypes.c_float * 3), ("bias", ctypes.c_float * 3),
                ("dst", ctypes.c_void_p),
                ("stride_n", ctypes.c_int64), ("stride_c", ctypes.c_int64), ("stride_h", ctypes.c_int64)]


ROI_MIRROR = 1
FILTER_TRIANGLE, FILTER_CUBIC = 0, 1      # M355_FILTER_*
RESIZE_CUBIC_MAX_N = 16384


class TensorRoi(ctypes.Structure):
    """m355_tensor_roi (include/de265_mi355x.h)"""
    _fields_ = [("x0", ctypes.c_int32), ("y0", ctypes.c_int32), ("width", ctypes.c_int32), ("height", ctypes.c_int32), ("flags", ctypes.c_int32)]


class ExportOpts(ctypes.Structure):
    """m355_export_opts: the filter (FILTER_*) and the chroma sample location type 0..3 of a 4:2:0 source; reserved stays 0, but for reserved[0],
    which is the header's `colour`: 0 or a handle of Context.colour_create"""
    _fields_ = [("filter", ctypes.c_int32), ("chroma_loc", ctypes.c_int32), ("reserved", ctypes.c_int32 * 6)]


COLOUR_ONE, COLOUR_IN_KNOTS, COLOUR_OUT_KNOTS, COLOUR_OBJECTS = 1 << 24, 1025, 1217, 16   # M355_COLOUR_*
TONE_CLIP, TONE_REINHARD = 0, 1               # M355_TONE_*
TONE_BT2390 = 2                               # (colour_preset_tone only)
TONE_GAIN_ONE = 1 << 24                       # M355_TONE_GAIN_ONE
NORM_MAXRGB, NORM_LUMA = 0, 1                 # M355_NORM_*


class ColourTables(ctypes.Structure):
    """m355_colour_tables (include/de265_mi355x.h)"""
    _fields_ = [("lut_in", ctypes.c_uint32 * COLOUR_IN_KNOTS), ("matrix", ctypes.c_int32 * 9), ("lut_out", ctypes.c_uint16 * COLOUR_OUT_KNOTS),
                ("pad", ctypes.c_uint16)]


class ColourPresetDesc(ctypes.Structure):
    """m355_colour_preset_desc (include/de265_mi355x.h)"""
    _fields_ = [(n, ctypes.c_int32) for n in ("in_transfer", "in_primaries", "out_transfer", "out_primaries", "tone", "white_nits", "peak_nits",
                                              "reserved")]


class ColourTone(ctypes.Structure):
    """m355_colour_tone (include/de265_mi355x.h)"""
    _fields_ = [("norm", ctypes.c_int32), ("weights", ctypes.c_int32 * 3), ("gain", ctypes.c_uint32 * COLOUR_OUT_KNOTS), ("reserved", ctypes.c_uint32 * 3)]


def colour_tone(norm, weights, gain, reserved=(0, 0, 0)):
    """a ColourTone from its norm and three sequences (3, 1217 and 3 entries)"""
    q = ColourTone(norm=norm)
    q.weights[:] = [int(v) for v in weights]
    q.gain[:] = [int(v) for v in gain]
    q.reserved[:] = [int(v) for v in reserved]
    return q


def colour_tables(lut_in, matrix, lut_out, pad=0):
    """a ColourTables from three sequences (1025, 9 and 1217 entries)"""
    t = ColourTables(pad=pad)
    t.lut_in[:] = [int(v) for v in lut_in]
    t.matrix[:] = [int(v) for v in matrix]
    t.lut_out[:] = [int(v) for v in lut_out]
    return t


class RgbCoeffs(ctypes.Structure):
    """m355_rgb_coeffs (include/de265_mi355x.h)"""
    _fields_ = [(n, ctypes.c_int32) for n in ("F", "y0", "c0", "cy", "crv", "cgu", "cgv", "cbu")]


class MeasureDesc(ctypes.Structure):
    """m355_measure_desc (include/de265_mi355x.h)"""
    _fields_ = [("ref_frame", ctypes.c_int32), ("x0", ctypes.c_int32), ("y0", ctypes.c_int32), ("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("ref", ctypes.c_void_p * 3), ("pitch", ctypes.c_int64 * 3)]


class Measure(ctypes.Structure):
    """m355_measure (include/de265_mi355x.h)"""
    _fields_ = [("ssd", ctypes.c_uint64 * 3), ("sad", ctypes.c_uint64 * 3), ("n_diff", ctypes.c_uint64 * 3), ("max_abs", ctypes.c_uint32 * 3),
                ("first_x", ctypes.c_int32 * 3), ("first_y", ctypes.c_int32 * 3), ("mse", ctypes.c_double * 3)]


SSIM_REQUESTS, SSIM_TAPS, SSIM_ONE = 16, 11, 1 << 30     # M355_SSIM_REQUESTS; the window's taps; q of two identical windows


class SsimDesc(ctypes.Structure):
    """m355_ssim_desc (include/de265_mi355x.h)"""
    _fields_ = [("ref_frame", ctypes.c_int32), ("x0", ctypes.c_int32), ("y0", ctypes.c_int32), ("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("ref", ctypes.c_void_p * 3), ("pitch", ctypes.c_int64 * 3), ("planes", ctypes.c_int32), ("reserved", ctypes.c_int32 * 7),
                ("map", ctypes.c_void_p * 3), ("map_pitch", ctypes.c_int64 * 3)]


class Ssim(ctypes.Structure):
    """m355_ssim (include/de265_mi355x.h)"""
    _fields_ = [("sum_q", ctypes.c_int64 * 3), ("n", ctypes.c_uint64 * 3), ("min_q", ctypes.c_int32 * 3), ("ssim", ctypes.c_double * 3)]


MSSSIM_REQUESTS, MSSSIM_LEVELS = 4, 5       # M355_MSSSIM_*
MSSSIM_WEIGHTS = [0.0448, 0.2856, 0.3001, 0.2363, 0.1333]   # Wang, Simoncelli, Bovik 2003: what m355_msssim_combine takes for weight == NULL


class MsssimDesc(ctypes.Structure):
    """m355_msssim_desc (include/de265_mi355x.h)"""
    _fields_ = [("ref_frame", ctypes.c_int32), ("x0", ctypes.c_int32), ("y0", ctypes.c_int32), ("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("ref", ctypes.c_void_p * 3), ("pitch", ctypes.c_int64 * 3), ("planes", ctypes.c_int32), ("levels", ctypes.c_int32), ("reserved", ctypes.c_int32 * 6)]


class Msssim(ctypes.Structure):
    """m355_msssim (include/de265_mi355x.h)"""
    _fields_ = [("sum_q", ctypes.c_int64 * MSSSIM_LEVELS * 3), ("sum_cs", ctypes.c_int64 * MSSSIM_LEVELS * 3), ("n", ctypes.c_uint64 * MSSSIM_LEVELS * 3),
                ("msssim", ctypes.c_double * 3)]


def msssim_list(out):
    """m355_msssim -> one dict per plane (always three): sum_q, sum_cs, n as lists over the five levels, msssim"""
    return [dict(sum_q=[int(v) for v in out.sum_q[c]], sum_cs=[int(v) for v in out.sum_cs[c]], n=[int(v) for v in out.n[c]], msssim=float(out.msssim[c])) for c in range(3)]


STATS_REQUESTS, STATS_BINS = 16, 256        # M355_STATS_*


class StatsDesc(ctypes.Structure):
    """m355_stats_desc (include/de265_mi355x.h)"""
    _fields_ = [(n, ctypes.c_int32) for n in ("x0", "y0", "width", "height", "black", "light", "matrix", "full_range", "chroma_loc")] + \
               [("reserved", ctypes.c_int32 * 7)]


class Stats(ctypes.Structure):
    """m355_stats (include/de265_mi355x.h)"""
    _fields_ = [("hist", (ctypes.c_uint32 * STATS_BINS) * 3), ("min", ctypes.c_uint32 * 3), ("max", ctypes.c_uint32 * 3), ("sum", ctypes.c_uint64 * 3),
                ("sum_sq", ctypes.c_uint64 * 3), ("box", ctypes.c_int32 * 4), ("n_active", ctypes.c_uint64), ("light_hist", ctypes.c_uint32 * STATS_BINS),
                ("light_min", ctypes.c_uint32), ("light_max", ctypes.c_uint32), ("light_sum", ctypes.c_uint64)]


N_MAPS, MAPS_REQUESTS, PICTURE_LAST = 7, 16, -1     # M355_N_MAPS, M355_MAPS_REQUESTS, M355_PICTURE_LAST
MAP_CU, MAP_QP, MAP_TU, MAP_INTRA, MAP_MV, MAP_REF, MAP_SLICE = range(7)
MAP_NAMES = ("cu", "qp", "tu", "intra", "mv", "ref", "slice")
# per map: the element as numpy sees it, and how many of them make one unit (MV: four int16, REF: four bytes)
MAP_DTYPES = (np.dtype("<u4"), np.dtype("i1"), np.dtype("u1"), np.dtype("u1"), np.dtype("<i2"), np.dtype("u1"), np.dtype("<u2"))
MAP_PER_UNIT = (1, 1, 1, 1, 4, 4, 1)
MAP_ELEM_BYTES = (4, 1, 1, 1, 8, 4, 2)


class MapsDesc(ctypes.Structure):
    """m355_maps_desc (include/de265_mi355x.h)"""
    _fields_ = [("log2_unit", ctypes.c_int32), ("reserved", ctypes.c_int32), ("dst", ctypes.c_void_p * N_MAPS), ("pitch", ctypes.c_int64 * N_MAPS)]


class MapsInfo(ctypes.Structure):
    """m355_maps_info (include/de265_mi355x.h)"""
    _fields_ = [("units_w", ctypes.c_int32), ("units_h", ctypes.c_int32), ("covered", ctypes.c_uint32), ("n_intra", ctypes.c_uint32),
                ("n_inter", ctypes.c_uint32), ("n_skip", ctypes.c_uint32), ("qp_sum", ctypes.c_int64), ("qp_min", ctypes.c_int32),
                ("qp_max", ctypes.c_int32), ("n_bipred", ctypes.c_uint32), ("skipped", ctypes.c_uint32 * 4)]


def maps_info_dict(out):
    """a MapsInfo structure as plain Python values (Context.picture_maps_result)"""
    d = {n: int(getattr(out, n)) for n in ("units_w", "units_h", "covered", "n_intra", "n_inter", "n_skip", "qp_sum", "qp_min", "qp_max", "n_bipred")}
    d["skipped"] = [int(v) for v in out.skipped]
    return d


class ArenaCaps(ctypes.Structure):
    """m355_arena_caps (include/de265_mi355x.h)"""
    _fields_ = [(n, ctypes.c_int32) for n in ("n_slices", "n_ctbs", "n_cus", "n_tus", "n_pbs", "n_wts", "n_ibs")] + \
               [("n_rbs", ctypes.c_int32 * 4), ("n_coeffs", ctypes.c_uint32), ("n_pcm", ctypes.c_uint32), ("scaling", ctypes.c_int32),
                ("rb_bin", ctypes.c_void_p * 4)]


def stats_dict(out, n_planes, light):
    """a Stats structure as plain Python values (Context.frame_stats_result)"""
    planes = [dict(hist=[int(v) for v in out.hist[c]], min=int(out.min[c]), max=int(out.max[c]), sum=int(out.sum[c]), sum_sq=int(out.sum_sq[c]))
              for c in range(n_planes)]
    return dict(planes=planes, box=None if out.box[0] < 0 else tuple(int(v) for v in out.box), n_active=int(out.n_active),
                light=dict(hist=[int(v) for v in out.light_hist], min=int(out.light_min), max=int(out.light_max), sum=int(out.light_sum)) if light else None)


class Library:
    """A loaded libde265_mi355x.so with typed entry points."""

    def __init__(self, path=None):
        # M355_LIB: an alternative BUILD of the same HIP library (kernel-variant experiments, tools/variants.sh)
        path = path or os.environ.get("M355_LIB") or DEFAULT_LIB
        if not os.path.exists(path):
            raise RuntimeError("MI355X backend library not found: %s (build it: make -C libde265_amd/csrc; "
                               "there is no CPU fallback)" % path)
        self.path = path
        L = self.lib = ctypes.CDLL(path)
        vp, i, cp = ctypes.c_void_p, ctypes.c_int, ctypes.c_char_p
        L.m355_last_error.restype = cp
        L.m355_version.restype = cp
        L.m355_device_count.restype = i
        L.m355_create.argtypes = [i, ctypes.POINTER(vp)]
        L.m355_destroy.argtypes = [vp]
        L.m355_destroy.restype = None
        L.m355_frame_create.argtypes = [vp, i, i, i, i, i]
        L.m355_frame_destroy.argtypes = [vp, i]
        L.m355_frame_upload.argtypes = [vp, i, i, vp, ctypes.c_ssize_t]
        L.m355_frame_download.argtypes = [vp, i, i, vp, ctypes.c_ssize_t]
        L.m355_frame_fill.argtypes = [vp, i, i, i]
        L.m355_measure_copy_rate.argtypes = [vp, ctypes.c_size_t, i, ctypes.POINTER(ctypes.c_double)]
        L.m355_arena_begin.argtypes = [vp, vp, vp]
        if hasattr(L, "m355_picture_arena_begin"):      # (absent from older builds loaded through M355_LIB for an A/B)
            L.m355_picture_arena_begin.argtypes = [vp, i, vp, vp, vp]
        if hasattr(L, "m355_pack_narrow"):
            L.m355_pack_narrow.argtypes = [vp, i, vp, ctypes.c_uint32, vp, vp, ctypes.POINTER(ctypes.c_uint32)]
        L.m355_frame_download_async.argtypes = [vp, i, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_ssize_t)]
        L.m355_frame_download_wait.argtypes = [vp, i]
        if hasattr(L, "m355_frame_export"):             # (absent from older builds loaded through M355_LIB for an A/B)
            L.m355_frame_export.argtypes = [vp, i, ctypes.POINTER(ExportDesc)]
            L.m355_frame_export_wait.argtypes = [vp, i]
            L.m355_frame_export_order.argtypes = [vp, i, vp]
            L.m355_device_alloc.argtypes = [vp, ctypes.c_size_t]
            L.m355_device_alloc.restype = vp
            L.m355_device_free.argtypes = [vp, vp]
            L.m355_device_free.restype = None
            L.m355_device_read.argtypes = [vp, vp, vp, ctypes.c_size_t]
            L.m355_device_write.argtypes = [vp, vp, vp, ctypes.c_size_t]
        if hasattr(L, "m355_frame_export_scaled"):      # (absent from older builds loaded through M355_LIB for an A/B)
            L.m355_frame_export_scaled.argtypes = [vp, i, ctypes.POINTER(ExportDesc), i]
        if hasattr(L, "m355_frame_export_rgb"):         # (absent from older builds loaded through M355_LIB for an A/B)
            L.m355_frame_export_rgb.argtypes = [vp, i, ctypes.POINTER(RgbDesc)]
            L.m355_rgb_coefficients.argtypes = [i, i, i, i, i, ctypes.POINTER(RgbCoeffs)]
        if hasattr(L, "m355_frame_export_resized"):     # (absent from older builds loaded through M355_LIB for an A/B)
            L.m355_frame_export_resized.argtypes = [vp, i, ctypes.POINTER(ResizeDesc)]
            L.m355_resize_taps.argtypes = [i, i, i, i, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]
        if hasattr(L, "m355_frame_export_resized_rgb"):  # (absent from older builds loaded through M355_LIB for an A/B)
            L.m355_frame_export_resized_rgb.argtypes = [vp, i, ctypes.POINTER(ResizeRgbDesc)]
        if hasattr(L, "m355_frames_export_tensor"):     # (absent from older builds loaded through M355_LIB for an A/B)
            L.m355_frames_export_tensor.argtypes = [vp, ctypes.POINTER(i), i, ctypes.POINTER(TensorDesc)]
            L.m355_tensor_element.argtypes = [ctypes.c_uint32, ctypes.c_float, ctypes.c_float, i, ctypes.POINTER(ctypes.c_uint32)]
        if hasattr(L, "m355_frames_export_tensor_rois"):  # (absent from older builds loaded through M355_LIB for an A/B)
            L.m355_frames_export_tensor_rois.argtypes = [vp, ctypes.POINTER(i), ctypes.POINTER(TensorRoi), i, ctypes.POINTER(TensorDesc)]
        if hasattr(L, "m355_frame_export_resized_filtered"):  # (absent from older builds loaded through M355_LIB for an A/B)
            L.m355_frame_export_resized_filtered.argtypes = [vp, i, ctypes.POINTER(ResizeDesc), i]
            L.m355_frame_export_resized_rgb_filtered.argtypes = [vp, i, ctypes.POINTER(ResizeRgbDesc), i]
            L.m355_frames_export_tensor_filtered.argtypes = [vp, ctypes.POINTER(i), i, ctypes.POINTER(TensorDesc), i]
            L.m355_frames_export_tensor_rois_filtered.argtypes = [vp, ctypes.POINTER(i), ctypes.POINTER(TensorRoi), i, ctypes.POINTER(TensorDesc), i]
            L.m355_resize_taps_filtered.argtypes = [i, i, i, i, i, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]
        if hasattr(L, "m355_frame_export_rgb_opts"):    # (absent from older builds loaded through M355_LIB for an A/B)
            po = ctypes.POINTER(ExportOpts)
            L.m355_frame_export_rgb_opts.argtypes = [vp, i, ctypes.POINTER(RgbDesc), po]
            L.m355_frame_export_resized_opts.argtypes = [vp, i, ctypes.POINTER(ResizeDesc), po]
            L.m355_frame_export_resized_rgb_opts.argtypes = [vp, i, ctypes.POINTER(ResizeRgbDesc), po]
            L.m355_frames_export_tensor_opts.argtypes = [vp, ctypes.POINTER(i), i, ctypes.POINTER(TensorDesc), po]
            L.m355_frames_export_tensor_rois_opts.argtypes = [vp, ctypes.POINTER(i), ctypes.POINTER(TensorRoi), i, ctypes.POINTER(TensorDesc), po]
        if hasattr(L, "m355_colour_create"):
            L.m355_colour_create.argtypes = [vp, ctypes.POINTER(ColourTables), ctypes.POINTER(i)]
            L.m355_colour_destroy.argtypes = [vp, i]
            L.m355_colour_preset.argtypes = [ctypes.POINTER(ColourPresetDesc), ctypes.POINTER(ColourTables)]
            L.m355_colour_pixel.argtypes = [ctypes.POINTER(ColourTables), ctypes.POINTER(ctypes.c_uint32), i, ctypes.POINTER(ctypes.c_uint32)]
        if hasattr(L, "m355_frame_export_pixels"):      # (absent from older builds loaded through M355_LIB for an A/B)
            L.m355_frame_export_pixels.argtypes = [vp, i, ctypes.POINTER(PixelDesc), ctypes.POINTER(ExportOpts)]
            L.m355_frame_export_resized_pixels.argtypes = [vp, i, ctypes.POINTER(PixelDesc), ctypes.POINTER(ExportOpts)]
            L.m355_pixel_pack.argtypes = [i, ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(i)]
        if hasattr(L, "m355_frame_export_oriented"):    # (absent from older builds loaded through M355_LIB for an A/B)
            L.m355_frame_export_oriented.argtypes = [vp, i, ctypes.POINTER(ExportDesc), i]
            L.m355_frame_export_pixels_oriented.argtypes = [vp, i, ctypes.POINTER(PixelDesc), ctypes.POINTER(ExportOpts), i]
            L.m355_orientation_compose.argtypes = [i, i, ctypes.POINTER(i)]
            L.m355_orientation_from_exif.argtypes = [i, ctypes.POINTER(i)]
        if hasattr(L, "m355_colour_create_tone"):
            L.m355_colour_create_tone.argtypes = [vp, ctypes.POINTER(ColourTables), ctypes.POINTER(ColourTone), ctypes.POINTER(i)]
            L.m355_colour_preset_tone.argtypes = [ctypes.POINTER(ColourPresetDesc), i, ctypes.POINTER(ColourTables), ctypes.POINTER(ColourTone)]
            L.m355_colour_pixel_tone.argtypes = [ctypes.POINTER(ColourTables), ctypes.POINTER(ColourTone), ctypes.POINTER(ctypes.c_uint32), i,
                                                 ctypes.POINTER(ctypes.c_uint32)]
        L.m355_host_alloc.argtypes = [ctypes.c_size_t]
        L.m355_host_alloc.restype = vp
        L.m355_host_free.argtypes = [vp]
        L.m355_frame_hash.argtypes = [vp, i, i, vp]
        if hasattr(L, "m355_frame_hash_async"):         # (absent from older builds loaded through M355_LIB for an A/B)
            L.m355_frame_hash_async.argtypes = [vp, i, i, ctypes.POINTER(ctypes.c_ulonglong)]
            L.m355_frame_hash_result.argtypes = [vp, ctypes.c_ulonglong, i, vp]
        if hasattr(L, "m355_frame_measure_async"):      # (absent from older builds loaded through M355_LIB for an A/B)
            L.m355_frame_measure_async.argtypes = [vp, i, ctypes.POINTER(MeasureDesc), ctypes.POINTER(ctypes.c_ulonglong)]
            L.m355_frame_measure_result.argtypes = [vp, ctypes.c_ulonglong, i, ctypes.POINTER(Measure)]
        if hasattr(L, "m355_frame_stats_async"):        # (absent from older builds loaded through M355_LIB for an A/B)
            L.m355_frame_stats_async.argtypes = [vp, i, ctypes.POINTER(StatsDesc), ctypes.POINTER(ctypes.c_ulonglong)]
            L.m355_frame_stats_result.argtypes = [vp, ctypes.c_ulonglong, i, ctypes.POINTER(Stats)]
            L.m355_stats_quantile.argtypes = [ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(i)]
        if hasattr(L, "m355_frame_ssim_async"):         # (absent from older builds loaded through M355_LIB for an A/B)
            L.m355_frame_ssim_async.argtypes = [vp, i, ctypes.POINTER(SsimDesc), ctypes.POINTER(ctypes.c_ulonglong)]
            L.m355_frame_ssim_result.argtypes = [vp, ctypes.c_ulonglong, i, ctypes.POINTER(Ssim)]
            L.m355_ssim_window.argtypes = [ctypes.POINTER(ctypes.c_uint64), i, ctypes.POINTER(ctypes.c_int32)]
            L.m355_ssim_weights.argtypes = [ctypes.POINTER(ctypes.c_int32)]
        if hasattr(L, "m355_frame_msssim_async"):       # (absent from older builds loaded through M355_LIB for an A/B)
            L.m355_frame_msssim_async.argtypes = [vp, i, ctypes.POINTER(MsssimDesc), ctypes.POINTER(ctypes.c_ulonglong)]
            L.m355_frame_msssim_result.argtypes = [vp, ctypes.c_ulonglong, i, ctypes.POINTER(Msssim)]
            L.m355_ssim_window_cs.argtypes = [ctypes.POINTER(ctypes.c_uint64), i, ctypes.POINTER(ctypes.c_int32)]
            L.m355_msssim_combine.argtypes = [ctypes.POINTER(ctypes.c_double), i, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]
            L.m355_colour_linear.argtypes = [ctypes.POINTER(ColourTables), ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)]
        if hasattr(L, "m355_picture_maps_async"):
            L.m355_picture_maps_async.argtypes = [vp, i, ctypes.POINTER(MapsDesc), ctypes.POINTER(ctypes.c_ulonglong)]
            L.m355_picture_maps_result.argtypes = [vp, ctypes.c_ulonglong, i, ctypes.POINTER(MapsInfo)]
            L.m355_picture_maps_order.argtypes = [vp, ctypes.c_ulonglong, vp]
            L.m355_maps_unit.argtypes = [vp, i, i, i, i, vp]
        L.m355_submit_picture.argtypes = [vp, vp]
        L.m355_wait.argtypes = [vp]
        L.m355_last_serial.argtypes = [vp]
        L.m355_last_serial.restype = ctypes.c_ulonglong
        L.m355_decode_status.argtypes = [vp, ctypes.c_ulonglong]
        L.m355_picture_upload.argtypes = [vp, vp]
        L.m355_picture_replace.argtypes = [vp, i, vp]
        L.m355_picture_release.argtypes = [vp, i]
        L.m355_decode_resident.argtypes = [vp, i]
        L.m355_decode_batch.argtypes = [vp, ctypes.POINTER(i), i]
        L.m355_set_stages.argtypes = [vp, i]
        L.m355_set_pipeline_depth.argtypes = [vp, i]
        L.m355_timing_reset.argtypes = [vp]
        L.m355_timing_collect.argtypes = [vp, ctypes.POINTER(i), ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)]
        L.m355_stream.argtypes = [vp]
        L.m355_stream.restype = vp
        L.m355_shard_set.argtypes = [vp, i, i]
        L.m355_shard_owner_of_tile.argtypes = [i, i, i]
        L.m355_shard_xbuf_bytes.argtypes = [vp, i, i]
        L.m355_shard_xbuf_bytes.restype = ctypes.c_int64
        L.m355_decode_phase.argtypes = [vp, i, i, vp]
        L.m355_decode_sharded.argtypes = [vp, i, i]
        L.m355_shard_set_comm.argtypes = [vp, vp]
        L.m355_rccl_unique_id.argtypes = [vp]
        L.m355_shard_rccl_init.argtypes = [vp, vp, i, i]
        L.m355_shard_rccl_selftest.argtypes = [vp, ctypes.c_size_t]
        L.m355_shard_ipc_init.argtypes = [vp, ctypes.c_char_p, i, i]
        L.m355_shard_ipc_close.argtypes = [vp]
        L.m355_group_create.argtypes = [ctypes.POINTER(vp), i, ctypes.POINTER(vp)]
        L.m355_group_destroy.argtypes = [vp]
        L.m355_group_destroy.restype = None
        L.m355_group_decode.argtypes = [vp, ctypes.POINTER(i), i]
        L.m355_shard_peers.argtypes = [vp, i, i, ctypes.POINTER(i), i]
        L.m355_shard_time_exchange.argtypes = [vp, i, i, i, ctypes.POINTER(ctypes.c_float)]
        L.init_acceleration_functions_mi355x.argtypes = [vp]
        L.m355_transform_add_batch.argtypes = [i, i, i, i, vp, ctypes.c_size_t, vp, ctypes.c_ssize_t, vp]

    def error(self):
        return (self.lib.m355_last_error() or b"").decode()

    def rccl_unique_id(self):
        """rank 0 of a tile-sharded job: the RCCL unique id (128 bytes) to hand to every rank (Context.shard_rccl_init)"""
        buf = ctypes.create_string_buffer(128)
        self.check(self.lib.m355_rccl_unique_id(buf))
        return buf.raw

    def check(self, rc):
        if rc != 0:
            raise M355Error(rc, self.error())

    def device_count(self):
        return self.lib.m355_device_count()

    def rgb_coefficients(self, matrix, full_range, bit_depth_luma, bit_depth_chroma, samples):
        """the integers of the R'G'B' conversion (m355_rgb_coefficients; host only) -> dict F, y0, c0, cy, crv, cgu, cgv, cbu"""
        k = RgbCoeffs()
        self.check(self.lib.m355_rgb_coefficients(matrix, full_range, bit_depth_luma, bit_depth_chroma, samples, ctypes.byref(k)))
        return {n: int(getattr(k, n)) for n, _ in RgbCoeffs._fields_}

    def resize_taps(self, src_n, dst_n, cosited, i, filter=0, filtered_entry=False):
        """row i of one axis of the resize filter (m355_resize_taps, or m355_resize_taps_filtered for filter != 0 or on request; host only) ->
        (first source index, [coefficients]), or None for arguments it rejects"""
        first, coeff = ctypes.c_int32(), (ctypes.c_int32 * RESIZE_MAX_TAPS)()
        if filter != 0 or filtered_entry:
            n = self.lib.m355_resize_taps_filtered(filter, src_n, dst_n, cosited, i, ctypes.byref(first), coeff)
        else:
            n = self.lib.m355_resize_taps(src_n, dst_n, cosited, i, ctypes.byref(first), coeff)
        return None if n < 0 else (int(first.value), [int(coeff[k]) for k in range(n)])

    def tensor_element(self, v, scale, bias, dtype):
        """the float stage of m355_frames_export_tensor for one integer (m355_tensor_element; host only) -> the element's bit pattern"""
        bits = ctypes.c_uint32(0)
        self.check(self.lib.m355_tensor_element(v, scale, bias, dtype, ctypes.byref(bits)))
        return int(bits.value)

    def colour_preset(self, in_transfer, in_primaries, out_transfer, out_primaries, tone=TONE_CLIP, white_nits=0, peak_nits=0, reserved=0):
        """the tables of a preset (m355_colour_preset; host only) -> ColourTables"""
        d = ColourPresetDesc(in_transfer, in_primaries, out_transfer, out_primaries, tone, white_nits, peak_nits, reserved)
        t = ColourTables()
        self.check(self.lib.m355_colour_preset(ctypes.byref(d), ctypes.byref(t)))
        return t

    def pixel_pack(self, format, rgb, alpha):
        """one pixel's bytes (m355_pixel_pack; host only) -> bytes of length 3 or 4"""
        out, n = (ctypes.c_uint8 * 4)(), ctypes.c_int(0)
        self.check(self.lib.m355_pixel_pack(format, (ctypes.c_uint32 * 3)(*[int(v) for v in rgb]), alpha, out, ctypes.byref(n)))
        return bytes(out[:n.value])

    def orientation_compose(self, first, then):
        """the one orientation equal to `first` and then `then` (m355_orientation_compose; host only)"""
        out = ctypes.c_int(-1)
        self.check(self.lib.m355_orientation_compose(first, then, ctypes.byref(out)))
        return out.value

    def orientation_from_exif(self, exif):
        """the orientation that brings a picture stored with EXIF Orientation 1..8 upright (m355_orientation_from_exif; host only)"""
        out = ctypes.c_int(-1)
        self.check(self.lib.m355_orientation_from_exif(exif, ctypes.byref(out)))
        return out.value

    def colour_pixel(self, tables, rgb16, samples):
        """the colour transform stage for one pixel (m355_colour_pixel; host only) -> (R, G, B)"""
        out = (ctypes.c_uint32 * 3)()
        self.check(self.lib.m355_colour_pixel(ctypes.byref(tables), (ctypes.c_uint32 * 3)(*[int(v) for v in rgb16]), samples, out))
        return tuple(int(v) for v in out)

    def colour_preset_tone(self, in_transfer, in_primaries, out_transfer, out_primaries, tone=TONE_BT2390, norm=NORM_MAXRGB, white_nits=0, peak_nits=0,
                           reserved=0):
        """the tables and the gain of a tone preset (m355_colour_preset_tone; host only) -> (ColourTables, ColourTone)"""
        d = ColourPresetDesc(in_transfer, in_primaries, out_transfer, out_primaries, tone, white_nits, peak_nits, reserved)
        t, q = ColourTables(), ColourTone()
        self.check(self.lib.m355_colour_preset_tone(ctypes.byref(d), norm, ctypes.byref(t), ctypes.byref(q)))
        return t, q

    def colour_pixel_tone(self, tables, tone, rgb16, samples):
        """the colour transform stage of a tone object for one pixel (m355_colour_pixel_tone; host only) -> (R, G, B)"""
        out = (ctypes.c_uint32 * 3)()
        self.check(self.lib.m355_colour_pixel_tone(ctypes.byref(tables), ctypes.byref(tone), (ctypes.c_uint32 * 3)(*[int(v) for v in rgb16]), samples, out))
        return tuple(int(v) for v in out)

    def stats_quantile(self, hist, num, den):
        """the smallest bin b of a 256-bin histogram with den * (hist[0] + ... + hist[b]) >= num * total (m355_stats_quantile; host only)"""
        b = ctypes.c_int(-1)
        h = None if hist is None else (ctypes.c_uint32 * STATS_BINS)(*[int(v) for v in hist])
        self.check(self.lib.m355_stats_quantile(h, num, den, ctypes.byref(b)))
        return int(b.value)

    def ssim_window(self, sums, bit_depth):
        """q (Q30) of one window from its five sums (MA, MB, SAA, SBB, SAB) at a plane's bit depth (m355_ssim_window; host only)"""
        q = ctypes.c_int32(0)
        v = None if sums is None else (ctypes.c_uint64 * 5)(*[int(x) for x in sums])
        self.check(self.lib.m355_ssim_window(v, bit_depth, ctypes.byref(q)))
        return int(q.value)

    def ssim_weights(self):
        """the window's eleven integer weights (m355_ssim_weights; host only)"""
        w = (ctypes.c_int32 * SSIM_TAPS)()
        self.check(self.lib.m355_ssim_weights(w))
        return [int(x) for x in w]

    def ssim_window_cs(self, sums, bit_depth):
        """qc (Q30), the contrast-structure term of one window, from its five sums at a plane's bit depth (m355_ssim_window_cs; host only)"""
        q = ctypes.c_int32(0)
        v = None if sums is None else (ctypes.c_uint64 * 5)(*[int(x) for x in sums])
        self.check(self.lib.m355_ssim_window_cs(v, bit_depth, ctypes.byref(q)))
        return int(q.value)

    def msssim_combine(self, means, weights=None):
        """the product over the levels of max(mean, 0) ** weight, in level order (m355_msssim_combine; host only); weights None: Wang's five"""
        m = (ctypes.c_double * MSSSIM_LEVELS)(*[float(x) for x in means])
        w = None if weights is None else (ctypes.c_double * MSSSIM_LEVELS)(*[float(x) for x in weights])
        out = ctypes.c_double(0.0)
        self.check(self.lib.m355_msssim_combine(m, len(means), w, ctypes.byref(out)))
        return float(out.value)

    def colour_linear(self, tables, v16):
        """step 1 of the colour transform stage for one 16-bit value (m355_colour_linear; host only) -> linear light, 0 .. COLOUR_ONE"""
        out = ctypes.c_uint32(0)
        self.check(self.lib.m355_colour_linear(ctypes.byref(tables), int(v16), ctypes.byref(out)))
        return int(out.value)

    def maps_unit(self, pic, map, log2_unit, ux, uy, c_pic=None):
        """element (ux, uy) of one side map from HOST lists (m355_maps_unit, host only) -> u32 / i8 / u8 / u8 / four int16 / four u8 / u16 as Python
        ints; c_pic: the (CPicture, keepalive) of pic.to_c(), for callers that ask for many units of one picture"""
        c, keep = c_pic if c_pic is not None else pic.to_c()
        buf = (ctypes.c_uint8 * 8)()
        self.check(self.lib.m355_maps_unit(ctypes.addressof(c), map, log2_unit, ux, uy, buf))
        v = np.frombuffer(bytes(buf)[:MAP_ELEM_BYTES[map]], MAP_DTYPES[map])
        del keep
        return int(v[0]) if MAP_PER_UNIT[map] == 1 else [int(x) for x in v]

    def pack_narrow(self, pic):
        """m355_pack_narrow on a picture's residual records and coefficient list (host only; worklist.pack_narrow is the numpy
        statement of the same): a copy with every block that fits in the 16-bit entry form (worklist.RBF_NARROW)"""
        out = pic.copy()
        rbs = np.ascontiguousarray(pic.rbs, dtype=worklist.RB)
        co = np.ascontiguousarray(pic.coeffs, dtype=np.dtype("<u4"))
        out.rbs, co_out, n = np.zeros(len(rbs), worklist.RB), np.zeros(len(co), np.dtype("<u4")), ctypes.c_uint32(0)
        self.check(self.lib.m355_pack_narrow(rbs.ctypes.data, len(rbs), co.ctypes.data, len(co), out.rbs.ctypes.data, co_out.ctypes.data, ctypes.byref(n)))
        out.coeffs = co_out[:n.value].copy()
        return out


class Context:
    """One decoding context = one GPU, one HIP stream, a device-resident frame pool."""

    def __init__(self, lib=None, device=0):
        self.L = lib or Library()
        h = ctypes.c_void_p()
        self.L.check(self.L.lib.m355_create(device, ctypes.byref(h)))
        self.h = h
        self._geom = {}
        self._hash_reqs = {}            # ticket -> (hash type, planes) of the requests not collected yet
        self._measure_reqs = {}         # ticket -> (planes, reference buffers to free, host?) of the comparison requests not collected yet
        self._stats_reqs = {}           # ticket -> (planes, light?) of the statistics requests not collected yet
        self._ssim_reqs = {}            # ticket -> (reference buffers to free, host?) of the SSIM requests not collected yet
        self._msssim_reqs = {}          # ticket -> (reference buffers to free, host?) of the MS-SSIM requests not collected yet
        self._maps_reqs = {}            # ticket -> (per map None or (buffer, offset, pitch, rows, row bytes), units, host?) of the side-map requests not collected yet
        self._pic_size = {}             # picture handle (PICTURE_LAST: the most recent submit) -> (width, height), for the side maps' unit grid

    def close(self):
        if self.h:
            self.L.lib.m355_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- frames ----
    def frame_create(self, width, height, chroma_format_idc=1, bit_depth_luma=8, bit_depth_chroma=8):
        f = self.L.lib.m355_frame_create(self.h, width, height, chroma_format_idc, bit_depth_luma, bit_depth_chroma)
        if f < 0:
            raise M355Error(-f, self.L.error())
        self._geom[f] = (width, height, chroma_format_idc, bit_depth_luma, bit_depth_chroma)
        return f

    def frame_create_for(self, pp):
        return self.frame_create(int(pp["width"]), int(pp["height"]), int(pp["chroma_format_idc"]),
                                 int(pp["bit_depth_luma"]), int(pp["bit_depth_chroma"]))

    def frame_destroy(self, f):
        self.L.check(self.L.lib.m355_frame_destroy(self.h, f))
        self._geom.pop(f, None)

    def frame_upload(self, f, planes):
        for c, a in enumerate(planes):
            a = np.ascontiguousarray(a)
            self.L.check(self.L.lib.m355_frame_upload(self.h, f, c, a.ctypes.data, a.shape[1]))

    def frame_download(self, f):
        w, h, cf, bdl, bdc = self._geom[f]
        out = []
        for c, (pw, ph) in enumerate(worklist.plane_dims(w, h, cf)):
            if pw == 0:
                continue
            a = np.zeros((ph, pw), np.uint8 if (bdl if c == 0 else bdc) <= 8 else np.uint16)
            self.L.check(self.L.lib.m355_frame_download(self.h, f, c, a.ctypes.data, pw))
            out.append(a)
        return out

    def frame_download_async(self, f):
        """start the download of all planes behind the frame's last writer (into pinned planes); -> token for frame_download_finish"""
        w, h, cf, bdl, bdc = self._geom[f]
        dst = (ctypes.c_void_p * 3)(); strides = (ctypes.c_ssize_t * 3)()
        arrays, bufs = [], []
        for c, (pw, ph) in enumerate(worklist.plane_dims(w, h, cf)):
            if pw == 0:
                continue
            dt = np.uint8 if (bdl if c == 0 else bdc) <= 8 else np.uint16
            nbytes = pw * ph * np.dtype(dt).itemsize
            p = self.L.lib.m355_host_alloc(nbytes)
            if not p:
                for q in bufs:                       # (the planes of this call that were already allocated)
                    self.L.lib.m355_host_free(q)
                raise M355Error(4, self.L.error())   # M355_ERR_NOMEM
            bufs.append(p)
            arrays.append(np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_uint8)), (nbytes,)).view(dt).reshape(ph, pw))
            dst[c] = p; strides[c] = pw
        self.L.check(self.L.lib.m355_frame_download_async(self.h, f, dst, strides))
        return (f, arrays, bufs)

    def pinned_planes(self, f):
        """pinned host planes for frame f (m355_host_alloc), for repeated frame_download_start calls -> (dst[3], strides[3], arrays, pointers)"""
        w, h, cf, bdl, bdc = self._geom[f]
        dst = (ctypes.c_void_p * 3)(); strides = (ctypes.c_ssize_t * 3)()
        arrays, bufs = [], []
        for c, (pw, ph) in enumerate(worklist.plane_dims(w, h, cf)):
            if pw == 0:
                continue
            dt = np.uint8 if (bdl if c == 0 else bdc) <= 8 else np.uint16
            nbytes = pw * ph * np.dtype(dt).itemsize
            p = self.L.lib.m355_host_alloc(nbytes)
            if not p:
                for q in bufs:                       # (the planes of this call that were already allocated)
                    self.L.lib.m355_host_free(q)
                raise M355Error(4, self.L.error())   # M355_ERR_NOMEM
            bufs.append(p)
            arrays.append(np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_uint8)), (nbytes,)).view(dt).reshape(ph, pw))
            dst[c] = p; strides[c] = pw
        return dst, strides, arrays, bufs

    def frame_download_start(self, f, planes):
        """m355_frame_download_async into planes from pinned_planes(); frame_download_wait(f) completes it"""
        self.L.check(self.L.lib.m355_frame_download_async(self.h, f, planes[0], planes[1]))

    def frame_download_wait(self, f):
        self.L.check(self.L.lib.m355_frame_download_wait(self.h, f))

    def pinned_free(self, planes):
        for p in planes[3]:
            self.L.lib.m355_host_free(p)

    def frame_download_finish(self, token):
        f, arrays, bufs = token
        self.L.check(self.L.lib.m355_frame_download_wait(self.h, f))
        out = [a.copy() for a in arrays]
        for p in bufs:
            self.L.lib.m355_host_free(p)
        return out

    # ---- export into device memory (m355_frame_export) ----
    def device_alloc(self, nbytes, fill=DEVICE_FILL):
        """device memory (m355_device_alloc), every byte set to `fill` through m355_device_write (None: left as it comes) -> pointer"""
        p = self.L.lib.m355_device_alloc(self.h, nbytes)
        if not p:
            raise M355Error(4, self.L.error())       # M355_ERR_NOMEM
        if fill is not None:
            a = np.full(nbytes, fill, np.uint8)
            rc = self.L.lib.m355_device_write(self.h, p, a.ctypes.data, nbytes)
            if rc:
                self.L.lib.m355_device_free(self.h, p)
                self.L.check(rc)
        return p

    def device_free(self, p):
        self.L.lib.m355_device_free(self.h, p)

    def device_read(self, p, nbytes):
        """blocking copy of device memory (m355_device_read) -> uint8 array"""
        a = np.zeros(nbytes, np.uint8)
        self.L.check(self.L.lib.m355_device_read(self.h, p, a.ctypes.data, nbytes))
        return a

    def export_shapes(self, f, layout, samples, rect=None, log2_scale=0):
        """the destination planes of an export of frame f: [(rows, elements per row, dtype)] — semi-planar: Y, then Cb and Cr interleaved;
        log2_scale: every plane's size divided by 1 << log2_scale (m355_frame_export_scaled)"""
        w, h, cf, bdl, bdc = self._geom[f]
        if rect is not None:
            w, h = rect[2], rect[3]
        out = []
        for c, (pw, ph) in enumerate(worklist.plane_dims(w, h, cf)):
            if pw == 0 or (layout == EXPORT_SEMIPLANAR and c == 2):
                continue
            pw, ph = pw >> log2_scale, ph >> log2_scale
            native = np.uint8 if (bdl if c == 0 else bdc) <= 8 else np.uint16
            dt = native if samples == EXPORT_NATIVE else (np.uint16 if samples == EXPORT_MSB16 else np.uint8)
            out.append((ph, pw * (2 if layout == EXPORT_SEMIPLANAR and c == 1 else 1), np.dtype(dt)))
        return out

    def _buffer(self, nbytes, host):
        """a destination buffer — device memory, or with host=True pinned host memory —, every byte of which holds DEVICE_FILL -> pointer"""
        if not host:
            return self.device_alloc(nbytes)
        p = self.L.lib.m355_host_alloc(nbytes)
        if not p:
            raise M355Error(4, self.L.error())
        ctypes.memset(p, DEVICE_FILL, nbytes)
        return p

    def _buffer_free(self, p, host):
        self.L.lib.m355_host_free(p) if host else self.device_free(p)

    def _export_into_planes(self, f, shapes, desc, host, pad, call):
        """what the four frame exports do with their destinations: a _buffer per entry (rows, n, dtype) of shapes, its pitch `pad` bytes LARGER than
        the row — so rows start at addresses that are no multiple of a vector —, into desc.dst[k] / desc.pitch[k]; then call(), the export itself; if
        anything raises, every buffer is freed again.  -> token for frame_export_finish"""
        bufs = []
        try:
            for k, (rows, n, dt) in enumerate(shapes):
                pitch = n * dt.itemsize + pad
                bufs.append(self._buffer(rows * pitch, host))
                desc.dst[k] = bufs[-1]; desc.pitch[k] = pitch
            call()
        except Exception:
            for p in bufs:
                self._buffer_free(p, host)
            raise
        return (f, shapes, bufs, [int(desc.pitch[k]) for k in range(len(shapes))], host)

    def _export_entry(self, base, args, filter=0, filtered_entry=False, chroma_loc=0, opts_entry=False, colour=0):
        """one export through the entry point its keywords pick: a chroma_loc or colour other than 0, or opts_entry, goes through base + "_opts" with
        an ExportOpts of filter, chroma_loc and colour (opts_entry=None: with a NULL options pointer); else a filter other than 0, or filtered_entry,
        through base + "_filtered"; else through base"""
        lib = self.L.lib
        if chroma_loc != 0 or colour != 0 or opts_entry or opts_entry is None:
            self.L.check(getattr(lib, base + "_opts")(*args, self._opts(filter, chroma_loc, opts_entry, colour)))
        elif filter != 0 or filtered_entry:
            self.L.check(getattr(lib, base + "_filtered")(*args, filter))
        else:
            self.L.check(getattr(lib, base)(*args))

    def frame_export(self, f, layout, samples, rect=None, host=False, pad=20, log2_scale=0, scaled_entry=False):
        """start m355_frame_export of frame f (rect = (x0, y0, width, height) in luma samples, None: the whole frame) into buffers of its
        own — device memory, or with host=True pinned host memory —, every byte of which holds DEVICE_FILL beforehand; the pitch is `pad`
        bytes LARGER than the row, so rows start at addresses that are no multiple of a vector.  log2_scale != 0: downscaled by 1 << log2_scale
        (m355_frame_export_scaled; scaled_entry=True takes that entry point for log2_scale 0 too).  -> token for frame_export_finish"""
        desc = ExportDesc(layout=layout, samples=samples)
        if rect is not None:
            desc.x0, desc.y0, desc.width, desc.height = rect

        def call():
            if log2_scale or scaled_entry:
                self.L.check(self.L.lib.m355_frame_export_scaled(self.h, f, ctypes.byref(desc), log2_scale))
            else:
                self.L.check(self.L.lib.m355_frame_export(self.h, f, ctypes.byref(desc)))
        return self._export_into_planes(f, self.export_shapes(f, layout, samples, rect, log2_scale), desc, host, pad, call)

    def frame_export_oriented(self, f, layout, samples, orientation, rect=None, host=False, pad=20):
        """start m355_frame_export_oriented of frame f: frame_export's buffers with the shapes of the ORIENTED planes (TRANSPOSE: rows and elements per
        row exchanged; an interleaved plane keeps its pairs).  -> token for frame_export_finish"""
        desc = ExportDesc(layout=layout, samples=samples)
        if rect is not None:
            desc.x0, desc.y0, desc.width, desc.height = rect
        shapes = self.export_shapes(f, layout, samples, rect)
        if orientation & ORIENT_TRANSPOSE:
            semi = [layout == EXPORT_SEMIPLANAR and k == 1 for k in range(len(shapes))]
            shapes = [(n // 2, rows * 2, dt) if s else (n, rows, dt) for (rows, n, dt), s in zip(shapes, semi)]
        return self._export_into_planes(f, shapes, desc, host, pad,
                                        lambda: self.L.check(self.L.lib.m355_frame_export_oriented(self.h, f, ctypes.byref(desc), orientation)))

    def frame_export_pixels_oriented(self, f, format, alpha, matrix, full_range, orientation, rect=None, host=False, pad=20, chroma_loc=0):
        """start m355_frame_export_pixels_oriented of frame f: frame_export_pixels' buffer with the shape of the ORIENTED picture.
        -> token for frame_export_finish"""
        w, h = self._geom[f][:2] if rect is None else rect[2:]
        if orientation & ORIENT_TRANSPOSE:
            w, h = h, w
        opts = self._opts(0, chroma_loc, False) if chroma_loc else None
        return self._frame_export_pixels("m355_frame_export_pixels_oriented", f, format, alpha, matrix, full_range, w, h, (0, 0), rect, host, pad, opts,
                                         (orientation,))

    def resize_taps(self, src_n, dst_n, cosited, i, filter=0, filtered_entry=False):
        """row i of one axis of the resize filter (m355_resize_taps) -> (first source index, [coefficients]), or None for arguments it rejects"""
        return self.L.resize_taps(src_n, dst_n, cosited, i, filter, filtered_entry)

    def frame_export_resized(self, f, layout, samples, out_size, rect=None, host=False, pad=20, filter=0, filtered_entry=False, chroma_loc=0,
                             opts_entry=False, colour=0):
        """start m355_frame_export_resized of frame f to out_size = (out_width, out_height) luma samples (rect = the source rectangle (x0, y0, width,
        height) in luma samples, None: the whole frame) into buffers of its own, made as frame_export makes them: every byte holds DEVICE_FILL
        beforehand, the pitch is `pad` bytes larger than the row.  filter, filtered_entry, chroma_loc, opts_entry and colour pick the plain, the
        _filtered or the _opts entry point as _export_entry states it, here and in the three helpers below.  -> token for frame_export_finish"""
        entry = (filter, filtered_entry, chroma_loc, opts_entry, colour)
        desc = ResizeDesc(layout=layout, samples=samples, out_width=out_size[0], out_height=out_size[1])
        if rect is not None:
            desc.x0, desc.y0, desc.width, desc.height = rect
        return self._export_into_planes(f, self.export_shapes(f, layout, samples, (0, 0, out_size[0], out_size[1])), desc, host, pad,
                                        lambda: self._export_entry("m355_frame_export_resized", (self.h, f, ctypes.byref(desc)), *entry))

    @staticmethod
    def _opts(filter, chroma_loc, opts_entry, colour=0):
        """the options argument of an _opts entry point: an ExportOpts by reference, or NULL for opts_entry=None"""
        if opts_entry is None:
            return None
        o = ExportOpts(filter=filter, chroma_loc=chroma_loc)
        o.reserved[0] = colour
        return ctypes.byref(o)

    def colour_create(self, tables):
        """m355_colour_create: the tables (ColourTables, or None for a NULL pointer) as an object of this context -> its handle (>= 0x100), which
        the `colour` keyword of the composed exports takes"""
        h = ctypes.c_int(0)
        self.L.check(self.L.lib.m355_colour_create(self.h, None if tables is None else ctypes.byref(tables), ctypes.byref(h)))
        return int(h.value)

    def colour_create_tone(self, tables, tone):
        """m355_colour_create_tone: the tables and the tone (ColourTables, ColourTone; None for a NULL pointer) as a tone object of this context ->
        its handle, which goes wherever colour_create's does; colour_destroy destroys it"""
        h = ctypes.c_int(0)
        self.L.check(self.L.lib.m355_colour_create_tone(self.h, None if tables is None else ctypes.byref(tables), None if tone is None else ctypes.byref(tone),
                                                        ctypes.byref(h)))
        return int(h.value)

    def colour_destroy(self, handle):
        self.L.check(self.L.lib.m355_colour_destroy(self.h, handle))

    def rgb_coefficients(self, matrix, full_range, bit_depth_luma, bit_depth_chroma, samples):
        """the integers of the R'G'B' conversion (m355_rgb_coefficients) -> dict F, y0, c0, cy, crv, cgu, cgv, cbu"""
        return self.L.rgb_coefficients(matrix, full_range, bit_depth_luma, bit_depth_chroma, samples)

    @staticmethod
    def _rgb_shapes(w, h, layout, samples):
        """packed: one plane of 3 * w elements per row; planar: R, G, B"""
        dt = np.dtype(np.uint16 if samples == RGB_U16 else np.uint8)
        return [(h, 3 * w, dt)] if layout == RGB_PACKED else [(h, w, dt)] * 3

    def frame_export_rgb(self, f, layout, samples, matrix, full_range, rect=None, host=False, pad=20, chroma_loc=0, opts_entry=False, colour=0):
        """start m355_frame_export_rgb of frame f (rect = (x0, y0, width, height) in luma samples, None: the whole frame) into buffers of its own,
        made as frame_export makes them: every byte holds DEVICE_FILL beforehand, the pitch is `pad` bytes larger than the row.  Packed: one plane
        of 3 * width elements per row; planar: R, G, B.  (The call has no _filtered form.)  -> token for frame_export_finish"""
        w, h = self._geom[f][:2] if rect is None else rect[2:]
        entry = (0, False, chroma_loc, opts_entry, colour)
        desc = RgbDesc(layout=layout, samples=samples, matrix=matrix, full_range=full_range)
        if rect is not None:
            desc.x0, desc.y0, desc.width, desc.height = rect
        return self._export_into_planes(f, self._rgb_shapes(w, h, layout, samples), desc, host, pad,
                                        lambda: self._export_entry("m355_frame_export_rgb", (self.h, f, ctypes.byref(desc)), *entry))

    def frame_export_resized_rgb(self, f, layout, samples, matrix, full_range, out_size, rect=None, host=False, pad=20, filter=0, filtered_entry=False,
                                 chroma_loc=0, opts_entry=False, colour=0):
        """start m355_frame_export_resized_rgb of frame f to out_size = (out_width, out_height) luma samples (rect = the source rectangle (x0, y0,
        width, height) in luma samples, None: the whole frame) into buffers of its own, made as frame_export_rgb makes them: every byte holds
        DEVICE_FILL beforehand, the pitch is `pad` bytes larger than the row.  Packed: one plane of 3 * out_width elements per row; planar: R, G, B.
        colour: 0, or the handle of a colour transform (colour_create), which goes through the _opts entry point like a chroma_loc other than 0 —
        so it does in the two tensor calls below.  -> token for frame_export_finish"""
        w, h = out_size
        entry = (filter, filtered_entry, chroma_loc, opts_entry, colour)
        desc = ResizeRgbDesc(layout=layout, samples=samples, matrix=matrix, full_range=full_range, out_width=w, out_height=h)
        if rect is not None:
            desc.x0, desc.y0, desc.width, desc.height = rect
        return self._export_into_planes(f, self._rgb_shapes(w, h, layout, samples), desc, host, pad,
                                        lambda: self._export_entry("m355_frame_export_resized_rgb", (self.h, f, ctypes.byref(desc)), *entry))

    def _frame_export_pixels(self, name, f, format, alpha, matrix, full_range, w, h, out_size, rect, host, pad, opts, more=()):
        """what the two pixel exports share: ONE buffer of h rows of w * pixel_bytes(format) bytes, made as frame_export_rgb makes its buffers — every
        byte holds DEVICE_FILL beforehand (the guard bytes), the pitch is `pad` bytes (a multiple of 4) larger than the row —, the descriptor, the call;
        the buffer is freed again if the call raises.  -> token for frame_export_finish, whose one plane is (h, w * pixel_bytes) uint8"""
        shapes = [(h, w * pixel_bytes(format), np.dtype(np.uint8))]
        desc = PixelDesc(format=format, alpha=alpha, matrix=matrix, full_range=full_range, out_width=out_size[0], out_height=out_size[1])
        if rect is not None:
            desc.x0, desc.y0, desc.width, desc.height = rect
        pitch = shapes[0][1] + pad
        buf = self._buffer(h * pitch, host)
        desc.dst, desc.pitch = buf, pitch
        try:
            self.L.check(getattr(self.L.lib, name)(self.h, f, ctypes.byref(desc), opts, *more))
        except Exception:
            self._buffer_free(buf, host)
            raise
        return (f, shapes, [buf], [pitch], host)

    def frame_export_pixels(self, f, format, alpha, matrix, full_range, rect=None, host=False, pad=20, chroma_loc=0, opts_entry=False, colour=0):
        """start m355_frame_export_pixels of frame f (PIXEL_* format; rect = (x0, y0, width, height) in luma samples, None: the whole frame) into a
        buffer of its own with guard bytes, as frame_export_rgb does.  A NULL options pointer unless chroma_loc, colour or opts_entry ask for one.
        -> token for frame_export_finish"""
        w, h = self._geom[f][:2] if rect is None else rect[2:]
        opts = self._opts(0, chroma_loc, opts_entry, colour) if (chroma_loc or colour or opts_entry) else None
        return self._frame_export_pixels("m355_frame_export_pixels", f, format, alpha, matrix, full_range, w, h, (0, 0), rect, host, pad, opts)

    def frame_export_resized_pixels(self, f, format, alpha, matrix, full_range, out_size, rect=None, host=False, pad=20, filter=0, chroma_loc=0,
                                    opts_entry=False, colour=0):
        """start m355_frame_export_resized_pixels of frame f to out_size = (out_width, out_height) luma samples, with the filter, the chroma siting and
        the colour / tone object of frame_export_resized_rgb; the buffer as in frame_export_pixels.  -> token for frame_export_finish"""
        opts = self._opts(filter, chroma_loc, opts_entry, colour) if (filter or chroma_loc or colour or opts_entry) else None
        return self._frame_export_pixels("m355_frame_export_resized_pixels", f, format, alpha, matrix, full_range, out_size[0], out_size[1], out_size,
                                         rect, host, pad, opts)

    def pixel_pack(self, format, rgb, alpha):
        """one pixel's bytes (m355_pixel_pack)"""
        return self.L.pixel_pack(format, rgb, alpha)

    def tensor_element(self, v, scale, bias, dtype):
        """the float stage of m355_frames_export_tensor for one integer (m355_tensor_element) -> the element's bit pattern"""
        return self.L.tensor_element(v, scale, bias, dtype)

    def frames_export_tensor(self, frames, layout, dtype, samples, matrix, full_range, out_size, scale, bias, rect=None, host=False, pad=20, filter=0,
                             filtered_entry=False, chroma_loc=0, opts_entry=False, colour=0):
        """start m355_frames_export_tensor of the frames (handles; the same one may repeat) to out_size = (out_width, out_height) luma samples each
        (rect = the source rectangle (x0, y0, width, height) in luma samples, the same in every frame; None: the whole frame) into ONE buffer of its
        own, made as frame_export_resized_rgb makes its buffers: every byte holds DEVICE_FILL beforehand, and every stride is `pad` bytes (a multiple
        of the element size) above the smallest one the call accepts — stride_h above the row, stride_c above a plane, stride_n above a slice.
        scale, bias: three floats each (R, G, B).  -> token for tensor_export_finish"""
        return self._frames_export_tensor(frames, None, layout, dtype, samples, matrix, full_range, out_size, scale, bias, rect, host, pad,
                                          (filter, filtered_entry, chroma_loc, opts_entry, colour))

    def frames_export_tensor_rois(self, frames, rois, layout, dtype, samples, matrix, full_range, out_size, scale, bias, host=False, pad=20, filter=0,
                                  filtered_entry=False, chroma_loc=0, opts_entry=False, colour=0):
        """start m355_frames_export_tensor_rois: slice i is the rectangle rois[i] = (x0, y0, width, height, flags) of frames[i] (None or width 0: the
        whole of that frame; flags: 0 or ROI_MIRROR), resized to out_size.  The buffer is made as frames_export_tensor makes it: DEVICE_FILL in every
        byte, every stride `pad` bytes above the smallest one the call accepts.  -> token for tensor_export_finish"""
        return self._frames_export_tensor(frames, [r if r is not None else (0, 0, 0, 0, 0) for r in rois], layout, dtype, samples, matrix, full_range,
                                          out_size, scale, bias, None, host, pad, (filter, filtered_entry, chroma_loc, opts_entry, colour))

    def _frames_export_tensor(self, frames, rois, layout, dtype, samples, matrix, full_range, out_size, scale, bias, rect, host, pad, entry):
        w, h = out_size
        n, eb = len(frames), (4 if dtype == TENSOR_F32 else 2)
        row = w * eb * (3 if layout == TENSOR_NHWC else 1)
        stride_h = row + pad
        extent = (h - 1) * stride_h + row
        stride_c = extent + pad if layout == TENSOR_NCHW else 0
        stride_n = (2 * stride_c + extent if layout == TENSOR_NCHW else extent) + pad
        nbytes = (n - 1) * stride_n + (2 * stride_c + extent)
        desc = TensorDesc(layout=layout, dtype=dtype, samples=samples, matrix=matrix, full_range=full_range, out_width=w, out_height=h,
                          stride_n=stride_n, stride_c=stride_c, stride_h=stride_h)
        desc.scale = (ctypes.c_float * 3)(*scale)
        desc.bias = (ctypes.c_float * 3)(*bias)
        if rect is not None:
            desc.x0, desc.y0, desc.width, desc.height = rect
        p = desc.dst = self._buffer(nbytes, host)
        try:
            if rois is None:
                self._export_entry("m355_frames_export_tensor", (self.h, (ctypes.c_int * n)(*frames), n, ctypes.byref(desc)), *entry)
            else:
                assert len(rois) == n
                arr = (TensorRoi * n)(*[TensorRoi(*r) for r in rois])
                self._export_entry("m355_frames_export_tensor_rois", (self.h, (ctypes.c_int * n)(*frames), arr, n, ctypes.byref(desc)), *entry)
        except Exception:
            self._buffer_free(p, host)
            raise
        return (list(frames), (n, h, w), layout, eb, p, nbytes, (stride_n, stride_c, stride_h), host)

    def tensor_export_finish(self, token, wait_frame=None):
        """the tensor of a frames_export_tensor, read back (device buffer: m355_device_read, which waits for the context's work; pinned host buffer:
        behind m355_frame_export_wait of wait_frame, default the batch's last frame) and freed -> (elements, raw, outside): the elements' bit
        patterns as a uint16 / uint32 array of shape (n, 3, h, w) or (n, h, w, 3), the whole buffer as bytes, and the bytes of it that are no
        element of the tensor"""
        frames, (n, h, w), layout, eb, p, nbytes, (stride_n, stride_c, stride_h), host = token
        if host:
            self.L.check(self.L.lib.m355_frame_export_wait(self.h, frames[-1] if wait_frame is None else wait_frame))
            raw = np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_uint8)), (nbytes,)).copy()
            self.L.lib.m355_host_free(p)
        else:
            raw = self.device_read(p, nbytes)
            self.device_free(p)
        if layout == TENSOR_NCHW:
            shape, strides = (n, 3, h, w, eb), (stride_n, stride_c, stride_h, eb, 1)
        else:
            shape, strides = (n, h, w, 3, eb), (stride_n, stride_h, 3 * eb, eb, 1)
        view = np.lib.stride_tricks.as_strided(raw, shape, strides)
        elements = np.ascontiguousarray(view).view(np.uint32 if eb == 4 else np.uint16).reshape(shape[:-1])
        inside = np.zeros(nbytes, np.uint8)
        np.lib.stride_tricks.as_strided(inside, shape, strides)[...] = 1
        return elements, raw, raw[inside == 0]

    def frame_export_finish(self, token, raw=False):
        """the planes of a frame_export, read back (device buffers: m355_device_read, which waits for the context's work; pinned host buffers:
        behind m355_frame_export_wait) and freed -> list of numpy planes; raw=True: (planes, the whole buffers as (rows, pitch) byte arrays)"""
        f, shapes, bufs, pitches, host = token
        if host:
            self.L.check(self.L.lib.m355_frame_export_wait(self.h, f))
        planes, raws = [], []
        for (rows, n, dt), p, pitch in zip(shapes, bufs, pitches):
            if host:
                b = np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_uint8)), (rows * pitch,)).copy()
                self.L.lib.m355_host_free(p)
            else:
                b = self.device_read(p, rows * pitch)
                self.device_free(p)
            b = b.reshape(rows, pitch)
            raws.append(b)
            planes.append(np.ascontiguousarray(b[:, :n * dt.itemsize]).view(dt))
        return (planes, raws) if raw else planes

    def frame_export_wait(self, f):
        self.L.check(self.L.lib.m355_frame_export_wait(self.h, f))

    def frame_export_order(self, f, stream):
        """the consumer's stream (a hipStream_t as an integer) waits for frame f's last export (m355_frame_export_order)"""
        self.L.check(self.L.lib.m355_frame_export_order(self.h, f, stream))

    def frame_fill(self, f, luma, chroma):
        self.L.check(self.L.lib.m355_frame_fill(self.h, f, luma, chroma))

    def measure_copy_rate(self, nbytes=1 << 30, iters=9):
        """device-to-device copy rate of this box in GB/s (m355_measure_copy_rate: read + written bytes / time)"""
        g = ctypes.c_double(0)
        self.L.check(self.L.lib.m355_measure_copy_rate(self.h, nbytes, iters, ctypes.byref(g)))
        return float(g.value)

    def frame_hash(self, f, hash_type):
        """SEI decoded picture hash (m355_frame_hash): list of per-plane values — bytes (MD5) or int (CRC, checksum)"""
        out = PictureHash()
        self.L.check(self.L.lib.m355_frame_hash(self.h, f, hash_type, ctypes.addressof(out)))
        w, h, cf, bdl, bdc = self._geom[f]
        n = 3 if cf else 1
        if hash_type == HASH_MD5:
            return [bytes(out.md5[c]) for c in range(n)]
        return [int((out.crc if hash_type == HASH_CRC else out.checksum)[c]) for c in range(n)]

    def frame_hash_async(self, f, hash_type):
        """enqueue the hash of the frame as its last writer leaves it (m355_frame_hash_async; nothing is waited for) -> ticket"""
        t = ctypes.c_ulonglong(0)
        self.L.check(self.L.lib.m355_frame_hash_async(self.h, f, hash_type, ctypes.byref(t)))
        self._hash_reqs[t.value] = (hash_type, 3 if self._geom[f][2] else 1)
        return int(t.value)

    def frame_hash_result(self, ticket, block=True):
        """collect a request (m355_frame_hash_result): the list frame_hash returns; None while it has not finished (block=False);
        raises M355Error for an unknown / collected ticket and for a hash queued behind a rejected decode"""
        out = PictureHash()
        rc = self.L.lib.m355_frame_hash_result(self.h, ticket, 1 if block else 0, ctypes.addressof(out))
        if rc == 6 and not block:                               # M355_ERR_BUSY
            return None
        self.L.check(rc)
        hash_type, n = self._hash_reqs.pop(ticket)
        if hash_type == HASH_MD5:
            return [bytes(out.md5[c]) for c in range(n)]
        return [int((out.crc if hash_type == HASH_CRC else out.checksum)[c]) for c in range(n)]

    # ---- comparison with another picture on the device (m355_frame_measure_async) ----
    def measure_reference(self, planes, host=False, pad=None):
        """the reference planes of a comparison (numpy arrays of the frame's element type, the RECTANGLE's planes) copied into device memory
        (m355_device_*; host=True: pinned host memory) at a pitch `pad` bytes above the row (default 6 for u8, 10 for u16: every row of the
        reference starts at another alignment than the frame's).  m355_device_write waits for the context's work, so a caller that must not wait
        between two enqueues prepares the reference beforehand -> token for frame_measure_async(ref_planes=...), which owns it from then on"""
        bufs, pitches = [], []
        try:
            for a in planes:
                a = np.ascontiguousarray(a)
                pitch = a.shape[1] * a.itemsize + ((6 if a.itemsize == 1 else 10) if pad is None else pad)
                raw = np.full((a.shape[0], pitch), DEVICE_FILL, np.uint8)
                raw[:, :a.shape[1] * a.itemsize] = a.view(np.uint8).reshape(a.shape[0], -1)
                if host:
                    p = self.L.lib.m355_host_alloc(raw.size)
                    if not p:
                        raise M355Error(4, self.L.error())
                    bufs.append(p)
                    ctypes.memmove(p, raw.ctypes.data, raw.size)
                else:
                    p = self.device_alloc(raw.size, fill=None)
                    bufs.append(p)
                    self.L.check(self.L.lib.m355_device_write(self.h, p, raw.ctypes.data, raw.size))
                pitches.append(pitch)
        except Exception:
            self._measure_free(bufs, host)
            raise
        return ("measure_reference", bufs, pitches, host)

    def frame_measure_async(self, f, ref_frame=None, ref_planes=None, rect=None, host=False, pad=None):
        """enqueue the comparison of frame f (rect = (x0, y0, width, height) in luma samples, None: the whole frame) with frame `ref_frame`, or
        with `ref_planes`: a token of measure_reference, or numpy planes, which go through measure_reference(host, pad) first.  Nothing is
        waited for behind the enqueue -> ticket for frame_measure_result, which frees the reference's buffers"""
        desc = MeasureDesc(ref_frame=-1 if ref_frame is None else ref_frame)
        if rect is not None:
            desc.x0, desc.y0, desc.width, desc.height = rect
        if ref_planes is not None and not (isinstance(ref_planes, tuple) and ref_planes[:1] == ("measure_reference",)):
            ref_planes = self.measure_reference(ref_planes, host, pad)
        _, bufs, pitches, host = ref_planes or (None, [], [], False)
        for k, (p, pitch) in enumerate(zip(bufs, pitches)):
            desc.ref[k] = p; desc.pitch[k] = pitch
        t = ctypes.c_ulonglong(0)
        rc = self.L.lib.m355_frame_measure_async(self.h, f, ctypes.byref(desc), ctypes.byref(t))
        if rc:
            text = self.L.error()
            self._measure_free(bufs, host)
            raise M355Error(rc, text)
        self._measure_reqs[t.value] = (3 if self._geom[f][2] else 1, bufs, host)
        return int(t.value)

    def _measure_free(self, bufs, host):
        for p in bufs:
            self.L.lib.m355_host_free(p) if host else self.device_free(p)

    def frame_measure_result(self, ticket, block=True):
        """collect a request (m355_frame_measure_result) -> one dict per plane of the frame: ssd, sad, n_diff, max_abs, first (x, y) or None, mse;
        None while it has not finished (block=False); raises M355Error for an unknown / collected ticket and behind a rejected decode"""
        out = Measure()
        rc = self.L.lib.m355_frame_measure_result(self.h, ticket, 1 if block else 0, ctypes.byref(out))
        if rc == 6 and not block:                               # M355_ERR_BUSY
            return None
        if rc:
            text = self.L.error()
            if rc == 3:                                         # M355_ERR_INVALID: collected without a value (behind a rejected decode), or no such request
                self._measure_free(*self._measure_reqs.pop(ticket, (3, [], False))[1:])
            # (any other failure — the wait itself failed — may leave the request outstanding and reading the reference's buffers: they stay)
            raise M355Error(rc, text)
        n, bufs, host = self._measure_reqs.pop(ticket)
        self._measure_free(bufs, host)                          # (collected: nothing reads the buffers any more)
        return [dict(ssd=int(out.ssd[c]), sad=int(out.sad[c]), n_diff=int(out.n_diff[c]), max_abs=int(out.max_abs[c]),
                     first=None if out.first_x[c] < 0 else (int(out.first_x[c]), int(out.first_y[c])), mse=float(out.mse[c])) for c in range(n)]

    # ---- what is in the frame (m355_frame_stats_async) ----
    def frame_stats_async(self, f, rect=None, black=0, light=False, matrix=0, full_range=0, chroma_loc=0):
        """enqueue the statistics of frame f (rect = (x0, y0, width, height) in luma samples, None: the whole frame): histograms, min, max and sums
        per plane, the box of the luma samples > black and, with light, the same for max(R, G, B) of every pixel's 16-bit R'G'B' under matrix /
        full_range / chroma_loc.  Nothing is waited for -> ticket for frame_stats_result"""
        desc = StatsDesc(black=black, light=1 if light else 0, matrix=matrix, full_range=full_range, chroma_loc=chroma_loc)
        if rect is not None:
            desc.x0, desc.y0, desc.width, desc.height = rect
        t = ctypes.c_ulonglong(0)
        self.L.check(self.L.lib.m355_frame_stats_async(self.h, f, ctypes.byref(desc), ctypes.byref(t)))
        self._stats_reqs[t.value] = (3 if self._geom[f][2] else 1, bool(light))
        return int(t.value)

    def frame_stats_result(self, ticket, block=True):
        """collect a request (m355_frame_stats_result) -> dict: planes = one dict per plane of the frame (hist: 256 ints, min, max, sum, sum_sq), box =
        (x0, y0, x1, y1) or None, n_active, light = None or a dict (hist, min, max, sum); None while it has not finished (block=False); raises M355Error
        for an unknown / collected ticket and behind a rejected decode"""
        out = Stats()
        rc = self.L.lib.m355_frame_stats_result(self.h, ticket, 1 if block else 0, ctypes.byref(out))
        if rc == 6 and not block:                               # M355_ERR_BUSY
            return None
        if rc:
            text = self.L.error()
            if rc == 3:                                         # M355_ERR_INVALID: collected without a value, or no such request
                self._stats_reqs.pop(ticket, None)
            raise M355Error(rc, text)
        n, light = self._stats_reqs.pop(ticket)
        return stats_dict(out, n, light)

    # ---- SSIM against another picture on the device (m355_frame_ssim_async) ----
    def frame_ssim_async(self, f, ref_frame=None, ref_planes=None, rect=None, planes=0, maps=None, host=False, pad=None):
        """enqueue the SSIM of frame f (rect = (x0, y0, width, height) in luma samples, None: the whole frame; planes: bit p = measure plane p, 0: all)
        against frame `ref_frame` or `ref_planes` (as frame_measure_async).  maps: None, or per plane None / (device pointer, pitch in bytes) for the
        map of q.  Nothing is waited for behind the enqueue -> ticket for frame_ssim_result, which frees the reference's buffers"""
        desc = SsimDesc(ref_frame=-1 if ref_frame is None else ref_frame, planes=planes)
        if rect is not None:
            desc.x0, desc.y0, desc.width, desc.height = rect
        if ref_planes is not None and not (isinstance(ref_planes, tuple) and ref_planes[:1] == ("measure_reference",)):
            ref_planes = self.measure_reference(ref_planes, host, pad)
        _, bufs, pitches, host = ref_planes or (None, [], [], False)
        for k, (p, pitch) in enumerate(zip(bufs, pitches)):
            desc.ref[k] = p; desc.pitch[k] = pitch
        for k, m in enumerate(maps or []):
            if m is not None:
                desc.map[k] = m[0]; desc.map_pitch[k] = m[1]
        t = ctypes.c_ulonglong(0)
        rc = self.L.lib.m355_frame_ssim_async(self.h, f, ctypes.byref(desc), ctypes.byref(t))
        if rc:
            text = self.L.error()
            self._measure_free(bufs, host)
            raise M355Error(rc, text)
        self._ssim_reqs[t.value] = (bufs, host)
        return int(t.value)

    def frame_ssim_result(self, ticket, block=True):
        """collect a request (m355_frame_ssim_result) -> one dict per plane (always three): sum_q, n, min_q, ssim — all 0 for a plane that was not
        measured; None while it has not finished (block=False); raises M355Error for an unknown / collected ticket and behind a rejected decode"""
        out = Ssim()
        rc = self.L.lib.m355_frame_ssim_result(self.h, ticket, 1 if block else 0, ctypes.byref(out))
        if rc == 6 and not block:                               # M355_ERR_BUSY
            return None
        if rc:
            text = self.L.error()
            if rc == 3:                                         # M355_ERR_INVALID: collected without a value (behind a rejected decode), or no such request
                self._measure_free(*self._ssim_reqs.pop(ticket, ([], False)))
            raise M355Error(rc, text)
        self._measure_free(*self._ssim_reqs.pop(ticket))        # (collected: nothing reads the buffers any more)
        return [dict(sum_q=int(out.sum_q[c]), n=int(out.n[c]), min_q=int(out.min_q[c]), ssim=float(out.ssim[c])) for c in range(3)]

    # ---- how the picture was coded (m355_picture_maps_async) ----
    def picture_maps_async(self, handle, log2_unit, maps=tuple(range(N_MAPS)), host=False, pad=20, misalign=0):
        """enqueue the side maps `maps` (MAP_* indices) of the lists of picture `handle` (a resident picture, or PICTURE_LAST) at units of
        1 << log2_unit samples.  Every destination is a buffer of its own holding DEVICE_FILL, its pitch `pad` bytes (rounded up to whole elements) larger than the row, with one
        guard row in front and one behind, and starts `misalign` ELEMENTS behind the buffer's (256-byte aligned) start.  Nothing is waited for ->
        ticket for picture_maps_result, which frees the buffers"""
        w, h = self._pic_size[handle]
        uw, uh = (w + (1 << log2_unit) - 1) >> log2_unit, (h + (1 << log2_unit) - 1) >> log2_unit
        desc = MapsDesc(log2_unit=log2_unit)
        bufs = [None] * N_MAPS
        try:
            for m in maps:
                es = MAP_ELEM_BYTES[m]
                row = uw * es
                pitch = row + -(-pad // es) * es                 # (a pitch is a multiple of the element: 20 bytes become 24 for MAP_MV)
                ofs = pitch + misalign * es                      # one guard row, then the misalignment
                nbytes = ofs + (uh + 1) * pitch
                p = self._buffer(nbytes, host)
                bufs[m] = (p, ofs, pitch, uh, row, nbytes)
                desc.dst[m] = p + ofs; desc.pitch[m] = pitch
            t = ctypes.c_ulonglong(0)
            self.L.check(self.L.lib.m355_picture_maps_async(self.h, handle, ctypes.byref(desc), ctypes.byref(t)))
        except Exception:
            for b in bufs:
                if b is not None:
                    self._buffer_free(b[0], host)
            raise
        self._maps_reqs[t.value] = (bufs, (uw, uh), host)
        return int(t.value)

    def picture_maps_result(self, ticket, block=True):
        """collect a request (m355_picture_maps_result) -> (maps, info, guards_intact): maps = {map index: numpy array (units_h, units_w), MV and
        REF (units_h, units_w, 4)}, info = the m355_maps_info as a dict, guards_intact = every byte of the buffers outside the rows still holds
        DEVICE_FILL; None while it has not finished (block=False); raises M355Error for an unknown / collected ticket"""
        out = MapsInfo()
        rc = self.L.lib.m355_picture_maps_result(self.h, ticket, 1 if block else 0, ctypes.byref(out))
        if rc == 6 and not block:                               # M355_ERR_BUSY
            return None
        bufs, (uw, uh), host = self._maps_reqs.pop(ticket, ([], (0, 0), False))
        if rc:
            text = self.L.error()
            for b in bufs:
                if b is not None:
                    self._buffer_free(b[0], host)
            raise M355Error(rc, text)
        maps, intact = {}, True
        for m, b in enumerate(bufs):
            if b is None:
                continue
            p, ofs, pitch, rows, row, nbytes = b
            if host:
                raw = np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_uint8)), (nbytes,)).copy()
            else:
                raw = self.device_read(p, nbytes)
            self._buffer_free(p, host)
            body = raw[ofs:ofs + rows * pitch].reshape(rows, pitch)
            a = np.ascontiguousarray(body[:, :row]).view(MAP_DTYPES[m])
            maps[m] = a.reshape(uh, uw, 4) if MAP_PER_UNIT[m] == 4 else a.reshape(uh, uw)
            inside = np.zeros(nbytes, bool)
            inside[ofs:ofs + rows * pitch].reshape(rows, pitch)[:, :row] = True
            intact = intact and bool((raw[~inside] == DEVICE_FILL).all())
        return maps, maps_info_dict(out), intact

    def picture_maps_order(self, ticket, stream):
        """the consumer's stream (a hipStream_t as an integer) waits for the request (m355_picture_maps_order)"""
        self.L.check(self.L.lib.m355_picture_maps_order(self.h, ticket, stream))

    # ---- MS-SSIM against another picture on the device (m355_frame_msssim_async) ----
    def frame_msssim_async(self, f, ref_frame=None, ref_planes=None, rect=None, planes=0, levels=MSSSIM_LEVELS, host=False, pad=None):
        """enqueue the multi-scale SSIM of frame f on `levels` levels (rect, planes, ref_frame / ref_planes, host, pad as frame_ssim_async).  Nothing is
        waited for behind the enqueue -> ticket for frame_msssim_result, which frees the reference's buffers"""
        desc = MsssimDesc(ref_frame=-1 if ref_frame is None else ref_frame, planes=planes, levels=levels)
        if rect is not None:
            desc.x0, desc.y0, desc.width, desc.height = rect
        if ref_planes is not None and not (isinstance(ref_planes, tuple) and ref_planes[:1] == ("measure_reference",)):
            ref_planes = self.measure_reference(ref_planes, host, pad)
        _, bufs, pitches, host = ref_planes or (None, [], [], False)
        for k, (p, pitch) in enumerate(zip(bufs, pitches)):
            desc.ref[k] = p; desc.pitch[k] = pitch
        t = ctypes.c_ulonglong(0)
        rc = self.L.lib.m355_frame_msssim_async(self.h, f, ctypes.byref(desc), ctypes.byref(t))
        if rc:
            text = self.L.error()
            self._measure_free(bufs, host)
            raise M355Error(rc, text)
        self._msssim_reqs[t.value] = (bufs, host)
        return int(t.value)

    def frame_msssim_result(self, ticket, block=True):
        """collect a request (m355_frame_msssim_result) -> one dict per plane (always three): sum_q, sum_cs and n as lists over the five levels (0 at the
        levels that were not asked for and for a plane that was not measured) and msssim; None while it has not finished (block=False); raises
        M355Error for an unknown / collected ticket and behind a rejected decode"""
        out = Msssim()
        rc = self.L.lib.m355_frame_msssim_result(self.h, ticket, 1 if block else 0, ctypes.byref(out))
        if rc == 6 and not block:                               # M355_ERR_BUSY
            return None
        if rc:
            text = self.L.error()
            if rc == 3:                                         # M355_ERR_INVALID: collected without a value (behind a rejected decode), or no such request
                self._measure_free(*self._msssim_reqs.pop(ticket, ([], False)))
            raise M355Error(rc, text)
        self._measure_free(*self._msssim_reqs.pop(ticket))      # (collected: nothing reads the buffers any more)
        return msssim_list(out)

    # ---- pictures ----
    def submit(self, pic):
        c, keep = pic.to_c()
        self.L.check(self.L.lib.m355_submit_picture(self.h, ctypes.addressof(c)))
        self._pic_size[PICTURE_LAST] = (int(pic.pp["width"][0]), int(pic.pp["height"][0]))
        del keep

    def submit_in_place(self, src_pic, slack=1.0, fill_threads=16, refill=True, state=None):
        """The in-place path: m355_arena_begin (capacities = the picture's counts x slack) -> the lists are written into the
        pinned arena by libm355synth's m355_synth_fill_arena (standing in for recorder threads) -> m355_submit_picture on
        those pointers (no host copy inside the library).  refill=False re-submits what the arena still holds from an
        earlier call with the same capacities (three arenas rotate): the library's own share of the work alone.
        `state` caches the marshalled source picture between calls."""
        from . import synth
        state = state if state is not None else {}
        if "src" not in state:
            src, state["keep"] = src_pic.to_c()
            caps = ArenaCaps()
            for n in ("n_slices", "n_ctbs", "n_cus", "n_tus", "n_pbs", "n_wts", "n_ibs"):
                setattr(caps, n, int(getattr(src, n)) if n in ("n_slices", "n_ctbs") else int(getattr(src, n) * slack) + 1)
            for b in range(4):
                caps.n_rbs[b] = int(src.rb_count[b] * slack) + 1
            caps.n_coeffs = int(src.n_coeffs * slack) + 1
            caps.n_pcm = int(src.n_pcm * slack) + 1
            caps.scaling = 1 if src.scaling_factors else 0
            state.update(src=src, caps=caps, dst=worklist.CPicture(), lib=synth._lib(), a_src=ctypes.addressof(src))
            state["a_caps"], state["a_dst"] = ctypes.addressof(caps), ctypes.addressof(state["dst"])
        src, dst, lib = state["src"], state["dst"], state["lib"]
        src.dst_frame = src_pic.dst_frame
        rc = self.L.lib.m355_arena_begin(self.h, state["a_caps"], state["a_dst"])
        if rc:
            self.L.check(rc)
        if refill or not state.get("filled", 0) >= 12:      # (every arena of the ring holds the lists)
            lib.m355_synth_fill_arena(state["a_src"], state["a_caps"], state["a_dst"], fill_threads)
            state["filled"] = state.get("filled", 0) + 1
        else:
            lib.m355_synth_fill_arena_header(state["a_src"], state["a_dst"])
        dst.dst_frame = src.dst_frame
        ctypes.memmove(dst.ref_frames, src.ref_frames, 4 * worklist.MAX_REF_FRAMES)
        rc = self.L.lib.m355_submit_picture(self.h, state["a_dst"])
        if rc:
            self.L.check(rc)
        self._pic_size[PICTURE_LAST] = (int(src_pic.pp["width"][0]), int(src_pic.pp["height"][0]))
        return state

    def wait(self):
        self.L.check(self.L.lib.m355_wait(self.h))

    # ---- tile-sharded picture in one call (m355_decode_sharded) ----
    def decode_sharded(self, handle, gather=True):
        self.L.check(self.L.lib.m355_decode_sharded(self.h, handle, 1 if gather else 0))

    def shard_time_exchange(self, handle, which, iters=20):
        ms = ctypes.c_float(0)
        self.L.check(self.L.lib.m355_shard_time_exchange(self.h, handle, which, iters, ctypes.byref(ms)))
        return float(ms.value)

    def shard_set_comm(self, comm_struct):
        """comm_struct: a ctypes m355_comm (kept alive by the caller) or None"""
        self.L.check(self.L.lib.m355_shard_set_comm(self.h, ctypes.addressof(comm_struct) if comm_struct is not None else None))

    def shard_rccl_selftest(self, words=1 << 16):
        """collective: real bytes through ncclSend / ncclRecv / ncclAllGather of this context's communicator, checked on the host"""
        self.L.check(self.L.lib.m355_shard_rccl_selftest(self.h, words))

    def shard_rccl_init(self, unique_id, rank, nranks):
        buf = ctypes.create_string_buffer(bytes(unique_id), 128)
        self.L.check(self.L.lib.m355_shard_rccl_init(self.h, buf, rank, nranks))

    def shard_ipc_init(self, name, rank, nranks):
        """tile sharding across the rank processes of one node without a collective library (m355_shard_ipc_init): `name` = a job-unique string, the same on every rank"""
        self.L.check(self.L.lib.m355_shard_ipc_init(self.h, name.encode(), rank, nranks))

    def shard_ipc_close(self):
        self.L.check(self.L.lib.m355_shard_ipc_close(self.h))

    def last_serial(self):
        """serial of the decode the last submit / decode call enqueued"""
        return int(self.L.lib.m355_last_serial(self.h))

    def decode_status(self, serial):
        """non-blocking: 0 finished and fine, 6 (M355_ERR_BUSY) still running, 3 (M355_ERR_INVALID) lists rejected on the device"""
        return int(self.L.lib.m355_decode_status(self.h, serial))

    def upload(self, pic):
        c, keep = pic.to_c()
        r = self.L.lib.m355_picture_upload(self.h, ctypes.addressof(c))
        del keep
        if r < 0:
            raise M355Error(-r, self.L.error())
        self._pic_size[r] = (int(pic.pp["width"][0]), int(pic.pp["height"][0]))
        return r

    def replace(self, handle, pic):
        """other lists into the arenas of an uploaded picture (m355_picture_replace)"""
        c, keep = pic.to_c()
        self.L.check(self.L.lib.m355_picture_replace(self.h, handle, ctypes.addressof(c)))
        self._pic_size[handle] = (int(pic.pp["width"][0]), int(pic.pp["height"][0]))
        del keep

    def upload_in_place(self, src_pic, handle=-1, slack=1.0, fill_threads=4):
        """The in-place path of a RESIDENT picture (m355_picture_arena_begin -> the lists are written into the handle's pinned arena
        by libm355synth, standing in for recorder threads -> m355_picture_replace copies nothing on the host); what a tile-sharded
        context offers instead of m355_arena_begin.  -> handle"""
        from . import synth
        src, keep = src_pic.to_c()
        caps = ArenaCaps()
        for n in ("n_slices", "n_ctbs", "n_cus", "n_tus", "n_pbs", "n_wts", "n_ibs"):
            setattr(caps, n, int(getattr(src, n)) if n in ("n_slices", "n_ctbs") else int(getattr(src, n) * slack) + 1)
        for b in range(4):
            caps.n_rbs[b] = int(src.rb_count[b] * slack) + 1
        caps.n_coeffs = int(src.n_coeffs * slack) + 1
        caps.n_pcm = int(src.n_pcm * slack) + 1
        caps.scaling = 1 if src.scaling_factors else 0
        dst = worklist.CPicture()
        h = self.L.lib.m355_picture_arena_begin(self.h, handle, ctypes.addressof(caps), ctypes.addressof(src) + worklist.CPicture.pp.offset, ctypes.addressof(dst))
        if h < 0:
            raise M355Error(-h, self.L.error())
        synth._lib().m355_synth_fill_arena(ctypes.addressof(src), ctypes.addressof(caps), ctypes.addressof(dst), fill_threads)
        dst.dst_frame = src.dst_frame
        ctypes.memmove(dst.ref_frames, src.ref_frames, 4 * worklist.MAX_REF_FRAMES)
        self.L.check(self.L.lib.m355_picture_replace(self.h, h, ctypes.addressof(dst)))
        self._pic_size[h] = (int(src_pic.pp["width"][0]), int(src_pic.pp["height"][0]))
        del keep
        return h

    def release(self, handle):
        self.L.check(self.L.lib.m355_picture_release(self.h, handle))

    def decode_resident(self, handle):
        self.L.check(self.L.lib.m355_decode_resident(self.h, handle))

    def decode_batch(self, handles):
        """several independent intra pictures with one intra stage (m355_decode_batch)"""
        a = (ctypes.c_int * len(handles))(*handles)
        self.L.check(self.L.lib.m355_decode_batch(self.h, a, len(handles)))

    def set_stages(self, mask):
        self.L.check(self.L.lib.m355_set_stages(self.h, mask))

    def set_pipeline_depth(self, depth):
        self.L.check(self.L.lib.m355_set_pipeline_depth(self.h, depth))

    def timing_reset(self):
        self.L.check(self.L.lib.m355_timing_reset(self.h))

    def timing_collect(self):
        """-> (n_decodes, avg_total_ms, {stage: avg_ms}) for all decodes since timing_reset()"""
        n = ctypes.c_int()
        total = ctypes.c_float()
        st = (ctypes.c_float * 6)()
        self.L.check(self.L.lib.m355_timing_collect(self.h, ctypes.byref(n), ctypes.byref(total), st))
        return n.value, total.value, dict(zip(["meta", "inter", "residual", "intra", "deblock", "sao"], list(st)))

    def stream(self):
        return self.L.lib.m355_stream(self.h)

    # ---- tile sharding (see libde265_amd/shard.py for the multi-GPU driver) ----
    def shard_set(self, rank, nranks):
        self.L.check(self.L.lib.m355_shard_set(self.h, rank, nranks))

    def shard_xbuf_bytes(self, handle, which):
        n = self.L.lib.m355_shard_xbuf_bytes(self.h, handle, which)
        if n < 0:
            raise M355Error(-n, self.L.error())
        return n

    def decode_phase(self, handle, phase, xbuf_ptr):
        self.L.check(self.L.lib.m355_decode_phase(self.h, handle, phase, xbuf_ptr))


# ---------------------------------------------------------------------------------------------------
# Slot layer: ctypes mirror of `struct m355_acceleration_functions` (= the reference's
# `struct acceleration_functions`, libde265/acceleration.h:29-231), member for member.
# ---------------------------------------------------------------------------------------------------
_vp, _i, _sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_ssize_t
_F = lambda *a: ctypes.CFUNCTYPE(None, *a)  # noqa: E731  (all slots return void)
_WAVG8, _UNW8 = _F(_vp, _sz, _vp, _vp, _sz, _i, _i), _F(_vp, _sz, _vp, _sz, _i, _i)
_W8, _WB8 = _F(_vp, _sz, _vp, _sz, _i, _i, _i, _i, _i), _F(_vp, _sz, _vp, _vp, _sz, _i, _i, _i, _i, _i, _i, _i)
_WAVG16, _UNW16 = _F(_vp, _sz, _vp, _vp, _sz, _i, _i, _i), _F(_vp, _sz, _vp, _sz, _i, _i, _i)
_W16, _WB16 = _F(_vp, _sz, _vp, _sz, _i, _i, _i, _i, _i, _i), _F(_vp, _sz, _vp, _vp, _sz, _i, _i, _i, _i, _i, _i, _i, _i)
_EPEL8 = _F(_vp, _sz, _vp, _sz, _i, _i, _i, _i, _vp)
_EPEL = _F(_vp, _sz, _vp, _sz, _i, _i, _i, _i, _vp, _i)
_QPEL8, _QPEL16 = _F(_vp, _sz, _vp, _sz, _i, _i, _vp), _F(_vp, _sz, _vp, _sz, _i, _i, _vp, _i)
_BYP, _TS8, _TSR8, _TA8 = _F(_vp, _vp, _i), _F(_vp, _vp, _sz), _F(_vp, _vp, _i, _sz), _F(_vp, _vp, _sz)
_TA16, _ROT, _IDCT = _F(_vp, _vp, _sz, _i), _F(_vp, _i), _F(_vp, _vp, _i, _i)
_ADDR, _DEQ = _F(_vp, _sz, _vp, _i, _i), _F(_vp, _vp, _vp, _i, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32)
_DBL, _DBC, _RDP = _F(_vp, _sz, _i, _i, _i, _i, _i, _i, _i), _F(_vp, _sz, _i, _i, _i, _i), _F(_vp, _vp, _i, _i, _i)
_IP, _IA = _F(_vp, _sz, _i, _i, _vp), _F(_vp, _sz, _i, _i, _i, _i, _i, _i, _i, _vp)
_FWD = _F(_vp, _vp, _sz)


class AccelerationFunctions(ctypes.Structure):
    _fields_ = [
        ("put_weighted_pred_avg_8", _WAVG8), ("put_unweighted_pred_8", _UNW8), ("put_weighted_pred_8", _W8),
        ("put_weighted_bipred_8", _WB8),
        ("put_weighted_pred_avg_16", _WAVG16), ("put_unweighted_pred_16", _UNW16), ("put_weighted_pred_16", _W16),
        ("put_weighted_bipred_16", _WB16),
        ("put_hevc_epel_8", _EPEL8), ("put_hevc_epel_h_8", _EPEL), ("put_hevc_epel_v_8", _EPEL), ("put_hevc_epel_hv_8", _EPEL),
        ("put_hevc_qpel_8", (_QPEL8 * 4) * 4),
        ("put_hevc_epel_16", _EPEL), ("put_hevc_epel_h_16", _EPEL), ("put_hevc_epel_v_16", _EPEL), ("put_hevc_epel_hv_16", _EPEL),
        ("put_hevc_qpel_16", (_QPEL16 * 4) * 4),
        ("transform_bypass", _BYP), ("transform_bypass_rdpcm_v", _BYP), ("transform_bypass_rdpcm_h", _BYP),
        ("transform_skip_8", _TS8), ("transform_skip_rdpcm_v_8", _TSR8), ("transform_skip_rdpcm_h_8", _TSR8),
        ("transform_4x4_dst_add_8", _TA8), ("transform_add_8", _TA8 * 4),
        ("transform_skip_16", _TA16), ("transform_4x4_dst_add_16", _TA16), ("transform_add_16", _TA16 * 4),
        ("rotate_coefficients", _ROT), ("transform_idst_4x4", _IDCT), ("transform_idct_4x4", _IDCT),
        ("transform_idct_8x8", _IDCT), ("transform_idct_16x16", _IDCT), ("transform_idct_32x32", _IDCT),
        ("add_residual_8", _ADDR), ("add_residual_16", _ADDR),
        ("dequant_coeff_block", _DEQ),
        ("deblock_luma_8", _DBL), ("deblock_chroma_8", _DBC),
        ("rdpcm_v", _RDP), ("rdpcm_h", _RDP), ("transform_skip_residual", _RDP),
        ("intra_pred_dc_8", _IP), ("intra_pred_dc_16", _IP), ("intra_pred_planar_8", _IP), ("intra_pred_planar_16", _IP),
        ("intra_pred_angular_8", _IA), ("intra_pred_angular_16", _IA),
        ("fwd_transform_4x4_dst_8", _FWD), ("fwd_transform_8", _FWD * 4), ("hadamard_transform_8", _FWD * 4),
    ]


assert ctypes.sizeof(AccelerationFunctions) == 94 * ctypes.sizeof(ctypes.c_void_p)


def acceleration_functions(lib=None):
    """A table filled by init_acceleration_functions_mi355x() (raises when no device is visible)."""
    lib = lib or Library()
    t = AccelerationFunctions()
    rc = lib.lib.init_acceleration_functions_mi355x(ctypes.byref(t))
    if rc != 0:
        raise M355Error(rc, "init_acceleration_functions_mi355x: no HIP device (there is no CPU fallback)")
    return t


class Group:
    """Tile sharding inside one process (m355_group_*): rank r = ctxs[r]; each context uploads its share of the picture
    (shard.shard_picture) and decode() issues every rank's phases with the exchanges as copies between the contexts."""

    def __init__(self, lib, ctxs):
        self.L, self.ctxs = lib, list(ctxs)
        arr = (ctypes.c_void_p * len(self.ctxs))(*[c.h for c in self.ctxs])
        self.h = ctypes.c_void_p()
        lib.check(lib.lib.m355_group_create(arr, len(self.ctxs), ctypes.byref(self.h)))

    def decode(self, handles, gather=True):
        arr = (ctypes.c_int * len(handles))(*handles)
        self.L.check(self.L.lib.m355_group_decode(self.h, arr, 1 if gather else 0))

    def wait(self):
        for c in self.ctxs:
            c.wait()

    def close(self):
        if self.h:
            self.L.lib.m355_group_destroy(self.h)
            self.h = None

