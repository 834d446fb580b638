"""The return codes of malformed m355_glue_export_* calls, as a table: what the glue's own checks reject before it waits for its worker or takes its
lock (a null image, no or too many pictures, pictures of two decoders in one batch, a null out_size / scale / destination array), what it resolves
from the stream (matrix -1, full range -1 and chroma_loc -1 on a stream that signals nothing: accepted), and what only the backend can judge (a
rectangle outside the picture: the backend's code, and the backend's text in m355_last_error()).  The codes are the ones the glue returned before its
six export bodies got one shared prologue.  CPU tier: the backend is the SIMT-interpreter build (M355_LIB), as in test_glue_export_tensor.py."""
import ctypes

from libde265_amd import capi
from test_emu_picture import emu_lib, EMU_SO  # noqa: F401  (fixture)
from test_glue_export import decode
from test_glue_export_siting import bind_sited
from test_glue_export_tensor import Tensor, bind_tensor
from test_glue_live import glue_lib
from test_streams import make_stream

OK, INVALID = 0, 3
W, H = 128, 64


def bind_all(glue):
    vp, i, f3, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_float), ctypes.c_int64
    pi, pv, p64 = ctypes.POINTER(i), ctypes.POINTER(vp), ctypes.POINTER(i64)
    glue.m355_glue_export_image_scaled.argtypes = [vp, i, i, pi, i, pv, p64, vp]
    glue.m355_glue_export_images_tensor_rois.argtypes = [pv, ctypes.POINTER(i * 5), i, i, i, i, i, i, pi, f3, f3, vp, i64, i64, i64, vp]
    bind_tensor(glue)
    return bind_sited(glue)


def test_malformed_glue_exports_return_the_recorded_codes(emu_lib, tmp_path, monkeypatch):  # noqa: F811
    monkeypatch.setenv("M355_LIB", EMU_SO)
    glue = bind_all(glue_lib())
    data = make_stream(tmp_path, W, H, 8, 1, 1, 2, 143, 10, 1, 1, 0, 1)              # 4:2:0, 8 bits, no VUI: the stream signals nothing
    ints, floats = lambda *v: (ctypes.c_int * len(v))(*v), lambda *v: (ctypes.c_float * 3)(*v)
    out, scale, bias = ints(64, 32), floats(1, 1, 1), floats(0, 0, 0)
    PL, NA, PK, U8, F16, NCHW = capi.EXPORT_PLANAR, capi.EXPORT_NATIVE, capi.RGB_PACKED, capi.RGB_U8, capi.TENSOR_F16, capi.TENSOR_NCHW

    def table(ex, img, foreign):
        """img: a picture of this decoder; foreign: one of another live decoder"""
        nbytes = 1 << 16
        buf = ex.L.m355_device_alloc(ex.mctx, nbytes)
        assert buf
        dst, pitch = (ctypes.c_void_p * 3)(buf, buf + 16384, buf + 32768), (ctypes.c_int64 * 3)(512, 512, 512)
        t = Tensor(ex, 2, NCHW, F16, (64, 32))
        pics = lambda *p: (ctypes.c_void_p * len(p))(*p)                              # noqa: E731
        whole = ((ctypes.c_int * 5) * 2)()

        def tensor(imgs, n, out_size=out, sc=scale, bi=bias, matrix=capi.MATRIX_BT709, full=0, loc=0):
            return lambda: glue.m355_glue_export_images_tensor_sited(imgs, n, NCHW, F16, U8, matrix, full, None, out_size, sc, bi, t.p, t.sn, t.sc, t.sh, 0, loc, None)

        def regions(imgs, rr, n, out_size=out, sc=scale, bi=bias):
            return lambda: glue.m355_glue_export_images_tensor_rois(imgs, rr, n, NCHW, F16, U8, capi.MATRIX_BT709, 0, out_size, sc, bi, t.p, t.sn, t.sc, t.sh, None)

        cases = [
            ("image: null image", lambda: glue.m355_glue_export_image(None, PL, NA, None, dst, pitch, None), INVALID),
            ("image: null destination array", lambda: glue.m355_glue_export_image(img, PL, NA, None, None, pitch, None), INVALID),
            ("image: null pitch array", lambda: glue.m355_glue_export_image(img, PL, NA, None, dst, None, None), INVALID),
            ("scaled: log2_scale 4", lambda: glue.m355_glue_export_image_scaled(img, PL, NA, None, 4, dst, pitch, None), INVALID),
            ("scaled: null image", lambda: glue.m355_glue_export_image_scaled(None, PL, NA, None, 1, dst, pitch, None), INVALID),
            ("rgb: null image", lambda: glue.m355_glue_export_image_rgb_sited(None, PK, U8, -1, -1, None, dst, pitch, 0, -1, None), INVALID),
            ("rgb: null destination array", lambda: glue.m355_glue_export_image_rgb_sited(img, PK, U8, -1, -1, None, None, pitch, 0, -1, None), INVALID),
            ("rgb: chroma_loc 4 given explicitly", lambda: glue.m355_glue_export_image_rgb_sited(img, PK, U8, 1, 0, None, dst, pitch, 0, 4, None), INVALID),
            ("resized: null image", lambda: glue.m355_glue_export_image_resized_sited(None, PL, NA, None, out, dst, pitch, 0, 0, None), INVALID),
            ("resized: null out_size", lambda: glue.m355_glue_export_image_resized_sited(img, PL, NA, None, None, dst, pitch, 0, 0, None), INVALID),
            ("resized: null destination array", lambda: glue.m355_glue_export_image_resized_sited(img, PL, NA, None, out, None, pitch, 0, 0, None), INVALID),
            ("resized rgb: null out_size", lambda: glue.m355_glue_export_image_resized_rgb_sited(img, PK, U8, -1, -1, None, None, dst, pitch, 0, -1, None), INVALID),
            ("resized rgb: null pitch array", lambda: glue.m355_glue_export_image_resized_rgb_sited(img, PK, U8, -1, -1, None, out, dst, None, 0, -1, None), INVALID),
            ("tensor: null array of images", tensor(None, 1), INVALID),
            ("tensor: n 0", tensor(pics(img, img), 0), INVALID),
            ("tensor: n 33", tensor(pics(*[img] * 33), 33), INVALID),
            ("tensor: a null image in the batch", tensor(pics(img, None), 2), INVALID),
            ("tensor: images of two decoders", tensor(pics(img, foreign), 2), INVALID),
            ("tensor: images of two decoders, the foreign one first", tensor(pics(foreign, img), 2), INVALID),
            ("tensor: null out_size", tensor(pics(img, img), 2, out_size=None), INVALID),
            ("tensor: null scale", tensor(pics(img, img), 2, sc=None), INVALID),
            ("tensor: null bias", tensor(pics(img, img), 2, bi=None), INVALID),
            ("regions: null rois", regions(pics(img, img), None, 2), INVALID),
            ("regions: n 0", regions(pics(img, img), whole, 0), INVALID),
            ("regions: n 33", regions(pics(*[img] * 33), ((ctypes.c_int * 5) * 33)(), 33), INVALID),
            ("regions: images of two decoders", regions(pics(img, foreign), whole, 2), INVALID),
            ("regions: null out_size", regions(pics(img, img), whole, 2, out_size=None), INVALID),
            # resolved from a stream that signals nothing: BT.709, limited range, type 0
            ("rgb: matrix, range and chroma_loc as signalled", lambda: glue.m355_glue_export_image_rgb_sited(img, PK, U8, -1, -1, None, dst, pitch, 0, -1, None), OK),
            ("resized rgb: matrix, range and chroma_loc as signalled",
             lambda: glue.m355_glue_export_image_resized_rgb_sited(img, PK, U8, -1, -1, None, out, dst, pitch, 0, -1, None), OK),
            ("resized: chroma_loc as signalled", lambda: glue.m355_glue_export_image_resized_sited(img, PL, NA, None, out, dst, pitch, 0, -1, None), OK),
            ("tensor: matrix, range and chroma_loc as signalled", tensor(pics(img, img), 2, matrix=-1, full=-1, loc=-1), OK),
        ]
        for name, call, want in cases:
            assert call() == want, name
        # the backend's to judge: its code, and its text for the calling thread
        assert glue.m355_glue_export_image(img, PL, NA, ints(100, 0, 64, 32), dst, pitch, None) == INVALID
        assert ex.L.m355_last_error().decode() == "m355_frame_export: rectangle 100,0 64x32 leaves the %dx%d frame" % (W, H)
        assert glue.m355_glue_export_image_resized_sited(img, PL, NA, ints(0, 0, 64, 66), out, dst, pitch, 0, 0, None) == INVALID
        assert ex.L.m355_last_error().decode() == "m355_frame_export_resized: rectangle 0,0 64x66 leaves the %dx%d frame" % (W, H)
        assert regions(pics(img, img), ((ctypes.c_int * 5) * 2)((ctypes.c_int * 5)(), (ctypes.c_int * 5)(64, 0, 128, 64, 0)), 2)() == INVALID
        assert ex.L.m355_last_error().decode() == "m355_frames_export_tensor_rois: rectangle 64,0 128x64 leaves the %dx%d frame" % (W, H)
        t.finish()
        ex.L.m355_device_free(ex.mctx, buf)

    ran = []

    def outer(ex, img, j):
        if j != 0:
            return

        def inner(ex2, foreign, k):
            if k == 0:
                table(ex, img, foreign)
                ran.append(1)

        assert decode(glue, emu_lib, inner, data=data)[0] == 2

    assert decode(glue, emu_lib, outer, data=data)[0] == 2
    assert ran == [1]
    assert glue.m355_glue_cpu_pixel_calls() == 0, "the decoder called into its CPU pixel table"
