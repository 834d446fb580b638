"""Shared by the m355_frame_export_rgb tests (SIMT-interpreter build, GPU and glue): the restatement of include/de265_mi355x.h in Python integers /
numpy int64 — the coefficients, the one chroma reconstruction filter, the matrix — applied to the planes m355_frame_download returns, and the drivers
that check exports against it.  Every comparison of pixels is exact, the untouched padding of the destination rows included."""
import numpy as np

from export_util import FORMATS, assert_export, chroma_grid_rect, decode_into_frame  # noqa: F401
from synth_util import assert_planes_equal, make_case
from libde265_amd import capi, worklist

M355_ERR_INVALID = 3   # (capi.ERRORS)
LAYOUTS = (capi.RGB_PACKED, capi.RGB_PLANAR)
SAMPLES = (capi.RGB_U8, capi.RGB_U16)
MATRICES = (capi.MATRIX_BT601, capi.MATRIX_BT709, capi.MATRIX_BT2020)
KR_KB = {capi.MATRIX_BT601: (2990, 1140), capi.MATRIX_BT709: (2126, 722), capi.MATRIX_BT2020: (2627, 593)}
# the rectangle of the format matrix: its source starts off a vector boundary
MATRIX_RECT = (2, 2, 48, 16)
# (matrix, full_range) of the format matrix
MATRIX_CONVERSIONS = ((capi.MATRIX_BT709, 0), (capi.MATRIX_BT2020, 1))


def format_id(cfg):
    return "bd%d_%d_cf%d" % (cfg["bit_depth"], cfg.get("bit_depth_chroma", cfg["bit_depth"]), cfg.get("chroma_format", 1))


def rdiv(a, b):
    return (2 * a + b) // (2 * b)


def coefficients(matrix, full_range, bdy, bdc, samples):
    """m355_rgb_coefficients in Python integers (+ ys, cs, M and the K's, which the float64 definition needs)"""
    kr, kb = KR_KB[matrix]
    kg = 10000 - kr - kb
    D = 16 if samples == capi.RGB_U16 else 8
    M, F = (1 << D) - 1, 29 - D
    if full_range:
        y0, ys, cs = 0, (1 << bdy) - 1, (1 << bdc) - 1
    else:
        y0, ys, cs = 16 << (bdy - 8), 219 << (bdy - 8), 224 << (bdc - 8)
    return dict(F=F, y0=y0, c0=1 << (bdc - 1),
                cy=rdiv(M << F, ys),
                crv=rdiv(2 * (10000 - kr) * (M << F), 10000 * cs),
                cgu=rdiv(2 * kb * (10000 - kb) * (M << F), 10000 * kg * cs),
                cgv=rdiv(2 * kr * (10000 - kr) * (M << F), 10000 * kg * cs),
                cbu=rdiv(2 * (10000 - kb) * (M << F), 10000 * cs),
                M=M, ys=ys, cs=cs, kr=kr, kb=kb, kg=kg)


COEFF_NAMES = ("F", "y0", "c0", "cy", "crv", "cgu", "cgv", "cbu")


def chroma_at_luma(C, cf, W, H, edge="clamp"):
    """the FRAME's chroma plane C brought to the W x H luma positions by the one filter of the header -> int64 (H, W).
    edge: "clamp" is the definition; "wrap" (indices modulo the plane) and "replicate" (the nearest sample, no filter) exist for the tests that
    show that the filter and its clamps are under test"""
    C = C.astype(np.int64)
    CH, CW = C.shape
    fix = (lambda a, n: np.clip(a, 0, n - 1)) if edge != "wrap" else (lambda a, n: a % n)
    X, Y = np.arange(W), np.arange(H)
    if cf == 3:
        return C[:H, :W].copy()
    i = X >> 1
    if edge == "replicate":
        return C[(Y >> 1) if cf == 1 else Y][:, i]
    i1 = fix(i + 1, CW)
    if cf == 2:
        T, r, s = C, 1, 1
    else:
        j = Y >> 1
        jn = fix(np.where(Y & 1, j + 1, j - 1), CH)
        T, r, s = 3 * C[j] + C[jn], 2, 2                       # (H, CW)
    even = (T[:, i] + (r if cf == 1 else 0)) >> (s if cf == 1 else 0)
    odd = (T[:, i] + T[:, i1] + (4 if cf == 1 else 1)) >> (3 if cf == 1 else 1)
    return np.where(X & 1, odd, even)


def yuv_at_luma(planes, cf, edge="clamp"):
    """-> Y, Cb', Cr' as int64 (H, W) arrays; a monochrome frame has no chroma: None, None"""
    Yp = planes[0].astype(np.int64)
    H, W = Yp.shape
    if cf == 0:
        return Yp, None, None
    return Yp, chroma_at_luma(planes[1], cf, W, H, edge), chroma_at_luma(planes[2], cf, W, H, edge)


def matrix_rgb(Yp, Cb, Cr, k):
    """the integer matrix on samples at the luma positions -> R, G, B as int64"""
    F, H = k["F"], 1 << (k["F"] - 1)
    y = Yp - k["y0"]
    u = Cb - k["c0"] if Cb is not None else np.zeros_like(y)
    v = Cr - k["c0"] if Cr is not None else np.zeros_like(y)
    sums = (k["cy"] * y + k["crv"] * v + H, k["cy"] * y - k["cgu"] * u - k["cgv"] * v + H, k["cy"] * y + k["cbu"] * u + H)
    for s in sums:
        assert np.abs(s).max() < (1 << 31), "a sum leaves the signed 32-bit range"
    return [np.clip(s >> F, 0, k["M"]) for s in sums]


def float_rgb(Yp, Cb, Cr, k):
    """the definition the integers approximate: the BT matrix in float64, clipped to 0 .. M, not rounded"""
    y = (Yp - k["y0"]) / k["ys"]
    u = (Cb - k["c0"]) / k["cs"]
    v = (Cr - k["c0"]) / k["cs"]
    kr, kb, kg = k["kr"] / 10000.0, k["kb"] / 10000.0, k["kg"] / 10000.0
    r = y + 2 * (1 - kr) * v
    g = y - 2 * kb * (1 - kb) / kg * u - 2 * kr * (1 - kr) / kg * v
    b = y + 2 * (1 - kb) * u
    return [np.clip(c * k["M"], 0, k["M"]) for c in (r, g, b)]


def shape_rgb(rgb, layout, samples, rect=None):
    dt = np.uint16 if samples == capi.RGB_U16 else np.uint8
    if rect is not None:
        x0, y0, w, h = rect
        rgb = [c[y0:y0 + h, x0:x0 + w] for c in rgb]
    rgb = [np.ascontiguousarray(c.astype(dt)) for c in rgb]
    if layout == capi.RGB_PACKED:
        return [np.ascontiguousarray(np.stack(rgb, axis=-1).reshape(rgb[0].shape[0], -1))]
    return rgb


def expected_rgb(planes, cf, bdl, bdc, layout, samples, matrix, full_range, rect=None, edge="clamp"):
    """what m355_frame_export_rgb delivers, from the planes m355_frame_download returns: the whole frame is converted and the rectangle cut from it"""
    k = coefficients(matrix, full_range, bdl, bdc if cf else bdl, samples)
    return shape_rgb(matrix_rgb(*yuv_at_luma(planes, cf, edge), k), layout, samples, rect)


def check_rgb(ctx, frame, planes, geom, layout, samples, matrix, full_range, rect=None, host=False, what=""):
    cf, bdl, bdc = geom
    got, raws = ctx.frame_export_finish(ctx.frame_export_rgb(frame, layout, samples, matrix, full_range, rect, host=host), raw=True)
    assert_export(got, raws, expected_rgb(planes, cf, bdl, bdc, layout, samples, matrix, full_range, rect),
                  "%s layout %d samples %d matrix %d full %d rect %s" % (what, layout, samples, matrix, full_range, rect))


def check_all(ctx, frame, planes, geom, rects, conversions, what=""):
    """every layout x sample type x conversion x rectangle of one frame"""
    for rect in rects:
        r = None if rect is None else chroma_grid_rect(rect, geom[0])
        for layout in LAYOUTS:
            for samples in SAMPLES:
                for matrix, full in conversions:
                    check_rgb(ctx, frame, planes, geom, layout, samples, matrix, full, r, what=what)


def check_format_matrix_rgb(ctx, o, cfg, rects, conversions=MATRIX_CONVERSIONS):
    frame, planes, geom, frames = decode_into_frame(ctx, o, cfg)
    try:
        check_all(ctx, frame, planes, geom, rects, conversions, what=format_id(cfg))
    finally:
        for f in frames:
            ctx.frame_destroy(f)


ALL_CONVERSIONS = tuple((m, r) for m in MATRICES for r in (0, 1))


def value_cases(bd):
    """4:4:4 frames of 128x32 -> [(name, planes)]: a ramp over the whole sample range on Y against reversed ramps on Cb and Cr, and the eight
    combinations of the extreme values, one per block of 16 columns"""
    dt = np.uint8 if bd <= 8 else np.uint16
    top = (1 << bd) - 1
    ramp = (np.arange(128 * 32, dtype=np.uint64) * top // (128 * 32 - 1)).astype(dt).reshape(32, 128)
    assert int(ramp.max()) == top and int(ramp.min()) == 0
    ext = [np.zeros((32, 128), dt) for _ in range(3)]
    for combo in range(8):
        for c in range(3):
            ext[c][:, 16 * combo:16 * combo + 16] = top if (combo >> c) & 1 else 0
    return [("ramp", [ramp, ramp[::-1, ::-1].copy(), ramp[::-1].copy()]), ("extremes", ext)]


def check_values(ctx, bd):
    """every matrix, range, sample type and layout on the value cases; the expected outputs of each conversion must hold 0, M and interior values
    on every channel, else the clips at both ends are not exercised"""
    frame = ctx.frame_create(128, 32, 3, bd, bd)
    try:
        cases = value_cases(bd)
        for matrix, full in ALL_CONVERSIONS:
            for samples in SAMPLES:
                want = [expected_rgb(planes, 3, bd, bd, capi.RGB_PLANAR, samples, matrix, full) for _, planes in cases]
                M = 65535 if samples == capi.RGB_U16 else 255
                for c in range(3):
                    seen = np.concatenate([w[c].ravel() for w in want])
                    assert (seen == 0).any() and (seen == M).any() and ((seen > 0) & (seen < M)).any(), \
                        "channel %d of matrix %d full %d samples %d does not reach both clips and the interior" % (c, matrix, full, samples)
        for name, planes in cases:
            ctx.frame_upload(frame, planes)
            check_all(ctx, frame, planes, (3, bd, bd), [None], ALL_CONVERSIONS, what="%s %d bit" % (name, bd))
    finally:
        ctx.frame_destroy(frame)


def chroma_case(cf, bd, seed, w=32, h=16):
    """a frame with constant luma and chroma that shows what the reconstruction filter does: pseudo-random samples and one impulse per plane corner"""
    dt = np.uint8 if bd <= 8 else np.uint16
    rng = np.random.default_rng(seed)
    (_, _), (cw, ch), _ = worklist.plane_dims(w, h, cf)
    planes = [np.full((h, w), 1 << (bd - 1), dt)]
    for c in range(2):
        p = rng.integers(1 << (bd - 2), 3 << (bd - 2), size=(ch, cw)).astype(dt)
        for y, x, val in ((0, 0, 0), (0, cw - 1, (1 << bd) - 1), (ch - 1, 0, (1 << bd) - 1), (ch - 1, cw - 1, 0)):
            p[y, x] = val if c == 0 else (1 << bd) - 1 - val
        planes.append(p)
    return planes


def check_gate_rgb(ctx, layout=capi.RGB_PACKED, samples=capi.RGB_U8, matrix=capi.MATRIX_BT709, full=0):
    """export_util.check_gate for the RGB export: behind a decode whose lists the device rejected it writes nothing, behind an accepted decode of
    the same lists it does"""
    cfg = dict(width=128, height=64, bit_depth=8, seed=7501, intra_pct=30)
    pic, refs = make_case(**cfg)
    pp = pic.pp[0]
    handles = []
    for planes in refs:
        f = ctx.frame_create_for(pp)
        ctx.frame_upload(f, planes)
        handles.append(f)
    dst = ctx.frame_create_for(pp)
    ctx.frame_fill(dst, 77, 99)
    tokens, serials = [], []
    for corrupt in (False, True):
        p = make_case(**cfg)[0]
        p.ref_frames = [handles[i] if i < len(handles) else -1 for i in range(worklist.MAX_REF_FRAMES)]
        p.dst_frame = dst
        if corrupt:
            arr = p.ibs.copy(); arr["mode"][len(arr) // 2] = 77; p.ibs = arr
        ctx.submit_in_place(p, fill_threads=1)
        serials.append(ctx.last_serial())
        tokens.append(ctx.frame_export_rgb(dst, layout, samples, matrix, full))
    good, bad = [ctx.frame_export_finish(t, raw=True) for t in tokens]
    assert ctx.decode_status(serials[0]) == 0 and ctx.decode_status(serials[1]) == M355_ERR_INVALID
    with_planes = ctx.frame_download(dst)           # (the rejected decode left the accepted picture in the frame)
    assert_export(good[0], good[1], expected_rgb(with_planes, 1, 8, 8, layout, samples, matrix, full), "behind the accepted decode")
    for raw in bad[1]:
        assert np.all(raw == capi.DEVICE_FILL), "an RGB export behind a rejected decode wrote to its destination"
    ctx.wait()
    for f in handles + [dst]:
        ctx.frame_destroy(f)


def check_hazard_rgb(ctx, depth, layout=capi.RGB_PACKED, samples=capi.RGB_U8, matrix=capi.MATRIX_BT709, full=0):
    """export_util.check_hazard for the RGB export: four 128x64 10-bit pictures decoded alternately into a pool of two frames, each exported right
    behind its decode into a buffer of its own, no host wait in between; every export must deliver what the export of the same picture decoded alone
    delivers.  (On the GPU with several pictures in flight this sees a decode that does not wait for the RGB export of its frame's previous picture;
    the SIMT interpreter finishes every launch before the next call and checks the bookkeeping's results only.)"""
    from libde265_amd import synth
    ctx.set_pipeline_depth(depth)
    try:
        cfg = dict(width=128, height=64, bit_depth=10, seed=5, n_refs=1)
        pics = [synth.picture(**dict(cfg, seed=5 + j)) for j in range(4)]
        pp = pics[0].pp[0]
        r0 = ctx.frame_create_for(pp)
        ctx.frame_upload(r0, synth.ref_planes(5, 128, 64, 1, 10))
        pool = [ctx.frame_create_for(pp) for _ in range(2)]
        rect = (2, 2, 122, 58)
        handles, tokens = [], []
        for j, pic in enumerate(pics):
            pic.ref_frames = [r0] + [-1] * (worklist.MAX_REF_FRAMES - 1)
            pic.dst_frame = pool[j % 2]
            handles.append(ctx.upload(pic))
            ctx.decode_resident(handles[-1])
            tokens.append(ctx.frame_export_rgb(pool[j % 2], layout, samples, matrix, full, rect))
        got = [ctx.frame_export_finish(t, raw=True) for t in tokens]
        ctx.wait()
        for j in range(4):
            ctx.decode_resident(handles[j])
            ctx.wait()
            planes = ctx.frame_download(pool[j % 2])
            alone = ctx.frame_export_finish(ctx.frame_export_rgb(pool[j % 2], layout, samples, matrix, full, rect))
            assert_planes_equal(alone, expected_rgb(planes, 1, 10, 10, layout, samples, matrix, full, rect), "picture %d alone" % j)
            assert_export(got[j][0], got[j][1], alone, "picture %d, depth %d" % (j, depth))
        for j in (0, 1):
            assert not np.array_equal(got[j][0][0], got[j + 2][0][0]), "the pictures that share a frame must differ for this test to see a hazard"
        for h in handles:
            ctx.release(h)
        for f in pool + [r0]:
            ctx.frame_destroy(f)
    finally:
        ctx.set_pipeline_depth(1)
