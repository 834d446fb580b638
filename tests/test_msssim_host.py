"""The host-only statement of the MS-SSIM definition (m355_ssim_window_cs: csrc/ssim_window.h; m355_msssim_combine) against the numpy restatement of
tests/msssim_util.py, that restatement against MS-SSIM as Wang, Simoncelli and Bovik define it, in float64 with unrounded 2 x 2 means and the same
window weights, and the layout of the two structures against the ctypes mirrors.  No device."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import msssim_util as mu
import ssim_util as su
from test_emu_picture import emu_lib  # noqa: F401  (fixture)
from libde265_amd import capi

INVALID = 3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_window_cs_equals_the_restatement(emu_lib):  # noqa: F811
    """sums of real windows (consistent with one another) and sums drawn independently (which no window gives: cs leaves -1..1 and qc is clamped at
    both ends)"""
    rng = np.random.default_rng(6100)
    for bd in (8, 10, 12, 16):
        peak = (1 << bd) - 1
        a = rng.integers(0, peak + 1, (24, 40)).astype(np.uint16)
        b = np.clip(a.astype(np.int64) + rng.integers(-peak // 8 - 1, peak // 8 + 2, a.shape), 0, peak).astype(np.uint16)
        for x, y in ((a, b), (a, (peak - a).astype(np.uint16))):
            sums = [s.ravel() for s in su.window_sums(x, y)]
            want = mu.point_cs(sums, bd)
            for k in range(0, len(want), 7):
                assert emu_lib.ssim_window_cs([s[k] for s in sums], bd) == int(want[k]), "window %d at %d bits" % (k, bd)
        assert want.max() < 0, "the inverted plane's windows are negative"
        free = [rng.integers(0, (peak << 28) + 1, 300, dtype=np.uint64) for _ in range(2)] + [rng.integers(0, ((peak * peak) << 28) + 1, 300, dtype=np.uint64) for _ in range(3)]
        want = mu.point_cs(free, bd)
        assert want.min() == -mu.ONE and want.max() == mu.ONE, "the clamp is not reached at both ends"
        for k in range(300):
            assert emu_lib.ssim_window_cs([s[k] for s in free], bd) == int(want[k]), "independent sums %d at %d bits" % (k, bd)
    q = ctypes.c_int32(0)
    sums = (ctypes.c_uint64 * 5)()
    for bd in (0, 17, -1):
        assert emu_lib.lib.m355_ssim_window_cs(sums, bd, ctypes.byref(q)) == INVALID
    assert emu_lib.lib.m355_ssim_window_cs(None, 8, ctypes.byref(q)) == INVALID and emu_lib.lib.m355_ssim_window_cs(sums, 8, None) == INVALID


def test_window_cs_is_one_where_both_windows_are_flat(emu_lib):  # noqa: F811
    for bd in (8, 16):
        peak = (1 << bd) - 1
        m, s = peak << 28, (peak * peak) << 28
        for sums in ([m, m, s, s, s], [m, 0, s, 0, 0], [0, m, 0, s, 0], [0] * 5):
            assert emu_lib.ssim_window_cs(sums, bd) == mu.ONE


def ulps(got, want):
    return abs(got - want) / math.ulp(want)


def test_combine_against_math_pow(emu_lib):  # noqa: F811
    """the product in level order from 1.0 of pow(max(m, 0), w): 8 ulp against math.pow (five pow results of at most 1 ulp each, four multiplications);
    exact at 0.0 and 1.0"""
    rng = np.random.default_rng(6200)
    for _ in range(200):
        m = [float(v) for v in rng.uniform(0.05, 1.0, 5)]
        assert ulps(emu_lib.msssim_combine(m), mu.combine(m)) <= 8
        assert abs(emu_lib.msssim_combine(m) - mu.combine(m)) <= 2.0 ** -49 * mu.combine(m)
        for levels in (1, 2, 3, 4, 5):
            w = [float(v) for v in rng.uniform(0.0, 1.5, levels)]
            assert ulps(emu_lib.msssim_combine(m[:levels], w), mu.combine(m[:levels], w)) <= 8
    assert emu_lib.msssim_combine([1.0] * 5) == 1.0
    assert emu_lib.msssim_combine([0.9, 0.9, -0.25, 0.9, 0.9]) == 0.0, "a level whose mean is negative"
    assert emu_lib.msssim_combine([0.9, 0.0, 0.9, 0.9, 0.9]) == 0.0
    assert emu_lib.msssim_combine([-0.0, 1.0, 1.0, 1.0, 1.0]) == 0.0
    assert emu_lib.msssim_combine([0.5], [1.0]) == 0.5 and emu_lib.msssim_combine([0.5, 0.25], [1.0, 0.0]) == 0.5
    assert capi.MSSSIM_WEIGHTS == mu.WANG and abs(sum(mu.WANG) - 1.0001) < 1e-12, "Wang's weights as published, not normalised"


def test_combine_rejections(emu_lib):  # noqa: F811
    L = emu_lib.lib
    five = (ctypes.c_double * 5)(0.5, 0.5, 0.5, 0.5, 0.5)
    out = ctypes.c_double(-1.0)
    assert L.m355_msssim_combine(None, 5, None, ctypes.byref(out)) == INVALID and L.m355_msssim_combine(five, 5, None, None) == INVALID
    for levels in (0, -1, 6, 1 << 20):
        assert L.m355_msssim_combine(five, levels, five, ctypes.byref(out)) == INVALID, "levels %d" % levels
    for levels in (1, 2, 3, 4):
        assert L.m355_msssim_combine(five, levels, None, ctypes.byref(out)) == INVALID, "the built-in weights with %d levels" % levels
        assert L.m355_msssim_combine(five, levels, five, ctypes.byref(out)) == 0
    for bad in (float("nan"), float("inf"), -0.5):
        w = (ctypes.c_double * 5)(0.2, 0.2, bad, 0.2, 0.2)
        assert L.m355_msssim_combine(five, 5, w, ctypes.byref(out)) == INVALID, "weight %r" % bad
        assert L.m355_msssim_combine(five, 2, w, ctypes.byref(out)) == 0, "a weight behind the levels is not looked at"
    assert L.m355_msssim_combine((ctypes.c_double * 5)(0.5, float("nan"), 0.5, 0.5, 0.5), 5, None, ctypes.byref(out)) == INVALID
    assert L.m355_msssim_combine(five, 5, None, ctypes.byref(out)) == 0 and out.value == mu.combine([0.5] * 5)


# ---- the restatement against float64 MS-SSIM ----
def float_msssim(a, b, bd, levels=5):
    """MS-SSIM in float64: every level the UNROUNDED 2 x 2 mean of the level above (trailing column / row dropped), valid 11 x 11 windows with the
    14-bit weights as fractions, the mean of cs on levels 0 .. L - 2 and of the full SSIM on the last, Wang's exponents"""
    g = np.array(su.WEIGHTS) / 16384.0
    peak = float((1 << bd) - 1)
    c1, c2 = (0.01 * peak) ** 2, (0.03 * peak) ** 2
    a, b = a.astype(np.float64), b.astype(np.float64)
    m = []
    for j in range(levels):
        ph, pw = a.shape

        def blur(f):
            rows = sum(g[k] * f[:, k:k + pw - 10] for k in range(11))
            return sum(g[k] * rows[k:k + ph - 10, :] for k in range(11))

        ma, mb = blur(a), blur(b)
        va, vb, cov = blur(a * a) - ma * ma, blur(b * b) - mb * mb, blur(a * b) - ma * mb
        cs = (2 * cov + c2) / (va + vb + c2)
        m.append(float((cs if j < levels - 1 else cs * (2 * ma * mb + c1) / (ma * ma + mb * mb + c1)).mean()))
        a, b = [(f[:ph & ~1:2, :pw & ~1:2] + f[1:ph & ~1:2, :pw & ~1:2] + f[:ph & ~1:2, 1:pw & ~1:2] + f[1:ph & ~1:2, 1:pw & ~1:2]) / 4.0 for f in (a, b)]
    return m


def noise_pair(w, h, bd, divisor, seed):
    """a plane of noise over the whole range and the same plane with a perturbation of up to +-peak / divisor (test_ssim_host.noise_pair at another size)"""
    rng = np.random.default_rng(seed)
    peak = (1 << bd) - 1
    a = rng.integers(0, peak + 1, (h, w))
    b = np.clip(a + rng.integers(-(peak // divisor), peak // divisor + 1, a.shape), 0, peak)
    dt = np.uint8 if bd <= 8 else np.uint16
    return a.astype(dt), b.astype(dt)


@pytest.mark.parametrize("w,h,bd,bound", [(176, 176, 8, 5.0e-4), (200, 183, 8, 1.1e-3), (176, 177, 16, 3.0e-6)])
def test_the_definition_is_msssim(w, h, bd, bound):
    """|integer-defined MS-SSIM - float64 MS-SSIM| on seeded noise perturbed by up to an eighth of the range (MS-SSIM 0.975).  Level 0 agrees to the
    Q30 rounding of the points; what separates the two above it is the rounding of the levels' samples to integers, which the float model does not
    do: it adds a quantisation noise of variance 1 / 12 to either side of every level, which enters both variances and not the covariance, and on the
    last level, where a plane of this size has one window or a few, nothing averages it out.  MEASURED with these seeds: 176 x 176 at 8 bits 2.49e-4
    (0.975340 against 0.975589), 200 x 183 at 8 bits 5.07e-4 (0.974193 against 0.974700), 176 x 177 at 16 bits 1.41e-6 (0.975289 against 0.975287);
    each bound is twice the measured distance, rounded up to two digits.  With a perturbation of a sixteenth / a quarter of the range the same sizes
    give 4.7e-4 / 4.1e-4, 5.2e-4 / 4.9e-4 and 3.1e-7 / 2.6e-6 (not bounded).  The float model is the thing measured against."""
    a, b = noise_pair(w, h, bd, 8, seed=6300 + w + bd)
    r = mu.msssim_plane(a, b, bd, 5)
    fm = float_msssim(a, b, bd)
    f = mu.combine(fm)
    print("%d x %d at %d bits: integer-defined %.6f, float64 %.6f, distance %.3g; level means %s against %s" % (
        w, h, bd, r["msssim"], f, abs(r["msssim"] - f), ["%.6f" % v for v in mu.means(r, 5)], ["%.6f" % v for v in fm]))
    assert abs(mu.means(r, 5)[0] - fm[0]) <= 2.0 ** -31 + 1e-11, "level 0 is the plane itself: only the points' rounding"
    assert 0.9 < r["msssim"] < 0.999
    assert abs(r["msssim"] - f) <= bound


def test_an_inverted_picture_is_exactly_zero():
    a, _ = noise_pair(176, 176, 8, 8, seed=6400)
    r = mu.msssim_plane(a, (255 - a).astype(np.uint8), 8, 5)
    m = mu.means(r, 5)
    print("inverted: level means", ["%.4f" % v for v in m])
    assert min(m[:4]) < 0 and r["msssim"] == 0.0


def test_levels_round_the_exact_sum_once():
    """level j is one rounding of the f x f sum, which is not the rounding of the level above: a plane where the two differ"""
    a = np.zeros((4, 4), np.uint8)
    a[0, 0] = a[2, 2] = 2                                         # 2 x 2 sums 2: level 1 = (2 + 2) >> 2 = 1 at (0, 0) and (1, 1); twice rounded: (2 + 2) >> 2 = 1
    assert mu.level(a, 1).tolist() == [[1, 0], [0, 1]]
    assert mu.level(a, 2).tolist() == [[0]]                       # (4 + 8) >> 4 = 0; rounding level 1 again would give (2 + 2) >> 2 = 1
    assert mu.level(mu.level(a, 1), 1).tolist() == [[1]]
    b = np.arange(35 * 37, dtype=np.uint16).reshape(35, 37)
    assert mu.level(b, 3).shape == (4, 4) and mu.level(b, 3)[3, 3] == (int(b[24:32, 24:32].sum()) + 32) >> 6


# ---- the ABI ----
STRUCTS = {"m355_msssim_desc": capi.MsssimDesc, "m355_msssim": capi.Msssim}


def test_structs_match_the_ctypes_mirrors(tmp_path):
    names = [(s, f) for s, mirror in STRUCTS.items() for f, _ in mirror._fields_]
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"de265_mi355x.h\"\nint main(void){\n"
    src += "".join("printf(\"%%zu\\n\", sizeof(%s));\n" % s for s in STRUCTS)
    src += "".join("printf(\"%%zu\\n\", offsetof(%s, %s));\n" % (s, f) for s, f in names)
    src += "printf(\"%d\\n%d\\n\", M355_MSSSIM_REQUESTS, M355_MSSSIM_LEVELS);\nreturn 0;}\n"
    exe = str(tmp_path / "msssim_layout")
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(ROOT, "include"), "-o", exe], input=src, text=True, check=True)
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got[:len(STRUCTS)] == [ctypes.sizeof(m) for m in STRUCTS.values()]
    for (s, f), off in zip(names, got[len(STRUCTS):]):
        assert off == getattr(STRUCTS[s], f).offset, "%s.%s" % (s, f)
    assert got[-2:] == [capi.MSSSIM_REQUESTS, capi.MSSSIM_LEVELS]
    assert ctypes.sizeof(capi.MsssimDesc) == 104 and ctypes.sizeof(capi.Msssim) == 384
