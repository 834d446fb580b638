"""The host-only statement of the SSIM definition (m355_ssim_weights, m355_ssim_window: csrc/ssim_window.h) against the numpy restatement of
tests/ssim_util.py, and that restatement against SSIM as Wang et al. define it, in float64 with unquantised Gaussian weights.  No device."""
import numpy as np
import pytest

import ssim_util as su
from test_emu_picture import emu_lib  # noqa: F401  (fixture)
from libde265_amd import capi

INVALID = 3


def test_weights_are_the_table_and_sum_to_2_14(emu_lib):  # noqa: F811
    w = emu_lib.ssim_weights()
    assert w == su.WEIGHTS and sum(w) == 1 << 14 and w == w[::-1]
    g = np.exp(-(np.arange(11) - 5.0) ** 2 / 4.5)
    assert w == [int(v) for v in np.floor(g / g.sum() * 16384.0 + 0.5)]
    assert emu_lib.lib.m355_ssim_weights(None) == INVALID


def test_window_equals_the_restatement_on_random_sums(emu_lib):  # noqa: F811
    """sums of real windows (consistent with one another) and sums drawn independently (which no window gives: s leaves -1..1 and q is clamped)"""
    rng = np.random.default_rng(5100)
    for bd in (8, 10, 12, 16):
        peak = (1 << bd) - 1
        a = rng.integers(0, peak + 1, (24, 40)).astype(np.uint16)
        b = np.clip(a.astype(np.int64) + rng.integers(-peak // 8 - 1, peak // 8 + 2, a.shape), 0, peak).astype(np.uint16)
        sums = [s.ravel() for s in su.window_sums(a, b)]
        want = su.point(sums, bd)
        for k in range(0, len(want), 7):
            assert emu_lib.ssim_window([s[k] for s in sums], bd) == int(want[k]), "window %d at %d bits" % (k, bd)
        free = [rng.integers(0, (peak << 28) + 1, 300, dtype=np.uint64) for _ in range(2)] + [rng.integers(0, ((peak * peak) << 28) + 1, 300, dtype=np.uint64) for _ in range(3)]
        want = su.point(free, bd)
        assert want.min() == -su.ONE and want.max() == su.ONE, "the clamp is not reached"
        for k in range(300):
            assert emu_lib.ssim_window([s[k] for s in free], bd) == int(want[k]), "independent sums %d at %d bits" % (k, bd)


def test_window_at_the_corner_values(emu_lib):  # noqa: F811
    for bd in (8, 10, 16):
        peak = (1 << bd) - 1
        m, s = peak << 28, (peak * peak) << 28                      # the sums of a window of `peak`
        cases = {"peak against peak": [m, m, s, s, s], "peak against zero": [m, 0, s, 0, 0], "zero against peak": [0, m, 0, s, 0], "zero against zero": [0] * 5}
        for what, sums in cases.items():
            want = int(su.point([np.array([v], np.uint64) for v in sums], bd)[0])
            assert emu_lib.ssim_window(sums, bd) == want, "%s at %d bits" % (what, bd)
            assert want == (su.PEAK_AGAINST_ZERO if "against zero" in what and what != "zero against zero" or what == "zero against peak" else su.ONE), what
    assert ((65535 * 65535) << 28) < 1 << 60                        # the 16-bit maxima fit 64 bits with room
    q = capi.ctypes.c_int32(0)
    sums = (capi.ctypes.c_uint64 * 5)()
    for bd in (0, 17, -1):
        assert emu_lib.lib.m355_ssim_window(sums, bd, capi.ctypes.byref(q)) == INVALID
    assert emu_lib.lib.m355_ssim_window(None, 8, capi.ctypes.byref(q)) == INVALID and emu_lib.lib.m355_ssim_window(sums, 8, None) == INVALID


def float_ssim(a, b, bd, g):
    """SSIM of every valid 11 x 11 window as Wang et al. define it, in float64, with the normalised window weights g"""
    a, b = a.astype(np.float64), b.astype(np.float64)
    ph, pw = a.shape

    def blur(f):
        rows = sum(g[k] * f[:, k:k + pw - 10] for k in range(11))
        return sum(g[k] * rows[k:k + ph - 10, :] for k in range(11))

    peak = float((1 << bd) - 1)
    c1, c2 = (0.01 * peak) ** 2, (0.03 * peak) ** 2
    ma, mb = blur(a), blur(b)
    va, vb, cov = blur(a * a) - ma * ma, blur(b * b) - mb * mb, blur(a * b) - ma * mb
    return ((2 * ma * mb + c1) * (2 * cov + c2)) / ((ma * ma + mb * mb + c1) * (va + vb + c2))


GAUSS = np.exp(-(np.arange(11) - 5.0) ** 2 / 4.5) / np.exp(-(np.arange(11) - 5.0) ** 2 / 4.5).sum()


def noise_pair(bd, divisor, seed):
    """a plane of noise over the whole range and the same plane with a perturbation of up to +-peak / divisor"""
    rng = np.random.default_rng(seed)
    peak = (1 << bd) - 1
    a = rng.integers(0, peak + 1, (48, 64))
    return a, np.clip(a + rng.integers(-(peak // divisor), peak // divisor + 1, a.shape), 0, peak)


@pytest.mark.parametrize("bd", [8, 10, 16])
def test_the_definition_is_ssim(bd):
    """Per window |q / 2^30 - float SSIM with unquantised Gaussian weights| <= 1e-5 on seeded noise-plus-perturbation planes (noise over the whole
    range, perturbed by up to a sixteenth of it: SSIM around 0.99).  Measured: 3.4e-6 at 8 bits, 2.7e-6 at 10 and 1.8e-6 at 16 bits; the plane
    means agree to 1.9e-8.  The difference is owed to the 14-bit weights alone — the next test pins that — and grows with the distortion: the same
    noise perturbed by up to a quarter of the range (SSIM 0.89) differs by 2.9e-5 .. 4.0e-5, by up to half of it (SSIM 0.67) by 7.0e-5 .. 8.2e-5
    (printed below, not bounded)."""
    for divisor in (16, 4, 2):
        a, b = noise_pair(bd, divisor, 5200 + bd)
        q = su.point(su.window_sums(a, b), bd) / 2.0 ** 30
        f = float_ssim(a, b, bd, GAUSS)
        diff = np.abs(q - f).max()
        print("bit depth %d, perturbation 1/%d of the range: SSIM %.4f, largest per-window difference %.3g, means differ by %.3g" % (bd, divisor, q.mean(), diff, abs(q.mean() - f.mean())))
        if divisor == 16:
            assert diff <= 1e-5


@pytest.mark.parametrize("bd", [8, 10, 16])
def test_the_difference_is_the_weights_alone(bd):
    """Against float64 SSIM computed with the QUANTISED weights w / 16384 the definition differs by the rounding of q to Q30 and no more, whatever the
    distortion: at most 2^-31 for the rounding, plus 1e-11 for the float evaluation of either side (sums of 121 terms in double: relative 1e-14)."""
    for divisor in (16, 4, 2, 1):
        a, b = noise_pair(bd, divisor, 5300 + bd)
        q = su.point(su.window_sums(a, b), bd) / 2.0 ** 30
        diff = np.abs(q - float_ssim(a, b, bd, np.array(su.WEIGHTS) / 16384.0)).max()
        print("bit depth %d, perturbation 1/%d of the range: largest per-window difference with quantised weights %.3g" % (bd, divisor, diff))
        assert diff <= 2.0 ** -31 + 1e-11
