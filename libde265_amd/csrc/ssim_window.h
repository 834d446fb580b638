/*
 * ssim_window.h — THE DEFINITION of the SSIM this library measures (m355_frame_ssim_async, include/de265_mi355x.h): the 11-tap window's integer
 * weights and the point computed from a window's five sums.  Host and device run this code (k_ssim.hip, runtime_ssim.hip: m355_ssim_window /
 * m355_ssim_weights); tests/ssim_util.py restates it in numpy, bit for bit.
 *
 * WEIGHTS.  exp(-(i - 5)^2 / 4.5), i = 0..10 (a Gaussian with sigma = 1.5), normalised, times 2^14, rounded half up: they sum to exactly 2^14.
 * A window's weight at (dx, dy) is w[dx] * w[dy]; the 121 of them sum to 2^28.
 * SUMS.  Over the window's samples a (the frame) and b (the reference), unsigned 64-bit and exact:
 *   MA = sum w a    MB = sum w b    SAA = sum w a^2    SBB = sum w b^2    SAB = sum w a b        (SAA <= 2^28 * 65535^2 < 2^60)
 * POINT.  In IEEE double, every operation rounded by itself in exactly the order written in m355_ssim_point.
 * m355_ssim_point_cs is the contrast-structure factor of the same point alone, for the levels of m355_frame_msssim_async (k_msssim.hip,
 * runtime_msssim.hip: m355_ssim_window_cs).
 *
 * CONTRACTION IS OFF: a fused multiply-add rounds once where this definition rounds twice.  The pragma below switches it off for the rest of
 * every translation unit that includes this header under clang (hipcc: host and device side); the SIMT-interpreter build (g++, which does not
 * know the pragma) compiles the objects that include it with -ffp-contract=off (Makefile).  Plain operators only: no fma(), no __d*_rn.
 */
#ifndef M355_SSIM_WINDOW_H
#define M355_SSIM_WINDOW_H
#include <math.h>
#include <stdint.h>

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#if defined(__HIPCC__) || defined(SIMT_EMU)
#define M355_SSIM_HD __host__ __device__ static inline
#else
#define M355_SSIM_HD static inline
#endif

#define M355_SSIM_TAPS 11
#define M355_SSIM_WEIGHT_BITS 14
#define M355_SSIM_WEIGHTS {17, 124, 590, 1792, 3490, 4358, 3490, 1792, 590, 124, 17}
#define M355_SSIM_ONE 1073741824    /* 2^30: q of two identical windows */

/* c1 = (K1 peak)^2 and c2 = (K2 peak)^2 on the scale of the sums (2^56 = the square of the windows' total weight), K1 = 0.01, K2 = 0.03 */
static inline double m355_ssim_c1(int bit_depth)
{
  const uint64_t peak = ((uint64_t)1 << bit_depth) - 1;
  return (double)(peak * peak) * 72057594037927936.0 / 10000.0;
}
static inline double m355_ssim_c2(int bit_depth)
{
  const uint64_t peak = ((uint64_t)1 << bit_depth) - 1;
  return (double)(peak * peak * 9) * 72057594037927936.0 / 10000.0;
}

/* the five sums of one window -> q = SSIM of the window in Q30, -2^30 .. 2^30 */
M355_SSIM_HD int32_t m355_ssim_point(uint64_t MA, uint64_t MB, uint64_t SAA, uint64_t SBB, uint64_t SAB, double c1, double c2)
{
  const double k28 = 268435456.0;
  const double fa = (double)MA, fb = (double)MB;
  const double ab = fa * fb, aa = fa * fa, bb = fb * fb;
  const double cov = k28 * (double)SAB - ab, va = k28 * (double)SAA - aa, vb = k28 * (double)SBB - bb;
  const double s = ((2.0 * ab + c1) * (2.0 * cov + c2)) / (((aa + bb) + c1) * ((va + vb) + c2));
  double r = floor(s * 1073741824.0 + 0.5);
  if (r < -1073741824.0) r = -1073741824.0;
  if (r > 1073741824.0) r = 1073741824.0;
  return (int32_t)(int64_t)r;
}

/* the five sums of one window -> qc = the window's contrast-structure term in Q30, -2^30 .. 2^30: the second factor of s above, from the same
   intermediates by the same expressions (m355_frame_msssim_async: every level of MS-SSIM but the last takes this term alone) */
M355_SSIM_HD int32_t m355_ssim_point_cs(uint64_t MA, uint64_t MB, uint64_t SAA, uint64_t SBB, uint64_t SAB, double c1, double c2)
{
  const double k28 = 268435456.0;
  const double fa = (double)MA, fb = (double)MB;
  const double ab = fa * fb, aa = fa * fa, bb = fb * fb;
  const double cov = k28 * (double)SAB - ab, va = k28 * (double)SAA - aa, vb = k28 * (double)SBB - bb;
  const double cs = (2.0 * cov + c2) / ((va + vb) + c2);
  double r = floor(cs * 1073741824.0 + 0.5);
  if (r < -1073741824.0) r = -1073741824.0;
  if (r > 1073741824.0) r = 1073741824.0;
  (void)c1;
  return (int32_t)(int64_t)r;
}

#endif
