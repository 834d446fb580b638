/* resize_taps.h — one row of the resize filters of m355_frame_export_resized (include/de265_mi355x.h states the definitions: the triangle, and behind it
 * the cubic filter of the _filtered entry points), ONE definition for the host's m355_resize_taps / m355_resize_taps_filtered (runtime.hip) and the
 * device's resize kernels (k_export_resized.hip, k_export_resized_rgb.hip), which derive the rows a workgroup needs in their
 * prologue: there are no host-built tables.  The results are those of 64-bit integer arithmetic, so every build makes the same coefficients.
 * Plain C++ apart from the qualifier: a program without any HIP header can call it. */
#ifndef M355_RESIZE_TAPS_H
#define M355_RESIZE_TAPS_H
#include <stdint.h>
#include "de265_mi355x.h"
#ifdef __HIPCC__
#define M355_RT_FN __host__ __device__ inline
#else
#define M355_RT_FN inline
#endif

/* floor(a / b), b > 0, |a / b| < 2^51: the double quotient is an estimate within 1 of it, which the integer comparisons then make exact — on a GPU a
   64-bit integer division is a hundred instructions, and a workgroup's prologue makes up to 34 per lane */
M355_RT_FN int64_t m355_rt_floor_div(int64_t a, int64_t b)
{
  int64_t q = (int64_t)((double)a / (double)b);
  while (q * b > a) q--;
  while ((q + 1) * b <= a) q++;
  return q;
}
/* the same with 1 / b at hand (a row of the filter divides by one N throughout) */
M355_RT_FN int64_t m355_rt_floor_div_by(int64_t a, int64_t b, double inv_b)
{
  int64_t q = (int64_t)((double)a * inv_b);
  while (q * b > a) q--;
  while ((q + 1) * b <= a) q++;
  return q;
}
/* the ratio limit of either axis: at most 8x down or 8x up, which bounds a row at M355_RESIZE_MAX_TAPS coefficients */
M355_RT_FN bool m355_resize_ratio_ok(int64_t sn, int64_t dn) { return sn >= 1 && dn >= 1 && sn <= 8 * dn && dn <= 8 * sn; }
/* no row of the axis has more coefficients than this (the integers strictly inside an interval of the length 2 max(sn, dn) / dn) */
M355_RT_FN int m355_resize_max_taps(int64_t sn, int64_t dn)
{
  const int64_t t = (2 * (sn > dn ? sn : dn) + dn - 1) / dn;
  return (int)(t < M355_RESIZE_MAX_TAPS ? t : M355_RESIZE_MAX_TAPS);
}

/* Row i of the axis that maps sn source samples to dn output samples (the caller has checked m355_resize_ratio_ok and 0 <= i < dn): the triangle
 * of half width M = 2 max(sn, dn) around C on the grid of 2 dn units per source sample, normalised to 1 << 14 through the prefix sums (every
 * coefficient >= 0, their sum exactly 1 << 14), source indices clamped to [0, sn - 1] and coefficients that meet there added.
 * -> the number of coefficients n (1..16); *first = the source index of coeff[0]; coeff[j * stride], j < 16, are written (0 behind the n-th). */
M355_RT_FN int m355_resize_row(int64_t sn, int64_t dn, int cosited, int64_t i, int32_t* first, int32_t* coeff, int stride)
{
  const int64_t M = 2 * (sn > dn ? sn : dn), D = 2 * dn;
  const int64_t C = cosited ? 2 * i * sn : (2 * i + 1) * sn - dn;
  const int64_t lo = m355_rt_floor_div(C - M, D) + 1, hi = -m355_rt_floor_div(-(C + M), D) - 1;   /* C - M < D k < C + M */
  int64_t N = 0;
  for (int64_t k = lo; k <= hi; k++) { const int64_t d = D * k - C; N += M - (d < 0 ? -d : d); }
  const int64_t f0 = lo < 0 ? 0 : (lo > sn - 1 ? sn - 1 : lo), f1 = hi < 0 ? 0 : (hi > sn - 1 ? sn - 1 : hi);
  for (int j = 0; j < M355_RESIZE_MAX_TAPS; j++) coeff[j * stride] = 0;
  const double inv = 1.0 / (double)(2 * N);                 /* rdiv(a, N) = floor((2a + N) / 2N) */
  int64_t P = 0, before = 0;
  for (int64_t k = lo; k <= hi; k++) {
    const int64_t d = D * k - C;
    P += M - (d < 0 ? -d : d);
    const int64_t upto = k == hi ? (int64_t)1 << 14 : m355_rt_floor_div_by(2 * (P << 14) + N, 2 * N, inv);
    const int64_t kk = k < 0 ? 0 : (k > sn - 1 ? sn - 1 : k);
    coeff[(kk - f0) * stride] += (int32_t)(upto - before);
    before = upto;
  }
  *first = (int32_t)f0;
  return (int)(f1 - f0 + 1);
}

/* The cubic filter (M355_FILTER_CUBIC): Catmull-Rom, Keys' kernel with a = -1/2, widened by the downscale ratio like the triangle.  n(d) = 2 M^3 w(d / M)
 * for the distance d < 2 M of a source sample from C: 3 d^3 - 5 M d^2 + 2 M^3 up to M, -d^3 + 5 M d^2 - 8 M^2 d + 4 M^3 beyond (negative there).
 * M <= 2^15 and d < 2^16, so every term is below 2^51 and a row's sum N below 2^49. */
M355_RT_FN int64_t m355_rt_cubic_n(int64_t d, int64_t M)
{
  return d <= M ? (3 * d - 5 * M) * d * d + 2 * M * M * M : ((5 * M - d) * d - 8 * M * M) * d + 4 * M * M * M;
}
/* the limits of an axis under `filter`: the triangle's, or for the cubic filter at most 4x down and 8x up — which bounds a row at M355_RESIZE_MAX_TAPS
   coefficients — and at most M355_RESIZE_CUBIC_MAX_N samples on either side (the row's sums stay inside 64 bits) */
M355_RT_FN bool m355_resize_ratio_ok_filtered(int filter, int64_t sn, int64_t dn)
{
  if (filter == M355_FILTER_TRIANGLE) return m355_resize_ratio_ok(sn, dn);
  return filter == M355_FILTER_CUBIC && sn >= 1 && dn >= 1 && sn <= 4 * dn && dn <= 8 * sn && sn <= M355_RESIZE_CUBIC_MAX_N && dn <= M355_RESIZE_CUBIC_MAX_N;
}
/* no row of the axis has more coefficients than this (cubic: the integers strictly inside an interval of the length 4 max(sn, dn) / dn) */
M355_RT_FN int m355_resize_max_taps_filtered(int filter, int64_t sn, int64_t dn)
{
  if (filter == M355_FILTER_TRIANGLE) return m355_resize_max_taps(sn, dn);
  const int64_t t = (4 * (sn > dn ? sn : dn) + dn - 1) / dn;
  return (int)(t < M355_RESIZE_MAX_TAPS ? t : M355_RESIZE_MAX_TAPS);
}

/* Row i of the axis under the cubic filter (the caller has checked m355_resize_ratio_ok_filtered and 0 <= i < dn): m355_resize_row with n(d) above
 * for the triangle and the support |D k - C| < 2 M.  The coefficients sum to exactly 1 << 14 and may be negative; a coefficient of 0 inside the support
 * is kept (out == source: {0, 1 << 14, 0}).  N has up to 48 bits, so rdiv(P << 14, N) is taken in two steps of 7 bits: with P << 7 = q1 N + r1,
 * floor((2 (P << 14) + N) / 2N) = (q1 << 7) + floor(((r1 << 8) + N) / 2N), every operand below 2^57 and both quotients below 2^9. */
M355_RT_FN int m355_resize_row_cubic(int64_t sn, int64_t dn, int cosited, int64_t i, int32_t* first, int32_t* coeff, int stride)
{
  const int64_t M = 2 * (sn > dn ? sn : dn), D = 2 * dn;
  const int64_t C = cosited ? 2 * i * sn : (2 * i + 1) * sn - dn;
  const int64_t lo = m355_rt_floor_div(C - 2 * M, D) + 1, hi = -m355_rt_floor_div(-(C + 2 * M), D) - 1;   /* C - 2M < D k < C + 2M */
  int64_t N = 0;
  for (int64_t k = lo; k <= hi; k++) { const int64_t d = D * k - C; N += m355_rt_cubic_n(d < 0 ? -d : d, M); }
  const int64_t f0 = lo < 0 ? 0 : (lo > sn - 1 ? sn - 1 : lo), f1 = hi < 0 ? 0 : (hi > sn - 1 ? sn - 1 : hi);
  for (int j = 0; j < M355_RESIZE_MAX_TAPS; j++) coeff[j * stride] = 0;
  const double inv1 = 1.0 / (double)N, inv2 = 1.0 / (double)(2 * N);
  int64_t P = 0, before = 0;
  for (int64_t k = lo; k <= hi; k++) {
    const int64_t d = D * k - C;
    P += m355_rt_cubic_n(d < 0 ? -d : d, M);
    int64_t upto = (int64_t)1 << 14;
    if (k != hi) {
      const int64_t q1 = m355_rt_floor_div_by(P * 128, N, inv1), r1 = P * 128 - q1 * N;
      upto = q1 * 128 + m355_rt_floor_div_by(r1 * 256 + N, 2 * N, inv2);
    }
    const int64_t kk = k < 0 ? 0 : (k > sn - 1 ? sn - 1 : k);
    coeff[(kk - f0) * stride] += (int32_t)(upto - before);
    before = upto;
  }
  *first = (int32_t)f0;
  return (int)(f1 - f0 + 1);
}
/* the row under `filter` (M355_FILTER_TRIANGLE or M355_FILTER_CUBIC; the caller has checked it) */
M355_RT_FN int m355_resize_row_filtered(int filter, int64_t sn, int64_t dn, int cosited, int64_t i, int32_t* first, int32_t* coeff, int stride)
{
  return filter == M355_FILTER_CUBIC ? m355_resize_row_cubic(sn, dn, cosited, i, first, coeff, stride) : m355_resize_row(sn, dn, cosited, i, first, coeff, stride);
}
#endif
