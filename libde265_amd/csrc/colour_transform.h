/*
 * colour_transform.h — the ONE definition of the colour transform stage of the composed exports (include/de265_mi355x.h, m355_colour_tables):
 * 1-D table -> 3x3 matrix -> 1-D table on the clipped 16-bit full-scale R'G'B' of a pixel, in integers.  Compiled three times, as resize_taps.h and
 * tensor_element.h are: into k_export_resized_rgb.hip (device, through k_colour_dev.h, which supplies the table reads), into the SIMT-interpreter
 * build of that kernel (SIMT_EMU, plain C++) and into m355_colour_pixel (runtime.hip, host), which the tests run against a restatement.
 *   1. linearise   k = v >> 6, f = v & 63:  L = (lut_in[k] (64 - f) + lut_in[k + 1] f + 32) >> 6            <= 2^30 + 32: 32 bits; L <= ONE
 *   2. matrix      P_c = clip(0, ONE, (m[c][0] L_r + m[c][1] L_g + m[c][2] L_b + (1 << 13)) >> 14)           42 bits and a sign, >> arithmetic
 *                  computed in 32 bits: L = Lh 4096 + Ll, Sh = sum m Lh, Sl = sum m Ll (each below 3 * 65535 * 4096 < 2^30 in magnitude), and
 *                  (Sh 4096 + Sl + 8192) >> 14 = (Sh + ((Sl + 8192) >> 12)) >> 2 exactly (floor of a floor); every product is 24 x 24 bits
 *   3. encode      P < 64: idx = P, fr = 0; else e = floor(log2 P), n = P << (24 - e), idx = 64 (e - 5) + ((n >> 18) & 63), fr = (n >> 10) & 255
 *                  o = (lut_out[idx] (256 - fr) + lut_out[min(idx + 1, 1216)] fr + 128) >> 8
 *   4. deliver     M355_RGB_U16: o; M355_RGB_U8: (2 o + 257) / 514 = o / 257 rounded
 * A TONE OBJECT (m355_colour_tone beside the tables; m355_colour_pixel_tone) puts step 2b between 2 and 3: ONE gain for the pixel's three channels
 *   2b. gain       n = max(P_r, P_g, P_b) (M355_NORM_MAXRGB) or the matrix row of step 2 with `weights` over P (M355_NORM_LUMA: its clip keeps n in
 *                  0 .. ONE); (idx, fr) of step 3 from n; g = (gain[idx] (256 - fr) + gain[min(idx + 1, 1216)] fr + 128) >> 8;
 *                  P'_c = (P_c g + (1 << 23)) >> 24, and steps 3 and 4 run on P'
 *                  computed as 32 x 32 -> 64-bit multiply-adds (the kernel: v_mad_u64_u32, or v_mul_lo_u32 / v_mul_hi_u32 and an add with carry): gain
 *                  entries are at most 2^24 and the two weights sum to 256, so the interpolation's sum is at most 2^32 + 128 — one bit more than 32, which
 *                  is why it is not taken in 32 bits as step 3's is — and g <= 2^24 again; P_c <= 2^24, so P_c g + 2^23 <= 2^48 + 2^23 < 2^64 and
 *                  P'_c <= (2^48 + 2^23) >> 24 = 2^24 = ONE.  Nothing is truncated before the one shift of each line, so both are the statements above
 *                  bit for bit.
 * M355_CT_MAD24(a, b, c) = a * b + c for operands that fit 24 bits signed, and M355_CT_FLOG2(x) = floor(log2 x) for x > 0, may be defined by the
 * including file (the kernel: v_mad_i32_i24 and v_ffbh_u32, k_resize_dev.h); the functions are static, so that a file with its own pair and one without
 * link into one library.
 */
#ifndef M355_COLOUR_TRANSFORM_H
#define M355_COLOUR_TRANSFORM_H

#include <stdint.h>
#include "de265_mi355x.h"

#ifdef __HIPCC__
#define M355_CT_FN __host__ __device__ static inline
#else
#define M355_CT_FN static inline
#endif
#ifndef M355_CT_MAD24
#define M355_CT_MAD24(a, b, c) ((int32_t)((uint32_t)(a) * (uint32_t)(b) + (uint32_t)(c)))
#endif
#ifndef M355_CT_FLOG2
#define M355_CT_FLOG2(x) (31 - __builtin_clz(x))
#endif

#define M355_COLOUR_OUT_LAST (M355_COLOUR_OUT_KNOTS - 1)     /* 1216: the knot of P = ONE */

/* step 1 for one channel: a = lut_in[v >> 6], b = lut_in[(v >> 6) + 1], f = v & 63 */
M355_CT_FN uint32_t m355_ct_linear(uint32_t a, uint32_t b, uint32_t f) { return (a * (64u - f) + b * f + 32u) >> 6; }

/* step 2 for one output channel: a row of the matrix (Q14, |entry| <= 65535) over the three linear values (<= ONE) */
M355_CT_FN uint32_t m355_ct_matrix_row(int32_t m0, int32_t m1, int32_t m2, uint32_t lr, uint32_t lg, uint32_t lb)
{
  const int32_t sh = M355_CT_MAD24(m2, (int32_t)(lb >> 12), M355_CT_MAD24(m1, (int32_t)(lg >> 12), M355_CT_MAD24(m0, (int32_t)(lr >> 12), 0)));
  const int32_t sl = M355_CT_MAD24(m2, (int32_t)(lb & 4095u), M355_CT_MAD24(m1, (int32_t)(lg & 4095u), M355_CT_MAD24(m0, (int32_t)(lr & 4095u), 8192)));
  const int32_t p = (sh + (sl >> 12)) >> 2;
  return (uint32_t)(p < 0 ? 0 : (p > M355_COLOUR_ONE ? M355_COLOUR_ONE : p));
}

/* step 3, the index: P in 0 .. ONE -> knot idx (0 .. 1216) and the fraction fr (0 .. 255) towards knot idx + 1 */
M355_CT_FN void m355_ct_out_index(uint32_t p, uint32_t* idx, uint32_t* fr)
{
  const int e = M355_CT_FLOG2(p | 64u);                       /* (6 below 64, where the result is not used) */
  const uint32_t n = p << (24 - e);
  const bool big = p >= 64u;
  *idx = big ? 64u * (uint32_t)(e - 5) + ((n >> 18) & 63u) : p;
  *fr = big ? (n >> 10) & 255u : 0u;
}
/* what knot idx stands for */
M355_CT_FN uint32_t m355_ct_out_knot(uint32_t idx) { return idx < 64u ? idx : (64u + (idx & 63u)) << ((idx >> 6) - 1u); }

/* step 3, the interpolation: lo = lut_out[idx], hi = lut_out[min(idx + 1, 1216)] */
M355_CT_FN uint32_t m355_ct_encode(uint32_t lo, uint32_t hi, uint32_t fr) { return (lo * (256u - fr) + hi * fr + 128u) >> 8; }

/* step 2b of a tone object, the interpolation: lo = gain[idx], hi = gain[min(idx + 1, 1216)], both <= GAIN_ONE: 33 bits before the shift */
M355_CT_FN uint32_t m355_ct_gain(uint32_t lo, uint32_t hi, uint32_t fr) { return (uint32_t)(((uint64_t)lo * (256u - fr) + (uint64_t)hi * fr + 128u) >> 8); }
/* step 2b, the gain on one channel: p <= ONE, g <= GAIN_ONE: 49 bits before the shift, at most ONE behind it */
M355_CT_FN uint32_t m355_ct_apply(uint32_t p, uint32_t g) { return (uint32_t)(((uint64_t)p * g + (1u << 23)) >> 24); }
/* step 2b, what the gain is looked up at */
M355_CT_FN uint32_t m355_ct_norm(int32_t norm, int32_t w0, int32_t w1, int32_t w2, uint32_t pr, uint32_t pg, uint32_t pb)
{
  if (norm == M355_NORM_LUMA) return m355_ct_matrix_row(w0, w1, w2, pr, pg, pb);
  const uint32_t a = pr > pg ? pr : pg;
  return a > pb ? a : pb;
}

/* step 4 */
M355_CT_FN uint32_t m355_ct_deliver(uint32_t o, bool u8) { return u8 ? (2u * o + 257u) / 514u : o; }

/* step 1 for one channel from tables in addressable memory, v = 0 .. 65535: what m355_colour_linear is */
M355_CT_FN uint32_t m355_ct_linear_of(const m355_colour_tables* t, uint32_t v)
{
  const uint32_t k = v >> 6;
  return m355_ct_linear(t->lut_in[k], t->lut_in[k + 1], v & 63u);
}

/* the whole stage for one pixel from tables in addressable memory: what m355_colour_pixel is */
M355_CT_FN void m355_ct_pixel(const m355_colour_tables* t, const uint32_t rgb16[3], int samples, uint32_t out[3])
{
  uint32_t l[3];
  for (int c = 0; c < 3; c++) l[c] = m355_ct_linear_of(t, rgb16[c] > 65535u ? 65535u : rgb16[c]);
  for (int c = 0; c < 3; c++) {
    const uint32_t p = m355_ct_matrix_row(t->matrix[3 * c], t->matrix[3 * c + 1], t->matrix[3 * c + 2], l[0], l[1], l[2]);
    uint32_t idx, fr;
    m355_ct_out_index(p, &idx, &fr);
    const uint32_t o = m355_ct_encode(t->lut_out[idx], t->lut_out[idx < M355_COLOUR_OUT_LAST ? idx + 1 : M355_COLOUR_OUT_LAST], fr);
    out[c] = m355_ct_deliver(o, samples == M355_RGB_U8);
  }
}

/* the whole stage of a tone object for one pixel: what m355_colour_pixel_tone is */
M355_CT_FN void m355_ct_pixel_tone(const m355_colour_tables* t, const m355_colour_tone* q, const uint32_t rgb16[3], int samples, uint32_t out[3])
{
  uint32_t l[3], p[3], idx, fr;
  for (int c = 0; c < 3; c++) l[c] = m355_ct_linear_of(t, rgb16[c] > 65535u ? 65535u : rgb16[c]);
  for (int c = 0; c < 3; c++) p[c] = m355_ct_matrix_row(t->matrix[3 * c], t->matrix[3 * c + 1], t->matrix[3 * c + 2], l[0], l[1], l[2]);
  m355_ct_out_index(m355_ct_norm(q->norm, q->weights[0], q->weights[1], q->weights[2], p[0], p[1], p[2]), &idx, &fr);
  const uint32_t g = m355_ct_gain(q->gain[idx], q->gain[idx < M355_COLOUR_OUT_LAST ? idx + 1 : M355_COLOUR_OUT_LAST], fr);
  for (int c = 0; c < 3; c++) {
    m355_ct_out_index(m355_ct_apply(p[c], g), &idx, &fr);
    const uint32_t o = m355_ct_encode(t->lut_out[idx], t->lut_out[idx < M355_COLOUR_OUT_LAST ? idx + 1 : M355_COLOUR_OUT_LAST], fr);
    out[c] = m355_ct_deliver(o, samples == M355_RGB_U8);
  }
}

/* the bounds m355_colour_create checks: 0 = within them */
M355_CT_FN int m355_ct_tables_check(const m355_colour_tables* t)
{
  for (int k = 0; k < M355_COLOUR_IN_KNOTS; k++) if (t->lut_in[k] > (uint32_t)M355_COLOUR_ONE) return 1;
  for (int k = 0; k < 9; k++) if (t->matrix[k] > 65535 || t->matrix[k] < -65535) return 2;
  return t->pad ? 3 : 0;
}
/* the bounds m355_colour_create_tone checks beyond those: 0 = within them */
M355_CT_FN int m355_ct_tone_check(const m355_colour_tone* q)
{
  if (q->norm != M355_NORM_MAXRGB && q->norm != M355_NORM_LUMA) return 1;
  for (int k = 0; k < 3; k++) if (q->weights[k] > 65535 || q->weights[k] < -65535 || (q->norm == M355_NORM_MAXRGB && q->weights[k])) return 2;
  for (int k = 0; k < M355_COLOUR_OUT_KNOTS; k++) if (q->gain[k] > (uint32_t)M355_TONE_GAIN_ONE) return 3;
  return q->reserved[0] || q->reserved[1] || q->reserved[2] ? 4 : 0;
}

#endif
