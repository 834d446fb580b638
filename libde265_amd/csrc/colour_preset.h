/*
 * colour_preset.h — the preset builder behind m355_colour_preset (include/de265_mi355x.h): the tables of colour_transform.h for the common cases, in
 * double arithmetic, host only.  Transfers and primaries are the H.265 code points of Tables E.3 / E.4; 2 (unspecified) counts as 1.
 *   lut_in[k]   E = min(64 k, 65535) / 65535 -> nits by in_transfer, over S = the nits at E = 1, times ONE, rounded, at most ONE
 *   matrix      RGB -> XYZ of in_primaries, then XYZ -> RGB of out_primaries (D65), Q14 rounded; the largest-magnitude entry of a row takes what the
 *               row lacks to 1 << 14; equal primaries: the identity
 *   lut_out[i]  nits = knot(i) / ONE * S, x = nits / white, the tone curve, the inverse of out_transfer, times 65535, rounded
 * Returns 0, or 1 for a descriptor outside the contract.
 * m355_cp_build_tone, behind m355_colour_preset_tone, builds a tone object's tables and gain from the same descriptor (stated at the function).
 */
#ifndef M355_COLOUR_PRESET_H
#define M355_COLOUR_PRESET_H

#include <math.h>
#include <string.h>
#include "colour_transform.h"

static inline int m355_cp_transfer(int t) { return t == 2 || t == 6 || t == 14 || t == 15 ? 1 : t; }   /* (the BT.1886 family) */
static inline bool m355_cp_primaries_ok(int p) { return p == 1 || p == 5 || p == 6 || p == 9; }

/* display light in nits for the non-linear value e of transfer t (1, 8, 13, 16, 18) */
static inline double m355_cp_eotf(int t, double e, double white)
{
  switch (t) {
  case 1: return white * pow(e, 2.4);
  case 13: return white * (e <= 0.04045 ? e / 12.92 : pow((e + 0.055) / 1.055, 2.4));
  case 8: return white * e;
  case 16: {
    const double m1 = 2610.0 / 16384.0, m2 = 2523.0 / 4096.0 * 128.0, c1 = 3424.0 / 4096.0, c2 = 2413.0 / 4096.0 * 32.0, c3 = 2392.0 / 4096.0 * 32.0;
    const double p = pow(e, 1.0 / m2), num = p - c1 > 0.0 ? p - c1 : 0.0;
    return 10000.0 * pow(num / (c2 - c3 * p), 1.0 / m1);
  }
  default: {                                                  /* 18: the inverse HLG OETF, then the OOTF per channel with gamma 1.2 */
    const double a = 0.17883277, b = 1.0 - 4.0 * a, c = 0.5 - a * log(4.0 * a);
    const double s = e <= 0.5 ? e * e / 3.0 : (exp((e - c) / a) + b) / 12.0;
    return 1000.0 * pow(s, 1.2);
  }
  }
}
/* the inverse of out transfer t (1, 8, 13) on y in 0 .. 1 */
static inline double m355_cp_oetf(int t, double y)
{
  if (t == 1) return pow(y, 1.0 / 2.4);
  if (t == 13) return y <= 0.0031308 ? 12.92 * y : 1.055 * pow(y, 1.0 / 2.4) - 0.055;
  return y;
}
static inline void m355_cp_inverse3(const double m[9], double o[9])
{
  const double c0 = m[4] * m[8] - m[5] * m[7], c1 = m[5] * m[6] - m[3] * m[8], c2 = m[3] * m[7] - m[4] * m[6];
  const double det = m[0] * c0 + m[1] * c1 + m[2] * c2;
  o[0] = c0 / det; o[1] = (m[2] * m[7] - m[1] * m[8]) / det; o[2] = (m[1] * m[5] - m[2] * m[4]) / det;
  o[3] = c1 / det; o[4] = (m[0] * m[8] - m[2] * m[6]) / det; o[5] = (m[2] * m[3] - m[0] * m[5]) / det;
  o[6] = c2 / det; o[7] = (m[1] * m[6] - m[0] * m[7]) / det; o[8] = (m[0] * m[4] - m[1] * m[3]) / det;
}
/* RGB -> XYZ of primaries p (xy of Table E.3, white D65) */
static inline void m355_cp_rgb_to_xyz(int p, double o[9])
{
  static const double XY[4][6] = {{0.640, 0.330, 0.300, 0.600, 0.150, 0.060}, {0.640, 0.330, 0.290, 0.600, 0.150, 0.060},
                                  {0.630, 0.340, 0.310, 0.595, 0.155, 0.070}, {0.708, 0.292, 0.170, 0.797, 0.131, 0.046}};
  const double* q = XY[p == 1 ? 0 : (p == 5 ? 1 : (p == 6 ? 2 : 3))];
  const double xw = 0.3127, yw = 0.3290, w[3] = {xw / yw, 1.0, (1.0 - xw - yw) / yw};
  double m[9], inv[9];
  for (int i = 0; i < 3; i++) { m[i] = q[2 * i] / q[2 * i + 1]; m[3 + i] = 1.0; m[6 + i] = (1.0 - q[2 * i] - q[2 * i + 1]) / q[2 * i + 1]; }
  m355_cp_inverse3(m, inv);
  for (int i = 0; i < 3; i++) {
    const double s = inv[3 * i] * w[0] + inv[3 * i + 1] * w[1] + inv[3 * i + 2] * w[2];
    for (int r = 0; r < 3; r++) o[3 * r + i] = m[3 * r + i] * s;
  }
}

static inline int m355_cp_build(const m355_colour_preset_desc* d, m355_colour_tables* out)
{
  if (!d || !out || d->reserved || d->white_nits < 0 || d->peak_nits < 0) return 1;
  const int it = m355_cp_transfer(d->in_transfer), ot = m355_cp_transfer(d->out_transfer);
  const int ip = d->in_primaries == 2 ? 1 : d->in_primaries, op = d->out_primaries == 2 ? 1 : d->out_primaries;
  if ((it != 1 && it != 8 && it != 13 && it != 16 && it != 18) || (ot != 1 && ot != 8 && ot != 13)) return 1;
  if (!m355_cp_primaries_ok(ip) || !m355_cp_primaries_ok(op)) return 1;
  if (d->tone != M355_TONE_CLIP && d->tone != M355_TONE_REINHARD) return 1;
  const double white = d->white_nits ? (double)d->white_nits : 203.0;
  if (d->peak_nits && (double)d->peak_nits < white) return 1;
  const double one = (double)M355_COLOUR_ONE, S = m355_cp_eotf(it, 1.0, white);
  memset(out, 0, sizeof(*out));
  for (int k = 0; k < M355_COLOUR_IN_KNOTS; k++) {
    const double e = (double)(64 * k < 65535 ? 64 * k : 65535) / 65535.0;
    const double v = floor(m355_cp_eotf(it, e, white) / S * one + 0.5);
    out->lut_in[k] = v >= one ? (uint32_t)M355_COLOUR_ONE : (v <= 0.0 ? 0u : (uint32_t)v);
  }
  if (ip == op) { out->matrix[0] = out->matrix[4] = out->matrix[8] = 1 << 14; }
  else {
    double a[9], b[9], binv[9];
    m355_cp_rgb_to_xyz(ip, a);
    m355_cp_rgb_to_xyz(op, b);
    m355_cp_inverse3(b, binv);
    for (int r = 0; r < 3; r++) {
      int32_t sum = 0, big = 0;
      for (int c = 0; c < 3; c++) {
        const double v = binv[3 * r] * a[c] + binv[3 * r + 1] * a[3 + c] + binv[3 * r + 2] * a[6 + c];
        const int32_t q = (int32_t)floor(v * 16384.0 + 0.5);
        out->matrix[3 * r + c] = q; sum += q;
        if ((q < 0 ? -q : q) > (out->matrix[3 * r + big] < 0 ? -out->matrix[3 * r + big] : out->matrix[3 * r + big])) big = c;
      }
      out->matrix[3 * r + big] += (1 << 14) - sum;
    }
  }
  const double peak = d->peak_nits ? (double)d->peak_nits : S, w = peak / white > 1.0 ? peak / white : 1.0;
  for (int i = 0; i < M355_COLOUR_OUT_KNOTS; i++) {
    const double x = (double)m355_ct_out_knot((uint32_t)i) / one * S / white;
    double y = d->tone == M355_TONE_REINHARD ? x * (1.0 + x / (w * w)) / (1.0 + x) : x;
    if (y > 1.0) y = 1.0;
    const double v = floor(m355_cp_oetf(ot, y) * 65535.0 + 0.5);
    out->lut_out[i] = (uint16_t)(v >= 65535.0 ? 65535.0 : (v <= 0.0 ? 0.0 : v));
  }
  return 0;
}

/* the inverse of the ST 2084 EOTF: nits -> the non-linear value */
static inline double m355_cp_pq_inverse(double nits)
{
  const double m1 = 2610.0 / 16384.0, m2 = 2523.0 / 4096.0 * 128.0, c1 = 3424.0 / 4096.0, c2 = 2413.0 / 4096.0 * 32.0, c3 = 2392.0 / 4096.0 * 32.0;
  const double p = pow((nits > 0.0 ? nits : 0.0) / 10000.0, m1);
  return pow((c1 + c2 * p) / (1.0 + c3 * p), m2);
}
/* The preset of a TONE OBJECT behind m355_colour_preset_tone: lut_in and matrix of m355_cp_build, lut_out that of M355_TONE_CLIP, and the curve y(x) of
 * d->tone as the gain min(1, y / x) at the knots of lut_out:
 *   gain[i]     x = knot(i) / ONE * S / white; M355_TONE_CLIP y = min(1, x); M355_TONE_REINHARD as in m355_cp_build; M355_TONE_BT2390 the EETF of BT.2390
 *               in the PQ domain, black 0: E1 = PQ^-1(x white) / PQ^-1(L_w) (at most 1), maxLum = PQ^-1(white) / PQ^-1(L_w), KS = 1.5 maxLum - 0.5,
 *               the Hermite spline above KS, E2 in 0 .. 1, y = PQ(E2 PQ^-1(L_w)) / white; maxLum >= 1: y = x.  floor(min(1, y / x) 2^24 + 0.5); gain[0] = 2^24
 *   weights     M355_NORM_LUMA: the Y row of RGB -> XYZ of out_primaries, Q14 rounded, the largest entry takes what the row lacks to 1 << 14
 * Returns 0, or 1 for what m355_cp_build rejects, an unknown tone or norm, or KS < 0. */
static inline int m355_cp_build_tone(const m355_colour_preset_desc* d, int norm, m355_colour_tables* out, m355_colour_tone* tone)
{
  if (!d || !out || !tone || (norm != M355_NORM_MAXRGB && norm != M355_NORM_LUMA)) return 1;
  if (d->tone != M355_TONE_CLIP && d->tone != M355_TONE_REINHARD && d->tone != M355_TONE_BT2390) return 1;
  m355_colour_preset_desc clip = *d;
  clip.tone = M355_TONE_CLIP;
  if (m355_cp_build(&clip, out)) return 1;
  const double white = d->white_nits ? (double)d->white_nits : 203.0, one = (double)M355_COLOUR_ONE;
  const double S = m355_cp_eotf(m355_cp_transfer(d->in_transfer), 1.0, white), peak = d->peak_nits ? (double)d->peak_nits : S;
  const double w = peak / white > 1.0 ? peak / white : 1.0;
  const double lw = m355_cp_pq_inverse(peak), max_lum = m355_cp_pq_inverse(white) / lw, ks = 1.5 * max_lum - 0.5;
  if (d->tone == M355_TONE_BT2390 && max_lum < 1.0 && ks < 0.0) return 1;
  memset(tone, 0, sizeof(*tone));
  tone->norm = norm;
  if (norm == M355_NORM_LUMA) {
    double m[9];
    int32_t sum = 0, big = 0;
    m355_cp_rgb_to_xyz(d->out_primaries == 2 ? 1 : d->out_primaries, m);
    for (int c = 0; c < 3; c++) {
      tone->weights[c] = (int32_t)floor(m[3 + c] * 16384.0 + 0.5); sum += tone->weights[c];
      if (tone->weights[c] > tone->weights[big]) big = c;
    }
    tone->weights[big] += (1 << 14) - sum;
  }
  tone->gain[0] = (uint32_t)M355_TONE_GAIN_ONE;
  for (int i = 1; i < M355_COLOUR_OUT_KNOTS; i++) {
    const double x = (double)m355_ct_out_knot((uint32_t)i) / one * S / white;
    double y = x;
    if (d->tone == M355_TONE_REINHARD) y = x * (1.0 + x / (w * w)) / (1.0 + x);
    else if (d->tone == M355_TONE_BT2390 && max_lum < 1.0) {
      double e1 = m355_cp_pq_inverse(x * white) / lw;
      if (e1 > 1.0) e1 = 1.0;
      if (e1 > ks) {
        const double t = (e1 - ks) / (1.0 - ks), t2 = t * t, t3 = t2 * t;
        double e2 = (2.0 * t3 - 3.0 * t2 + 1.0) * ks + (t3 - 2.0 * t2 + t) * (1.0 - ks) + (-2.0 * t3 + 3.0 * t2) * max_lum;
        e2 = e2 < 0.0 ? 0.0 : (e2 > 1.0 ? 1.0 : e2);
        y = m355_cp_eotf(16, e2 * lw, white) / white;
      }
    }
    if (y > 1.0) y = 1.0;
    const double g = y / x < 1.0 ? y / x : 1.0;
    tone->gain[i] = (uint32_t)floor(g * (double)M355_TONE_GAIN_ONE + 0.5);
  }
  return 0;
}

#endif
