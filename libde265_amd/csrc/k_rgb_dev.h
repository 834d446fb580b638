/*
 * k_rgb_dev.h — what the kernels that bring a frame's pixels to R'G'B' at the luma positions share: k_export_rgb.hip, which stores them, and
 * k_stats.hip, which measures them (m355_frame_stats_async, light == 1).  One definition, so that "the R'G'B' the export delivers" is the same
 * code in both: the loads of a lane's luma vector and its chroma vectors, the one bilinear chroma reconstruction of the header (chroma sample
 * location type 0, or the type 1..3 of m355_export_opts: a template parameter) and the matrix of m355_rgb_coefficients in signed 32 bits.
 * k_export_rgb.hip's header comment holds the arguments for the vector shapes, the ranges and the reads that stay inside the allocation.
 */
#pragma once
#include "k_common.h"
#include "pixel_pack.h"   /* m355_pp_dword: d_rgb_pixels_lane */

#ifdef SIMT_EMU
static inline int d_mad24(int a, int b, int c) { return (int)((unsigned)a * (unsigned)b + (unsigned)c); }
#else
/* v_mad_i32_i24: a, b within 24 signed bits */
__device__ __forceinline__ int d_mad24(int a, int b, int c) { return (int)((unsigned)__mul24(a, b) + (unsigned)c); }
#endif

/* sample k of a 16-byte vector */
template <int SB> __device__ __forceinline__ int d_rgb_sample(const unsigned* w, int k)
{
  return SB == 1 ? (int)((w[k >> 2] >> (8 * (k & 3))) & 0xFFu) : (int)((w[k >> 1] >> (16 * (k & 1))) & 0xFFFFu);
}

/* the NP chroma samples of one plane at the lane's luma positions, minus c0.  r0 / r1: the vectors of chroma rows j / jn (4:2:0; else r0 only),
   last = CW - 1 - i0 >= 0: the index inside the vector of the plane's last column */
template <int SB, int CF, int LOC>
__device__ __forceinline__ void d_rgb_chroma(const unsigned* r0, const unsigned* r1, int last, int c0, int* out, bool yodd, bool lead)
{
  constexpr int NP = 16 / SB, NC = NP / 2;
  if (CF == 3) {
#pragma unroll
    for (int k = 0; k < NP; k++) out[k] = d_rgb_sample<SB>(r0, k) - c0;
    return;
  }
  if constexpr (LOC != 0) {
    /* chroma sample location types 1..3 (4:2:0 only): the vertical sums T in quarters — MID 3 C[j] + C[jn], TOP 4 C[j] on an even luma row (yodd,
       wave-uniform: a wave is one row) and 2 C[j] + 2 C[j + 1] on an odd one —, then LEFT as type 0, or CENTRE {i: 3, i -+ 1: 1} with one
       rounding, (sum + 8) >> 4, c0 folded into the constant.  CENTRE: the vectors start at column i0 - 1 (lead) or, for the lane at column 0, at
       i0 = 0, where the clamp makes sample 0 its own left neighbour: s[m] is column max(i0 - 1 + m, 0), m = 0 .. NC + 1 <= NP - 1 */
    constexpr bool CENTRE = (LOC & 1) != 0, TOP = (LOC >> 1) != 0;
    constexpr int NT = NC + 1 + (CENTRE ? 1 : 0);
    int t[NT];
    if (TOP && !yodd) {
#pragma unroll
      for (int k = 0; k < NT; k++) t[k] = 4 * d_rgb_sample<SB>(r0, k);
    } else {
#pragma unroll
      for (int k = 0; k < NT; k++) t[k] = TOP ? 2 * (d_rgb_sample<SB>(r0, k) + d_rgb_sample<SB>(r1, k)) : 3 * d_rgb_sample<SB>(r0, k) + d_rgb_sample<SB>(r1, k);
    }
    if (!CENTRE) {
#pragma unroll
      for (int k = 0; k < NC; k++) {
        const int tn = k < last ? t[k + 1] : t[k];
        out[2 * k] = (t[k] + 2 - 4 * c0) >> 2;
        out[2 * k + 1] = (t[k] + tn + 4 - 8 * c0) >> 3;
      }
    } else {
      int s[NT];
#pragma unroll
      for (int m = 0; m < NT; m++) s[m] = lead ? t[m] : t[m ? m - 1 : 0];
#pragma unroll
      for (int k = 0; k < NC; k++) {
        const int tr = k < last ? s[k + 2] : s[k + 1];            /* column min(i + 1, CW - 1) */
        out[2 * k] = (3 * s[k + 1] + s[k] + 8 - 16 * c0) >> 4;
        out[2 * k + 1] = (3 * s[k + 1] + tr + 8 - 16 * c0) >> 4;
      }
    }
    return;
  }
  int t[NC + 1];
#pragma unroll
  for (int k = 0; k <= NC; k++) {
    const int s = d_rgb_sample<SB>(r0, k);
    t[k] = CF == 1 ? 3 * s + d_rgb_sample<SB>(r1, k) : s;
  }
  const int ke = CF == 1 ? 2 - 4 * c0 : -c0, ko = CF == 1 ? 4 - 8 * c0 : 1 - 2 * c0;
#pragma unroll
  for (int k = 0; k < NC; k++) {
    const int tn = k < last ? t[k + 1] : t[k];                /* column min(i + 1, CW - 1) */
    out[2 * k] = CF == 1 ? (t[k] + ke) >> 2 : t[k] + ke;
    out[2 * k + 1] = (t[k] + tn + ko) >> (CF == 1 ? 3 : 1);
  }
}

/* What a lane needs of the frame for the NP = 16 / SB pixels from luma column X0 of luma row Y: its luma vector and, per chroma plane, one 16-byte
   vector from each chroma row the filter reads, all issued before the first use.  `a` holds the FRAME's planes (a.src[3], a.src_pitch[2] in bytes,
   a.cw x a.ch chroma samples).  last / lead / yodd: what d_rgb_chroma takes. */
template <int SB, int CF, int LOC> struct RgbLane {
  unsigned ry[4], rc[2][2][4];
  int last = 0;
  bool lead = false;                                            /* CENTRE: the chroma vectors start one column before i0 */
  bool yodd = false;                                            /* TOP: an odd luma row (wave-uniform: a wave is one row) */
};
template <int SB, int CF, int LOC, class A>
__device__ __forceinline__ void d_rgb_load(const A& a, uint32_t X0, uint32_t Y, RgbLane<SB, CF, LOC>& l)
{
  d_ldg16((const M355_GLOBAL uint8_t*)a.src[0] + (size_t)Y * a.src_pitch[0] + (size_t)X0 * SB, l.ry);
  if constexpr ((LOC >> 1) != 0) l.yodd = (Y & 1u) != 0;
  if (CF != 0) {
    const uint32_t i0 = CF == 3 ? X0 : X0 >> 1;
    uint32_t j = Y, jn = Y;
    if (CF == 1) {
      j = Y >> 1;
      if constexpr ((LOC >> 1) != 0) jn = j + 1 < a.ch ? j + 1 : a.ch - 1;   /* TOP: row j + 1, read on odd rows only */
      else jn = (Y & 1u) ? (j + 1 < a.ch ? j + 1 : a.ch - 1) : (j ? j - 1 : 0u);
    }
    l.last = (int)(a.cw - 1u - i0);
    uint32_t is = i0;
    if constexpr ((LOC & 1) != 0) { l.lead = i0 != 0u; is = l.lead ? i0 - 1u : 0u; }
#pragma unroll
    for (int c = 0; c < 2; c++) {
      const M355_GLOBAL uint8_t* s = (const M355_GLOBAL uint8_t*)a.src[1 + c] + (size_t)is * SB;
      d_ldg16(s + (size_t)j * a.src_pitch[1], l.rc[c][0]);
      if constexpr ((LOC >> 1) != 0) { if (l.yodd) d_ldg16(s + (size_t)jn * a.src_pitch[1], l.rc[c][1]); }
      else if (CF == 1) d_ldg16(s + (size_t)jn * a.src_pitch[1], l.rc[c][1]);
    }
  }
}

/* the constants of a launch (scalar): the rounding term and the luma offset in one (ky), the signs folded into the coefficients */
struct RgbMatrix {
  int F, ky, cy, crv, ncgu, ncgv, cbu, c0;
};
__device__ __forceinline__ RgbMatrix d_rgb_matrix_of(const m355_rgb_coeffs& k)
{
  RgbMatrix m;
  m.F = k.F; m.ky = (int)((1u << (k.F - 1)) - (unsigned)k.cy * (unsigned)k.y0);
  m.cy = k.cy; m.crv = k.crv; m.ncgu = -k.cgu; m.ncgv = -k.cgv; m.cbu = k.cbu; m.c0 = k.c0;
  return m;
}
/* one pixel: luma sample y, chroma u, v (minus c0; not read for CF == 0) -> R, G, B clipped to 0 .. M */
template <int CF>
__device__ __forceinline__ void d_rgb_pixel(const RgbMatrix& m, int y, int u, int v, int M, unsigned& R, unsigned& G, unsigned& B)
{
  const int base = d_mad24(m.cy, y, m.ky);
  int r = base, g = base, b = base;
  if (CF != 0) {
    r = d_mad24(m.crv, v, base);
    g = d_mad24(m.ncgv, v, d_mad24(m.ncgu, u, base));
    b = d_mad24(m.cbu, u, base);
  }
  R = (unsigned)d_clip3(0, M, r >> m.F);
  G = (unsigned)d_clip3(0, M, g >> m.F);
  B = (unsigned)d_clip3(0, M, b >> m.F);
}

/* The NP = 16 / SB pixels from luma column X0 (even where chroma is subsampled) of luma row Y as the dwords of a 4-byte pixel format (pixel_pack.h; TEN: a
   2:10:10:10 format, the matrix with the coefficients of M355_RGB_U16; a.alpha_bits: the alpha in its place): the lane's work in k_export_pixels and in the
   oriented pixel export (k_export_oriented.hip), which differ in where the dwords go. */
template <int SB, bool TEN, int CF, int LOC, class A>
__device__ __forceinline__ void d_rgb_pixels_lane(const A& a, uint32_t X0, uint32_t Y, unsigned* o)
{
  constexpr int NP = 16 / SB, M = TEN ? 65535 : 255;
  RgbLane<SB, CF, LOC> l;
  d_rgb_load<SB, CF, LOC>(a, X0, Y, l);
  const RgbMatrix m = d_rgb_matrix_of(a.k);
  int u[NP], v[NP];
  if (CF != 0) {
    d_rgb_chroma<SB, CF, LOC>(l.rc[0][0], l.rc[0][1], l.last, m.c0, u, l.yodd, l.lead);
    d_rgb_chroma<SB, CF, LOC>(l.rc[1][0], l.rc[1][1], l.last, m.c0, v, l.yodd, l.lead);
  }
  const uint32_t alpha_bits = a.alpha_bits;
#pragma unroll
  for (int k = 0; k < NP; k++) {
    unsigned R, G, B;
    d_rgb_pixel<CF>(m, d_rgb_sample<SB>(l.ry, k), CF != 0 ? u[k] : 0, CF != 0 ? v[k] : 0, M, R, G, B);
    o[k] = m355_pp_dword(TEN, R, G, B, alpha_bits);
  }
}
