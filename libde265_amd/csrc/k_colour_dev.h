/*
 * k_colour_dev.h — the colour transform stage of k_export_resized_rgb.hip: colour_transform.h with the kernel's primitives (v_mad_i32_i24, v_ffbh_u32:
 * k_resize_dev.h, each with its twin for the SIMT interpreter) and the table reads of the device.  Include behind k_resize_dev.h.
 * Where the tables live: lut_out (1217 x 16 bits) in LDS — d_colour_fill copies it there in the tile's prologue, 609 dwords with the last entry
 * repeated at 1217, so that idx + 1 needs no clamp — and lut_in (1025 x 32 bits) in global memory, read through the vector cache.  Both tables in
 * LDS (6.5 KB more, 54 560 B for the F32 instantiations: three workgroups per CU with 160 bytes to spare) was built and measured too and is no faster
 * (profiles/export_colour_bench.txt), so the smaller footprint stays.  Per pixel: three gathers of two neighbouring dwords from lut_in, eighteen
 * 24-bit multiplies, three v_ffbh_u32, six 16-bit LDS reads.
 * Reads: lut_in[k], lut_in[k + 1] with k = v >> 6 <= 1023 for v <= 65535 (the caller's clip); LDS entries idx, idx + 1 with idx <= 1216 (P <= ONE by
 * the clip of m355_ct_matrix_row), of the 1218 the fill wrote.
 * A tone object's gain table (1217 x 32 bits, and the last entry once more: 1218 dwords behind the tables in the object's allocation) stays in GLOBAL
 * memory like lut_in: in LDS it is 4 880 bytes more, 55 344 B for the F32 instantiations, which is two workgroups per CU instead of three
 * (3 x 55 344 = 166 032 > 163 840), and was built and measured no faster (profiles/export_tone_bench.txt): one gather of two neighbouring dwords per
 * pixel beside the three of lut_in is cheap.  LDS is what it is for a
 * plain object: 44 320 B, F32 50 464 B.  Reads: gain[idx], gain[idx + 1] with idx <= 1216 — n is a maximum of three values the clip of
 * m355_ct_matrix_row holds in 0 .. ONE, or such a clipped row itself — of the 1218 m355_colour_create_tone wrote; the LDS entries as above, since
 * P' <= ONE (m355_ct_apply with g <= GAIN_ONE, which m355_ct_gain keeps for entries <= GAIN_ONE, checked at creation).  Per pixel beyond the plain
 * stage: that gather, five 32 x 32 -> 64-bit multiply-adds, one more v_ffbh_u32, and for M355_NORM_LUMA six 24-bit multiplies.
 */
#pragma once
#include <stddef.h>
#define M355_CT_MAD24(a, b, c) d_mad24((a), (b), (c))
#define M355_CT_FLOG2(x) d_flog2(x)
#include "colour_transform.h"

#define M355_COLOUR_LDS_DWORDS ((M355_COLOUR_OUT_KNOTS + 2) / 2)   /* 609: the table, its pad entry and nothing more (offsetof lut_out is a multiple of 4) */
static_assert(offsetof(m355_colour_tables, lut_out) % 4 == 0 && offsetof(m355_colour_tables, lut_out) + 4 * M355_COLOUR_LDS_DWORDS == sizeof(m355_colour_tables),
              "the fill reads lut_out and pad as dwords, to the end of the object");

/* lut_out into LDS by a workgroup of 256 lanes (no barrier here: the caller's next one covers it) */
__device__ __forceinline__ void d_colour_fill(const uint8_t* tables, unsigned* lds, uint32_t tid)
{
  const M355_GLOBAL unsigned* g = (const M355_GLOBAL unsigned*)(tables + offsetof(m355_colour_tables, lut_out));
  for (uint32_t q = tid; q < (uint32_t)M355_COLOUR_LDS_DWORDS; q += 256u) {
    unsigned v = g[q];
    if (q == (uint32_t)M355_COLOUR_LDS_DWORDS - 1u) v = (v & 0xFFFFu) * 0x10001u;   /* entry 1217 = entry 1216 */
    lds[q] = v;
  }
}
/* steps 1 to 3 of colour_transform.h for one pixel: e = its clipped 16-bit R'G'B' in, the three o out; m = the matrix (scalars) */
__device__ __forceinline__ void d_colour_pixel(const uint8_t* tables, const unsigned short* lo, const int32_t* m, unsigned (&e)[3])
{
  const M355_GLOBAL uint32_t* lin = (const M355_GLOBAL uint32_t*)tables;
  uint32_t ta[3], tb[3], l[3];
#pragma unroll
  for (int c = 0; c < 3; c++) { const uint32_t k = e[c] >> 6; ta[c] = lin[k]; tb[c] = lin[k + 1]; }   /* (the six loads in flight together) */
#pragma unroll
  for (int c = 0; c < 3; c++) l[c] = m355_ct_linear(ta[c], tb[c], e[c] & 63u);
#pragma unroll
  for (int c = 0; c < 3; c++) {
    uint32_t idx, fr;
    m355_ct_out_index(m355_ct_matrix_row(m[3 * c], m[3 * c + 1], m[3 * c + 2], l[0], l[1], l[2]), &idx, &fr);
    e[c] = m355_ct_encode(lo[idx], lo[idx + 1], fr);
  }
}
/* the same for a tone object: step 2b between the matrix and the output table — gain = the object's gain table (global memory, two neighbouring
   dwords in one gather per pixel), norm and w = its norm and weights (scalars) */
__device__ __forceinline__ void d_colour_pixel_tone(const uint8_t* tables, const unsigned short* lo, const int32_t* m, const uint32_t* gain, int32_t norm, const int32_t* w,
                                                    unsigned (&e)[3])
{
  const M355_GLOBAL uint32_t* lin = (const M355_GLOBAL uint32_t*)tables;
  const M355_GLOBAL uint32_t* gt = (const M355_GLOBAL uint32_t*)gain;
  uint32_t ta[3], tb[3], l[3], p[3], idx, fr;
#pragma unroll
  for (int c = 0; c < 3; c++) { const uint32_t k = e[c] >> 6; ta[c] = lin[k]; tb[c] = lin[k + 1]; }
#pragma unroll
  for (int c = 0; c < 3; c++) l[c] = m355_ct_linear(ta[c], tb[c], e[c] & 63u);
#pragma unroll
  for (int c = 0; c < 3; c++) p[c] = m355_ct_matrix_row(m[3 * c], m[3 * c + 1], m[3 * c + 2], l[0], l[1], l[2]);
  m355_ct_out_index(m355_ct_norm(norm, w[0], w[1], w[2], p[0], p[1], p[2]), &idx, &fr);
  const uint32_t g = m355_ct_gain(gt[idx], gt[idx + 1], fr);
#pragma unroll
  for (int c = 0; c < 3; c++) {
    m355_ct_out_index(m355_ct_apply(p[c], g), &idx, &fr);
    e[c] = m355_ct_encode(lo[idx], lo[idx + 1], fr);
  }
}
