/*
 * pixel_pack.h — the ONE definition of the pixel formats of m355_frame_export_pixels and m355_frame_export_resized_pixels (include/de265_mi355x.h,
 * M355_PIXEL_*): the three channel values the R'G'B' export delivers for a pixel — 8 bits each (M355_RGB_U8) for RGBA8, BGRA8 and BGR8, 16 bits
 * each (M355_RGB_U16) for the two 2:10:10:10 formats — become the pixel's bytes.  Compiled three times, as tensor_element.h and colour_transform.h
 * are: into k_export_rgb.hip and k_export_resized_rgb.hip (device), into the SIMT-interpreter build of those kernels (SIMT_EMU, plain C++) and into
 * m355_pixel_pack (runtime_export.hip, host), which the tests run over every channel value.
 *   8-bit formats   the values as they are: the dword lo | G << 8 | hi << 16 | A << 24, little-endian, of which BGR8 has the low three bytes
 *   10-bit formats  c10 = (2046 c + 65535) / 131070 per channel in unsigned 32 bits (at most 2046 * 65535 + 65535 < 2^27) = round(c * 1023 / 65535),
 *                   the 10-bit sibling of m355_ct_deliver's (2 o + 257) / 514; then the dword lo | G << 10 | hi << 20 | A << 30, little-endian
 *   (lo, hi) = (R, B) for RGBA8 and A2B10G10R10, (B, R) for BGRA8, BGR8 and A2R10G10B10: m355_pp_swapped.
 * The kernels take the alpha already in its place (m355_pp_alpha_bits: a wave-uniform kernel argument) and `ten` as a template parameter.
 */
#ifndef M355_PIXEL_PACK_H
#define M355_PIXEL_PACK_H

#include <stdint.h>
#include "de265_mi355x.h"

#ifdef __HIPCC__
#define M355_PP_FN __host__ __device__ static inline
#else
#define M355_PP_FN static inline
#endif

M355_PP_FN bool m355_pp_known(int format) { return format >= M355_PIXEL_RGBA8 && format <= M355_PIXEL_A2R10G10B10; }
M355_PP_FN bool m355_pp_ten(int format) { return format == M355_PIXEL_A2B10G10R10 || format == M355_PIXEL_A2R10G10B10; }
M355_PP_FN bool m355_pp_swapped(int format) { return format == M355_PIXEL_BGRA8 || format == M355_PIXEL_BGR8 || format == M355_PIXEL_A2R10G10B10; }
M355_PP_FN int m355_pp_bytes(int format) { return format == M355_PIXEL_BGR8 ? 3 : 4; }
M355_PP_FN uint32_t m355_pp_channel_max(int format) { return m355_pp_ten(format) ? 65535u : 255u; }
M355_PP_FN uint32_t m355_pp_alpha_max(int format) { return format == M355_PIXEL_BGR8 ? 0u : (m355_pp_ten(format) ? 3u : 255u); }
M355_PP_FN uint32_t m355_pp_alpha_bits(int format, uint32_t alpha) { return format == M355_PIXEL_BGR8 ? 0u : alpha << (m355_pp_ten(format) ? 30 : 24); }

/* a 16-bit full-scale value as 10 bits: round(c * 1023 / 65535) */
M355_PP_FN uint32_t m355_pp_c10(uint32_t c) { return (2046u * c + 65535u) / 131070u; }

/* the pixel's dword from the channel that goes lowest, G, the channel that goes highest and the alpha in its place */
M355_PP_FN uint32_t m355_pp_dword(bool ten, uint32_t lo, uint32_t g, uint32_t hi, uint32_t alpha_bits)
{
  if (ten) return m355_pp_c10(lo) | (m355_pp_c10(g) << 10) | (m355_pp_c10(hi) << 20) | alpha_bits;
  return lo | (g << 8) | (hi << 16) | alpha_bits;
}
/* the same from (R, G, B) and the format's channel order */
M355_PP_FN uint32_t m355_pp_pixel(bool ten, bool swapped, const uint32_t* rgb, uint32_t alpha_bits)
{
  return m355_pp_dword(ten, swapped ? rgb[2] : rgb[0], rgb[1], swapped ? rgb[0] : rgb[2], alpha_bits);
}

#endif
