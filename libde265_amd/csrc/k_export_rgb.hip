/*
 * k_export_rgb.hip — a decoded frame (or a rectangle of it) into memory of the caller as R'G'B', packed or planar, 8 or 16 bits per channel
 * (m355_frame_export_rgb, include/de265_mi355x.h).  Integer-exact: chroma is brought to the luma positions by the one bilinear filter of the
 * header (chroma sample location type 0, or the type 1..3 of m355_export_opts: a template parameter), then the eight integers of
 * m355_rgb_coefficients are applied in signed 32-bit arithmetic.
 *
 * ONE launch per export.  The destination is the larger side of the traffic, so units follow destination rows: a wavefront converts one
 * 64-lane chunk of one row of the rectangle — row and chunk are decided once per wavefront, in scalar registers —, a lane the NP = 16 / SB
 * pixels behind ONE 16-byte luma vector.  All of a lane's loads are issued before the first use: its luma vector and, per chroma plane,
 * one 16-byte vector from each chroma row it needs (4:2:0: rows j and jn; 4:2:2 / 4:4:4: the one row), starting at the chroma sample of its
 * first pixel.  A subsampled lane needs NP / 2 chroma samples and the one to their right: the vector holds NP, so the right neighbour comes
 * with the same load — neither a neighbour lane nor an extra load is needed —, and where the frame's plane ends inside the vector the sample
 * of column CW - 1 stands for it (the clamp of the definition).  No LDS, no atomics.
 * Types 1 and 3 (CENTRE) also need the sample to the LEFT of the lane's first one: the vector then starts at column i0 - 1 — for the lane at
 * column 0 at i0 itself, where the clamp makes sample 0 its own left neighbour — and holds columns i0 - 1 .. i0 + NP / 2, NP / 2 + 2 <= NP
 * samples, so it is still one load without a neighbour lane.  Types 2 and 3 (TOP) need chroma row j alone on even luma rows and rows j, j + 1 on odd
 * ones; the row's parity is wave-uniform, so even rows skip the second load.
 * Arithmetic: 4:2:0 sums T = 3 C[j] + C[jn] and their pairs stay below 2^19 and are kept in 32-bit registers; the offset c0 is folded into
 * the rounding constant of the filter's shift ((T + 2 - 4 c0) >> 2 = ((T + 2) >> 2) - c0, arithmetic shift), so u and v come out signed.
 * The matrix is five v_mad_i32_i24 per pixel (coefficients < 2^23, |u|, |v|, Y < 2^16), a shift and a clip per channel.  The luma offset and
 * the rounding term are one constant (H - cy y0) and sums are accumulated modulo 2^32: whatever a partial sum does, the complete sum is the
 * one the header defines, which fits a signed 32-bit register (its largest magnitude is 0.54 * 2^31).
 * Stores are whole vectors: a lane's channels are packed into dwords with v_perm_b32 (8-bit: four values per dword, three perms) and go out
 * as 16-byte stores (+ one of 8 bytes where the lane's bytes are 24 or 8); the last lane of a row stores its valid bytes only, as dwords and
 * single bytes (the idiom of k_export.hip's d_export_store for any number of dwords; d_scaled_store's whole-lane sizes end at 32 bytes, a
 * lane here has up to 96), so nothing beyond the exported row is written.
 *
 * No out-of-bounds read.  Every load is 16 bytes from a sample INSIDE a row of the frame's plane: luma column x0 + p0 < W of row y0 + row <
 * H; chroma column i0 = (x0 + p0) / SubWidthC <= CW - 1 — CENTRE: column max(i0 - 1, 0), which is no less inside the row — of a row clamped to
 * 0 .. CH - 1 (TOP: row min(j + 1, CH - 1)).  Rows are padded to 128 bytes and a plane's allocation ends with a 256-byte tail
 * (runtime_internal.h frame_alloc), so even the vector of the last sample of the last row ends inside the allocation — half the span k_export.hip argues for.  Bytes of a vector beyond column CW - 1 (padding, or the next row's start) are
 * loaded and never used: every use is indexed through the clamp.
 * Roofline: traffic (every luma byte read once, every chroma row once or twice, every destination byte written once) against ~40 VALU
 * issues per pixel — profiles/export_rgb_bench.txt.
 */
#include "k_common.h"

#include "k_rgb_dev.h"   /* d_mad24, d_rgb_sample, d_rgb_chroma, d_rgb_load, d_rgb_pixel: shared with k_stats.hip; d_rgb_pixels_lane: with k_export_oriented.hip */

/* N values of one byte / one 16-bit half each -> N * DB / 4 dwords */
template <int DB, int N> __device__ __forceinline__ void d_rgb_pack(const unsigned* e, unsigned* o)
{
  if (DB == 1) {
#pragma unroll
    for (int i = 0; i < N / 4; i++) o[i] = d_pack_lo16(d_perm(e[4 * i + 1], e[4 * i], 0x0c0c0400u), d_perm(e[4 * i + 3], e[4 * i + 2], 0x0c0c0400u));
  } else {
#pragma unroll
    for (int i = 0; i < N / 2; i++) o[i] = d_pack_lo16(e[2 * i], e[2 * i + 1]);
  }
}

/* ND dwords (nb >= 4 ND) or the first nb bytes of them to d: whole lanes store vectors, the end of a row goes out as dwords and single bytes */
template <int ND> __device__ __forceinline__ void d_rgb_store(M355_GLOBAL uint8_t* d, const unsigned* o, uint32_t nb)
{
  if (nb >= 4u * ND) {
#pragma unroll
    for (int i = 0; i + 4 <= ND; i += 4) d_stg16(d + 4 * i, o + i);
    if (ND % 4 == 2) d_stg8(d + 4 * (ND - 2), o + ND - 2);
    return;
  }
#pragma unroll
  for (uint32_t i = 0; i < (uint32_t)ND; i++) {
    if (4 * i + 4 <= nb) d_stg4(d + 4 * i, o[i]);
    else for (uint32_t k = 0; k < 3; k++) if (4 * i + k < nb) d[4 * i + k] = (uint8_t)(o[i] >> (8 * k));
  }
}

template <int SB, int DB, int PLANAR, int CF, int LOC>
__global__ void __launch_bounds__(256) k_export_rgb(ExportRgbArgs a)
{
  M355_GATE(a);
  constexpr int NP = 16 / SB, M = DB == 1 ? 255 : 65535;
  /* this wavefront's unit: row of the rectangle, position in the row */
  const uint32_t unit = __builtin_amdgcn_readfirstlane((uint32_t)(blockIdx.x * 4u + (threadIdx.x >> 6)));
  if (unit >= a.units) return;
  const uint32_t row = unit / a.chunks, chunk = unit - row * a.chunks;
  const uint32_t p0 = (chunk * 64u + (threadIdx.x & 63u)) * NP;
  if (p0 >= a.width) return;
  const uint32_t n = a.width - p0 < (uint32_t)NP ? a.width - p0 : (uint32_t)NP;
  const uint32_t X0 = a.x0 + p0, Y = a.y0 + row;
  RgbLane<SB, CF, LOC> l;
  d_rgb_load<SB, CF, LOC>(a, X0, Y, l);
  const RgbMatrix m = d_rgb_matrix_of(a.k);
  int u[NP], v[NP];
  if (CF != 0) {
    d_rgb_chroma<SB, CF, LOC>(l.rc[0][0], l.rc[0][1], l.last, m.c0, u, l.yodd, l.lead);
    d_rgb_chroma<SB, CF, LOC>(l.rc[1][0], l.rc[1][1], l.last, m.c0, v, l.yodd, l.lead);
  }
  unsigned e[3][NP];
#pragma unroll
  for (int k = 0; k < NP; k++) d_rgb_pixel<CF>(m, d_rgb_sample<SB>(l.ry, k), CF != 0 ? u[k] : 0, CF != 0 ? v[k] : 0, M, e[0][k], e[1][k], e[2][k]);
  if (PLANAR) {
    constexpr int ND = NP * DB / 4;
#pragma unroll
    for (int c = 0; c < 3; c++) {
      unsigned o[ND];
      d_rgb_pack<DB, NP>(e[c], o);
      d_rgb_store<ND>((M355_GLOBAL uint8_t*)a.dst[c] + (size_t)row * a.dst_pitch[c] + (size_t)p0 * DB, o, n * (uint32_t)DB);
    }
  } else {
    constexpr int ND = 3 * NP * DB / 4;
    unsigned w[3 * NP], o[ND];
#pragma unroll
    for (int k = 0; k < NP; k++) { w[3 * k] = e[0][k]; w[3 * k + 1] = e[1][k]; w[3 * k + 2] = e[2][k]; }
    d_rgb_pack<DB, 3 * NP>(w, o);
    d_rgb_store<ND>((M355_GLOBAL uint8_t*)a.dst[0] + (size_t)row * a.dst_pitch[0] + (size_t)p0 * (3 * DB), o, n * (uint32_t)(3 * DB));
  }
}

void m355_launch_export_rgb(const ExportRgbArgs& a, int src_bytes, int dst_bytes, bool planar, int chroma_format, int chroma_loc, hipStream_t st)
{
  if (!a.units) return;
  const dim3 grid((a.units + 3) / 4), block(256);
  const int loc = chroma_format == 1 ? chroma_loc : 0;          /* (the siting is 4:2:0's alone) */
#define M355_EXPORT_RGB_CF(SB, DB, PL, CF, LOC) \
  if (chroma_format == CF && loc == LOC) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_export_rgb<SB, DB, PL, CF, LOC>), grid, block, 0, st, a);
#define M355_EXPORT_RGB_PL(SB, DB, PL) \
  M355_EXPORT_RGB_CF(SB, DB, PL, 0, 0) M355_EXPORT_RGB_CF(SB, DB, PL, 1, 0) M355_EXPORT_RGB_CF(SB, DB, PL, 2, 0) M355_EXPORT_RGB_CF(SB, DB, PL, 3, 0) \
  M355_EXPORT_RGB_CF(SB, DB, PL, 1, 1) M355_EXPORT_RGB_CF(SB, DB, PL, 1, 2) M355_EXPORT_RGB_CF(SB, DB, PL, 1, 3)
#define M355_EXPORT_RGB_CASE(SB, DB) \
  if (src_bytes == SB && dst_bytes == DB) { \
    if (planar) { M355_EXPORT_RGB_PL(SB, DB, 1) } \
    else { M355_EXPORT_RGB_PL(SB, DB, 0) } \
  }
  M355_EXPORT_RGB_CASE(1, 1) M355_EXPORT_RGB_CASE(1, 2) M355_EXPORT_RGB_CASE(2, 1) M355_EXPORT_RGB_CASE(2, 2)
#undef M355_EXPORT_RGB_CASE
#undef M355_EXPORT_RGB_PL
#undef M355_EXPORT_RGB_CF
}

/* The pixel-format store path (m355_frame_export_pixels; pixel_pack.h): the same units, loads, chroma reconstruction and matrix — k_rgb_dev.h as it
   is —, then a DWORD per pixel: the three channels (TEN: matrix with the coefficients of M355_RGB_U16, clip to 65535, then c10 per channel) and the
   alpha, which arrives in its place (a.alpha_bits, wave-uniform), joined by shift-or / v_perm_b32.  A lane's NP dwords (64 or 32 bytes) leave as 16-byte
   stores; a pixel is a dword, so the row's last lane stores whole dwords only (d_rgb_store with a multiple of 4: its byte tail is never reached).
   The channel order is not the kernel's business: B, G, R is R, G, B of the frame with Cb and Cr and their coefficients exchanged (R = cy y + crv v,
   B = cy y + cbu u, G is symmetric in the two), which the host does (runtime_export.hip) — the sums are the same integers modulo 2^32, so BGRA8,
   A2R10G10B10 and BGR8 (the packed path above, unchanged) cost no instruction and no instantiation.  Reads and bounds: as argued in the header
   comment; writes: dwords p0 .. p0 + n - 1 of row `row`, p0 + n <= width. */
template <int SB, bool TEN, int CF, int LOC>
__global__ void __launch_bounds__(256) k_export_pixels(ExportRgbArgs a)
{
  M355_GATE(a);
  constexpr int NP = 16 / SB;
  const uint32_t unit = __builtin_amdgcn_readfirstlane((uint32_t)(blockIdx.x * 4u + (threadIdx.x >> 6)));
  if (unit >= a.units) return;
  const uint32_t row = unit / a.chunks, chunk = unit - row * a.chunks;
  const uint32_t p0 = (chunk * 64u + (threadIdx.x & 63u)) * NP;
  if (p0 >= a.width) return;
  const uint32_t n = a.width - p0 < (uint32_t)NP ? a.width - p0 : (uint32_t)NP;
  const uint32_t X0 = a.x0 + p0, Y = a.y0 + row;
  unsigned o[NP];
  d_rgb_pixels_lane<SB, TEN, CF, LOC>(a, X0, Y, o);
  d_rgb_store<NP>((M355_GLOBAL uint8_t*)a.dst[0] + (size_t)row * a.dst_pitch[0] + (size_t)p0 * 4u, o, n * 4u);
}

void m355_launch_export_pixels(const ExportRgbArgs& a, int src_bytes, bool ten, int chroma_format, int chroma_loc, hipStream_t st)
{
  if (!a.units) return;
  const dim3 grid((a.units + 3) / 4), block(256);
  const int loc = chroma_format == 1 ? chroma_loc : 0;          /* (the siting is 4:2:0's alone) */
#define M355_EXPORT_PX_CF(SB, TEN, CF, LOC) \
  if (chroma_format == CF && loc == LOC) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_export_pixels<SB, TEN, CF, LOC>), grid, block, 0, st, a);
#define M355_EXPORT_PX_CASE(SB, TEN) \
  if (src_bytes == SB && ten == TEN) { \
    M355_EXPORT_PX_CF(SB, TEN, 0, 0) M355_EXPORT_PX_CF(SB, TEN, 1, 0) M355_EXPORT_PX_CF(SB, TEN, 2, 0) M355_EXPORT_PX_CF(SB, TEN, 3, 0) \
    M355_EXPORT_PX_CF(SB, TEN, 1, 1) M355_EXPORT_PX_CF(SB, TEN, 1, 2) M355_EXPORT_PX_CF(SB, TEN, 1, 3) \
  }
  M355_EXPORT_PX_CASE(1, false) M355_EXPORT_PX_CASE(1, true) M355_EXPORT_PX_CASE(2, false) M355_EXPORT_PX_CASE(2, true)
#undef M355_EXPORT_PX_CASE
#undef M355_EXPORT_PX_CF
}
