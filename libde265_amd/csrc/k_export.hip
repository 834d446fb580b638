/*
 * k_export.hip — a decoded frame (or a rectangle of it) into memory of the caller, in the layout a consumer on the same GPU
 * reads: planar or semi-planar (NV12 / P010 shapes), samples as they are, MSB-aligned 16-bit, or rounded to 8 bits
 * (m355_frame_export, include/de265_mi355x.h).  Integer-exact: no colour conversion, no scaling.
 *
 * ONE launch covers every plane.  A lane produces 16 destination bytes of one row — a vector load (two for 16 -> 8 bits, one per
 * chroma plane for an interleaved row), the conversion in packed 16-bit arithmetic, one vector store —, a wavefront 1024
 * consecutive destination bytes of one row: which plane, row and chunk is decided once per wavefront, in scalar registers.
 * (Several rows per wavefront with all their loads in flight before the first store, and streaming stores, were built and measured:
 * 2, 4 and 8 rows each cost the 8K export 1-3 %, the stores change nothing — profiles/export_bench.txt.)
 * A crop starts the source rows at any sample and the caller's pitch starts the destination rows at any byte: loads and stores
 * are the byte-aligned vector forms of k_asm.h (one global_load / global_store_dwordx4 each, whatever the address); the last lane
 * of a row stores its valid bytes only, as dwords and single bytes, so nothing beyond the exported row is written.  A lane reads
 * up to 32 bytes from its first source sample, which lies inside the row: that stays inside the plane's allocation (rows are
 * padded to 128 bytes and a plane ends with a 256-byte tail, runtime_internal.h frame_alloc).
 * Roofline: pure traffic — every source byte read once, every destination byte written once; plain stores (the consumer reads
 * the data next).
 */
#include "k_common.h"

/* min(255, (s + (1 << (sh - 1))) >> sh) on both halves; sh = bit depth - 8 = 1..8.  The saturating add stands for the 17th bit: a sum
   that overflows 16 bits is >= 256 after the shift, and so is 0xFFFF >> sh */
__device__ __forceinline__ unsigned d_round_clip8(unsigned v, int sh, unsigned half)
{
  return d_pk_min_u16(d_pk_lshr16(d_pk_addsat_u16(v, half), sh), 0x00FF00FFu);
}

/* A lane's work in two steps: d_export_load fetches the source bytes behind 16 destination bytes (raw[]: up to 8 dwords), d_export_convert
   makes the 16 bytes.
   INTER: an interleaved chroma row — Cb, Cr, Cb, Cr, ... from the matching spans of both planes (s, s2). */
template <int SB, int DB, bool INTER>
__device__ __forceinline__ void d_export_load(const M355_GLOBAL uint8_t* s, const M355_GLOBAL uint8_t* s2, unsigned* raw)
{
  if (!INTER) {
    if (SB == DB) d_ldg16(s, raw);
    else if (SB == 1) d_ldg8(s, raw);
    else { d_ldg16(s, raw); d_ldg16(s + 16, raw + 4); }
  } else {
    if (SB == DB) { d_ldg8(s, raw); d_ldg8(s2, raw + 2); }
    else if (SB == 1) { raw[0] = d_ldg4(s); raw[1] = d_ldg4(s2); }
    else { d_ldg16(s, raw); d_ldg16(s2, raw + 4); }
  }
}
template <int SB, int DB, bool INTER>
__device__ __forceinline__ void d_export_convert(const unsigned* raw, int sh, unsigned* o)
{
  const unsigned half = SB == 2 && DB == 1 ? 0x00010001u << (sh - 1) : 0u;
  if (!INTER) {
    if (SB == DB) for (int i = 0; i < 4; i++) o[i] = SB == 2 ? d_pk_shl16(raw[i], sh) : raw[i];
    else if (SB == 1)                                      /* byte k -> the high byte of 16-bit value k */
      for (int i = 0; i < 2; i++) { o[2 * i] = d_perm(0, raw[i], 0x010c000cu); o[2 * i + 1] = d_perm(0, raw[i], 0x030c020cu); }
    else for (int i = 0; i < 4; i++) o[i] = d_pack_bytes(d_round_clip8(raw[2 * i], sh, half), d_round_clip8(raw[2 * i + 1], sh, half));
  } else {
    if (SB == 2 && DB == 2)
      for (int i = 0; i < 2; i++) {
        const unsigned x = d_pk_shl16(raw[i], sh), y = d_pk_shl16(raw[2 + i], sh);
        o[2 * i] = d_pack_lo16(x, y); o[2 * i + 1] = d_pack_hi16(x, y);
      }
    else if (SB == 1 && DB == 1)
      for (int i = 0; i < 2; i++) { o[2 * i] = d_perm(raw[2 + i], raw[i], 0x05010400u); o[2 * i + 1] = d_perm(raw[2 + i], raw[i], 0x07030602u); }
    else if (SB == 1) {
      o[0] = d_perm(raw[1], raw[0], 0x040c000cu); o[1] = d_perm(raw[1], raw[0], 0x050c010cu);
      o[2] = d_perm(raw[1], raw[0], 0x060c020cu); o[3] = d_perm(raw[1], raw[0], 0x070c030cu);
    } else for (int i = 0; i < 4; i++) o[i] = d_round_clip8(raw[i], sh, half) | (d_round_clip8(raw[4 + i], sh, half) << 8);   /* (both <= 255 per half) */
  }
}

/* 16 bytes (n >= 16) or the first n of them to d: the end of a row goes out as dwords and single bytes */
__device__ __forceinline__ void d_export_store(M355_GLOBAL uint8_t* d, const unsigned* o, uint32_t n)
{
  if (n >= 16) { d_stg16(d, o); return; }
  for (uint32_t i = 0; i < 4; i++) {
    if (4 * i + 4 <= n) d_stg4(d + 4 * i, o[i]);
    else for (uint32_t k = 0; k < 3; k++) if (4 * i + k < n) d[4 * i + k] = (uint8_t)(o[i] >> (8 * k));
  }
}

/* a table entry of the wavefront's plane, selected from the three entries of the argument tables by two scalar compares: with constant
   indices hipcc fetches whole tables with one scalar load each — indexing the argument segment with the plane is a chain of dependent
   scalar loads (plane -> chunks -> row -> pointers) in front of the first sample load (cf. M355_SEL3) */
#define M355_EXPORT_SEL(arr) (p2 ? (arr)[2] : (p1 ? (arr)[1] : (arr)[0]))

template <int SB, int DB, int SEMI>
__global__ void __launch_bounds__(256) k_export(ExportArgs a)
{
  M355_GATE(a);
  /* this wavefront's unit: plane, row, position in the row */
  const uint32_t unit = __builtin_amdgcn_readfirstlane((uint32_t)(blockIdx.x * 4u + (threadIdx.x >> 6)));
  if (unit >= a.unit_end[2]) return;
  const bool p1 = unit >= a.unit_end[0], p2 = unit >= a.unit_end[1];
  const uint32_t u = unit - (p2 ? a.unit_end[1] : (p1 ? a.unit_end[0] : 0u));
  const uint32_t chunks = M355_EXPORT_SEL(a.chunks), row = u / chunks, chunk = u - row * chunks;
  const uint32_t rb = M355_EXPORT_SEL(a.row_bytes), ofs = (chunk * 64u + (threadIdx.x & 63u)) * 16u;
  if (ofs >= rb) return;
  const int sh = M355_EXPORT_SEL(a.shift);
  const bool inter = SEMI && p1;                            /* (semi-planar: plane 1 is the last one) */
  /* source bytes in front of this lane's first sample: ofs / DB samples of the row, half as many per plane of an interleaved one */
  const size_t sofs = (size_t)row * M355_EXPORT_SEL(a.src_pitch) + (size_t)(ofs / (inter ? 2 * DB : DB)) * SB;
  const M355_GLOBAL uint8_t* s = (const M355_GLOBAL uint8_t*)M355_EXPORT_SEL(a.src) + sofs;
  unsigned raw[8], o[4];
  if (inter) { d_export_load<SB, DB, true>(s, (const M355_GLOBAL uint8_t*)a.src[2] + sofs, raw); d_export_convert<SB, DB, true>(raw, sh, o); }
  else { d_export_load<SB, DB, false>(s, s, raw); d_export_convert<SB, DB, false>(raw, sh, o); }
  d_export_store((M355_GLOBAL uint8_t*)M355_EXPORT_SEL(a.dst) + (size_t)row * M355_EXPORT_SEL(a.dst_pitch) + ofs, o, rb - ofs);
}

void m355_launch_export(const ExportArgs& a, int src_bytes, int dst_bytes, bool semiplanar, hipStream_t st)
{
  const uint32_t units = a.unit_end[2];
  if (!units) return;
  const dim3 grid((units + 3) / 4), block(256);
#define M355_EXPORT_CASE(SB, DB) \
  if (src_bytes == SB && dst_bytes == DB) { \
    if (semiplanar) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_export<SB, DB, 1>), grid, block, 0, st, a); \
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_export<SB, DB, 0>), grid, block, 0, st, a); \
  }
  M355_EXPORT_CASE(1, 1) M355_EXPORT_CASE(1, 2) M355_EXPORT_CASE(2, 1) M355_EXPORT_CASE(2, 2)
#undef M355_EXPORT_CASE
}
