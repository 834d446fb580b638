/*
 * k_export_dev.h — what the kernels that export a frame's planes sample by sample share: k_export.hip, which stores rows as they are, and
 * k_export_oriented.hip, which turns them.  One definition, so that "the bytes m355_frame_export delivers" is the same code in both: the loads behind 16
 * destination bytes, their conversion (NATIVE / MSB16 / U8, an interleaved chroma row) and the store of a row's end.  k_export.hip's header comment holds
 * the argument for the reads that stay inside the allocation.
 */
#pragma once
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
