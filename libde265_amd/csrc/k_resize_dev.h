/*
 * k_resize_dev.h — the primitives the resize kernels share (k_export_resized.hip, k_export_resized_rgb.hip) and k_asm.h does not have (it has the
 * signed dot product only, d_dot2, which the cubic filter's vertical pass uses), each with its twin for the SIMT interpreter.  Include behind k_common.h.
 */
#pragma once

/* c + a.lo * b.lo + a.hi * b.hi on packed unsigned 16-bit pairs (v_dot2_u32_u16: two rows of the vertical filter per issue; samples and coefficients
   fit 16 bits), c + a * b for a, b < 2^24 (v_mad_u32_u24; a full 32-bit multiply is a quarter-rate instruction), the signed v_mad_i32_i24, and a
   2-byte store at any address; floor(log2 x) for x > 0 (v_ffbh_u32: the exponent of the colour transform's output table, colour_transform.h) */
#ifdef SIMT_EMU
static inline int d_flog2(unsigned x) { int e = 0; while (x >>= 1) e++; return e; }
static inline unsigned d_udot2(unsigned a, unsigned b, unsigned c) { return c + (a & 0xFFFFu) * (b & 0xFFFFu) + (a >> 16) * (b >> 16); }
static inline unsigned d_umad24(unsigned a, unsigned b, unsigned c) { return c + a * b; }
static inline int d_mad24(int a, int b, int c) { return (int)((unsigned)a * (unsigned)b + (unsigned)c); }
static inline void d_stg2(void* p, unsigned v) { const unsigned short t = (unsigned short)v; memcpy(p, &t, 2); }
#else
__device__ __forceinline__ unsigned d_udot2(unsigned a, unsigned b, unsigned c)
{
  return __builtin_amdgcn_udot2(__builtin_bit_cast(m355_ushort2, a), __builtin_bit_cast(m355_ushort2, b), c, false);
}
__device__ __forceinline__ unsigned d_umad24(unsigned a, unsigned b, unsigned c) { return __umul24(a, b) + c; }
__device__ __forceinline__ int d_mad24(int a, int b, int c) { return (int)((unsigned)__mul24(a, b) + (unsigned)c); }
__device__ __forceinline__ void d_stg2(M355_GLOBAL void* p, unsigned v) { *(M355_GLOBAL m355_h1*)p = (unsigned short)v; }
__device__ __forceinline__ int d_flog2(unsigned x) { return 31 - (int)__builtin_clz(x); }
#endif

/* sample e of the 16-byte vectors of two rows as one 16-bit pair (row ra in the low half): what d_udot2 takes beside the rows' coefficients */
template <int SB> __device__ __forceinline__ unsigned d_pair(const unsigned* ra, const unsigned* rb, int e)
{
  if (SB == 1) return d_perm(rb[e >> 2], ra[e >> 2], 0x0c000c00u | (unsigned)(e & 3) | ((unsigned)(4 + (e & 3)) << 16));
  return (e & 1) ? d_pack_hi16(ra[e >> 1], rb[e >> 1]) : d_pack_lo16(ra[e >> 1], rb[e >> 1]);
}
