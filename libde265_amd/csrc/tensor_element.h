/*
 * tensor_element.h — the ONE definition of the float stage of m355_frames_export_tensor (include/de265_mi355x.h): an integer channel value v of
 * the R'G'B' stage becomes  r = (float)v * scale + bias  — one binary32 multiplication and one binary32 addition, each rounded to nearest even,
 * NOT a fused multiply-add — delivered as binary32, as binary16 or as bfloat16, both rounded to nearest even from r.  Compiled three times, as
 * resize_taps.h is: into k_export_resized_rgb.hip (device), into the SIMT-interpreter build of that kernel (SIMT_EMU, plain C++) and into
 * m355_tensor_element (runtime.hip, host), which the tests run over every v.
 *   binary16  gradual underflow (subnormals are produced), overflow gives infinity.  Device: v_cvt_f16_f32 (round to nearest even, binary16
 *             denormals on, as HIP code objects have them); host and interpreter: the integer statement below.
 *   bfloat16  (bits + 0x7FFF + ((bits >> 16) & 1)) >> 16 on the binary32 bit pattern, on every build (r is never a NaN: v, scale, bias are finite).
 * A product or a sum that is a nonzero binary32 subnormal is outside the contract (the device may flush it).
 */
#ifndef M355_TENSOR_ELEMENT_H
#define M355_TENSOR_ELEMENT_H

#include <stdint.h>
#include <string.h>

#ifdef __HIPCC__
#define M355_TE_FN __host__ __device__ inline
#else
#define M355_TE_FN inline
#endif
#if defined(__HIP_DEVICE_COMPILE__) && !defined(SIMT_EMU)
#define M355_TE_DEVICE 1
#endif

/* r = (float)v * scale + bias, two roundings */
M355_TE_FN float m355_te_affine(uint32_t v, float scale, float bias)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#ifdef M355_TE_DEVICE
  /* HIP's __fmul_rn / __fadd_rn are the plain operators, and the device back end fuses a multiplication into an addition under the HIP compiler's
     default contraction mode whatever the pragma says (seen in the code it made: v_fma_f32): the product passes through an empty asm statement,
     which the optimiser cannot look through and which costs no instruction */
  float t = __fmul_rn((float)v, scale);
  asm volatile("" : "+v"(t));
  return __fadd_rn(t, bias);
#else
  const float t = (float)v * scale;
  return t + bias;
#endif
#else
  volatile float t = (float)v * scale;                       /* (no contraction across a volatile object) */
  return t + bias;
#endif
}

M355_TE_FN uint32_t m355_te_bits(float r)
{
#ifdef M355_TE_DEVICE
  return __float_as_uint(r);
#else
  uint32_t b;
  memcpy(&b, &r, 4);
  return b;
#endif
}

/* binary32 -> binary16, round to nearest even, in integers */
M355_TE_FN uint32_t m355_te_f16_int(uint32_t x)
{
  const uint32_t sign = (x >> 16) & 0x8000u, e = (x >> 23) & 0xFFu;
  uint32_t m = x & 0x7FFFFFu;
  if (e == 0xFFu) return sign | 0x7C00u | (m ? 0x200u | (m >> 13) : 0u);
  const int32_t E = (int32_t)e - 127 + 15;
  if (E >= 31) return sign | 0x7C00u;
  if (E <= 0) {                                              /* a binary16 subnormal or zero: 1.m x 2^(E - 15) in units of 2^-24 */
    if (E < -10) return sign;                                /* below 2^-25: zero */
    m |= 0x800000u;
    const int sh = 14 - E;                                   /* 14 .. 24 */
    uint32_t h = m >> sh;
    const uint32_t rem = m & ((1u << sh) - 1u), half = 1u << (sh - 1);
    if (rem > half || (rem == half && (h & 1u))) h++;
    return sign | h;
  }
  uint32_t h = ((uint32_t)E << 10) | (m >> 13);
  const uint32_t rem = m & 0x1FFFu;
  if (rem > 0x1000u || (rem == 0x1000u && (h & 1u))) h++;    /* (a carry out of the mantissa raises the exponent, up to infinity) */
  return sign | h;
}

M355_TE_FN uint32_t m355_te_f16(float r)
{
#ifdef M355_TE_DEVICE
  const _Float16 h = (_Float16)r;
  return (uint32_t)__builtin_bit_cast(unsigned short, h);
#else
  return m355_te_f16_int(m355_te_bits(r));
#endif
}

M355_TE_FN uint32_t m355_te_bf16(float r)
{
  const uint32_t b = m355_te_bits(r);
  return (b + 0x7FFFu + ((b >> 16) & 1u)) >> 16;
}

/* a 2-byte element without a branch, for the kernel, where the format is a uniform run-time switch: both conversions and a bitwise select by
   bf16_mask = all ones (bfloat16) or zero (binary16).  (A branch per channel and row cost the kernel 3 % of its time.) */
M355_TE_FN uint32_t m355_te_half(float r, uint32_t bf16_mask) { return (m355_te_bf16(r) & bf16_mask) | (m355_te_f16(r) & ~bf16_mask); }

/* the element's bit pattern in the low 32 (F32) or 16 bits; dtype = M355_TENSOR_F32 / _F16 / _BF16 (0 / 1 / 2) */
M355_TE_FN uint32_t m355_te_element(uint32_t v, float scale, float bias, int dtype)
{
  const float r = m355_te_affine(v, scale, bias);
  return dtype == 0 ? m355_te_bits(r) : (dtype == 1 ? m355_te_f16(r) : m355_te_bf16(r));
}

#endif
