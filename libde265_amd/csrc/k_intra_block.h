/*
 * k_intra_block.h — the arithmetic of ONE intra block, shared by k_intra's two paths (k_intra.hip: the CTB workgroup that keeps the CTB's body in
 * LDS; k_intra_light.h: one wave per CTB and component that reads and writes the picture).  Everything here works on a border that has been
 * gathered already — where its samples come from, where the residual lives and where the block's samples go is the caller's business.
 *   4x4 / 8x8:     the border lives in ONE register, entry e = i + 2nT in lane e (cross-lane reads): d_intra_small_predict;
 *   16x16 / 32x32: the border lives in LDS, entry e at P[e]: d_intra_big_filter (smoothing), d_intra_big_dc, d_intra_big_fixed / _taps / _value
 *                  (what does not depend on the row, the border taps of one sample, the sample).
 * intra_prediction_sample_filtering (intrapred.h:185-258), intra_prediction_planar / _DC / _angular (intrapred.h:261-433).
 */
#ifndef M355_K_INTRA_BLOCK_H
#define M355_K_INTRA_BLOCK_H
#include "k_common.h"

/* the lane's predicted sample of a 4x4 / 8x8 block (no residual yet).  Every lane runs the arithmetic (a cross-lane read needs its source lane
   active); the lanes beyond the block alias its samples.  (branch-free where it is cheap: a taken branch costs a lone wave more than the few
   instructions it skips) */
template <int LOG2>
__device__ __forceinline__ int d_intra_small_predict(uint32_t bv, const uint32_t e0, const int cls, const int angle, const int inv, const bool vert, const bool bfilt, const int pix_max)
{
  constexpr int NT = 1 << LOG2, Z = 2 * NT, NENT = 4 * NT + 1;
  const int lane = threadIdx.x & 63;
  const int x = lane & (NT - 1), y = lane >> LOG2;
  {   /* intra_prediction_sample_filtering (intrapred.h:185-258), [1 2 1] only (strong smoothing is 32x32) */
    const uint32_t nb = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)bv, 0x138, 0xF, 0xF, false) + (uint32_t)__builtin_amdgcn_update_dpp(0, (int)bv, 0x130, 0xF, 0xF, false);
    const uint32_t fbv = (nb + 2u * bv + 2u) >> 2;
    if ((e0 & M355_IBX_FILT) && lane > 0 && lane < NENT - 1) bv = fbv;
  }
#define BRL(i) ((int)__builtin_amdgcn_readlane((int)bv, (i) + Z))                 /* border entry i, the same for every lane */
#define BRP(i) ((int)__builtin_amdgcn_ds_bpermute(((i) + Z) << 2, (int)bv))       /* border entry i, per lane */
  int v;
  if (__builtin_expect(cls >= 3, 1)) {
    /* angular (33 of the 35 modes; first in line, and one formula for both signs of the angle): ref[] of the reference is not
       built — its entry i is border entry sgn*i for i >= 0 and, left of the corner (negative angles only), -sgn*((i*invAngle+128)>>8) */
    const int a_ = vert ? y : x, b_ = vert ? x : y;
    const int tt = __mul24(a_ + 1, angle), iIdx = tt >> 5, iFact = tt & 31;
    const int x1 = b_ + iIdx + 1, x2 = x1 + 1;
    const int p1 = (__mul24(x1, inv) + 128) >> 8, p2 = (__mul24(x2, inv) + 128) >> 8;     /* (invAngle is 0 for a positive angle, whose x1 is never negative) */
    int i1 = x1 >= 0 ? x1 : -p1, i2 = x2 >= 0 ? x2 : -p2;
    if (!vert) { i1 = -i1; i2 = -i2; }
    const int r1 = BRP(i1), r2 = BRP(i2);
    v = (32 * r1 + __mul24(iFact, r2 - r1) + 16) >> 5;   /* (= r1 when iFact is 0) */
  } else if (cls == 0) {        /* planar (intrapred.h:261-285) */
    const int l = BRP(-1 - y), t = BRP(1 + x), tr = BRL(1 + NT), bl = BRL(-1 - NT);
    v = (__mul24(NT - 1 - x, l) + __mul24(x + 1, tr) + __mul24(NT - 1 - y, t) + __mul24(y + 1, bl) + NT) >> (LOG2 + 1);   /* (24-bit multiplies: full rate) */
  } else if (cls == 1) {        /* DC (intrapred.h:288-310, 378-392) */
    int s_ = (lane >= Z - NT && lane <= Z + NT && lane != Z) ? (int)bv : 0;
    s_ += __builtin_amdgcn_update_dpp(0, s_, 0xB1, 0xF, 0xF, false);     /* quad_perm [1,0,3,2] */
    s_ += __builtin_amdgcn_update_dpp(0, s_, 0x4E, 0xF, 0xF, false);     /* quad_perm [2,3,0,1] */
    s_ += __builtin_amdgcn_update_dpp(0, s_, 0x141, 0xF, 0xF, false);    /* row_half_mirror */
    s_ += __builtin_amdgcn_update_dpp(0, s_, 0x140, 0xF, 0xF, false);    /* row_mirror: every lane of a row of 16 holds the row's sum */
    int sum = __builtin_amdgcn_readlane(s_, 0) + __builtin_amdgcn_readlane(s_, 16);
    const int dc = (sum + NT) >> (LOG2 + 1);
    v = dc;
    if (bfilt) {
      const int eb = BRP(y == 0 ? x + 1 : -y - 1), e2c = BRL(-1) + BRL(1);
      if (x == 0 || y == 0) v = (eb + 3 * dc + 2) >> 2;
      if (lane == 0) v = (e2c + 2 * dc + 2) >> 2;
    }
  } else {                      /* pure horizontal / vertical (intrapred.h:330-433 with intraPredAngle 0) */
    const int l = BRP(-1 - y), t = BRP(1 + x), corner = BRL(0), first = vert ? BRL(1) : BRL(-1);
    v = vert ? t : l;
    if (bfilt && (vert ? x == 0 : y == 0)) v = d_clip3(0, pix_max, first + (((vert ? l : t) - corner) >> 1));
  }
#undef BRL
#undef BRP
  return v;
}

/* 16x16 / 32x32: intra_prediction_sample_filtering (intrapred.h:185-258) of the border in raw[] into pf[] (entry index = i + 2nT; the
   caller makes raw[] visible to the wave before and pf[] behind) */
__device__ __forceinline__ void d_intra_big_filter(const uint16_t* raw, uint16_t* pf, const uint32_t e0, const int nT, const int thr_strong)
{
  const int lane = threadIdx.x & 63;
  const int nEnt = 4 * nT + 1, Z = 2 * nT;
  const bool bi = (e0 & M355_IBX_STRONG) && d_abs((int)raw[Z] + raw[Z + 64] - 2 * raw[Z + 32]) < thr_strong && d_abs((int)raw[Z] + raw[Z - 64] - 2 * raw[Z - 32]) < thr_strong;
#pragma unroll
  for (int q = 0; q < 3; q++) {
    if (64 * q >= nEnt) continue;
    const int e = lane + 64 * q;
    if (e < nEnt) {
      const int i = e - Z;
      int v;
      if (i == -Z || i == Z) v = raw[e];
      else if (bi) {
        if (i == 0) v = raw[Z];
        else if (i < 0) v = raw[Z] + (((-i) * ((int)raw[Z - 64] - raw[Z]) + 32) >> 6);
        else v = raw[Z] + ((i * ((int)raw[Z + 64] - raw[Z]) + 32) >> 6);
      } else v = (raw[e + 1] + 2 * raw[e] + raw[e - 1] + 2) >> 2;
      pf[e] = (uint16_t)v;
    }
  }
}

#define M355_BRD(i) ((int)P[(i) + Z])
/* the DC value of a 16x16 / 32x32 block (every lane calls) */
__device__ __forceinline__ int d_intra_big_dc(const uint16_t* P, const int nT, const int log2)
{
  const int lane = threadIdx.x & 63, Z = 2 * nT;
  int s_ = 0;
  if (lane < nT) s_ = M355_BRD(lane + 1) + M355_BRD(-lane - 1);
  s_ += __builtin_amdgcn_update_dpp(0, s_, 0xB1, 0xF, 0xF, false);     /* sums over rows of 16 lanes, as in the 4x4 / 8x8 path */
  s_ += __builtin_amdgcn_update_dpp(0, s_, 0x4E, 0xF, 0xF, false);
  s_ += __builtin_amdgcn_update_dpp(0, s_, 0x141, 0xF, 0xF, false);
  s_ += __builtin_amdgcn_update_dpp(0, s_, 0x140, 0xF, 0xF, false);
  return (__builtin_amdgcn_readlane(s_, 0) + __builtin_amdgcn_readlane(s_, 16) + nT) >> (log2 + 1);
}
/* what a lane's samples of a 16x16 / 32x32 block share (its column x is the same in every pass) */
struct IntraBigFixed { int t_x, u_tr, u_bl, u_c, u_f, u_e2; };
template <int CLS>
__device__ __forceinline__ IntraBigFixed d_intra_big_fixed(const uint16_t* P, const int nT, const int x, const bool vert)
{
  const int Z = 2 * nT;
  IntraBigFixed f;
  f.t_x = (CLS == 0 || CLS == 2) ? M355_BRD(1 + x) : 0;
  f.u_tr = CLS == 0 ? M355_BRD(1 + nT) : 0; f.u_bl = CLS == 0 ? M355_BRD(-1 - nT) : 0;
  f.u_c = CLS == 2 ? M355_BRD(0) : 0; f.u_f = CLS == 2 ? (vert ? M355_BRD(1) : M355_BRD(-1)) : 0;
  f.u_e2 = CLS == 1 ? M355_BRD(-1) + M355_BRD(1) : 0;
  return f;
}
/* the border taps of sample (x, y): ta, tb and the weight fa of the second one (angular) */
template <int CLS>
__device__ __forceinline__ void d_intra_big_taps(const uint16_t* P, const int nT, const int x, const int y, const bool vert, const int angle, const int inv, int& ta, int& tb, int& fa)
{
  const int Z = 2 * nT;
  fa = 0; tb = 0;
  if (CLS == 0 || CLS == 2) ta = M355_BRD(-1 - y);
  else if (CLS == 1) ta = M355_BRD(y == 0 ? x + 1 : -y - 1);
  else {
    const int a_ = vert ? y : x, b_ = vert ? x : y;
    const int tt = __mul24(a_ + 1, angle), iIdx = tt >> 5;
    fa = tt & 31;
    const int x1 = b_ + iIdx + 1, x2 = x1 + 1;
    int i1, i2;
    if (CLS == 3) { i1 = vert ? x1 : -x1; i2 = vert ? x2 : -x2; }
    else {
      const int p1 = (__mul24(x1, inv) + 128) >> 8, p2 = (__mul24(x2, inv) + 128) >> 8;
      i1 = x1 >= 0 ? x1 : -p1; i2 = x2 >= 0 ? x2 : -p2;
      if (!vert) { i1 = -i1; i2 = -i2; }
    }
    ta = M355_BRD(i1); tb = M355_BRD(fa ? i2 : i1);   /* (no read beyond the border when the second tap has weight 0) */
  }
}
#undef M355_BRD
/* ... and the predicted sample (no residual yet) */
template <int CLS>
__device__ __forceinline__ int d_intra_big_value(const IntraBigFixed& f, const int nT, const int log2, const int x, const int y, const bool vert, const bool bfilt, const int dcVal, const int pix_max, const int ta, const int tb, const int fa)
{
  int v;
  if (CLS == 0) v = (__mul24(nT - 1 - x, ta) + __mul24(x + 1, f.u_tr) + __mul24(nT - 1 - y, f.t_x) + __mul24(y + 1, f.u_bl) + nT) >> (log2 + 1);
  else if (CLS == 1) {
    v = dcVal;
    if (bfilt) {
      if (x == 0 || y == 0) v = (ta + 3 * dcVal + 2) >> 2;
      if (x == 0 && y == 0) v = (f.u_e2 + 2 * dcVal + 2) >> 2;
    }
  } else if (CLS == 2) {
    v = vert ? f.t_x : ta;
    if (bfilt && (vert ? x == 0 : y == 0)) v = d_clip3(0, pix_max, f.u_f + (((vert ? ta : f.t_x) - f.u_c) >> 1));
  } else v = (32 * ta + __mul24(fa, tb - ta) + 16) >> 5;
  return v;
}

#endif
