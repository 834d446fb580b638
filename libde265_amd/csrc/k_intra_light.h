/*
 * k_intra_light.h — the LIGHT path of an inter picture's intra stage: one WAVE per (CTB, colour component) for the CTBs that take no part in a
 * cross-CTB intra dependency (runtime_upload.hip: the work items behind DevPic.n_intra_heavy; eight in ten of an 8K inter picture's).
 *
 * Such a CTB's blocks read only samples that the preceding kernels of the stream have finished, and samples of the CTB's own blocks.  So nothing of
 * k_intra's cross-CTB machinery is needed — no ticket, no granules, no halo staging, no poll — and the CTB's body need not live in LDS either:
 *   - the wave walks its component's blocks in the order of the CTB's sorted run (level by level: producers precede their readers);
 *   - a block's border is gathered STRAIGHT FROM THE PICTURE through the block's plan (k_intra_plan.h): a plan entry is an element index into the CTB
 *     workgroup's LDS array, and that index is position-based — it decodes to a picture coordinate (body or halo) or to the constant cell;
 *   - the residual comes from the residual buffer, the block's samples go straight to the picture;
 *   - a later block of the wave may read what an earlier one stored: the stores are drained before the next gather, and the gather uses agent-scope
 *     relaxed loads (served by the L2 — the CU's L1 is not refreshed by stores).
 * Components never read each other here, so the items of one CTB share nothing: no barrier, wave_sync only.  The block arithmetic is k_intra_block.h's,
 * the same definition the CTB workgroups run.  LDS per wave: the gathered and the smoothed border of a 16x16 / 32x32 block (the caller's arrays).
 */
#ifndef M355_K_INTRA_LIGHT_H
#define M355_K_INTRA_LIGHT_H
#include "k_common.h"
#include "k_intra_plan.h"
#include "k_intra_block.h"

/* the sample behind plan entry `code` of a block of the CTB at (x0c, y0c): body -> inside the CTB, halo -> the row above / the column on the left,
   else the constant cell.  (Coordinates are clamped into the plane: an available entry lies inside the picture, intrapred.h:534-633.) */
template <class PIX, int CF>
__device__ __forceinline__ uint32_t d_light_gather(const PIX* plane, const int stride, const int pw, const int ph, const int x0c, const int y0c, const int cs, const uint32_t code, const uint32_t cval)
{
  constexpr int PITCH_L = BODY_PITCH_OF(MAXCTB), PITCH_C = BODY_PITCH_OF(IntraGeo<CF>::CW_C);
  const int HALO_BASE = cs == 0 ? IntraGeo<CF>::BODY_L : IntraGeo<CF>::BODY_C;
  int sx, sy;
  bool konst = false;
  if ((int)code < HALO_BASE) {
    sy = cs == 0 ? (int)(code / (uint32_t)PITCH_L) : (int)(code / (uint32_t)PITCH_C);
    sx = (int)code - sy * (cs == 0 ? PITCH_L : PITCH_C) - BODY_X0;
  } else if ((int)code < HALO_BASE + HALO_TOP_N) { sy = -1; sx = (int)code - HALO_BASE - 1; }
  else if ((int)code < HALO_BASE + HALO_N) { sx = -1; sy = (int)code - HALO_BASE - HALO_TOP_N; }
  else { konst = true; sx = sy = 0; }
  const int x = min(max(x0c + sx, 0), pw - 1), y = min(max(y0c + sy, 0), ph - 1);
  const uint32_t v = (uint32_t)__hip_atomic_load(plane + (size_t)y * stride + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return konst ? cval : v;
}

/* light item `slot` of the picture (DevPic.intra_light), run by the calling wave; raw / pf: 4 * 32 + 8 elements of LDS each, the wave's own */
template <class PIX, int CF>
__device__ __forceinline__ void k_intra_light_item(const DevPic& p, const int slot, uint16_t* raw, uint16_t* pf)
{
  const int lane = threadIdx.x & 63;
  if (slot >= p.n_intra_light) return;                       /* (wave-uniform) */
  /* the item (runtime_upload.hip): one 16-byte scalar load carries what the CTB's descriptor would have to be fetched for */
  const uint4 it = p.intra_light[slot];
  const int ctb = __builtin_amdgcn_readfirstlane((int)(it.x & 0x3FFFFFFFu)), c = __builtin_amdgcn_readfirstlane((int)(it.x >> 30));
  const uint32_t ib_first = (uint32_t)__builtin_amdgcn_readfirstlane((int)it.y), ib_n = (uint32_t)__builtin_amdgcn_readfirstlane((int)it.z);
  const uint32_t plan_base = (uint32_t)__builtin_amdgcn_readfirstlane((int)it.w);
  const int ctbX = ctb % p.ctbW, ctbY = ctb / p.ctbW;
  const int l2c = p.pp.log2_ctb_size;
  const int csw = c ? (p.sw == 2) : 0, csh = c ? (p.sh == 2) : 0;
  const int x0c = (ctbX << l2c) >> csw, y0c = (ctbY << l2c) >> csh;
  const int bd = c ? p.pp.bit_depth_chroma : p.pp.bit_depth_luma;
  PIX* plane = (PIX*)p.plane[c];
  const int stride = p.stride[c], pw = p.pw[c], ph = p.ph[c];
  const int thr_strong = 1 << (p.pp.bit_depth_luma - 5);
  const int pix_max = (1 << bd) - 1;
  const uint32_t cval = 1u << (bd - 1);                      /* the constant cell: what a border is made of when nothing is available */

  /* the CTB's exec records from the component's first block to its last one, 64 at a time (one per lane); the wave's blocks are those of its component */
  for (uint32_t kbase = 0; kbase < ib_n; kbase += 64) {
    const int nvalid = (int)min(64u, ib_n - kbase);
    uint4 ex = make_uint4(0, 0, 0, 0);
    if (lane < nvalid) ex = ((const uint4*)p.ib_aux)[ib_first + kbase + lane];
    unsigned long long mine = __ballot((int)(lane < nvalid && ((ex.x >> 17) & 3u) == (uint32_t)c));
    while (mine) {
      const int src = __ffsll(mine) - 1;
      mine &= mine - 1;
      const uint32_t e0 = (uint32_t)__builtin_amdgcn_readlane((int)ex.x, src), e1 = (uint32_t)__builtin_amdgcn_readlane((int)ex.y, src);
      const uint32_t e2 = (uint32_t)__builtin_amdgcn_readlane((int)ex.z, src), e3 = (uint32_t)__builtin_amdgcn_readlane((int)ex.w, src);
      const int log2 = (int)((e0 >> 14) & 7u), nT = 1 << log2;
      const int lx = (int)(e0 & 127u), ly = (int)((e0 >> 7) & 127u);
      const int cls = (int)((e2 >> 8) & 7u), angle = (int)(int8_t)(e2 & 0xFFu), inv = (int)(int16_t)(e2 >> 16);
      const int mode = (int)((e0 >> 19) & 63u);
      const bool vert = mode >= 18;
      const bool has_res = (e0 & M355_IBX_HAS_RES) != 0, bfilt = (e0 & M355_IBX_BFILT) != 0;
      const int bx = x0c + lx, by = y0c + ly;                /* the block in the plane */
      PIX* const dst = plane + (size_t)by * stride + bx;
      const uint16_t* pl = p.iplan + plan_base + (e3 & 0xFFFFu);
      /* a sample of the block goes to the picture (a block lies inside it: the test costs nothing and keeps a bad record harmless) */
      auto put = [&](int x, int y, int v) { if (bx + x < pw && by + y < ph) dst[(size_t)y * stride + x] = (PIX)v; };

      if (e0 & M355_IBX_PCM) {                               /* raw block (slice.cc:4211-4255) */
        for (int o = lane; o < nT * nT; o += 64) put(o & (nT - 1), o >> log2, (int)p.pcm[e1 + o]);
      } else if (log2 <= 3) {
        /* ---- 4x4 / 8x8: border entry e in lane e of one register, one sample per lane (lane = y * nT + x) ---- */
        const uint32_t code = pl[min(lane, 4 << log2)];
        const uint32_t bv = d_light_gather<PIX, CF>(plane, stride, pw, ph, x0c, y0c, c, code, cval);
        const bool inb = lane < nT * nT;
        const int rs = (has_res && inb) ? (int)p.resbuf[e1 + lane] : 0;
        int v = log2 == 2 ? d_intra_small_predict<2>(bv, e0, cls, angle, inv, vert, bfilt, pix_max) : d_intra_small_predict<3>(bv, e0, cls, angle, inv, vert, bfilt, pix_max);
        v = d_clip3(0, pix_max, v + rs);
        if (inb) put(lane & (nT - 1), lane >> log2, v);
      } else {
        /* ---- 16x16 / 32x32: the border lives in LDS (65 / 129 entries), all of it requested at once ---- */
        const int nEnt = 4 * nT + 1;
        uint32_t cd[3] = {0, 0, 0}, val[3] = {0, 0, 0};
#pragma unroll
        for (int q = 0; q < 3; q++) {
          if (64 * q >= nEnt) continue;                      /* wave-uniform */
          cd[q] = (uint32_t)pl[min(lane + 64 * q, nEnt - 1)];
        }
#pragma unroll
        for (int q = 0; q < 3; q++) {
          if (64 * q >= nEnt) continue;
          val[q] = d_light_gather<PIX, CF>(plane, stride, pw, ph, x0c, y0c, c, cd[q], cval);
        }
#pragma unroll
        for (int q = 0; q < 3; q++) {
          if (64 * q >= nEnt) continue;
          if (lane + 64 * q < nEnt) raw[lane + 64 * q] = (uint16_t)val[q];
        }
        wave_sync();
        const uint16_t* P = raw;                             /* border in use, entry index = i + 2nT */
        if (e0 & M355_IBX_FILT) {
          d_intra_big_filter(raw, pf, e0, nT, thr_strong);
          wave_sync();
          P = pf;
        }
        const int dcVal = mode == 1 ? d_intra_big_dc(P, nT, log2) : 0;
        const int x = lane & (nT - 1), yb = lane >> log2, ystep = 64 >> log2, nPass = (nT * nT) >> 6;      /* a pass = 64 samples = 4 / 2 whole rows */
        const int16_t* res = p.resbuf + e1;
        /* one loop per mode class, four samples per lane in flight: their border taps and residuals are requested together */
        auto big_loop = [&](auto cls_) {
          constexpr int CLS = decltype(cls_)::value;
          const IntraBigFixed fx = d_intra_big_fixed<CLS>(P, nT, x, vert);
          for (int it0 = 0; it0 < nPass; it0 += 4) {         /* (nPass is 4 or 16) */
            int ta[4], tb[4], fa[4], rs[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
              const int y = yb + (it0 + u) * ystep;
              d_intra_big_taps<CLS>(P, nT, x, y, vert, angle, inv, ta[u], tb[u], fa[u]);
              rs[u] = has_res ? (int)res[y * nT + x] : 0;
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
              const int y = yb + (it0 + u) * ystep;
              int v = d_intra_big_value<CLS>(fx, nT, log2, x, y, vert, bfilt, dcVal, pix_max, ta[u], tb[u], fa[u]);
              put(x, y, d_clip3(0, pix_max, v + rs[u]));
            }
          }
        };
        if (cls == 0) big_loop(std::integral_constant<int, 0>());
        else if (cls == 1) big_loop(std::integral_constant<int, 1>());
        else if (cls == 2) big_loop(std::integral_constant<int, 2>());
        else if (cls == 3) big_loop(std::integral_constant<int, 3>());
        else big_loop(std::integral_constant<int, 4>());
        wave_sync();                                         /* raw[] / pf[] are the next block's */
      }
      /* the block's samples are in the L2 before the next block's border is gathered */
      if (mine || kbase + 64 < ib_n) d_drain_vmem();
    }
  }
}

#endif
