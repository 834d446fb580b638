/*
 * k_stats.hip — what is IN a device frame (or a rectangle of it), measured where it lies (m355_frame_stats_async, include/de265_mi355x.h): per
 * plane a 256-bin histogram of the samples' top eight bits, min, max, sum and sum of squares; the box around the luma samples above a
 * threshold and their number; and, on request, the same for the light level m = max(R, G, B) of every pixel's 16-bit R'G'B'.  All integer.
 *
 * ONE launch per request.  The work is cut into PARTS that whole workgroups take (k_stats.h): the rectangle on plane 0, 1 and 2, each walked as
 * k_measure_req walks it — a lane takes 16 bytes of a row per step, a wavefront 1 KB (a UNIT: one chunk of one row), the lane at the end of a
 * row loads its valid bytes one by one, so nothing beyond the row is read.  With light == 1 the part of plane 0 is the LIGHT part instead: per
 * unit a lane loads what k_export_rgb loads for the pixels behind its luma vector (d_rgb_load of k_rgb_dev.h: the luma vector and one 16-byte
 * vector per chroma row the filter reads — that file argues why these stay inside the plane's allocation), reconstructs chroma with the
 * export's filter (d_rgb_chroma; siting type and chroma format are template parameters), applies the export's matrix (d_rgb_pixel, the
 * coefficients of m355_rgb_coefficients for M355_RGB_U16) and keeps max(R, G, B); no R'G'B' sample passes through memory.  It holds the luma
 * vector anyway, so it takes plane 0's statistics along and luma is read once.  A wavefront takes `units_per_wave` CONSECUTIVE units — the host
 * sizes that for about STATS_TARGET_WAVES wavefronts per launch — and issues the loads of the next unit before it works on the current one;
 * every loop bound is wave-uniform (a lane beyond the row's end takes part with n = 0), so the wave collectives below are reached by all 64 lanes.
 *
 * THE HISTOGRAM.  Every wavefront has histograms OF ITS OWN in LDS (16 wavefronts x {plane, light} x 256 words = 32 KB per workgroup), filled
 * with LDS atomics: sixteen replicated sub-histograms selected by wavefront, so wavefronts never contend.  Constant and near-constant planes
 * (black frames, fades, flat chroma) would still put 64 lanes x 16 samples on one LDS word.  Equal bins are therefore combined BEFORE the
 * atomic, at two levels that cost one comparison each because min and max of the vector are computed anyway:
 *   - a lane whose vector falls into one bin (min >> shift == max >> shift) adds its sample count with ONE atomic;
 *   - a wavefront whose 64 full vectors all fall into the bin of lane 0 (one vote) adds 64 * NP from one lane.
 * A constant plane is one LDS atomic per KB, a smooth gradient about one per lane and step, and only vectors that straddle bins fall back to
 * one atomic per sample.  Chosen over match-any within the wave (several rounds of votes for the random case, where nothing is gained) and
 * over sub-histograms selected by lane (64 lanes of a constant plane would still meet on a few words; more LDS per workgroup).
 * At the end a workgroup adds its sixteen copies and flushes NON-ZERO bins only into the slot's device record, one agent-scope atomic each:
 * thread t < 512 owns bin t & 255 of histogram t >> 8.
 *
 * RANGES of the 32-bit partial sums.  They cover ONE vector of one lane and are added to 64-bit sums of the lane right behind it:
 *   8-bit planes:  sum <= 16 * 255 = 4080; sum of squares <= 16 * 255^2 = 1 040 400.
 *   16-bit planes: sum <= 8 * 65535 = 524 280; a square, 65535^2 = 4 294 836 225, fits 32 bits, two of them do not: every square is added to
 *     the 64-bit sum by itself.
 *   light: m <= 65535, sum of a vector <= 16 * 65535 = 1 048 560.
 *   counts: a lane's count of samples above `black` and every histogram bin are 32-bit: a launch has at most 16384 * 16384 = 2^28 samples per plane.
 * The 64-bit sums hold 2^28 samples of the largest square (2^60).
 *
 * WHERE THE VALUES GO — k_measure_req's argument, for this record (k_stats.h: 1052 words of 32 bits, the 64-bit sums on even indices).  Every
 * quantity's neutral value is 0 — minima are gathered as max of ~s, the box as max of ~x0, ~y0, x1 + 1, y1 + 1 —, so an atomic whose operand is
 * neutral is left out, no fill precedes a launch and a reused slot is clean.  ONE set of atomics and ONE arrival ticket PER WORKGROUP, and
 * workgroups of 1024 threads, about one per CU: every agent-scope atomic of a launch meets all the others on the same few words, where they are
 * performed one after the other.  Measured (profiles/stats_rate.txt names the final figures): with a ticket and a set of scalar atomics per
 * WAVEFRONT a planes-only request of an 8K frame took 0.38 ms at 4140 wavefronts and 0.63 ms at 8280; per workgroup of 16 it takes 0.074 ms.
 * Behind the workgroup's barrier the flushing wavefronts issue their bins' atomics, every wavefront reduces its scalars across its lanes into
 * LDS and waits for its own atomics (s_waitcnt vmcnt(0)); behind a second barrier thread 0 adds the sixteen wavefronts' scalars, issues their
 * atomics, waits for them and draws the ticket (fetch_add, acquire-release at agent scope): everything the workgroup added has been performed
 * before its ticket is visible.  The workgroup that draws the last ticket synchronises with every earlier one; ALL ITS THREADS move the record
 * with atomicExch(..., 0) — complete value out, zero in — into the pinned record, thread 0 zeroes the counter and writes the verdict.  Nobody
 * else touches the record in this launch, and the slot's next launch is enqueued only after the host has collected this one.
 * A GATED launch (the decode that wrote the frame was rejected) writes the verdict "no value" from one lane and reads nothing.
 *
 * Roofline: pure traffic — every byte of the rectangle read once (99.5 MB for an 8K 10-bit 4:2:0 frame; light == 1 reads chroma rows twice, as
 * the export does) — with about 12 VALU issues and at most one LDS atomic per sample.  MEASURED (tools/stats_rate.py, profiles/stats_rate.txt,
 * per request, host clock around sixteen back to back): planes only 0.074 ms for random content = 1.3 TB/s of frame bytes, 0.27 of the box's
 * copy rate, and 0.26 of the time of the comparison request that reads twice the bytes (yardstick met); a constant frame 0.060 ms.  With
 * light == 1: 0.123 ms random, 0.097 ms constant against 0.070 ms of m355_frame_export_rgb_opts (packed U16) of the same frame: that YARDSTICK
 * IS MISSED by a factor of 1.4 to 1.8, although the request stores nothing.  Supposed cause, NOT measured (no counter run, no trace): the
 * export is 64 800 independent wavefronts that load, convert and store once, at up to 8 per SIMD; a LIGHT wavefront holds the next unit's five
 * vectors beside the current one's (98 to 102 VGPRs: 4 to 5 wavefronts per SIMD), walks its units one after the other, ends each in up to 2 x
 * 8 LDS atomics, and the launch ends in a tail where the last workgroups flush and the last one moves the record.
 */
#include "k_common.h"
#include "k_stats.h"
#include "k_rgb_dev.h"

static_assert(STATS_BLOCK >= 512, "the flush maps thread t < 512 to bin t & 255 of histogram t >> 8");

__device__ __forceinline__ unsigned long long d_stats_add64(unsigned long long v)
{
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}
__device__ __forceinline__ unsigned d_stats_add32(unsigned v)
{
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}
__device__ __forceinline__ unsigned d_stats_min32(unsigned v)
{
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) { const unsigned o = __shfl_xor(v, m, 64); v = o < v ? o : v; }
  return v;
}
__device__ __forceinline__ unsigned d_stats_max32(unsigned v)
{
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) { const unsigned o = __shfl_xor(v, m, 64); v = o > v ? o : v; }
  return v;
}

/* the first n (1..16) bytes at p, the rest 0: nothing beyond the row is read */
__device__ __forceinline__ void d_stats_load(const M355_GLOBAL uint8_t* p, int n, unsigned w[4])
{
  if (n >= 16) { d_ldg16(p, w); return; }
  w[0] = w[1] = w[2] = w[3] = 0;
  for (int k = 0; k < n; k++) w[k >> 2] |= (unsigned)p[k] << (8 * (k & 3));
}

/* what a lane gathers over its units: of a plane's samples, or of the light values */
struct StatsAcc {
  unsigned long long sum = 0, sq = 0;
  unsigned mn = 0xFFFFFFFFu, mx = 0;
};
/* ... and of the luma samples above `black`: their number, x0, y0 and x1 + 1, y1 + 1 in frame coordinates */
struct StatsBox {
  unsigned n = 0, x0 = 0xFFFFFFFFu, y0 = 0xFFFFFFFFu, x1 = 0, y1 = 0;
};

/* n values with bins lo .. hi (of the n valid ones) into the wavefront's histogram h; b[k] = bin of value k.  Reached by all 64 lanes (n = 0: a
   lane beyond the row's end) */
template <int NP>
__device__ __forceinline__ void d_stats_hist(const unsigned* b, int n, unsigned lo, unsigned hi, unsigned* h, int lane)
{
  const unsigned b0 = __builtin_amdgcn_readfirstlane(lo);
  if (__all(n == NP && lo == hi && lo == b0)) {                 /* 64 full vectors in one bin */
    if (lane == 0) atomicAdd(&h[b0], 64u * NP);
    return;
  }
  if (n > 0 && lo == hi) atomicAdd(&h[lo], (unsigned)n);        /* this lane's vector in one bin */
  else {
#pragma unroll
    for (int k = 0; k < NP; k++) if (k < n) atomicAdd(&h[b[k]], 1u);
  }
}

/* the n (0 .. NP) leading samples of the vector w: sums, min, max, histogram; luma: the samples above `black` at (x + k, y) */
template <int SB>
__device__ __forceinline__ void d_stats_vec(const unsigned w[4], int n, unsigned shift, StatsAcc& acc, unsigned* h, int lane, bool luma, unsigned black,
                                            unsigned x, unsigned y, StatsBox& box)
{
  constexpr int NP = 16 / SB;
  unsigned s32 = 0, q32 = 0, mn = 0xFFFFFFFFu, mx = 0, b[NP];
  unsigned long long q64 = 0;
  bool any = false;
#pragma unroll
  for (int k = 0; k < NP; k++) {
    const unsigned s = (unsigned)d_rgb_sample<SB>(w, k);
    b[k] = s >> shift;
    if (k < n) {
      s32 += s;
      if (SB == 1) q32 += s * s;
      else q64 += (unsigned long long)s * s;
      mn = min(mn, s); mx = max(mx, s);
      if (luma && s > black) {
        any = true;
        box.n++;
        box.x0 = min(box.x0, x + (unsigned)k); box.x1 = max(box.x1, x + (unsigned)k + 1u);
      }
    }
  }
  acc.sum += s32;
  acc.sq += SB == 1 ? (unsigned long long)q32 : q64;
  acc.mn = min(acc.mn, mn); acc.mx = max(acc.mx, mx);
  if (any) { box.y0 = min(box.y0, y); box.y1 = max(box.y1, y + 1u); }
  d_stats_hist<NP>(b, n, mn >> shift, mx >> shift, h, lane);
}

/* what a wavefront leaves in LDS for the workgroup's one set of atomics: its lanes' values reduced (plain data: __shared__ takes no initialisers) */
struct StatsWave {
  unsigned long long sum, sq, lsum;
  unsigned mn, mx, lmn, lmx, bn, bx0, by0, bx1, by1;
};

template <int SB, int CF, int LOC, bool LIGHT>
__global__ void __launch_bounds__(STATS_BLOCK) k_stats_req(StatsArgs a, StatsReq q)
{
  if (q.timeout[1] == q.epoch) {                                /* M355_GATE, with the verdict */
    if (blockIdx.x == 0 && threadIdx.x == 0) { q.res[STATS_ARRIVED + 1] = q.seq; q.res[STATS_ARRIVED] = STATS_RES_GATED; }
    return;
  }
  constexpr int NP = 16 / SB;
  __shared__ unsigned s_hist[STATS_WAVES][2][256];
  __shared__ StatsWave s_wave[STATS_WAVES];
  __shared__ unsigned s_last;
  for (int i = threadIdx.x; i < STATS_WAVES * 2 * 256; i += STATS_BLOCK) (&s_hist[0][0][0])[i] = 0u;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const uint32_t wv = __builtin_amdgcn_readfirstlane((uint32_t)(threadIdx.x >> 6));
  const uint32_t wg = blockIdx.x;
  const int c = wg >= a.part[2].first_wg ? 2 : (wg >= a.part[1].first_wg ? 1 : 0);   /* (a part that does not exist starts at n_wg) */
  const StatsPart pt = a.part[c];
  const bool light_part = LIGHT && c == 0;
  /* this wavefront's units u0 .. u1 - 1 (none: the last workgroup of a part may have idle wavefronts; they still take part in the barriers) */
  const uint32_t wip = (wg - pt.first_wg) * STATS_WAVES + wv;
  const uint32_t u0 = min(wip * pt.units_per_wave, pt.units), u1 = min(u0 + pt.units_per_wave, pt.units);
  uint32_t row = pt.chunks ? u0 / pt.chunks : 0u, chunk = pt.chunks ? u0 - row * pt.chunks : 0u;
  unsigned* h = s_hist[wv][0];
  StatsAcc acc, lacc;
  StatsBox box;
  if (light_part) {
    if constexpr (LIGHT) {
      unsigned* hl = s_hist[wv][1];
      const RgbMatrix m = d_rgb_matrix_of(a.k);
      /* the loads of unit u + 1 are issued before unit u is worked on: a wavefront always has a unit in flight */
      const auto fetch = [&](uint32_t r, uint32_t ck, RgbLane<SB, CF, LOC>& l) -> int {
        const uint32_t p0 = (ck * 64u + (uint32_t)lane) * NP;
        const int n = p0 < a.width ? (int)min((uint32_t)NP, a.width - p0) : 0;
        l.ry[0] = l.ry[1] = l.ry[2] = l.ry[3] = 0u;
        if (n > 0) d_rgb_load<SB, CF, LOC>(a, a.x0 + p0, a.y0 + r, l);
        return n;
      };
      RgbLane<SB, CF, LOC> ln;
      int nn = u0 < u1 ? fetch(row, chunk, ln) : 0;
      for (uint32_t u = u0; u < u1; u++) {
        const RgbLane<SB, CF, LOC> l = ln;
        const int n = nn;
        const uint32_t p0 = (chunk * 64u + (uint32_t)lane) * NP, y = row;
        if (++chunk == pt.chunks) { chunk = 0u; row++; }
        if (u + 1 < u1) nn = fetch(row, chunk, ln);
        unsigned mb[NP], s32 = 0, mn = 0xFFFFFFFFu, mx = 0;
        if (n > 0) {
          int cu[NP], cv[NP];
          if (CF != 0) {
            d_rgb_chroma<SB, CF, LOC>(l.rc[0][0], l.rc[0][1], l.last, m.c0, cu, l.yodd, l.lead);
            d_rgb_chroma<SB, CF, LOC>(l.rc[1][0], l.rc[1][1], l.last, m.c0, cv, l.yodd, l.lead);
          }
#pragma unroll
          for (int k = 0; k < NP; k++) {
            unsigned R, G, B;
            d_rgb_pixel<CF>(m, d_rgb_sample<SB>(l.ry, k), CF != 0 ? cu[k] : 0, CF != 0 ? cv[k] : 0, 65535, R, G, B);
            const unsigned v = max(R, max(G, B));
            mb[k] = v >> 8;
            if (k < n) { s32 += v; mn = min(mn, v); mx = max(mx, v); }
          }
        } else {
#pragma unroll
          for (int k = 0; k < NP; k++) mb[k] = 0u;
        }
        lacc.sum += s32;
        lacc.mn = min(lacc.mn, mn); lacc.mx = max(lacc.mx, mx);
        d_stats_hist<NP>(mb, n, mn >> 8, mx >> 8, hl, lane);
        d_stats_vec<SB>(l.ry, n, pt.shift, acc, h, lane, true, a.black, a.px + p0, a.py + y, box);
      }
    }
  } else {
    const auto fetch = [&](uint32_t r, uint32_t ck, unsigned* w) -> int {
      const uint32_t o = (ck * 64u + (uint32_t)lane) * 16u;
      const int nb = o < pt.row_bytes ? (int)min(16u, pt.row_bytes - o) : 0;
      w[0] = w[1] = w[2] = w[3] = 0u;
      if (nb > 0) d_stats_load((const M355_GLOBAL uint8_t*)pt.p + (size_t)r * pt.pitch + o, nb, w);
      return nb;
    };
    unsigned wn[4];
    int nbn = u0 < u1 ? fetch(row, chunk, wn) : 0;
    for (uint32_t u = u0; u < u1; u++) {
      const unsigned w[4] = {wn[0], wn[1], wn[2], wn[3]};
      const int nb = nbn;
      const uint32_t o = (chunk * 64u + (uint32_t)lane) * 16u, y = row;
      if (++chunk == pt.chunks) { chunk = 0u; row++; }
      if (u + 1 < u1) nbn = fetch(row, chunk, wn);
      d_stats_vec<SB>(w, nb / SB, pt.shift, acc, h, lane, c == 0, a.black, a.px + o / SB, a.py + y, box);
    }
  }
  __syncthreads();                                              /* every wavefront's LDS atomics are in */
  if (threadIdx.x < 512) {                                      /* the histograms: thread t owns bin t & 255 of histogram t >> 8 */
    const int hi = threadIdx.x >> 8, bin = threadIdx.x & 255;
    if (hi == 0 || light_part) {
      unsigned v = 0;
#pragma unroll
      for (int w = 0; w < STATS_WAVES; w++) v += s_hist[w][hi][bin];
      if (v) atomicAdd(q.rec + STATS_HIST + 256 * (hi ? 3 : c) + bin, v);
    }
  }
  {                                                             /* the scalars: across the wavefront here, across the workgroup by thread 0 below */
    StatsWave r;
    r.sum = d_stats_add64(acc.sum); r.sq = d_stats_add64(acc.sq); r.lsum = d_stats_add64(lacc.sum);
    r.mn = d_stats_min32(acc.mn); r.mx = d_stats_max32(acc.mx); r.lmn = d_stats_min32(lacc.mn); r.lmx = d_stats_max32(lacc.mx);
    r.bn = d_stats_add32(box.n);
    r.bx0 = d_stats_min32(box.x0); r.by0 = d_stats_min32(box.y0); r.bx1 = d_stats_max32(box.x1); r.by1 = d_stats_max32(box.y1);
    if (lane == 0) s_wave[wv] = r;
  }
  d_drain_vmem();                                               /* this wavefront's flush has been performed ... */
  __syncthreads();                                              /* ... and so has every other's, before thread 0 goes on */
  if (threadIdx.x == 0) {
    StatsWave t = s_wave[0];
#pragma unroll 1
    for (int w = 1; w < STATS_WAVES; w++) {
      const StatsWave o = s_wave[w];
      t.sum += o.sum; t.sq += o.sq; t.lsum += o.lsum; t.bn += o.bn;
      t.mn = min(t.mn, o.mn); t.mx = max(t.mx, o.mx); t.lmn = min(t.lmn, o.lmn); t.lmx = max(t.lmx, o.lmx);
      t.bx0 = min(t.bx0, o.bx0); t.by0 = min(t.by0, o.by0); t.bx1 = max(t.bx1, o.bx1); t.by1 = max(t.by1, o.by1);
    }
    if (t.sum) atomicAdd((unsigned long long*)(q.rec + STATS_SUM + 2 * c), t.sum);
    if (t.sq) atomicAdd((unsigned long long*)(q.rec + STATS_SQ + 2 * c), t.sq);
    if (t.mn != 0xFFFFFFFFu) atomicMax(q.rec + STATS_MIN + c, ~t.mn);
    if (t.mx) atomicMax(q.rec + STATS_MAX + c, t.mx);
    if (t.bn) {                                                 /* (plane 0 only: nothing else counts) */
      atomicAdd((unsigned long long*)(q.rec + STATS_NACT), (unsigned long long)t.bn);
      atomicMax(q.rec + STATS_BOX + 0, ~t.bx0); atomicMax(q.rec + STATS_BOX + 1, ~t.by0);
      atomicMax(q.rec + STATS_BOX + 2, t.bx1); atomicMax(q.rec + STATS_BOX + 3, t.by1);
    }
    if (t.lsum) atomicAdd((unsigned long long*)(q.rec + STATS_SUM + 2 * 3), t.lsum);
    if (t.lmn != 0xFFFFFFFFu) atomicMax(q.rec + STATS_MIN + 3, ~t.lmn);
    if (t.lmx) atomicMax(q.rec + STATS_MAX + 3, t.lmx);
    d_drain_vmem();                                             /* the workgroup's atomics have been performed ... */
    __threadfence();                                            /* ... before the ticket can be seen */
    s_last = __hip_atomic_fetch_add(q.rec + STATS_ARRIVED, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) + 1u == a.n_wg ? 1u : 0u;
  }
  __syncthreads();
  if (!s_last) return;
  __threadfence();
  for (int i = threadIdx.x; i < STATS_VALUES; i += STATS_BLOCK) q.res[i] = atomicExch(q.rec + i, 0u);
  if (threadIdx.x != 0) return;
  __hip_atomic_store(q.rec + STATS_ARRIVED, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  q.res[STATS_ARRIVED + 1] = q.seq;
  q.res[STATS_ARRIVED] = STATS_RES_VALID;
}

void m355_launch_stats(const StatsArgs& a, const StatsReq& q, int bytes_per_sample, int light, int chroma_format, int chroma_loc, hipStream_t st)
{
  const dim3 grid(a.n_wg), block(STATS_BLOCK);
  if (!light) {
    if (bytes_per_sample == 1) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_stats_req<1, 0, 0, false>), grid, block, 0, st, a, q);
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_stats_req<2, 0, 0, false>), grid, block, 0, st, a, q);
    return;
  }
  const int loc = chroma_format == 1 ? chroma_loc : 0;          /* (the siting is 4:2:0's alone) */
#define M355_STATS_CF(SB, CF, LOC) \
  if (bytes_per_sample == SB && chroma_format == CF && loc == LOC) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_stats_req<SB, CF, LOC, true>), grid, block, 0, st, a, q);
#define M355_STATS_SB(SB) \
  M355_STATS_CF(SB, 0, 0) M355_STATS_CF(SB, 1, 0) M355_STATS_CF(SB, 2, 0) M355_STATS_CF(SB, 3, 0) M355_STATS_CF(SB, 1, 1) M355_STATS_CF(SB, 1, 2) M355_STATS_CF(SB, 1, 3)
  M355_STATS_SB(1) M355_STATS_SB(2)
#undef M355_STATS_SB
#undef M355_STATS_CF
}
