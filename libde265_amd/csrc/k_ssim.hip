/*
 * k_ssim.hip — the SSIM of a device frame (or a rectangle of it) against another picture in device-addressable memory, per plane, as
 * ssim_window.h defines it (m355_frame_ssim_async, include/de265_mi355x.h): valid 11 x 11 windows with integer Gaussian weights, five exact
 * 64-bit sums per window, the point in IEEE double without contraction, q in Q30.  Per plane sum q, the worst q, and optionally q of every
 * window into a map of the caller.
 *
 * ONE launch covers every selected plane.  One workgroup (SSIM_BLOCK threads) takes one tile of SSIM_TILE_W x SSIM_TILE_H windows of one plane:
 *   1. LOAD    the (TW + 10) x (TH + 10) samples of a and of b that the tile's windows cover, each once, into LDS (s_a, s_b; positions outside
 *              the plane read 0 — only windows that are not valid, and are dropped in step 3, would see them).
 *   2. ROWS    the horizontal 11-tap pass: for each of the TH + 10 rows and TW columns the row's five sums, into LDS.
 *              sum w a, sum w b <= 2^14 * 65535 < 2^30 fit 32 bits at every bit depth.  sum w a^2 (b^2, a b) <= 2^14 * 255^2 < 2^30 for 8-bit
 *              samples, <= 2^14 * 65535^2 < 2^46 for 16-bit ones: the template's SQ type is uint32_t / uint64_t.
 *   3. WINDOWS the vertical 11-tap pass over the row sums in 64 bits (the taps are symmetric: rows k and 10 - k are added first, which
 *              stays below 2^31 / 2^47, then six products), m355_ssim_point, the map store, and the thread's sum of q and max of 2^30 - q.
 *   4. REDUCE  across the wavefront by shuffles, across the workgroup's wavefronts through LDS; thread 0 issues one 64-bit atomic add
 *              (q summed as two's complement) and one atomic max per workgroup into the slot's device record, then draws the arrival ticket.
 * No intermediate value passes through global memory.
 *
 * LDS per workgroup: samples 2 x 42 x 42 elements, row sums 2 x 42 x 32 x 4 bytes + 3 x 42 x 32 x sizeof(SQ):
 *   8-bit 3528 + 10752 + 16128 = 30408 bytes, 16-bit 7056 + 10752 + 32256 = 50064 bytes, plus the reduction's 192: two workgroups of sixteen
 *   wavefronts fill a CU's 32 wavefront slots with either, on 61 / 100 KB of its 160 KiB.
 * profiles/ssim_codegen.txt has the compiler's resource lines (no scratch).
 *
 * WHERE THE VALUES GO: the argument written in k_measure.hip, with a workgroup in place of a wavefront as in k_stats.hip.  Every access to
 * q.rec is an agent-scope atomic read-modify-write; thread 0's accumulator atomics are sequenced before its ticket fetch_add (release +
 * acquire); the workgroup that draws the last ticket takes the values with atomicExch(..., 0), which leaves the device record zero for the
 * slot's next request, and writes the pinned record, which the host reads behind the request's mark only.  The map is written with plain
 * stores: every element belongs to one thread, nobody reads it on the device, and the end of the kernel releases it.
 * A GATED launch (a decode that wrote the frame or the reference frame was rejected) writes the verdict "no value" from one thread of its
 * first workgroup and touches nothing else — no sample is read, the map is not written, the device record stays zero.
 */
#include "k_common.h"
#include "k_ssim.h"
#include "ssim_window.h"

#define SSIM_SW (SSIM_TILE_W + 10)   /* samples per tile row */
#define SSIM_SH (SSIM_TILE_H + 10)

template <class T>
__device__ __forceinline__ T d_ssim_wave_add(T v)
{
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}
__device__ __forceinline__ unsigned d_ssim_wave_max(unsigned v)
{
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) { const unsigned o = __shfl_xor(v, m, 64); v = o > v ? o : v; }
  return v;
}

/* one workgroup per tile; workgroup index -> plane by the prefix counts in a.first[]; T: the planes' element type, SQ: see step 2 above */
template <class T, class SQ>
__global__ void __launch_bounds__(SSIM_BLOCK) k_ssim_req(SsimArgs a, SsimReq q)
{
  if (q.timeout[0][1] == q.epoch[0] || q.timeout[1][1] == q.epoch[1]) {      /* M355_GATE for either frame, with the verdict */
    if (blockIdx.x == 0 && threadIdx.x == 0) { q.res[7] = q.seq; q.res[6] = SSIM_RES_GATED; }
    return;
  }
  __shared__ T s_a[SSIM_SH][SSIM_SW], s_b[SSIM_SH][SSIM_SW];
  __shared__ uint32_t s_ma[SSIM_SH][SSIM_TILE_W], s_mb[SSIM_SH][SSIM_TILE_W];
  __shared__ SQ s_aa[SSIM_SH][SSIM_TILE_W], s_bb[SSIM_SH][SSIM_TILE_W], s_ab[SSIM_SH][SSIM_TILE_W];
  __shared__ long long s_sum[SSIM_BLOCK / 64];
  __shared__ unsigned s_worst[SSIM_BLOCK / 64];
  const uint32_t w[M355_SSIM_TAPS] = M355_SSIM_WEIGHTS;

  const int wg = blockIdx.x, t = threadIdx.x;
  const int c = wg >= a.first[2] ? 2 : (wg >= a.first[1] ? 1 : 0);
  const SsimPlane pl = a.pl[c];
  const int tile = wg - a.first[c];
  const int x0 = (tile % pl.tiles_x) * SSIM_TILE_W, y0 = (tile / pl.tiles_x) * SSIM_TILE_H;   /* the tile's first window = its first sample */

  /* 1. the samples: consecutive threads take consecutive samples of a row */
  for (int i = t; i < SSIM_SH * SSIM_SW; i += SSIM_BLOCK) {
    const int r = i / SSIM_SW, k = i - r * SSIM_SW;
    T va = 0, vb = 0;
    if (x0 + k < pl.pw && y0 + r < pl.ph) {
      va = *(const T*)(pl.a + (size_t)(y0 + r) * pl.pitch_a + (size_t)(x0 + k) * sizeof(T));
      vb = *(const T*)(pl.b + (size_t)(y0 + r) * pl.pitch_b + (size_t)(x0 + k) * sizeof(T));
    }
    s_a[r][k] = va; s_b[r][k] = vb;
  }
  __syncthreads();

  /* 2. the rows' sums */
  for (int i = t; i < SSIM_SH * SSIM_TILE_W; i += SSIM_BLOCK) {
    const int r = i / SSIM_TILE_W, k = i % SSIM_TILE_W;
    uint32_t ma = 0, mb = 0;
    SQ aa = 0, bb = 0, ab = 0;
#pragma unroll
    for (int j = 0; j < M355_SSIM_TAPS; j++) {
      const uint32_t va = s_a[r][k + j], vb = s_b[r][k + j];
      ma += w[j] * va; mb += w[j] * vb;
      aa += (SQ)w[j] * (va * va); bb += (SQ)w[j] * (vb * vb); ab += (SQ)w[j] * (va * vb);
    }
    s_ma[r][k] = ma; s_mb[r][k] = mb; s_aa[r][k] = aa; s_bb[r][k] = bb; s_ab[r][k] = ab;
  }
  __syncthreads();

  /* 3. the windows (every thread walks all its rounds: the reduction below is a collective) */
  const int nwx = pl.pw - 10, nwy = pl.ph - 10;
  long long sum = 0;
  unsigned worst = 0;
  for (int i = t; i < SSIM_TILE_H * SSIM_TILE_W; i += SSIM_BLOCK) {
    const int r = i / SSIM_TILE_W, k = i % SSIM_TILE_W;
    if (x0 + k >= nwx || y0 + r >= nwy) continue;
    unsigned long long MA = (unsigned long long)w[5] * s_ma[r + 5][k], MB = (unsigned long long)w[5] * s_mb[r + 5][k];
    unsigned long long SAA = (unsigned long long)w[5] * s_aa[r + 5][k], SBB = (unsigned long long)w[5] * s_bb[r + 5][k], SAB = (unsigned long long)w[5] * s_ab[r + 5][k];
#pragma unroll
    for (int j = 0; j < 5; j++) {
      MA += (unsigned long long)w[j] * (s_ma[r + j][k] + s_ma[r + 10 - j][k]);
      MB += (unsigned long long)w[j] * (s_mb[r + j][k] + s_mb[r + 10 - j][k]);
      SAA += (unsigned long long)w[j] * (SQ)(s_aa[r + j][k] + s_aa[r + 10 - j][k]);
      SBB += (unsigned long long)w[j] * (SQ)(s_bb[r + j][k] + s_bb[r + 10 - j][k]);
      SAB += (unsigned long long)w[j] * (SQ)(s_ab[r + j][k] + s_ab[r + 10 - j][k]);
    }
    const int32_t v = m355_ssim_point(MA, MB, SAA, SBB, SAB, pl.c1, pl.c2);
    if (pl.map) *(int32_t*)(pl.map + (size_t)(y0 + r) * pl.map_pitch + (size_t)(x0 + k) * 4) = v;
    sum += v;
    worst = max(worst, (unsigned)(M355_SSIM_ONE - v));
  }

  /* 4. one set of atomics and one arrival per workgroup */
  sum = d_ssim_wave_add(sum);
  worst = d_ssim_wave_max(worst);
  if ((t & 63) == 0) { s_sum[t >> 6] = sum; s_worst[t >> 6] = worst; }
  __syncthreads();
  if (t != 0) return;
  for (int k = 1; k < SSIM_BLOCK / 64; k++) { sum += s_sum[k]; worst = max(worst, s_worst[k]); }
  if (sum) atomicAdd(&q.rec[SSIM_SUM + c], (unsigned long long)sum);
  if (worst) atomicMax(&q.rec[SSIM_WORST + c], (unsigned long long)worst);
  const unsigned long long drawn = __hip_atomic_fetch_add(&q.rec[SSIM_REC_WORDS - 1], 1ull, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
  if (drawn + 1ull != (unsigned long long)a.first[3]) return;
  for (int i = 0; i < SSIM_VALUES; i++) q.res[i] = atomicExch(&q.rec[i], 0ull);
  __hip_atomic_store(&q.rec[SSIM_REC_WORDS - 1], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  q.res[7] = q.seq;
  q.res[6] = SSIM_RES_VALID;
}

void m355_launch_ssim(const SsimArgs& a, const SsimReq& q, int bytes_per_sample, hipStream_t st)
{
  if (bytes_per_sample == 1) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ssim_req<uint8_t, uint32_t>), dim3(a.first[3]), dim3(SSIM_BLOCK), 0, st, a, q);
  else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ssim_req<uint16_t, uint64_t>), dim3(a.first[3]), dim3(SSIM_BLOCK), 0, st, a, q);
}
