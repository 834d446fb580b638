/*
 * k_msssim.hip — multi-scale SSIM of a device frame (or a rectangle of it) against another picture in device-addressable memory, per plane and
 * per level, as m355_frame_msssim_async defines it (include/de265_mi355x.h): level j of a plane is the f x f box average (f = 2^j) of the
 * ORIGINAL samples with one rounding, (S + f f / 2) >> 2j — the native formula of k_export_scaled.hip, continued to f = 16 —; on every level
 * the valid 11 x 11 windows of ssim_window.h, and per window two points from the same five sums: q (m355_ssim_point) and qc
 * (m355_ssim_point_cs).  Per plane and level the sum of q and the sum of qc.
 *
 * TWO launches on one stream cover every selected plane and every level; the tile, the workgroup and the two LDS passes are k_ssim.hip's
 * (SSIM_TILE_W x SSIM_TILE_H windows from 42 x 42 samples of either side, SSIM_BLOCK threads; steps LOAD, ROWS, WINDOWS, REDUCE as described
 * there — d_msssim_tile below is that code with the second point and without the map).
 *   LAUNCH 1 (k_msssim_base) measures level 0 and builds the pyramid.  Its grid is sized by SAMPLES, ceil(pw / 32) x ceil(ph / 32) tiles: a tile
 *     OWNS the 32 x 32 samples at its origin, which are in LDS anyway, and since origins are multiples of 32 every f x f block up to f = 16 lies
 *     in one tile.  A tile at the right or bottom rim may hold no valid window and still owes its blocks.
 *       level 1: 2 x 16 x 16 sums of 2 x 2 samples, one per thread of the upper half of the workgroup, beside the ROWS step (both only read the
 *                samples); the sums stay in LDS (s_p1);
 *       levels 2, 3, 4: the last wavefront, beside the WINDOWS step: lane (bx, by) of 8 x 8 adds four level-1 sums, then the 4 x 4 and 2 x 2
 *                grids form by two shuffles each (lanes ^1, ^8, then ^2, ^16) — every level's sum from the level below, in 32 bits
 *                (256 x 65535 < 2^24), no further barrier.
 *     Each ROUNDED sample inside (pw >> j) x (ph >> j) is stored to the slot's scratch; blocks that reach beyond f (pw >> j) columns or
 *     f (ph >> j) rows are not.  The originals are read once, plus the tiles' 10-sample halo, and never again.
 *   LAUNCH 2 (k_msssim_levels) measures levels 1 .. L - 1 of every plane in ONE grid: workgroup -> (plane, level) by the prefix table
 *     MsssimLevelArgs.first[], tiles by windows as in k_ssim.hip, samples from scratch.  It reads a third of what launch 1 read.  With levels
 *     == 1 it is not launched.
 * Both launches: one 64-bit atomic add per non-zero accumulator per workgroup, then one arrival.  The arrival count covers BOTH launches'
 * workgroups, and launch 2 runs behind launch 1 on the stream, so the workgroup that draws the last ticket is one of the last launch's; it moves
 * the thirty values to the pinned record with atomicExch(..., 0), which leaves the device record zero for the slot's next request (the argument
 * about visibility is the one written in k_ssim.hip / k_measure.hip).  Scratch written by launch 1 is read by launch 2 only: the kernel
 * boundary orders them.
 * A GATED request (a decode that wrote the frame or the reference frame was rejected): both launches test the gates first; launch 1 writes the
 * verdict from one thread of its first workgroup; launch 2 returns without a write.  No sample is read, scratch and the device record are untouched.
 *
 * LDS per workgroup: k_ssim.hip's, plus the level-1 sums (2 KiB) and a second reduction row: 8-bit 32.7 KB, 16-bit 52.4 KB.
 * profiles/msssim_codegen.txt has the compiler's resource lines of the four instances (no scratch memory, no spills, 60 .. 62 registers: two
 * workgroups per CU); profiles/msssim_bench.txt the cost: 1.31 .. 1.33 times the SSIM request on the same planes, the work model's 4/3 (a third more
 * windows), which is why no other split of the work into launches was tried.
 */
#include "k_common.h"
#include "k_msssim.h"
#include "ssim_window.h"

#define MSSSIM_SW (SSIM_TILE_W + 10)   /* samples per tile row */
#define MSSSIM_SH (SSIM_TILE_H + 10)
static_assert(SSIM_TILE_W == 32 && SSIM_TILE_H == 32 && SSIM_BLOCK == 1024, "the pyramid's thread mapping is written for 32 x 32 tiles and sixteen wavefronts");

__device__ __forceinline__ long long d_msssim_wave_add(long long v)
{
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

/* where launch 1 leaves the pyramid of one plane (null in launch 2) */
template <class T>
struct MsssimPyr {
  T* lv[2][MSSSIM_LEVELS - 1];   /* [side][j - 1] */
  int levels;
};

/* one rounded level-j sample of the tile at (x0, y0), block (bx, by) of the tile's 32 >> j per axis, if the level has it */
template <class T>
__device__ __forceinline__ void d_msssim_put(T* lv, int j, uint32_t S, int x0, int y0, int bx, int by, int pw, int ph)
{
  const int X = (x0 >> j) + bx, Y = (y0 >> j) + by, lw = pw >> j;
  if (X < lw && Y < (ph >> j)) lv[(size_t)Y * lw + X] = (T)((S + (1u << (2 * j - 1))) >> (2 * j));
}

/* One tile of one picture pair: the workgroup's sums of q and qc over the tile's valid windows, in thread 0 (the others return garbage).
   PYR: the tile also owes levels 1 .. pyr.levels - 1 its 32 x 32 samples. */
template <class T, class SQ, bool PYR>
__device__ __forceinline__ void d_msssim_tile(const uint8_t* pa, const uint8_t* pb, long long pitch_a, long long pitch_b, int pw, int ph, int x0, int y0,
                                              double c1, double c2, const MsssimPyr<T>& pyr, long long& out_q, long long& out_cs)
{
  __shared__ T s_a[MSSSIM_SH][MSSSIM_SW], s_b[MSSSIM_SH][MSSSIM_SW];
  __shared__ uint32_t s_ma[MSSSIM_SH][SSIM_TILE_W], s_mb[MSSSIM_SH][SSIM_TILE_W];
  __shared__ SQ s_aa[MSSSIM_SH][SSIM_TILE_W], s_bb[MSSSIM_SH][SSIM_TILE_W], s_ab[MSSSIM_SH][SSIM_TILE_W];
  __shared__ uint32_t s_p1[2][SSIM_TILE_H / 2][SSIM_TILE_W / 2];
  __shared__ long long s_sum[2][SSIM_BLOCK / 64];
  const uint32_t w[M355_SSIM_TAPS] = M355_SSIM_WEIGHTS;
  const int t = threadIdx.x;

  /* 1. the samples: consecutive threads take consecutive samples of a row; positions outside the plane read 0 */
  for (int i = t; i < MSSSIM_SH * MSSSIM_SW; i += SSIM_BLOCK) {
    const int r = i / MSSSIM_SW, k = i - r * MSSSIM_SW;
    T va = 0, vb = 0;
    if (x0 + k < pw && y0 + r < ph) {
      va = *(const T*)(pa + (size_t)(y0 + r) * pitch_a + (size_t)(x0 + k) * sizeof(T));
      vb = *(const T*)(pb + (size_t)(y0 + r) * pitch_b + (size_t)(x0 + k) * sizeof(T));
    }
    s_a[r][k] = va; s_b[r][k] = vb;
  }
  __syncthreads();

  /* 2. the rows' sums */
  for (int i = t; i < MSSSIM_SH * SSIM_TILE_W; i += SSIM_BLOCK) {
    const int r = i / SSIM_TILE_W, k = i % SSIM_TILE_W;
    uint32_t ma = 0, mb = 0;
    SQ aa = 0, bb = 0, ab = 0;
#pragma unroll
    for (int j = 0; j < M355_SSIM_TAPS; j++) {      /* (side a alone first: as one loop over both sides the 16-bit instances take 67 registers, one */
      const uint32_t va = s_a[r][k + j];            /*  workgroup per CU; split, 60 .. 62 and two) */
      ma += w[j] * va; aa += (SQ)w[j] * (va * va);
    }
#pragma unroll
    for (int j = 0; j < M355_SSIM_TAPS; j++) {
      const uint32_t va = s_a[r][k + j], vb = s_b[r][k + j];
      mb += w[j] * vb; bb += (SQ)w[j] * (vb * vb); ab += (SQ)w[j] * (va * vb);
    }
    s_ma[r][k] = ma; s_mb[r][k] = mb; s_aa[r][k] = aa; s_bb[r][k] = bb; s_ab[r][k] = ab;
  }
  /* ... and level 1 of the tile's own samples, on the threads that have one item of the loop above, not two */
  if (PYR && pyr.levels > 1 && t >= SSIM_BLOCK / 2) {
    const int side = (t >> 8) & 1, by = (t >> 4) & 15, bx = t & 15;
    const T(*s)[MSSSIM_SW] = side ? s_b : s_a;
    const uint32_t S = (uint32_t)s[2 * by][2 * bx] + s[2 * by][2 * bx + 1] + s[2 * by + 1][2 * bx] + s[2 * by + 1][2 * bx + 1];
    s_p1[side][by][bx] = S;
    d_msssim_put(side ? pyr.lv[1][0] : pyr.lv[0][0], 1, S, x0, y0, bx, by, pw, ph);
  }
  __syncthreads();

  /* levels 2, 3, 4: the last wavefront, every lane in every shuffle */
  if (PYR && pyr.levels > 2 && t >= SSIM_BLOCK - 64) {
    const int bx = t & 7, by = (t >> 3) & 7;
#pragma unroll
    for (int side = 0; side < 2; side++) {
      uint32_t S = s_p1[side][2 * by][2 * bx] + s_p1[side][2 * by][2 * bx + 1] + s_p1[side][2 * by + 1][2 * bx] + s_p1[side][2 * by + 1][2 * bx + 1];
      d_msssim_put(pyr.lv[side][1], 2, S, x0, y0, bx, by, pw, ph);
      if (pyr.levels > 3) {
        S += __shfl_xor(S, 1, 64); S += __shfl_xor(S, 8, 64);
        if (!((bx | by) & 1)) d_msssim_put(pyr.lv[side][2], 3, S, x0, y0, bx >> 1, by >> 1, pw, ph);
      }
      if (pyr.levels > 4) {
        S += __shfl_xor(S, 2, 64); S += __shfl_xor(S, 16, 64);
        if (!((bx | by) & 3)) d_msssim_put(pyr.lv[side][3], 4, S, x0, y0, bx >> 2, by >> 2, pw, ph);
      }
    }
  }

  /* 3. the windows (every thread walks all its rounds: the reduction below is a collective) */
  const int nwx = pw - 10, nwy = ph - 10;
  long long sum_q = 0, sum_cs = 0;
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
    sum_q += m355_ssim_point(MA, MB, SAA, SBB, SAB, c1, c2);
    sum_cs += m355_ssim_point_cs(MA, MB, SAA, SBB, SAB, c1, c2);
  }

  /* 4. across the wavefront by shuffles, across the wavefronts through LDS */
  sum_q = d_msssim_wave_add(sum_q);
  sum_cs = d_msssim_wave_add(sum_cs);
  if ((t & 63) == 0) { s_sum[0][t >> 6] = sum_q; s_sum[1][t >> 6] = sum_cs; }
  __syncthreads();
  if (t != 0) return;
  for (int k = 1; k < SSIM_BLOCK / 64; k++) { sum_q += s_sum[0][k]; sum_cs += s_sum[1][k]; }
  out_q = sum_q; out_cs = sum_cs;
}

/* thread 0 of a workgroup: one add per non-zero accumulator, then the arrival; the last one of the request moves the record */
__device__ __forceinline__ void d_msssim_arrive(const MsssimReq& q, int acc, long long sum_q, long long sum_cs, int arrivals)
{
  if (sum_q) atomicAdd(&q.rec[MSSSIM_Q + acc], (unsigned long long)sum_q);
  if (sum_cs) atomicAdd(&q.rec[MSSSIM_CS + acc], (unsigned long long)sum_cs);
  const unsigned long long drawn = __hip_atomic_fetch_add(&q.rec[MSSSIM_REC_WORDS - 1], 1ull, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
  if (drawn + 1ull != (unsigned long long)arrivals) return;
  for (int i = 0; i < MSSSIM_VALUES; i++) q.res[i] = atomicExch(&q.rec[i], 0ull);
  __hip_atomic_store(&q.rec[MSSSIM_REC_WORDS - 1], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  q.res[MSSSIM_REC_WORDS - 1] = q.seq;
  q.res[MSSSIM_REC_WORDS - 2] = MSSSIM_RES_VALID;
}

#define MSSSIM_GATED(q) ((q).timeout[0][1] == (q).epoch[0] || (q).timeout[1][1] == (q).epoch[1])   /* M355_GATE for either frame */

/* launch 1: one workgroup per tile of SAMPLES; workgroup index -> plane by the prefix counts in a.first[] */
template <class T, class SQ>
__global__ void __launch_bounds__(SSIM_BLOCK) k_msssim_base(MsssimArgs a, MsssimReq q)
{
  if (MSSSIM_GATED(q)) {
    if (blockIdx.x == 0 && threadIdx.x == 0) { q.res[MSSSIM_REC_WORDS - 1] = q.seq; q.res[MSSSIM_REC_WORDS - 2] = MSSSIM_RES_GATED; }
    return;
  }
  const int wg = blockIdx.x;
  const int c = wg >= a.first[2] ? 2 : (wg >= a.first[1] ? 1 : 0);
  const MsssimPlane pl = a.pl[c];
  const int tile = wg - a.first[c];
  MsssimPyr<T> pyr;
  pyr.lv[0][0] = (T*)pl.a1; pyr.lv[0][1] = (T*)pl.a2; pyr.lv[0][2] = (T*)pl.a3; pyr.lv[0][3] = (T*)pl.a4;
  pyr.lv[1][0] = (T*)pl.b1; pyr.lv[1][1] = (T*)pl.b2; pyr.lv[1][2] = (T*)pl.b3; pyr.lv[1][3] = (T*)pl.b4;
  pyr.levels = a.levels;
  long long sum_q = 0, sum_cs = 0;
  d_msssim_tile<T, SQ, true>(pl.a, pl.b, pl.pitch_a, pl.pitch_b, pl.pw, pl.ph, (tile % pl.tiles_x) * SSIM_TILE_W, (tile / pl.tiles_x) * SSIM_TILE_H,
                             pl.c1, pl.c2, pyr, sum_q, sum_cs);
  if (threadIdx.x == 0) d_msssim_arrive(q, pl.acc, sum_q, sum_cs, a.arrivals);
}

/* launch 2: one workgroup per tile of windows of one (plane, level >= 1) */
template <class T, class SQ>
__global__ void __launch_bounds__(SSIM_BLOCK) k_msssim_levels(MsssimLevelArgs a, MsssimReq q)
{
  if (MSSSIM_GATED(q)) return;
  const int wg = blockIdx.x;
  int e = 0;
  while (e + 1 < a.n && wg >= a.first[e + 1]) e++;
  const MsssimLevel lv = a.lv[e];
  const int tile = wg - a.first[e];
  const long long pitch = (long long)lv.pw * sizeof(T);
  MsssimPyr<T> none = {};
  long long sum_q = 0, sum_cs = 0;
  d_msssim_tile<T, SQ, false>(lv.a, lv.b, pitch, pitch, lv.pw, lv.ph, (tile % lv.tiles_x) * SSIM_TILE_W, (tile / lv.tiles_x) * SSIM_TILE_H, lv.c1, lv.c2,
                              none, sum_q, sum_cs);
  if (threadIdx.x == 0) d_msssim_arrive(q, lv.acc, sum_q, sum_cs, a.arrivals);
}

template <class T, class SQ>
static void launch_msssim(const MsssimArgs& a, const MsssimLevelArgs& lv, const MsssimReq& q, hipStream_t st)
{
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_msssim_base<T, SQ>), dim3(a.first[3]), dim3(SSIM_BLOCK), 0, st, a, q);
  if (lv.n) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_msssim_levels<T, SQ>), dim3(lv.first[lv.n]), dim3(SSIM_BLOCK), 0, st, lv, q);
}

void m355_launch_msssim(const MsssimArgs& a, const MsssimLevelArgs& lv, const MsssimReq& q, int bytes_per_sample, hipStream_t st)
{
  if (bytes_per_sample == 1) launch_msssim<uint8_t, uint32_t>(a, lv, q, st);
  else launch_msssim<uint16_t, uint64_t>(a, lv, q, st);
}
