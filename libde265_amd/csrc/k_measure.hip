/*
 * k_measure.hip — a device frame (or a rectangle of it) compared with another picture in device-addressable memory, where both lie:
 * what libde265/quality.cc computes on host planes (SSD, SAD, MSE; `dec265 -m` calls MSE per plane, dec265.cc:388-419) plus the number of
 * differing samples, the largest difference and the raster-first differing sample (m355_frame_measure_async, include/de265_mi355x.h).
 * All integer: per plane, with d = a - b of the element values as stored,
 *   row_ssd[y] = sum d^2   ssd = sum row_ssd   sad = sum |d|   n_diff = #{d != 0}   max_abs = max |d|   first = min (y, x) with d != 0.
 * The row sums go to pinned memory: MSE() adds (double)row_ssd / width row by row, which the host repeats in that order when the request is
 * collected (runtime.hip) — as MD5 finishes on the host.
 *
 * ONE launch covers every plane, shaped like k_frame_hash_req (k_hash.hip): one wavefront per (plane, span of rows); a lane takes 16 bytes
 * of a row from both sources per step, the wavefront a row in steps of 1 KB.  The frame side starts at the rectangle's first sample and the
 * reference side at the caller's pointer with the caller's pitch, so neither is 16-byte aligned in general: both are the byte-aligned
 * vector loads of k_asm.h (one global_load_dwordx4 each), as in k_export.  The lane at the end of a row loads its valid bytes one by one
 * on BOTH sides: the reference is memory of the caller, which ends with its last row.
 *
 * ARITHMETIC AND RANGES.  |a - b| of two unsigned 16-bit values is subsat(a, b) | subsat(b, a) — packed, exact for the whole 16-bit range
 * (the signed difference does not fit int16; the absolute one fits uint16).  8-bit samples are widened to such pairs by v_perm first.
 *   8-bit planes: |d| <= 255, so the pairs are valid SIGNED 16-bit operands of v_dot2: d.d, d.(1,1) and min(d,1).(1,1) accumulate squares,
 *     absolute values and the count.  These three 32-bit sums cover ONE STEP of one lane = 16 samples: <= 16 * 255^2 = 1 040 400, 16 * 255
 *     and 16.  max |d| is kept packed (v_pk_max_i16: both halves <= 255).
 *   16-bit planes: d^2 <= 65535^2 = 4 294 836 225 fits 32 bits, two of them do not: every square goes into a 64-bit sum by itself
 *     (v_mad_u64_u32).  The 32-bit sum of absolute values covers one step of one lane = 8 samples: <= 8 * 65535 = 524 280.
 * Behind every step the lane adds the step's sums to 64-bit sums (of the row: squares; of the span: absolute values, count), so no
 * 32-bit sum ever covers more than one step, whatever the frame's width.  A 64-bit total holds 2^32 samples of the largest square.
 *
 * WHERE THE VALUES GO — the argument written above k_frame_hash_req, for this record.  Each row's sum of squares is reduced across the
 * wavefront and stored by lane 0 with a plain store into the request's pinned row array: every row belongs to exactly one wavefront, nobody
 * reads the array on the device, and the host reads it only behind the request's mark (an event recorded behind the launch: the end of the
 * kernel releases the stores to the system).  Everything else is reduced over the span in registers and across the wavefront FIRST; then
 * lane 0 issues one agent-scope atomic per quantity into the slot's device record q.rec: 64-bit add for ssd / sad / n_diff, max for
 * max_abs, and max for "first" in the encoding ~(y << 32 | x) — larger = earlier in raster order, and the empty value is 0, so the record
 * is zero between requests without a fill in front of the launch (an atomic whose operand is the neutral 0 is left out).  Then the lane
 * draws an arrival ticket from q.rec[15]:
 *   - every access to q.rec is an agent-scope atomic read-modify-write, performed where such atomics are performed for the whole device: no
 *     lane holds a word of the record in its CU's L1 or its XCD's L2, so no copy can go stale;
 *   - the lane's accumulator atomics are sequenced before its ticket fetch_add, which is a RELEASE at agent scope: they have been performed
 *     before the ticket becomes visible;
 *   - the same fetch_add is an ACQUIRE, and read-modify-writes continue a release sequence: the wavefront that reads first[3] - 1 from the
 *     counter synchronises with EVERY earlier ticket, hence every other wavefront's accumulator atomics happen before its later accesses;
 *   - it takes the values with atomicExch(..., 0) — agent-scope read-modify-writes behind the acquire — which returns the complete value and
 *     zeroes the word in one step, and zeroes the counter with an agent-scope atomic store.  All tickets are drawn, so nobody else touches the
 *     record in this launch, and the slot's NEXT launch is enqueued only after the host has seen this request's mark pass (a slot is free
 *     again when its result was collected): the zeroes are in place before that launch starts;
 *   - the pinned record q.res is written by that one lane with ordinary stores and read by the host behind the request's mark only.
 * A GATED launch (a decode that wrote the frame or the reference frame was rejected: the planes hold an older picture) writes the verdict
 * "no value" from one lane of its first workgroup and touches nothing else: no sample is read, the device record stays zero.
 *
 * Roofline: in bytes the work is pure traffic — every byte of both pictures read once (2 x 99.5 MB for an 8K 10-bit frame against a frame),
 * 8 bytes written per row — with about 3 VALU issues per sample pair and six 64-bit exchanges per row beside it.  MEASURED it is far from that
 * roof: 0.29 ms per request for such a frame, 0.14 of the box's copy rate (profiles/measure_rate.txt).  The cause is not measured (no counter
 * run, no trace); the launch has only about 8640 wavefronts, each walking its row in dependent steps.
 */
#include "k_common.h"
#include "k_measure.h"

#define MEAS_BLOCK 1024   /* bytes of a row per wave step: 64 lanes x 16 */
#define MEAS_NO_POS 0xFFFFFFFFFFFFFFFFull

__device__ __forceinline__ unsigned long long d_wave_add64(unsigned long long v)
{
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}
__device__ __forceinline__ unsigned long long d_wave_min64(unsigned long long v)
{
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) { const unsigned long long o = __shfl_xor(v, m, 64); v = o < v ? o : v; }
  return v;
}
__device__ __forceinline__ unsigned d_wave_max32(unsigned v)
{
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) { const unsigned o = __shfl_xor(v, m, 64); v = o > v ? o : v; }
  return v;
}

/* the lane's 16 bytes of a row at p, or the first n of them (the rest reads as 0 on both sides: no difference) */
__device__ __forceinline__ void d_meas_load(const M355_GLOBAL uint8_t* p, int n, unsigned w[4])
{
  if (n >= 16) { d_ldg16(p, w); return; }
  w[0] = w[1] = w[2] = w[3] = 0;
  for (int k = 0; k < n; k++) w[k >> 2] |= (unsigned)p[k] << (8 * (k & 3));
}

/* what one step of one lane adds (the header states the bound of each 32-bit member) */
struct MeasStep { unsigned sq32; unsigned long long sq64; unsigned ad, nz; };

/* one packed pair of 16-bit samples from each side */
template <int BPP>
__device__ __forceinline__ void d_meas_pair(unsigned pa, unsigned pb, MeasStep& s, unsigned& mx)
{
  const unsigned d = d_pk_subsat_u16(pa, pb) | d_pk_subsat_u16(pb, pa);      /* |a - b| in both halves */
  if (BPP == 1) {
    s.sq32 = (unsigned)d_dot2(d, d, (int)s.sq32);
    s.ad = (unsigned)d_dot2(d, 0x00010001u, (int)s.ad);
    s.nz = (unsigned)d_dot2(d_pk_min_u16(d, 0x00010001u), 0x00010001u, (int)s.nz);
    mx = d_pk_max_i16(mx, d);                                                /* (packed: two running maxima) */
  } else {
    const unsigned lo = d & 0xFFFFu, hi = d >> 16;
    s.sq64 += (unsigned long long)lo * lo;
    s.sq64 += (unsigned long long)hi * hi;
    s.ad += lo + hi;
    s.nz += (lo != 0u) + (hi != 0u);
    mx = max(mx, max(lo, hi));
  }
}

/* sample k of the lane's 16 bytes */
template <int BPP>
__device__ __forceinline__ unsigned d_meas_sample(const unsigned w[4], int k)
{
  return BPP == 1 ? (w[k >> 2] >> (8 * (k & 3))) & 0xFFu : (w[k >> 1] >> (16 * (k & 1))) & 0xFFFFu;
}

/* one wave per (plane, span of rows); wave index -> plane by the prefix counts in a.first[]; a.first[3] >= 1 */
template <int BPP>
__global__ void __launch_bounds__(256) k_measure_req(MeasArgs a, MeasReq q)
{
  if (q.timeout[0][1] == q.epoch[0] || q.timeout[1][1] == q.epoch[1]) {      /* M355_GATE for either frame, with the verdict */
    if (blockIdx.x == 0 && threadIdx.x == 0) { q.res[16] = q.seq; q.res[15] = MEAS_RES_GATED; }
    return;
  }
  const int lane = threadIdx.x & 63;
  const int wv = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (wv >= a.first[3]) return;                                              /* (draws no ticket: a.first[3] is the number of arrivals) */
  const int c = wv >= a.first[2] ? 2 : (wv >= a.first[1] ? 1 : 0);
  const MeasPlane pl = a.pl[c];
  const int y0 = (wv - a.first[c]) * a.rows_per_wave, y1 = min(y0 + a.rows_per_wave, pl.h);
  unsigned long long ssd = 0, sad = 0, ndiff = 0, first = MEAS_NO_POS;
  unsigned mx = 0;
  for (int y = y0; y < y1; y++) {
    const M355_GLOBAL uint8_t* ra = (const M355_GLOBAL uint8_t*)pl.a + (size_t)y * pl.pitch_a;
    const M355_GLOBAL uint8_t* rb = (const M355_GLOBAL uint8_t*)pl.b + (size_t)y * pl.pitch_b;
    unsigned long long row = 0;
    for (int o = lane * 16; o < pl.row_bytes; o += MEAS_BLOCK) {
      const int n = min(16, pl.row_bytes - o);
      unsigned wa[4], wb[4];
      d_meas_load(ra + o, n, wa);
      d_meas_load(rb + o, n, wb);
      MeasStep s = {0u, 0ull, 0u, 0u};
#pragma unroll
      for (int i = 0; i < 4; i++) {
        if (BPP == 1) {                                                      /* bytes 0,1 and 2,3 -> two pairs of 16-bit values */
          d_meas_pair<1>(d_perm(0u, wa[i], 0x0c010c00u), d_perm(0u, wb[i], 0x0c010c00u), s, mx);
          d_meas_pair<1>(d_perm(0u, wa[i], 0x0c030c02u), d_perm(0u, wb[i], 0x0c030c02u), s, mx);
        } else d_meas_pair<2>(wa[i], wb[i], s, mx);
      }
      row += BPP == 1 ? (unsigned long long)s.sq32 : s.sq64;
      sad += s.ad;
      ndiff += s.nz;
      if (s.nz && first == MEAS_NO_POS) {                                    /* a lane walks its samples in raster order: its first hit is its earliest */
        int idx = 0;
#pragma unroll
        for (int k = 16 / BPP - 1; k >= 0; k--) if (d_meas_sample<BPP>(wa, k) != d_meas_sample<BPP>(wb, k)) idx = k;
        first = ((unsigned long long)(unsigned)(pl.py + y) << 32) | (unsigned)(pl.px + o / BPP + idx);
      }
    }
    row = d_wave_add64(row);                                                 /* (every lane of the wave gets here: the loop above only skips steps) */
    if (lane == 0) q.rows[pl.row0 + y] = row;
    ssd += row;
  }
  sad = d_wave_add64(sad);
  ndiff = d_wave_add64(ndiff);
  if (BPP == 1) mx = max(mx & 0xFFFFu, mx >> 16);
  mx = d_wave_max32(mx);
  first = d_wave_min64(first);
  if (lane != 0) return;
  unsigned long long* rec = q.rec + c * MEAS_PER_PLANE;
  if (ssd) atomicAdd(&rec[MEAS_SSD], ssd);
  if (sad) atomicAdd(&rec[MEAS_SAD], sad);
  if (ndiff) atomicAdd(&rec[MEAS_NDIFF], ndiff);
  if (mx) atomicMax(&rec[MEAS_MAX], (unsigned long long)mx);
  if (first != MEAS_NO_POS) atomicMax(&rec[MEAS_FIRST], ~first);
  const unsigned long long drawn = __hip_atomic_fetch_add(&q.rec[MEAS_REC_WORDS - 1], 1ull, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
  if (drawn + 1ull != (unsigned long long)a.first[3]) return;
  for (int i = 0; i < 3 * MEAS_PER_PLANE; i++) q.res[i] = atomicExch(&q.rec[i], 0ull);
  __hip_atomic_store(&q.rec[MEAS_REC_WORDS - 1], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  q.res[16] = q.seq;
  q.res[15] = MEAS_RES_VALID;
}

void m355_launch_measure(const MeasArgs& a, const MeasReq& q, int bytes_per_sample, hipStream_t st)
{
  const int nw = a.first[3];
  if (bytes_per_sample == 1) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_measure_req<1>), dim3((nw + 3) / 4), dim3(256), 0, st, a, q);
  else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_measure_req<2>), dim3((nw + 3) / 4), dim3(256), 0, st, a, q);
}
