/*
 * k_maps.hip — the side maps of a picture (m355_picture_maps_async): the work lists of one picture turned into dense per-unit maps in the caller's
 * memory.  map_element.h is the definition; this file is how it runs.  Two launches per request, behind a zero fill of the scratch:
 *
 * RASTER (k_maps_raster).  A unit takes its value at a point of the picture's 4x4 grid, so the lists are painted onto planes on that grid first: the
 * CU and PB index + 1 (32 bit), the TU element and the shown intra block's mode + 1 (bytes).  One wavefront takes 64 consecutive records of one list,
 * one per lane: the lane loads its record, decides whether it counts (map_element.h) and how many cells it covers, clipped to the picture.  The cells
 * of all 64 records are then numbered through (a prefix sum across the wavefront) and written 64 at a time: lane l of step s owns cell 64 s + l,
 * finds the record that cell belongs to by a binary search over the prefix sums (six shuffles) and fetches that record's rectangle and value from its
 * lane.  Consecutive lanes therefore write consecutive cells of a record, row by row — a 64x64 CU is four full steps of 64-byte row segments — and 64
 * 4x4 transform units are ONE step, not 64: no lane ever loops over a block alone, and lanes idle only in a batch's last step.  Records that do not
 * count are counted per wavefront (a ballot) and added with one atomic.
 *
 * GATHER (k_maps_gather).  A lane owns four horizontally adjacent units of one row of the unit grid.  With 4x4 units its four cells are one aligned
 * 16-byte load per plane (scratch rows are padded to four cells); with larger units the loads are strided, and there are 4 to 256 times fewer of them.
 * Neighbouring units mostly share a record, so the record loads (12 / 24 bytes, whole dwords) hit in L1 / L2.  Stores: a lane that has all its four
 * units stores them at once — the byte maps as one dword, MAP_SLICE as 8 bytes, the 32-bit maps as 16 bytes, MAP_MV as two 16-byte stores — with
 * the byte-aligned vector forms of k_asm.h, which are single instructions at ANY address (the exports store through them): pointer and pitch need
 * only be multiples of the element, and no destination falls back to bytes.  Only the lane at a row's tail stores element by element.  The summary
 * is reduced across the wavefront (__shfl_xor), across the workgroup of sixteen wavefronts through LDS, and leaves the workgroup as ONE record of
 * plain stores in a table of its own (MapsArgs::part); the workgroup then draws an arrival ticket, and the one that arrives last adds the table up
 * and writes the slot's pinned record.  One atomic per workgroup: the first version added every field with one atomic per wavefront, and those
 * 65 000 atomics on eight words WERE the request (0.76 of 0.82 ms at 8K).  The device record holds the ticket and the raster pass's skip counts;
 * both are left zero, so a reused slot is clean without a fill.
 */
#include "k_maps.h"
#include <k_asm.h> /* (through the include path, as k_common.h takes it) */

template <class T> __device__ __forceinline__ T d_maps_add(T v)
{
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}
__device__ __forceinline__ unsigned d_maps_max(unsigned v)
{
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) { const unsigned o = __shfl_xor(v, m, 64); v = o > v ? o : v; }
  return v;
}

/* a record of a list (12, 8 or 24 bytes, 4-byte aligned in the arena) as whole dwords: one load of 12 / 8 / 16 + 8 bytes, not one per field */
template <class T> __device__ __forceinline__ T d_maps_rec(const T* p)
{
  static_assert(sizeof(T) == 8 || sizeof(T) == 12 || sizeof(T) == 24, "record size");
  unsigned w[sizeof(T) / 4];
  if (sizeof(T) == 8) d_ldg8((const M355_GLOBAL void*)p, w);
  else if (sizeof(T) == 12) d_ldg12((const M355_GLOBAL void*)p, w);
  else { d_ldg16((const M355_GLOBAL void*)p, w); d_ldg8((const M355_GLOBAL void*)((const uint8_t*)p + 16), w + 4); }
  T r;
  memcpy(&r, w, sizeof(T));
  return r;
}

/* what a lane knows of its record: the cells it covers, [cx, cx + cw) x [cy, cy + ch), and what is written there */
struct MapsRect { int cx, cy, cw, ch; uint32_t value; };

/* the wavefront's 64 rectangles onto `plane` (T = uint32_t or uint8_t), rows of `sp` cells */
template <class T> __device__ __forceinline__ void d_maps_paint(const MapsRect r, T* plane, int sp, int lane)
{
  const int n = r.cw * r.ch;                                    /* (0: the record does not count, or covers no point of the grid) */
  int incl = n;                                                 /* inclusive prefix sum across the wavefront */
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(incl, d, 64); if (lane >= d) incl += o; }
  const int total = __shfl(incl, 63, 64);
  for (int base = 0; base < total; base += 64) {                /* (uniform across the wavefront: every lane reaches every shuffle) */
    const int k = base + lane;
    int owner = 0;                                              /* the first lane whose inclusive sum exceeds k (at most 63: an idle lane of the last step, k >= total, names lane 63) */
#pragma unroll
    for (int b = 32; b >= 1; b >>= 1) { const int probe = __shfl(incl, owner + b - 1, 64); if (probe <= k) owner += b; }
    const int o_incl = __shfl(incl, owner, 64), o_cw = __shfl(r.cw, owner, 64), o_ch = __shfl(r.ch, owner, 64);
    const int o_cx = __shfl(r.cx, owner, 64), o_cy = __shfl(r.cy, owner, 64);
    const uint32_t o_val = __shfl(r.value, owner, 64);
    if (k < total) {
      const int i = k - (o_incl - o_cw * o_ch);                 /* the cell inside the owner's rectangle, row by row */
      const int row = i / o_cw, col = i - row * o_cw;
      plane[(size_t)(o_cy + row) * sp + (o_cx + col)] = (T)o_val;
    }
  }
}

__global__ void __launch_bounds__(MAPS_RASTER_BLOCK) k_maps_raster(MapsArgs a)
{
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint32_t wg = blockIdx.x;
  const int list = wg < a.wg_end[0] ? 0 : (wg < a.wg_end[1] ? 1 : (wg < a.wg_end[2] ? 2 : 3));
  const uint32_t first = list ? a.wg_end[list - 1] : 0u;
  const long long i = ((long long)(wg - first) * (MAPS_RASTER_BLOCK / 64) + wv) * 64 + lane;     /* this lane's record */
  MapsRect r = {0, 0, 0, 0, 0u};
  int bad = 0;
  int x = 0, y = 0, w = 0, h = 0, ok = 0;
  if (list == 0) {
    if (i < a.n_cus) { const m355_cu cu = d_maps_rec(a.cus + i); ok = m355_me_cu_ok(cu, a.lim); bad = !ok; x = cu.x; y = cu.y; w = h = ok ? 1 << cu.log2_size : 0; r.value = (uint32_t)i + 1u; }
  } else if (list == 1) {
    if (i < a.n_tus) { const m355_tu tu = d_maps_rec(a.tus + i); ok = m355_me_tu_ok(tu, a.lim); bad = !ok; x = tu.x; y = tu.y; w = h = ok ? 1 << tu.log2_size : 0; r.value = m355_me_tu(tu); }
  } else if (list == 2) {
    if (i < a.n_pbs) { const m355_pb pb = d_maps_rec(a.pbs + i); ok = m355_me_pb_ok(pb, a.lim); bad = !ok; x = pb.x; y = pb.y; w = pb.w; h = pb.h; r.value = (uint32_t)i + 1u; }
  } else {
    if (i < a.n_ibs) {
      const m355_ib ib = d_maps_rec(a.ibs + i);
      ok = m355_me_ib_ok(ib, a.lim); bad = !ok;
      ok = ok && m355_me_ib_shown(ib);
      x = ib.x; y = ib.y; w = h = ok ? 1 << ib.log2_size : 0; r.value = (uint32_t)ib.mode + 1u;
    }
  }
  if (ok) {
    int c0, c1;
    m355_me_cells(x, w, a.g.w4, &c0, &c1); r.cx = c0; r.cw = c1 > c0 ? c1 - c0 : 0;
    m355_me_cells(y, h, a.g.h4, &c0, &c1); r.cy = c0; r.ch = c1 > c0 ? c1 - c0 : 0;
    if (!r.cw || !r.ch) r.cw = r.ch = 0;
  }
  if (list == 0) d_maps_paint(r, a.s_cu, a.sp, lane);
  else if (list == 1) d_maps_paint(r, a.s_tu, a.sp, lane);
  else if (list == 2) d_maps_paint(r, a.s_pb, a.sp, lane);
  else d_maps_paint(r, a.s_ib, a.sp, lane);
  const unsigned n_bad = (unsigned)__popcll(__ballot(bad));
  if (lane == 0 && n_bad) atomicAdd(a.rec + MAPS_SKIPPED + list, n_bad);
}

/* four consecutive elements of a row, of which the first `nv` exist: ONE store of 4 / 8 / 16 / 2 x 16 bytes for a lane that has all four — the
   byte-aligned vector forms of k_asm.h, single instructions whatever the address, as the exports use them: a destination needs to be a multiple of
   its element only — and element by element at a row's tail */
__device__ __forceinline__ void d_maps_store_u8(uint8_t* p, const uint32_t v[4], int nv)
{
  if (nv == 4) { d_stg4((M355_GLOBAL void*)p, v[0] | v[1] << 8 | v[2] << 16 | v[3] << 24); return; }
  for (int k = 0; k < 3; k++) if (k < nv) p[k] = (uint8_t)v[k];
}
__device__ __forceinline__ void d_maps_store_u16(uint8_t* p, const uint32_t v[4], int nv)
{
  if (nv == 4) { const unsigned w[2] = {v[0] | v[1] << 16, v[2] | v[3] << 16}; d_stg8((M355_GLOBAL void*)p, w); return; }
  for (int k = 0; k < 3; k++) if (k < nv) ((uint16_t*)p)[k] = (uint16_t)v[k];
}
__device__ __forceinline__ void d_maps_store_u32(uint8_t* p, const uint32_t v[4], int nv)
{
  if (nv == 4) { d_stg16((M355_GLOBAL void*)p, v); return; }
  for (int k = 0; k < 3; k++) if (k < nv) ((uint32_t*)p)[k] = v[k];
}
__device__ __forceinline__ void d_maps_store_u64(uint8_t* p, const uint32_t v[8], int nv)
{
  if (nv == 4) { d_stg16((M355_GLOBAL void*)p, v); d_stg16((M355_GLOBAL void*)(p + 16), v + 4); return; }
  for (int k = 0; k < 3; k++) if (k < nv) d_stg8((M355_GLOBAL void*)(p + 8 * k), v + 2 * k);
}
/* the lane's four cells of a scratch plane: cells cx0, cx0 + step, ... of row `row` (step == 1: cx0 is a multiple of 4 and the row is padded) */
__device__ __forceinline__ void d_maps_cells_u32(const uint32_t* plane, size_t row, int cx0, int step, int nv, uint32_t v[4])
{
  if (step == 1) { const uint4 q = *(const uint4*)(plane + row + cx0); v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w; return; }
  for (int k = 0; k < 4; k++) v[k] = k < nv ? plane[row + cx0 + k * step] : 0u;
}
__device__ __forceinline__ void d_maps_cells_u8(const uint8_t* plane, size_t row, int cx0, int step, int nv, uint32_t v[4])
{
  if (step == 1) { const uint32_t q = *(const uint32_t*)(plane + row + cx0); v[0] = q & 255u; v[1] = (q >> 8) & 255u; v[2] = (q >> 16) & 255u; v[3] = q >> 24; return; }
  for (int k = 0; k < 4; k++) v[k] = k < nv ? plane[row + cx0 + k * step] : 0u;
}

/* n summary records of MAPS_PART_WORDS words at `src` (and, with `acc`, one more) combined into out[]: counts and the 64-bit sum added, the two
   encoded extremes (neutral 0) by max */
__device__ __forceinline__ void d_maps_combine(uint32_t out[MAPS_PART_WORDS], const uint32_t* src, int n, const uint32_t* acc = nullptr)
{
  uint32_t t[MAPS_PART_WORDS];
  for (int k = 0; k < MAPS_PART_WORDS; k++) t[k] = acc ? acc[k] : 0u;
  unsigned long long q = (unsigned long long)t[MAPS_QP_SUM] | (unsigned long long)t[MAPS_QP_SUM + 1] << 32;
#pragma unroll 1
  for (int i = 0; i < n; i++) {                                 /* (rolled: one thread runs it, and unrolled its registers would halve the kernel's occupancy) */
    const uint32_t* w = src + i * MAPS_PART_WORDS;
    for (int k = 0; k < MAPS_PART_WORDS; k++) {
      if (k == MAPS_QP_SUM || k == MAPS_QP_SUM + 1) continue;
      if (k == MAPS_QP_MIN || k == MAPS_QP_MAX) t[k] = w[k] > t[k] ? w[k] : t[k];
      else t[k] += w[k];
    }
    q += (unsigned long long)w[MAPS_QP_SUM] | (unsigned long long)w[MAPS_QP_SUM + 1] << 32;
  }
  t[MAPS_QP_SUM] = (uint32_t)q; t[MAPS_QP_SUM + 1] = (uint32_t)(q >> 32);
  for (int k = 0; k < MAPS_PART_WORDS; k++) out[k] = t[k];
}

__global__ void __launch_bounds__(MAPS_BLOCK) k_maps_gather(MapsArgs a)
{
  __shared__ unsigned s_last;
  __shared__ uint32_t s_wave[MAPS_WAVES][MAPS_PART_WORDS];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long long tid = (long long)blockIdx.x * MAPS_BLOCK + threadIdx.x;
  const int uy = (int)(tid / a.quads), q = (int)(tid - (long long)uy * a.quads);
  const int sh = a.g.log2_unit - 2, step = 1 << sh;             /* cells per unit */
  const int ux0 = 4 * q;
  int nv = uy < a.g.units_h ? a.g.units_w - ux0 : 0;            /* units of this lane that exist (lanes behind the grid: none; they stay for the shuffles) */
  nv = nv > 4 ? 4 : (nv < 0 ? 0 : nv);
  const size_t row = (size_t)(uy << sh) * a.sp;
  const int cx0 = ux0 << sh;
  uint32_t covered = 0, cls[3] = {0, 0, 0}, qmin_e = 0, qmax_e = 0, bipred = 0;
  long long qsum = 0;
  if (nv) {
    if (a.dst[M355_MAP_CU] || a.dst[M355_MAP_QP]) {
      uint32_t idx[4], cu_e[4], qp_e[4];
      d_maps_cells_u32(a.s_cu, row, cx0, step, nv, idx);
      for (int k = 0; k < 4; k++) {
        cu_e[k] = M355_ME_NONE_CU; qp_e[k] = (uint32_t)(uint8_t)M355_ME_NONE_QP;
        if (k < nv && idx[k]) {
          const m355_cu cu = d_maps_rec(a.cus + (idx[k] - 1u));
          cu_e[k] = m355_me_cu(cu); qp_e[k] = (uint32_t)(uint8_t)cu.qp_y;
          if (a.dst[M355_MAP_QP]) {
            const int qp = cu.qp_y;
            qsum += qp;
            const uint32_t lo = (uint32_t)(128 - qp), hi = (uint32_t)(qp + 129);
            qmin_e = lo > qmin_e ? lo : qmin_e; qmax_e = hi > qmax_e ? hi : qmax_e;
          }
          if (a.dst[M355_MAP_CU]) { covered++; const int c = m355_me_cu_class(cu_e[k]); cls[0] += c == 0; cls[1] += c == 1; cls[2] += c == 2; }
        }
      }
      if (a.dst[M355_MAP_CU]) d_maps_store_u32(a.dst[M355_MAP_CU] + (long long)uy * a.pitch[M355_MAP_CU] + 4ll * ux0, cu_e, nv);
      if (a.dst[M355_MAP_QP]) d_maps_store_u8(a.dst[M355_MAP_QP] + (long long)uy * a.pitch[M355_MAP_QP] + ux0, qp_e, nv);
    }
    if (a.dst[M355_MAP_TU]) {
      uint32_t v[4];
      d_maps_cells_u8(a.s_tu, row, cx0, step, nv, v);
      d_maps_store_u8(a.dst[M355_MAP_TU] + (long long)uy * a.pitch[M355_MAP_TU] + ux0, v, nv);
    }
    if (a.dst[M355_MAP_INTRA]) {
      uint32_t v[4];
      d_maps_cells_u8(a.s_ib, row, cx0, step, nv, v);
      for (int k = 0; k < 4; k++) v[k] = (v[k] - 1u) & 255u;    /* (mode + 1; 0 = nothing shown -> 255) */
      d_maps_store_u8(a.dst[M355_MAP_INTRA] + (long long)uy * a.pitch[M355_MAP_INTRA] + ux0, v, nv);
    }
    if (a.dst[M355_MAP_MV] || a.dst[M355_MAP_REF]) {
      uint32_t idx[4], mv_e[8], ref_e[4];
      d_maps_cells_u32(a.s_pb, row, cx0, step, nv, idx);
      for (int k = 0; k < 4; k++) {
        mv_e[2 * k] = mv_e[2 * k + 1] = 0u; ref_e[k] = M355_ME_NONE_REF;
        if (k < nv && idx[k]) {
          const m355_pb pb = d_maps_rec(a.pbs + (idx[k] - 1u));
          m355_me_mv(pb, mv_e + 2 * k); ref_e[k] = m355_me_ref(pb);
          if (a.dst[M355_MAP_REF]) bipred += (uint32_t)m355_me_ref_bipred(ref_e[k]);
        }
      }
      if (a.dst[M355_MAP_MV]) d_maps_store_u64(a.dst[M355_MAP_MV] + (long long)uy * a.pitch[M355_MAP_MV] + 8ll * ux0, mv_e, nv);
      if (a.dst[M355_MAP_REF]) d_maps_store_u32(a.dst[M355_MAP_REF] + (long long)uy * a.pitch[M355_MAP_REF] + 4ll * ux0, ref_e, nv);
    }
    if (a.dst[M355_MAP_SLICE]) {
      uint32_t v[4];
      const int cy = ((uy << a.g.log2_unit) >> a.g.log2_ctb) * a.g.ctbW;
      for (int k = 0; k < 4; k++) v[k] = k < nv ? a.ctbs[cy + (((ux0 + k) << a.g.log2_unit) >> a.g.log2_ctb)].slice_idx : 0u;
      d_maps_store_u16(a.dst[M355_MAP_SLICE] + (long long)uy * a.pitch[M355_MAP_SLICE] + 2ll * ux0, v, nv);
    }
  }
  /* the summary: across the wavefront, across the workgroup through LDS, then ONE record per workgroup, written with plain stores by thread 0 alone,
     which then draws the workgroup's arrival ticket — atomics of many wavefronts on the same few words are performed one after the other (about 12 ns
     each here: 65 000 of them were 0.76 ms of an 8K request, profiles/side_maps_bench.txt), so the only contended word left is the ticket */
  covered = d_maps_add(covered); cls[0] = d_maps_add(cls[0]); cls[1] = d_maps_add(cls[1]); cls[2] = d_maps_add(cls[2]);
  bipred = d_maps_add(bipred);
  const unsigned long long qs = d_maps_add((unsigned long long)qsum);
  qmin_e = d_maps_max(qmin_e); qmax_e = d_maps_max(qmax_e);
  if (lane == 0) {
    uint32_t* w = s_wave[wv];
    w[MAPS_COVERED] = covered; w[MAPS_INTRA] = cls[0]; w[MAPS_INTER] = cls[1]; w[MAPS_SKIP] = cls[2];
    w[MAPS_QP_SUM] = (uint32_t)qs; w[MAPS_QP_SUM + 1] = (uint32_t)(qs >> 32);
    w[MAPS_QP_MIN] = qmin_e; w[MAPS_QP_MAX] = qmax_e; w[MAPS_BIPRED] = bipred;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t t[MAPS_PART_WORDS];
    d_maps_combine(t, &s_wave[0][0], MAPS_WAVES);
    uint32_t* mine = a.part + (size_t)blockIdx.x * MAPS_PART_WORDS;
    for (int k = 0; k < MAPS_PART_WORDS; k++) mine[k] = t[k];
    d_drain_vmem();                                             /* the workgroup's record has been written ... */
    __threadfence();                                            /* ... and released before the ticket can be seen */
    s_last = __hip_atomic_fetch_add(a.rec + MAPS_ARRIVED, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) + 1u == a.n_wg ? 1u : 0u;
  }
  __syncthreads();
  if (!s_last) return;
  __threadfence();                                              /* (every thread of the last workgroup reads the others' records) */
  {
    uint32_t t[MAPS_PART_WORDS];
    for (int k = 0; k < MAPS_PART_WORDS; k++) t[k] = 0u;
    for (uint32_t g = threadIdx.x; g < a.n_wg; g += MAPS_BLOCK) d_maps_combine(t, a.part + (size_t)g * MAPS_PART_WORDS, 1, t);
    unsigned long long q = (unsigned long long)t[MAPS_QP_SUM] | (unsigned long long)t[MAPS_QP_SUM + 1] << 32;
    q = d_maps_add(q);
    for (int k = 0; k < MAPS_PART_WORDS; k++) if (k != MAPS_QP_SUM && k != MAPS_QP_SUM + 1) t[k] = (k == MAPS_QP_MIN || k == MAPS_QP_MAX) ? d_maps_max(t[k]) : d_maps_add(t[k]);
    t[MAPS_QP_SUM] = (uint32_t)q; t[MAPS_QP_SUM + 1] = (uint32_t)(q >> 32);
    if (lane == 0) for (int k = 0; k < MAPS_PART_WORDS; k++) s_wave[wv][k] = t[k];      /* (free again: thread 0 read it in front of the barrier that published s_last) */
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  uint32_t t[MAPS_PART_WORDS];
  d_maps_combine(t, &s_wave[0][0], MAPS_WAVES);
  for (int k = 0; k < MAPS_SKIPPED; k++) a.res[k] = t[k];
  for (int k = 0; k < 4; k++) a.res[MAPS_SKIPPED + k] = atomicExch(a.rec + MAPS_SKIPPED + k, 0u);     /* (the raster pass's counts: it ran before this launch) */
  __hip_atomic_store(a.rec + MAPS_ARRIVED, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  a.res[MAPS_ARRIVED + 1] = a.seq;
  a.res[MAPS_ARRIVED] = 1u;
}

void m355_launch_maps(const MapsArgs& a, hipStream_t st)
{
  if (a.wg_end[3]) hipLaunchKernelGGL(k_maps_raster, dim3(a.wg_end[3]), dim3(MAPS_RASTER_BLOCK), 0, st, a);
  hipLaunchKernelGGL(k_maps_gather, dim3(a.n_wg), dim3(MAPS_BLOCK), 0, st, a);
}
