/*
 * k_export.hip — a decoded frame (or a rectangle of it) into memory of the caller, in the layout a consumer on the same GPU
 * reads: planar or semi-planar (NV12 / P010 shapes), samples as they are, MSB-aligned 16-bit, or rounded to 8 bits
 * (m355_frame_export, include/de265_mi355x.h).  Integer-exact: no colour conversion, no scaling.
 *
 * ONE launch covers every plane.  A lane produces 16 destination bytes of one row — a vector load (two for 16 -> 8 bits, one per
 * chroma plane for an interleaved row), the conversion in packed 16-bit arithmetic, one vector store —, a wavefront 1024
 * consecutive destination bytes of one row: which plane, row and chunk is decided once per wavefront, in scalar registers.
 * (Several rows per wavefront with all their loads in flight before the first store, and streaming stores, were built and measured:
 * 2, 4 and 8 rows each cost the 8K export 1-3 %, the stores change nothing — profiles/export_bench.txt.)
 * A crop starts the source rows at any sample and the caller's pitch starts the destination rows at any byte: loads and stores
 * are the byte-aligned vector forms of k_asm.h (one global_load / global_store_dwordx4 each, whatever the address); the last lane
 * of a row stores its valid bytes only, as dwords and single bytes, so nothing beyond the exported row is written.  A lane reads
 * up to 32 bytes from its first source sample, which lies inside the row: that stays inside the plane's allocation (rows are
 * padded to 128 bytes and a plane ends with a 256-byte tail, runtime_internal.h frame_alloc).
 * Roofline: pure traffic — every source byte read once, every destination byte written once; plain stores (the consumer reads
 * the data next).
 */
#include "k_common.h"
#include "k_export_dev.h"   /* d_export_load, d_export_convert, d_export_store: shared with k_export_oriented.hip */

template <int SB, int DB, int SEMI>
__global__ void __launch_bounds__(256) k_export(ExportArgs a)
{
  M355_GATE(a);
  /* this wavefront's unit: plane, row, position in the row */
  const uint32_t unit = __builtin_amdgcn_readfirstlane((uint32_t)(blockIdx.x * 4u + (threadIdx.x >> 6)));
  if (unit >= a.unit_end[2]) return;
  const bool p1 = unit >= a.unit_end[0], p2 = unit >= a.unit_end[1];
  const uint32_t u = unit - (p2 ? a.unit_end[1] : (p1 ? a.unit_end[0] : 0u));
  const uint32_t chunks = M355_EXPORT_SEL(a.chunks), row = u / chunks, chunk = u - row * chunks;
  const uint32_t rb = M355_EXPORT_SEL(a.row_bytes), ofs = (chunk * 64u + (threadIdx.x & 63u)) * 16u;
  if (ofs >= rb) return;
  const int sh = M355_EXPORT_SEL(a.shift);
  const bool inter = SEMI && p1;                            /* (semi-planar: plane 1 is the last one) */
  /* source bytes in front of this lane's first sample: ofs / DB samples of the row, half as many per plane of an interleaved one */
  const size_t sofs = (size_t)row * M355_EXPORT_SEL(a.src_pitch) + (size_t)(ofs / (inter ? 2 * DB : DB)) * SB;
  const M355_GLOBAL uint8_t* s = (const M355_GLOBAL uint8_t*)M355_EXPORT_SEL(a.src) + sofs;
  unsigned raw[8], o[4];
  if (inter) { d_export_load<SB, DB, true>(s, (const M355_GLOBAL uint8_t*)a.src[2] + sofs, raw); d_export_convert<SB, DB, true>(raw, sh, o); }
  else { d_export_load<SB, DB, false>(s, s, raw); d_export_convert<SB, DB, false>(raw, sh, o); }
  d_export_store((M355_GLOBAL uint8_t*)M355_EXPORT_SEL(a.dst) + (size_t)row * M355_EXPORT_SEL(a.dst_pitch) + ofs, o, rb - ofs);
}

void m355_launch_export(const ExportArgs& a, int src_bytes, int dst_bytes, bool semiplanar, hipStream_t st)
{
  const uint32_t units = a.unit_end[2];
  if (!units) return;
  const dim3 grid((units + 3) / 4), block(256);
#define M355_EXPORT_CASE(SB, DB) \
  if (src_bytes == SB && dst_bytes == DB) { \
    if (semiplanar) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_export<SB, DB, 1>), grid, block, 0, st, a); \
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_export<SB, DB, 0>), grid, block, 0, st, a); \
  }
  M355_EXPORT_CASE(1, 1) M355_EXPORT_CASE(1, 2) M355_EXPORT_CASE(2, 1) M355_EXPORT_CASE(2, 2)
#undef M355_EXPORT_CASE
}
