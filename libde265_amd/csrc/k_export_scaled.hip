/*
 * k_export_scaled.hip — a decoded frame (or a rectangle of it) into memory of the caller, downscaled by f = 2, 4 or 8 in both directions:
 * every output sample is the rounded average of an f x f block of its plane (m355_frame_export_scaled, include/de265_mi355x.h).  Layouts
 * and sample formats are those of k_export.hip; the sample formats are applied to the block SUM (one rounding).  Integer-exact.
 *
 * ONE launch covers every plane.  The traffic is the source, so lanes are mapped to the source: a lane loads the same 16 bytes of the f
 * source rows behind one output row (for an interleaved row: of both chroma planes) — all loads issued before the first use —, reduces them
 * to the 16 / (f * SB) output samples they cover and stores those; a wavefront covers 1024 consecutive bytes of each of its source rows:
 * which plane, output row and chunk is decided once per wavefront, in scalar registers.  Stores are 1 / f^2 of the bytes, 1 to 32 bytes
 * per lane, plain (the consumer reads the data next); the last lane of a row stores its valid samples only.
 * Arithmetic, exact for the whole sample range: 8-bit samples are summed in pairs inside 16-bit lanes ((v & 0x00FF00FF) + ((v >> 8) &
 * 0x00FF00FF)) and rows are added with packed 16-bit adds — a lane holds at most 2 * 8 * 255; 16-bit samples are widened to 32-bit pair
 * sums ((v & 0xFFFF) + (v >> 16)) before anything is added.  A block sum has up to 22 bits and lives in 32.
 * A lane's 16 bytes start at a sample of the row (the row's bytes are a multiple of f * SB, so a vector that starts inside the row covers
 * whole output samples) and rows row * f .. row * f + f - 1 lie inside the rectangle: a lane reads at most 16 bytes from a sample inside
 * a row of the plane, which stays inside the plane's allocation (rows are padded to 128 bytes and a plane ends with a 256-byte tail,
 * runtime_internal.h frame_alloc) — half the span k_export.hip argues for.
 * Roofline: pure traffic — every source byte read once.
 */
#include "k_common.h"

/* a 2-byte store at any address (k_asm.h has none) */
#ifdef SIMT_EMU
static inline void d_stg2(void* p, unsigned v) { const unsigned short t = (unsigned short)v; memcpy(p, &t, 2); }
#else
__device__ __forceinline__ void d_stg2(M355_GLOBAL void* p, unsigned v) { *(M355_GLOBAL m355_h1*)p = (unsigned short)v; }
#endif

/* F rows of 16 bytes -> the 16 / (F * SB) block sums they cover.  First the sums of horizontal sample pairs, added over the rows (P: 8 / SB
   of them), then F / 2 neighbours of those each */
template <int SB, int F>
__device__ __forceinline__ void d_block_sums(const unsigned (*raw)[4], unsigned* S)
{
  constexpr int NP = 8 / SB, G = F / 2;
  unsigned P[NP];
  if (SB == 1) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
      unsigned acc = 0;
#pragma unroll
      for (int r = 0; r < F; r++) acc = d_pk_add16(acc, (raw[r][i] & 0x00FF00FFu) + ((raw[r][i] >> 8) & 0x00FF00FFu));
      P[2 * i] = acc & 0xFFFFu; P[2 * i + 1] = acc >> 16;
    }
  } else {
#pragma unroll
    for (int i = 0; i < 4; i++) {
      unsigned acc = 0;
#pragma unroll
      for (int r = 0; r < F; r++) acc += (raw[r][i] & 0xFFFFu) + (raw[r][i] >> 16);
      P[i] = acc;
    }
  }
#pragma unroll
  for (int j = 0; j < NP / G; j++) {
    unsigned s = 0;
#pragma unroll
    for (int t = 0; t < G; t++) s += P[j * G + t];
    S[j] = s;
  }
}

/* a block sum -> the output sample: min(clip, (S + half) >> rs) << ls  (NATIVE: rs = 2k; MSB16: rs = 2k, ls = 16 - bit depth; U8: rs = 2k + bit depth - 8,
   and 255 is what the clip is for: the maximum sample rounds to 256) */
template <int DB>
__device__ __forceinline__ unsigned d_scaled_sample(unsigned S, int rs, int ls)
{
  const unsigned v = (S + (1u << (rs - 1))) >> rs;
  return (DB == 1 ? (v < 255u ? v : 255u) : v) << ls;
}

/* NS samples of DB bytes as OB = NS * DB bytes at d, or the first nb of them: whole lanes store one vector (two for 32 bytes), the end of a row
   goes out as dwords, a 16-bit half and a single byte */
template <int DB, int NS>
__device__ __forceinline__ void d_scaled_store(M355_GLOBAL uint8_t* d, const unsigned* w, uint32_t nb)
{
  constexpr int OB = NS * DB, ND = (OB + 3) / 4;
  unsigned o[ND];
#pragma unroll
  for (int i = 0; i < ND; i++) {
    o[i] = 0;
    if (DB == 1) {
#pragma unroll
      for (int b = 0; b < 4; b++) if (4 * i + b < NS) o[i] |= w[4 * i + b] << (8 * b);
    } else {
#pragma unroll
      for (int b = 0; b < 2; b++) if (2 * i + b < NS) o[i] |= w[2 * i + b] << (16 * b);
    }
  }
  if (nb >= (uint32_t)OB) {
    if (OB == 32) { d_stg16(d, o); d_stg16(d + 16, o + 4); }
    else if (OB == 16) d_stg16(d, o);
    else if (OB == 8) d_stg8(d, o);
    else if (OB == 4) d_stg4(d, o[0]);
    else if (OB == 2) d_stg2(d, o[0]);
    else d[0] = (uint8_t)o[0];
    return;
  }
#pragma unroll
  for (int i = 0; i < ND; i++) {
    if (4u * i + 4 <= nb) d_stg4(d + 4 * i, o[i]);
    else {
      if (4u * i + 2 <= nb) d_stg2(d + 4 * i, o[i]);
      if (nb > 4u * i && (nb & 1u)) d[nb - 1] = (uint8_t)(o[i] >> (8 * ((nb - 1) & 3u)));
    }
  }
}

/* one lane: load, reduce, convert, store.  s2: the Cr plane of an interleaved row.  n: the lane's valid output samples (per plane) */
template <int SB, int DB, int K, bool INTER>
__device__ __forceinline__ void d_export_scaled_lane(const M355_GLOBAL uint8_t* s, const M355_GLOBAL uint8_t* s2, long long pitch, M355_GLOBAL uint8_t* d,
                                                     uint32_t n, int rs, int ls)
{
  constexpr int F = 1 << K, NOUT = 16 / (F * SB), NS = INTER ? 2 * NOUT : NOUT;
  unsigned raw[F][4], raw2[INTER ? F : 1][4];
#pragma unroll
  for (int r = 0; r < F; r++) d_ldg16(s + (size_t)r * pitch, raw[r]);
  if (INTER) {
#pragma unroll
    for (int r = 0; r < F; r++) d_ldg16(s2 + (size_t)r * pitch, raw2[r]);
  }
  unsigned S[NOUT], w[NS];
  d_block_sums<SB, F>(raw, S);
#pragma unroll
  for (int j = 0; j < NOUT; j++) w[INTER ? 2 * j : j] = d_scaled_sample<DB>(S[j], rs, ls);
  if (INTER) {
    d_block_sums<SB, F>(raw2, S);
#pragma unroll
    for (int j = 0; j < NOUT; j++) w[2 * j + 1] = d_scaled_sample<DB>(S[j], rs, ls);
  }
  d_scaled_store<DB, NS>(d, w, n * (uint32_t)(DB * (INTER ? 2 : 1)));
}

/* (the selection idiom of k_export.hip: the three entries of an argument table as scalars, two scalar compares) */
#define M355_EXPORT_SEL(arr) (p2 ? (arr)[2] : (p1 ? (arr)[1] : (arr)[0]))

template <int SB, int DB, int SEMI, int K>
__global__ void __launch_bounds__(256) k_export_scaled(ExportScaledArgs a)
{
  M355_GATE(a);
  constexpr int F = 1 << K, NOUT = 16 / (F * SB);
  /* this wavefront's unit: plane, output row, position in the source rows */
  const uint32_t unit = __builtin_amdgcn_readfirstlane((uint32_t)(blockIdx.x * 4u + (threadIdx.x >> 6)));
  if (unit >= a.unit_end[2]) return;
  const bool p1 = unit >= a.unit_end[0], p2 = unit >= a.unit_end[1];
  const uint32_t u = unit - (p2 ? a.unit_end[1] : (p1 ? a.unit_end[0] : 0u));
  const uint32_t chunks = M355_EXPORT_SEL(a.chunks), row = u / chunks, chunk = u - row * chunks;
  const uint32_t ow = M355_EXPORT_SEL(a.out_w), vec = chunk * 64u + (threadIdx.x & 63u), o0 = vec * NOUT;
  if (o0 >= ow) return;
  const uint32_t n = ow - o0 < (uint32_t)NOUT ? ow - o0 : (uint32_t)NOUT;
  const int rs = M355_EXPORT_SEL(a.rshift), ls = M355_EXPORT_SEL(a.lshift);
  const bool inter = SEMI && p1;                            /* (semi-planar: plane 1 is the last one) */
  const long long pitch = M355_EXPORT_SEL(a.src_pitch);
  const size_t sofs = (size_t)row * F * (size_t)pitch + (size_t)vec * 16u;
  const M355_GLOBAL uint8_t* s = (const M355_GLOBAL uint8_t*)M355_EXPORT_SEL(a.src) + sofs;
  M355_GLOBAL uint8_t* d = (M355_GLOBAL uint8_t*)M355_EXPORT_SEL(a.dst) + (size_t)row * M355_EXPORT_SEL(a.dst_pitch) + (size_t)o0 * (inter ? 2 * DB : DB);
  if (inter) d_export_scaled_lane<SB, DB, K, true>(s, (const M355_GLOBAL uint8_t*)a.src[2] + sofs, pitch, d, n, rs, ls);
  else d_export_scaled_lane<SB, DB, K, false>(s, s, pitch, d, n, rs, ls);
}

void m355_launch_export_scaled(const ExportScaledArgs& a, int src_bytes, int dst_bytes, bool semiplanar, int log2_scale, hipStream_t st)
{
  const uint32_t units = a.unit_end[2];
  if (!units) return;
  const dim3 grid((units + 3) / 4), block(256);
#define M355_EXPORT_SCALED_K(SB, DB, K) \
  if (log2_scale == K) { \
    if (semiplanar) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_export_scaled<SB, DB, 1, K>), grid, block, 0, st, a); \
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_export_scaled<SB, DB, 0, K>), grid, block, 0, st, a); \
  }
#define M355_EXPORT_SCALED_CASE(SB, DB) \
  if (src_bytes == SB && dst_bytes == DB) { M355_EXPORT_SCALED_K(SB, DB, 1) M355_EXPORT_SCALED_K(SB, DB, 2) M355_EXPORT_SCALED_K(SB, DB, 3) }
  M355_EXPORT_SCALED_CASE(1, 1) M355_EXPORT_SCALED_CASE(1, 2) M355_EXPORT_SCALED_CASE(2, 1) M355_EXPORT_SCALED_CASE(2, 2)
#undef M355_EXPORT_SCALED_CASE
#undef M355_EXPORT_SCALED_K
}
