/*
 * k_export_oriented.hip — m355_frame_export and m355_frame_export_pixels with the picture turned in the same launch: mirrored, flipped, transposed, or
 * any composition of the three (m355_frame_export_oriented, m355_frame_export_pixels_oriented, include/de265_mi355x.h; orientation.h is the
 * definition).  A pure permutation of ELEMENTS of 1, 2 or 4 bytes — a u8 sample; a u16 sample or a u8 (Cb, Cr) pair; a u16 pair or a pixel —, whose
 * values are made by the code of the plain exports: d_export_load / d_export_convert (k_export_dev.h) and d_rgb_pixels_lane (k_rgb_dev.h, pixel_pack.h).
 *
 * ONE launch covers every plane; every source byte is read once, every destination byte written once.  The orientation's three bits are wave-uniform
 * kernel arguments: they change addresses, a byte permute and which of two paths a workgroup takes, not the instantiation.
 *
 * WITHOUT TRANSPOSE the units are k_export's (k_export_pixels'): a wavefront takes 64 lanes' worth of one row, a lane 16 destination bytes (the pixels:
 * the 16 / SB pixels behind one luma vector), with vector loads and vector stores.  FLIP is the destination row ph - 1 - row.  MIRROR: the lane loads
 * the MIRRORED chunk — the source elements pw - x - n .. pw - x - 1 behind its destination elements x .. x + n - 1 — and reverses the elements in
 * registers (one v_perm_b32 per dword with a selector picked by the element size, and the dwords in reverse order).  The row's last lane has m < n
 * elements left: it loads n elements from source element 0, m of which are its own, and after the reversal they are the LAST m elements of the
 * vector; the planes' path shifts the vector down by 16 - m * E bytes (two selects and a v_alignbyte_b32 per dword) and stores as d_export_store
 * does, dwords and single bytes; the pixels' path stores its last m dwords one by one.  No LDS is touched.
 *
 * WITH TRANSPOSE a workgroup takes one tile of 64 x 64 elements of the SOURCE rectangle through LDS:
 *   1. LOAD     as above along source rows: a lane loads and converts 16 destination bytes' worth (the pixels: 16 / SB pixels), 256 lanes 64 / E rows
 *               of the tile per pass, E passes (the pixels: SB passes); all passes are unrolled, so every load is in flight before the first use.
 *   2. LDS      the converted dwords go to a padded image of the tile: row r starts at dword r * (16 E + 1) + 2 * (r >> 5).
 *   3. READ     column-wise: a lane gathers the 16 / E elements of ONE source column c from consecutive tile rows — 16 destination bytes of
 *               destination row c — with one ds_read_u8 / _u16 / _b32 each and packs them (v_perm_b32).  MIRROR reads the rows in reverse order, which
 *               costs nothing; FLIP is the destination row pw - 1 - c.
 *   4. STORE    16-byte vectors along DESTINATION rows, the byte-aligned forms of k_asm.h; 4 E consecutive lanes write the 64 E bytes of one
 *               destination row of the tile, a wavefront 64 / (4 E) rows.  A row's end leaves as dwords and single bytes (d_export_store).  No lane
 *               ever stores a single element per row.
 * Partial tiles: R <= 64 source rows and C <= 64 source columns are valid; lanes beyond them neither load nor store, and every lane reaches the
 * barrier.  With MIRROR the tile's destination columns start at ph - sy0 - R, so a partial tile's rows still start at their first valid element.
 *
 * LDS BANKS (gfx950: bank (a / 4) % 32 per 32-lane half for ds_write_b32, ds_read_b32 and the sub-dword reads).
 *   READ   the lanes of a half are 4 E row groups q (rows q * 16 / E + j) x 8 / E columns c: bank = (q * (16 / E) * (16 E + 1) + 2 * (r >> 5) + j (16 E
 *          + 1) + c E / 4) % 32 = (16 q / E + 2 (q >= 2 E) + j + c E / 4 + const) % 32.  E = 4: 4 q % 32 has 8 values, each for q and q + 8, which the
 *          + 2 of the upper 32 rows separates, and c adds 0 or 1: 32 distinct banks.  E = 2: 8 q % 32 has 4 values, + 2 for q >= 4, four columns share
 *          two dwords: 16 distinct dwords on 16 banks.  E = 1: 16 q % 32 has 2 values, + 2 for q >= 2, eight columns share two dwords: 8 dwords on 8
 *          banks.  0 conflicts in every case — without the 2 dwords between the halves of the tile each would be 2-way.
 *   WRITE  dword i of the lane at tile row r, chunk k goes to bank (r (16 E + 1) + 2 (r >> 5) + 4 k + i) % 32.  Planes, E = 2: 8 chunks x 4 rows of a
 *          half, 4 k + r distinct: 0 conflicts.  E = 4: 16 chunks x 2 rows, 4 k wraps at k = 8: 2-way.  E = 1: 4 chunks x 8 rows, 17 r + 4 k: 2-way.
 *          Pixels: 16 / SB dwords per lane, chunks 16 or 8 dwords apart: 2-way.  A 2-way conflict of a ds_write_b32 costs no cycle: the store's
 *          cycles are set by the transfer of its registers to the LDS, not by the LDS array.
 * profiles/export_oriented_codegen.txt has the compiler's resource lines (no scratch) and this count per instantiation.
 *
 * No out-of-bounds read.  Every global load is one of the plain exports' loads at a first element INSIDE a row of the rectangle: row sy0 + r < ph, element
 * sx0 + k n < pw (MIRROR without TRANSPOSE: element pw - x - m >= 0, m >= 1).  A lane reads up to 32 bytes from there — beyond the rectangle where it
 * ends, never beyond the plane's allocation: rows are padded to 128 bytes and a plane ends with a 256-byte tail (runtime_internal.h frame_alloc), the
 * argument of k_export.hip; for the pixels it is the argument of k_export_rgb.hip with X0 < x0 + width, Y < y0 + height.  LDS reads stay inside the
 * image: tile rows are taken modulo 64 (a lane of a partial tile may read rows nobody wrote; it stores none of them).
 * No out-of-bounds write: a lane stores min(16, (R - q n) E) bytes at destination element Xb + q n of a destination row 0 <= Y < pw, Xb + R <= ph.
 * Roofline: pure traffic, as the plain exports; the tile's 64 E-byte destination runs are half a cache line for E = 1, one for E = 2, two for E = 4.
 */
#include "k_common.h"
#include "k_export_dev.h"   /* d_export_load, d_export_convert, d_export_store, M355_EXPORT_SEL: shared with k_export.hip */
#include "k_rgb_dev.h"      /* d_rgb_pixels_lane: shared with k_export_rgb.hip */

#define OT M355_ORIENT_TILE
/* the padded LDS image of a tile of elements of E bytes: dwords per row, the first dword of row r, the dwords of the image */
#define OT_PITCH(E) (OT * (E) / 4 + 1)
#define OT_ROW(r, E) ((r) * (uint32_t)OT_PITCH(E) + (((r) >> 5) << 1))
#define OT_DWORDS(E) (OT * OT_PITCH(E) + 2)

/* the elements of a 16-byte vector in reverse order; le = log2 of the element's bytes (wave-uniform) */
__device__ __forceinline__ void d_orient_reverse16(unsigned* o, int le)
{
  const unsigned sel = le == 0 ? 0x00010203u : (le == 1 ? 0x01000302u : 0x03020100u);
  const unsigned t0 = d_perm(0, o[3], sel), t1 = d_perm(0, o[2], sel), t2 = d_perm(0, o[1], sel), t3 = d_perm(0, o[0], sel);
  o[0] = t0; o[1] = t1; o[2] = t2; o[3] = t3;
}
/* bytes sh .. 15 of a 16-byte vector to its front (sh = 0 .. 15) */
__device__ __forceinline__ void d_orient_shift_down16(unsigned* o, uint32_t sh)
{
  if (sh & 8u) { o[0] = o[2]; o[1] = o[3]; o[2] = 0; o[3] = 0; }
  if (sh & 4u) { o[0] = o[1]; o[1] = o[2]; o[2] = o[3]; o[3] = 0; }
  const unsigned b = sh & 3u;
  o[0] = __builtin_amdgcn_alignbyte(o[1], o[0], b); o[1] = __builtin_amdgcn_alignbyte(o[2], o[1], b);
  o[2] = __builtin_amdgcn_alignbyte(o[3], o[2], b); o[3] = __builtin_amdgcn_alignbyte(0u, o[3], b);
}

/* element c of tile row r of the image */
template <int E> __device__ __forceinline__ unsigned d_orient_elem(const unsigned* s_tile, uint32_t r, uint32_t c)
{
  if (E == 4) return s_tile[OT_ROW(r, E) + c];
  if (E == 2) return ((const uint16_t*)s_tile)[2u * OT_ROW(r, E) + c];
  return ((const uint8_t*)s_tile)[4u * OT_ROW(r, E) + c];
}

/* Steps 3 and 4 of a tile: R x C valid elements (source rows x source columns) of the image to the destination.  Source column c is destination row
   Yb + ystep * c, tile row r destination element Xb + r — mirror: Xb + R - 1 - r. */
template <int E>
__device__ __forceinline__ void d_orient_tile_store(const unsigned* s_tile, M355_GLOBAL uint8_t* dst, long long dst_pitch, uint32_t R, uint32_t C,
                                                    uint32_t Xb, uint32_t Yb, int ystep, bool mirror)
{
  constexpr uint32_t N = 16 / E, LPR = 4 * E;                /* elements per lane, lanes per destination row of the tile */
#pragma unroll
  for (uint32_t p = 0; p < (uint32_t)E; p++) {
    const uint32_t t = p * 256u + threadIdx.x, q = t % LPR, c = t / LPR, r0 = q * N;
    if (c >= C || r0 >= R) continue;
    unsigned e[N], o[4];
#pragma unroll
    for (uint32_t j = 0; j < N; j++) e[j] = d_orient_elem<E>(s_tile, (mirror ? R - 1u - (r0 + j) : r0 + j) & (uint32_t)(OT - 1), c);
    if constexpr (E == 4) { o[0] = e[0]; o[1] = e[1]; o[2] = e[2]; o[3] = e[3]; }
    else if constexpr (E == 2) {
#pragma unroll
      for (int i = 0; i < 4; i++) o[i] = d_pack_lo16(e[2 * i], e[2 * i + 1]);
    } else {
#pragma unroll
      for (int i = 0; i < 4; i++) o[i] = d_pack_lo16(d_perm(e[4 * i + 1], e[4 * i], 0x0c0c0400u), d_perm(e[4 * i + 3], e[4 * i + 2], 0x0c0c0400u));
    }
    const size_t Y = (size_t)((int64_t)Yb + (int64_t)ystep * (int64_t)c);
    d_export_store(dst + Y * (size_t)dst_pitch + (size_t)(Xb + r0) * E, o, (R - r0) * (uint32_t)E);
  }
}

/* Steps 1 and 2 of a tile of one plane: source rows sy0 .. sy0 + R - 1, elements sx0 .. sx0 + C - 1 of them */
template <int SB, int DB, bool INTER>
__device__ __forceinline__ void d_orient_tile_load(unsigned* s_tile, const M355_GLOBAL uint8_t* s, const M355_GLOBAL uint8_t* s2, long long src_pitch, int sh,
                                                   uint32_t sx0, uint32_t sy0, uint32_t R, uint32_t C)
{
  constexpr int E = INTER ? 2 * DB : DB;
  constexpr uint32_t N = 16 / E, LPR = 4 * E;
#pragma unroll
  for (uint32_t p = 0; p < (uint32_t)E; p++) {
    const uint32_t t = p * 256u + threadIdx.x, k = t % LPR, r = t / LPR;
    if (r >= R || k * N >= C) continue;
    const size_t sofs = (size_t)(sy0 + r) * (size_t)src_pitch + (size_t)(sx0 + k * N) * SB;
    unsigned raw[8], o[4];
    d_export_load<SB, DB, INTER>(s + sofs, s2 + sofs, raw);
    d_export_convert<SB, DB, INTER>(raw, sh, o);
#pragma unroll
    for (int i = 0; i < 4; i++) s_tile[OT_ROW(r, E) + 4u * k + i] = o[i];
  }
}

template <int SB, int DB, int SEMI>
__global__ void __launch_bounds__(256) k_export_oriented(ExportOrientedArgs a)
{
  M355_GATE(a);
  __shared__ unsigned s_tile[OT_DWORDS(SEMI ? 2 * DB : DB)];
  if (!a.transpose) {
    /* k_export's unit: plane, row, position in the row */
    const uint32_t unit = __builtin_amdgcn_readfirstlane((uint32_t)(blockIdx.x * 4u + (threadIdx.x >> 6)));
    if (unit >= a.unit_end[2]) return;
    const bool p1 = unit >= a.unit_end[0], p2 = unit >= a.unit_end[1];
    const uint32_t u = unit - (p2 ? a.unit_end[1] : (p1 ? a.unit_end[0] : 0u));
    const uint32_t chunks = M355_EXPORT_SEL(a.per_row), row = u / chunks, chunk = u - row * chunks;
    const bool inter = SEMI && p1;
    const int le = (DB == 2 ? 1 : 0) + (inter ? 1 : 0);       /* log2 of the element's bytes */
    const uint32_t pw = M355_EXPORT_SEL(a.pw), rb = pw << le, ofs = (chunk * 64u + (threadIdx.x & 63u)) * 16u;
    if (ofs >= rb) return;
    const uint32_t nb = rb - ofs, x = ofs >> le, n = 16u >> le;
    const uint32_t valid = pw - x < n ? pw - x : n;
    const uint32_t sx = a.mirror ? pw - x - valid : x;       /* first source element */
    const int sh = M355_EXPORT_SEL(a.shift);
    const size_t sofs = (size_t)row * M355_EXPORT_SEL(a.src_pitch) + (size_t)sx * SB;
    const M355_GLOBAL uint8_t* s = (const M355_GLOBAL uint8_t*)M355_EXPORT_SEL(a.src) + sofs;
    unsigned raw[8], o[4];
    if (inter) { d_export_load<SB, DB, true>(s, (const M355_GLOBAL uint8_t*)a.src[2] + sofs, raw); d_export_convert<SB, DB, true>(raw, sh, o); }
    else { d_export_load<SB, DB, false>(s, s, raw); d_export_convert<SB, DB, false>(raw, sh, o); }
    if (a.mirror) {
      d_orient_reverse16(o, le);
      if (nb < 16u) d_orient_shift_down16(o, 16u - nb);
    }
    const uint32_t drow = a.flip ? M355_EXPORT_SEL(a.ph) - 1u - row : row;
    d_export_store((M355_GLOBAL uint8_t*)M355_EXPORT_SEL(a.dst) + (size_t)drow * M355_EXPORT_SEL(a.dst_pitch) + ofs, o, nb);
    return;
  }
  /* this workgroup's tile: plane, position in the source rectangle */
  const uint32_t unit = blockIdx.x;
  const bool p1 = unit >= a.unit_end[0], p2 = unit >= a.unit_end[1];
  const uint32_t u = unit - (p2 ? a.unit_end[1] : (p1 ? a.unit_end[0] : 0u));
  const uint32_t tiles_x = M355_EXPORT_SEL(a.per_row), ty = u / tiles_x, tx = u - ty * tiles_x;
  const uint32_t pw = M355_EXPORT_SEL(a.pw), ph = M355_EXPORT_SEL(a.ph), sx0 = tx * OT, sy0 = ty * OT;
  const uint32_t C = pw - sx0 < (uint32_t)OT ? pw - sx0 : (uint32_t)OT, R = ph - sy0 < (uint32_t)OT ? ph - sy0 : (uint32_t)OT;
  const bool inter = SEMI && p1;
  const int sh = M355_EXPORT_SEL(a.shift);
  const long long src_pitch = M355_EXPORT_SEL(a.src_pitch), dst_pitch = M355_EXPORT_SEL(a.dst_pitch);
  const M355_GLOBAL uint8_t* s = (const M355_GLOBAL uint8_t*)M355_EXPORT_SEL(a.src);
  M355_GLOBAL uint8_t* d = (M355_GLOBAL uint8_t*)M355_EXPORT_SEL(a.dst);
  const uint32_t Xb = a.mirror ? ph - sy0 - R : sy0, Yb = a.flip ? pw - 1u - sx0 : sx0;
  const int ystep = a.flip ? -1 : 1;
  if (inter) d_orient_tile_load<SB, DB, true>(s_tile, s, (const M355_GLOBAL uint8_t*)a.src[2], src_pitch, sh, sx0, sy0, R, C);
  else d_orient_tile_load<SB, DB, false>(s_tile, s, s, src_pitch, sh, sx0, sy0, R, C);
  __syncthreads();
  if (inter) d_orient_tile_store<2 * DB>(s_tile, d, dst_pitch, R, C, Xb, Yb, ystep, a.mirror != 0u);
  else d_orient_tile_store<DB>(s_tile, d, dst_pitch, R, C, Xb, Yb, ystep, a.mirror != 0u);
}

void m355_launch_export_oriented(const ExportOrientedArgs& a, int src_bytes, int dst_bytes, bool semiplanar, hipStream_t st)
{
  const uint32_t units = a.unit_end[2];
  if (!units) return;
  const dim3 grid(a.transpose ? units : (units + 3) / 4), block(256);
#define M355_ORIENT_CASE(SB, DB) \
  if (src_bytes == SB && dst_bytes == DB) { \
    if (semiplanar) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_export_oriented<SB, DB, 1>), grid, block, 0, st, a); \
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_export_oriented<SB, DB, 0>), grid, block, 0, st, a); \
  }
  M355_ORIENT_CASE(1, 1) M355_ORIENT_CASE(1, 2) M355_ORIENT_CASE(2, 1) M355_ORIENT_CASE(2, 2)
#undef M355_ORIENT_CASE
}

/* The pixels: k_export_pixels' units, loads, chroma reconstruction, matrix and pack — d_rgb_pixels_lane as it is, in the SOURCE's orientation —, then
   the dwords go where the orientation puts them.  An element is a dword, so a row's end is whole dwords. */
template <int SB, bool TEN, int CF, int LOC>
__global__ void __launch_bounds__(256) k_export_pixels_oriented(ExportPixelsOrientedArgs a)
{
  M355_GATE(a.r);
  constexpr int NP = 16 / SB;
  __shared__ unsigned s_tile[OT_DWORDS(4)];
  if (!a.transpose) {
    const uint32_t unit = __builtin_amdgcn_readfirstlane((uint32_t)(blockIdx.x * 4u + (threadIdx.x >> 6)));
    if (unit >= a.r.units) return;
    const uint32_t row = unit / a.r.chunks, chunk = unit - row * a.r.chunks;
    const uint32_t p0 = (chunk * 64u + (threadIdx.x & 63u)) * NP;
    if (p0 >= a.r.width) return;
    const uint32_t n = a.r.width - p0 < (uint32_t)NP ? a.r.width - p0 : (uint32_t)NP;
    unsigned o[NP];
    d_rgb_pixels_lane<SB, TEN, CF, LOC>(a.r, a.r.x0 + (a.mirror ? a.r.width - p0 - n : p0), a.r.y0 + row, o);
    const uint32_t drow = a.flip ? a.r.height - 1u - row : row;
    M355_GLOBAL uint8_t* d = (M355_GLOBAL uint8_t*)a.r.dst[0] + (size_t)drow * a.r.dst_pitch[0] + (size_t)p0 * 4u;
    if (a.mirror) {
#pragma unroll
      for (int k = 0; k < NP / 2; k++) { const unsigned t = o[k]; o[k] = o[NP - 1 - k]; o[NP - 1 - k] = t; }
      if (n < (uint32_t)NP) {                                   /* the row's last lane: its pixels are the last n of the reversed vector */
#pragma unroll
        for (uint32_t k = 0; k < (uint32_t)NP; k++) if (k + n >= (uint32_t)NP) d_stg4(d + 4u * (k + n - NP), o[k]);
        return;
      }
    }
#pragma unroll
    for (uint32_t k = 0; k < (uint32_t)NP; k += 4) if (k < n) d_export_store(d + 4u * k, o + k, (n - k) * 4u);
    return;
  }
  const uint32_t tiles_x = a.r.chunks, ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x, sx0 = tx * OT, sy0 = ty * OT;
  const uint32_t C = a.r.width - sx0 < (uint32_t)OT ? a.r.width - sx0 : (uint32_t)OT, R = a.r.height - sy0 < (uint32_t)OT ? a.r.height - sy0 : (uint32_t)OT;
  constexpr uint32_t LPR = OT / NP;                            /* lanes per source row of the tile */
#pragma unroll
  for (uint32_t p = 0; p < (uint32_t)SB; p++) {
    const uint32_t t = p * 256u + threadIdx.x, k = t % LPR, r = t / LPR;
    if (r >= R || k * NP >= C) continue;
    unsigned o[NP];
    d_rgb_pixels_lane<SB, TEN, CF, LOC>(a.r, a.r.x0 + sx0 + k * NP, a.r.y0 + sy0 + r, o);
#pragma unroll
    for (int i = 0; i < NP; i++) s_tile[OT_ROW(r, 4) + k * NP + i] = o[i];
  }
  __syncthreads();
  d_orient_tile_store<4>(s_tile, (M355_GLOBAL uint8_t*)a.r.dst[0], a.r.dst_pitch[0], R, C, a.mirror ? a.r.height - sy0 - R : sy0,
                         a.flip ? a.r.width - 1u - sx0 : sx0, a.flip ? -1 : 1, a.mirror != 0u);
}

void m355_launch_export_pixels_oriented(const ExportPixelsOrientedArgs& a, int src_bytes, bool ten, int chroma_format, int chroma_loc, hipStream_t st)
{
  if (!a.r.units) return;
  const dim3 grid(a.transpose ? a.r.units : (a.r.units + 3) / 4), block(256);
  const int loc = chroma_format == 1 ? chroma_loc : 0;          /* (the siting is 4:2:0's alone) */
#define M355_ORIENT_PX_CF(SB, TEN, CF, LOC) \
  if (chroma_format == CF && loc == LOC) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_export_pixels_oriented<SB, TEN, CF, LOC>), grid, block, 0, st, a);
#define M355_ORIENT_PX_CASE(SB, TEN) \
  if (src_bytes == SB && ten == TEN) { \
    M355_ORIENT_PX_CF(SB, TEN, 0, 0) M355_ORIENT_PX_CF(SB, TEN, 1, 0) M355_ORIENT_PX_CF(SB, TEN, 2, 0) M355_ORIENT_PX_CF(SB, TEN, 3, 0) \
    M355_ORIENT_PX_CF(SB, TEN, 1, 1) M355_ORIENT_PX_CF(SB, TEN, 1, 2) M355_ORIENT_PX_CF(SB, TEN, 1, 3) \
  }
  M355_ORIENT_PX_CASE(1, false) M355_ORIENT_PX_CASE(1, true) M355_ORIENT_PX_CASE(2, false) M355_ORIENT_PX_CASE(2, true)
#undef M355_ORIENT_PX_CASE
#undef M355_ORIENT_PX_CF
}
