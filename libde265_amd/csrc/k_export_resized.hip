/*
 * k_export_resized.hip — a decoded frame (or a rectangle of it) into memory of the caller, every plane RESIZED on its own grid to the size the
 * consumer asks for (m355_frame_export_resized, include/de265_mi355x.h holds the definition): a separable triangle filter widened by the downscale
 * ratio, coefficients of 14 bits from resize_taps.h — the function m355_resize_taps is —, vertical pass, ONE rounding to an 18-bit intermediate t,
 * horizontal pass, the sample formats of k_export.hip applied to the horizontal sum (one rounding).  Integer-exact.  The filter is a template parameter:
 * M355_FILTER_CUBIC (Catmull-Rom, m355_frame_export_resized_filtered) runs the same procedure in signed arithmetic, as the comment at the template says.
 * Which axes of a plane are co-sited are two flags per plane of the kernel arguments (cosited, cosited_y: the chroma sample location type of
 * m355_export_opts), wave-uniform, read where the filter rows are derived.
 *
 * ONE launch covers every plane.  A workgroup of 256 lanes owns a tile of up to 256 output columns x 16 output rows of one plane (of Cb AND Cr for an
 * interleaved plane).  Prologue: lane i derives the horizontal row of output column i into registers (through LDS: the row function indexes its
 * result, registers cannot be indexed), the last 16 lanes the vertical rows of the tile's output rows into LDS; the tile's first and last column
 * give the span of source columns the tile reads.  There are no tables from the host.  Then, per output row:
 *   1. vertical: the lanes are mapped to the SOURCE — lane v owns the same 16 bytes (the v-th vector of the span, starting at the span's first
 *      sample, whatever its alignment) of each of the at most 16 source rows of the filter row, loads them in batches of 8 rows, all loads of a
 *      batch issued before the first use — the first batch of the NEXT output row before the horizontal pass of this one —, and accumulates u for its 16 / SB samples, two rows per v_dot2_u32_u16 (samples and coefficients fit
 *      16 bits); the first row and the row count are wave-uniform and held in scalar registers (readfirstlane), the coefficient pairs are broadcast
 *      reads from LDS at their use.  No global load per tap anywhere: a lane's load serves 8 or 16 samples of one tap
 *   2. u is rounded to t and the tile's t row, halo included, goes to LDS (32-bit entries; two rows alternate, so a row costs one barrier)
 *   3. horizontal: lane i sums its at most 16 t values from LDS against the coefficients in its registers, converts and stores its sample — a row
 *      of consecutive samples per wavefront; Cb and Cr of an interleaved row as one pair per lane; a lane beyond the row's end stores nothing
 * Reads stay inside the plane's allocation: a filter row's source indices are clamped to the rectangle (resize_taps.h), so every row read is a row
 * of the rectangle and every vector starts at a sample of the span, which ends at a sample of the rectangle; a lane reads at most 16 bytes from
 * there, i.e. less than 16 bytes beyond a sample inside a row of the plane, and rows are padded to 128 bytes and a plane ends with a 256-byte tail
 * (runtime_internal.h frame_alloc) — the argument of k_export_scaled.hip.  The t row holds RS_SPAN entries: 256 columns advance by at most
 * 255 * 8 + 1 source samples, a row adds at most 16 and the last vector at most 15 more (the cubic filter: at most 255 * 4 + 1, and 16, and 15); the
 * vector count is clamped to the array all the same.
 * Arithmetic in unsigned 32 bits: u < 2^(bd + 14) <= 2^30, t < 2^18, v < 2^32 (the coefficients of a row sum to 1 << 14), and
 * ((v >> 1) + (1 << (30 - b))) >> (31 - b) is (v + (1 << (31 - b))) >> (32 - b) without the 33rd bit (b: the bit depth, 8 for U8).
 * Traffic: every source row is read by the two output rows it contributes to when downscaling (the second read is served by the caches) and once
 * per tile by the halo; stores are 1 to 4 bytes per lane.  At the 8K 10-bit geometry the kernel takes 46 to 67 us against the 37 us of the plain
 * export (profiles/export_resized_bench.txt says what was and was not tried): feeding both output rows from one load of a source row is the next step.
 */
#include "k_common.h"
#include "resize_taps.h"
#include "k_resize_dev.h"

#define RS_TW M355_RESIZE_TILE_W
#define RS_TH M355_RESIZE_TILE_H
#define RS_SPAN 2112                /* >= 255 * 8 + 1 + 16 + 15 = 2072, and 2 * RS_SPAN >= 16 * RS_TW for the prologue's coefficient rows */

/* (the selection idiom of k_export.hip: the three entries of an argument table as scalars, two scalar compares) */
#define M355_EXPORT_SEL(arr) (p2 ? (arr)[2] : (p1 ? (arr)[1] : (arr)[0]))

/* FILTER = M355_FILTER_CUBIC: the same procedure in signed 32 bits — rows of resize_taps.h's cubic filter (coefficients of 16 bits, some negative), the
   vertical pass with the signed dot product, the rounding to a t of 16 bits of fraction (a.tshift = bd - 2), v_mad_i32_i24 in the horizontal pass
   (|t| < 2^18, |q| < 2^15), an arithmetic shift (a.oshift = 30 - bd, 22 for U8) and the clip to the sample range.  Samples of 16 bits are no signed
   16-bit operands: they are taken less 2^15 (one XOR per packed pair) and 2^15 * 2^14 is added to the sum, which is exact since a row sums to 1 << 14. */
template <int SB, int DB, int SEMI, int FILTER>
__global__ void __launch_bounds__(256) k_export_resized(ExportResizedArgs a)
{
  M355_GATE(a);
  constexpr int S = 16 / SB;
  constexpr bool CUBIC = FILTER == M355_FILTER_CUBIC;
  __shared__ unsigned s_t[2][2][RS_SPAN];         /* [output row & 1][plane]: the t row of the plane (of Cb and Cr); in the prologue: the lanes' horizontal rows */
  __shared__ int32_t s_vy[RS_TH][2 + M355_RESIZE_MAX_TAPS];   /* per output row of the tile: first source row, number of rows, coefficients */
  __shared__ int32_t s_span[2];                   /* first and last source column of the tile */
  const uint32_t tid = threadIdx.x, unit = blockIdx.x;
  if (unit >= a.unit_end[2]) return;
  const bool p1 = unit >= a.unit_end[0], p2 = unit >= a.unit_end[1];
  const uint32_t u0 = unit - (p2 ? a.unit_end[1] : (p1 ? a.unit_end[0] : 0u));
  const uint32_t tiles_x = M355_EXPORT_SEL(a.tiles_x), run = u0 / tiles_x, tile = u0 - run * tiles_x;
  const uint32_t snx = M355_EXPORT_SEL(a.sn_x), sny = M355_EXPORT_SEL(a.sn_y), dnx = M355_EXPORT_SEL(a.dn_x), dny = M355_EXPORT_SEL(a.dn_y);
  const bool inter = SEMI && p1;                            /* (semi-planar: plane 1 is the last one) */
  const int nc = inter ? 2 : 1;
  const uint32_t tw = M355_EXPORT_SEL(a.tile_w), c0 = tile * tw, j0 = run * RS_TH;
  const uint32_t ncols = dnx - c0 < tw ? dnx - c0 : tw, nrows = dny - j0 < (uint32_t)RS_TH ? dny - j0 : (uint32_t)RS_TH;

  /* prologue: the filter rows of this tile */
  int32_t* hrow = (int32_t*)&s_t[0][0][0];                     /* coefficient k of lane i at [k * RS_TW + i] */
  int32_t hfirst = 0;
  unsigned hq[M355_RESIZE_MAX_TAPS];
  if (tid < ncols) {
    int hn;
    if constexpr (CUBIC) hn = m355_resize_row_cubic(snx, dnx, (int)M355_EXPORT_SEL(a.cosited), c0 + tid, &hfirst, hrow + tid, RS_TW);
    else hn = m355_resize_row(snx, dnx, (int)M355_EXPORT_SEL(a.cosited), c0 + tid, &hfirst, hrow + tid, RS_TW);
    if (tid == 0) s_span[0] = hfirst;
    if (tid == ncols - 1) s_span[1] = hfirst + hn - 1;
  }
  if (tid >= 256u - RS_TH && tid - (256u - RS_TH) < nrows) {
    const uint32_t jj = tid - (256u - RS_TH);
    if constexpr (CUBIC) s_vy[jj][1] = m355_resize_row_cubic(sny, dny, (int)M355_EXPORT_SEL(a.cosited_y), j0 + jj, &s_vy[jj][0], &s_vy[jj][2], 1);
    else s_vy[jj][1] = m355_resize_row(sny, dny, (int)M355_EXPORT_SEL(a.cosited_y), j0 + jj, &s_vy[jj][0], &s_vy[jj][2], 1);
  }
#pragma unroll
  for (int k = 0; k < M355_RESIZE_MAX_TAPS; k++) hq[k] = tid < ncols ? (unsigned)hrow[k * RS_TW + tid] : 0u;
  __syncthreads();

  const int32_t span0 = s_span[0];
  uint32_t nvec = (uint32_t)(s_span[1] - span0 + S) / S;
  if (nvec > (uint32_t)(RS_SPAN / S)) nvec = RS_SPAN / S;
  const int hmax = m355_resize_max_taps_filtered(FILTER, snx, dnx);
  const int32_t hofs = hfirst - span0;
  const uint32_t pitch = (uint32_t)M355_EXPORT_SEL(a.src_pitch);    /* (a frame's rows are far below 4 GiB) */
  const long long dpitch = M355_EXPORT_SEL(a.dst_pitch);
  const M355_GLOBAL uint8_t* src0 = (const M355_GLOBAL uint8_t*)M355_EXPORT_SEL(a.src);
  const M355_GLOBAL uint8_t* src1 = (const M355_GLOBAL uint8_t*)a.src[2];
  /* this lane's sample of the tile's first row */
  M355_GLOBAL uint8_t* d = (M355_GLOBAL uint8_t*)M355_EXPORT_SEL(a.dst) + (size_t)j0 * (size_t)dpitch + (size_t)(c0 + tid) * (inter ? 2 * DB : DB);
  const int tsh = M355_EXPORT_SEL(a.tshift), osh = M355_EXPORT_SEL(a.oshift), lsh = M355_EXPORT_SEL(a.lshift);
  /* cubic: the bias of 16-bit samples (tsh = bd - 2) and the largest sample (one destination byte: 8 bits, NATIVE or U8) */
  const unsigned sbias = CUBIC && SB == 2 && tsh == 14 ? 0x80008000u : 0u;
  const int top = DB == 1 ? 255 : (1 << (tsh + 2)) - 1;

  /* the first batch of rows of this lane's first vector, loaded one output row ahead: the loads of row jj + 1 are issued before the horizontal pass
     of row jj, which hides their latency */
  unsigned raw[8][4];
#define RS_LOAD_BATCH(s, b, vn) \
  _Pragma("unroll") for (int r = 0; r < 8; r++) { \
    if ((b) + r < (vn)) d_ldg16((s) + (size_t)((b) + r) * (size_t)pitch, raw[r]); \
    else raw[r][0] = raw[r][1] = raw[r][2] = raw[r][3] = 0; \
  }
  const M355_GLOBAL uint8_t* const mine = src0 + ((size_t)span0 + (size_t)tid * S) * SB;
  if (tid < nvec) {
    const int vfirst = s_vy[0][0], vn = s_vy[0][1];
    RS_LOAD_BATCH(mine + (size_t)vfirst * (size_t)pitch, 0, vn)
  }
  for (uint32_t jj = 0; jj < nrows; jj++) {
    /* 1. vertical, lanes on the source */
    const int vfirst = __builtin_amdgcn_readfirstlane((int)s_vy[jj][0]), vn = __builtin_amdgcn_readfirstlane((int)s_vy[jj][1]);
    unsigned (*const trow)[RS_SPAN] = s_t[jj & 1u];
    for (uint32_t v = tid; v < nvec; v += 256u) {
      for (int c = 0; c < nc; c++) {
        const M355_GLOBAL uint8_t* s = (c ? src1 : src0) + (size_t)vfirst * (size_t)pitch + ((size_t)span0 + (size_t)v * S) * SB;
        unsigned u[S];
#pragma unroll
        for (int e = 0; e < S; e++) u[e] = 0;
#pragma unroll
        for (int b = 0; b < M355_RESIZE_MAX_TAPS; b += 8) {
          if (b >= vn) break;
          if (b != 0 || c != 0 || v != tid) { RS_LOAD_BATCH(s, b, vn) }    /* (else: loaded ahead) */
#pragma unroll
          for (int r = 0; r < 8; r += 2) {
            if (b + r < vn) {
              /* the coefficients of rows b + r and b + r + 1 as a 16-bit pair: a broadcast read, the same in every lane (a row's eight pairs held in
                 scalar registers across this loop spilled up to 12 of them in the 16-bit semi-planar instantiations; 2 spills are left there) */
              if constexpr (CUBIC) {
                const unsigned q2 = (unsigned)(s_vy[jj][2 + b + r] & 0xFFFF) | ((unsigned)s_vy[jj][3 + b + r] << 16);
#pragma unroll
                for (int e = 0; e < S; e++) u[e] = (unsigned)d_dot2(SB == 2 ? d_pair<SB>(raw[r], raw[r + 1], e) ^ sbias : d_pair<SB>(raw[r], raw[r + 1], e), q2, (int)u[e]);
              } else {
                const unsigned q2 = (unsigned)(s_vy[jj][2 + b + r] | (s_vy[jj][3 + b + r] << 16));
#pragma unroll
                for (int e = 0; e < S; e++) u[e] = d_udot2(d_pair<SB>(raw[r], raw[r + 1], e), q2, u[e]);
              }
            }
          }
        }
        /* 2. the rounding to t */
#pragma unroll
        for (int e = 0; e < S; e++) {
          if constexpr (CUBIC) trow[c][v * S + e] = (unsigned)(((int)u[e] + (sbias ? 1 << 29 : 0) + (1 << (tsh - 1))) >> tsh);
          else trow[c][v * S + e] = (u[e] + (1u << (tsh - 1))) >> tsh;
        }
      }
    }
    if (jj + 1 < nrows && tid < nvec) {
      const int nfirst = s_vy[jj + 1][0], nn = s_vy[jj + 1][1];
      RS_LOAD_BATCH(mine + (size_t)nfirst * (size_t)pitch, 0, nn)
    }
    __syncthreads();
    /* 3. horizontal, a lane per output column */
    if (tid < ncols) {
      unsigned o[2] = {0, 0};
#pragma unroll
      for (int c = 0; c < (SEMI ? 2 : 1); c++) {
        if (c >= nc) break;
        unsigned v = 0;
#pragma unroll
        for (int k = 0; k < M355_RESIZE_MAX_TAPS; k++) {
          if (k >= hmax) break;
          const int32_t x = hofs + k;
          if constexpr (CUBIC) v = (unsigned)d_mad24((int)hq[k], (int)trow[c][x < RS_SPAN ? x : RS_SPAN - 1], (int)v);
          else v = d_umad24(hq[k], trow[c][x < RS_SPAN ? x : RS_SPAN - 1], v);     /* (behind the row's last coefficient: 0 times an entry of the array) */
        }
        unsigned w;
        if constexpr (CUBIC) w = (unsigned)d_clip3(0, top, ((int)v + (1 << (osh - 1))) >> osh);
        else {
          w = ((v >> 1) + (1u << (osh - 1))) >> osh;
          if (DB == 1) w = w < 255u ? w : 255u;
        }
        o[c] = w << lsh;
      }
      if (inter) {
        if (DB == 1) d_stg2(d, o[0] | (o[1] << 8));
        else d_stg4(d, o[0] | (o[1] << 16));
      } else {
        if (DB == 1) d[0] = (uint8_t)o[0];
        else d_stg2(d, o[0]);
      }
    }
    d += dpitch;
    /* (no second barrier: the next row's t goes to the other half of s_t, and the row after it is written behind the next barrier) */
  }
#undef RS_LOAD_BATCH
}

void m355_launch_export_resized(const ExportResizedArgs& a, int src_bytes, int dst_bytes, bool semiplanar, int filter, hipStream_t st)
{
  const uint32_t units = a.unit_end[2];
  if (!units) return;
  const dim3 grid(units), block(256);
#define M355_EXPORT_RESIZED_CASE(SB, DB) \
  if (src_bytes == SB && dst_bytes == DB) { \
    if (filter == M355_FILTER_CUBIC) { \
      if (semiplanar) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_export_resized<SB, DB, 1, M355_FILTER_CUBIC>), grid, block, 0, st, a); \
      else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_export_resized<SB, DB, 0, M355_FILTER_CUBIC>), grid, block, 0, st, a); \
    } else if (semiplanar) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_export_resized<SB, DB, 1, M355_FILTER_TRIANGLE>), grid, block, 0, st, a); \
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_export_resized<SB, DB, 0, M355_FILTER_TRIANGLE>), grid, block, 0, st, a); \
  }
  M355_EXPORT_RESIZED_CASE(1, 1) M355_EXPORT_RESIZED_CASE(1, 2) M355_EXPORT_RESIZED_CASE(2, 1) M355_EXPORT_RESIZED_CASE(2, 2)
#undef M355_EXPORT_RESIZED_CASE
}
