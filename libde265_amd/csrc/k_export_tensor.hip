/*
 * k_export_tensor.hip — a BATCH of decoded frames (or one rectangle of each) resized, converted to R'G'B', normalised and delivered as one float
 * tensor in one launch (m355_frames_export_tensor, include/de265_mi355x.h).  No new integer arithmetic: the tile procedure is that of
 * k_export_resized_rgb.hip, statement for statement — prologue filter rows, chroma phase into LDS, luma phase, chroma filter, matrix, clip; that
 * file's header describes the passes and segments —, with two changes:
 *   Grid.  blockIdx.x runs over n * units: slice i = blockIdx.x / units picks its source pointers, its two source pitches, its gate word and epoch
 *   from the per-frame array of the kernel arguments (a wave-uniform index: scalar loads), the rest of blockIdx.x is the tile inside the slice.
 *   Rectangle size, output size, tile width, filter rows and coefficients are the batch's, so the rows are derived as there.  The gate is per slice:
 *   a slice whose frame sits behind a rejected decode returns before it touches anything.
 *   Epilogue.  The three clipped integers go through tensor_element.h (one multiplication, one addition, the conversion) and are staged in LDS as
 *   EB-byte elements, EB = 2 (F16 / BF16) or 4 (F32): NCHW three segments of 256 elements, NHWC one of 768.  They leave as dwords, a lane per dword
 *   of consecutive addresses; a tile's row that ends in half a dword (EB = 2, an odd number of elements) stores that element alone.  A staged row
 *   is 256 * 3 * EB bytes, so the static LDS is 41 872 bytes for EB = 2 (as k_export_resized_rgb) and 48 016 bytes for EB = 4: three workgroups per
 *   CU in both (160 KiB of LDS).
 * F16 against BF16, the layout, the chroma format and U8 against U16 of the integer stage are wave-uniform run-time switches (kernel arguments in
 * scalar registers): source sample bytes and element bytes are the template parameters, four instantiations.  The helpers are duplicated from
 * k_export_resized_rgb.hip, as that file duplicates k_export_resized.hip's: its instantiations stay byte for byte what they were.
 *
 * ROI = true (m355_frames_export_tensor_rois, four more instantiations): a rectangle per slice.  The tile procedure is the same statements; what
 * moves from the batch to the slice's record (ExportTensorRoi, read by scalar loads at the same wave-uniform index as the pointers) is the source
 * size on both grids, the tile width, the tiles per row of tiles and the slice's unit count, each derived by the host from the slice's own source
 * size, and the flags.  The filter rows still come from m355_resize_row in the prologue, now with the slice's source size.
 *   Grid.  Slices have different unit counts, so the grid is two-dimensional: blockIdx.y = slice, blockIdx.x = the unit inside it, as wide as the
 *   slice with the most units; a workgroup beyond its slice's count returns, behind the gate, before it touches anything.
 *   Mirror.  M355_ROI_MIRROR touches the epilogue only: the lane of tile column t stages its pixel at position ncols - 1 - t of the staged row
 *   (the channels of an NHWC pixel keep their order), and the tile's first destination column is out_width - c0 - ncols; loads, filter rows, LDS
 *   tiles, the dword stores and the single trailing 2-byte element are unchanged.
 * ROI = false reads the batch's fields as before; its four instantiations compile to the instructions, registers and LDS they had.
 *
 * Reads stay inside the planes' allocations, by the argument of k_export_resized_rgb.hip applied to every frame of the batch: the host admits a
 * frame only if it contains the rectangle (export_plan per frame; ROI: entry i only if frames[i] contains rois[i], and the record's source size is
 * that rectangle's), so in every slice a filter row's source indices, clamped to the slice's rectangle on the plane's grid, name rows and samples
 * of that frame's rectangle; every vector starts at a sample of the span, a lane reads at most 16 bytes from there, and every frame's rows are
 * padded to 128 bytes and its planes end with a 256-byte tail (runtime_internal.h frame_alloc).  The slice index is below
 * n <= M355_TENSOR_MAX_FRAMES, the size of the per-frame array, because blockIdx.x < n * units (ROI: because blockIdx.y < n).  LDS indices are those
 * of k_export_resized_rgb.hip — the host derives every slice's tile width by that kernel's rule from the slice's source size, so a tile's span fits
 * s_t as there —; the staged row is indexed below 256 * 3 * EB bytes (position < ncols <= 256, channel < 3).
 * Writes: element (slice, c, row, column) only, with row < out_height and column < out_width (mirrored: the tile's columns
 * out_width - c0 - ncols .. out_width - c0 - 1); the host has checked that the strides keep rows, planes and slices apart.
 */
#include "k_common.h"
#include "resize_taps.h"
#include "tensor_element.h"

#define TE_TW M355_RESIZE_TILE_W
#define TE_TH M355_RESIZE_TILE_H
#define TE_SPAN 2112                /* >= 255 * 8 + 1 + 16 + 15 = 2072, and 2 * TE_SPAN >= 16 * TE_TW for the prologue's coefficient rows */
#define TE_CW 258                   /* entries of a row of the chroma tile: 4:4:4 256, 4:2:0 / 4:2:2 256 / 2 + 1 */

/* the helpers of k_export_resized_rgb.hip (there: of k_export_resized.hip and k_export_rgb.hip) that this kernel needs too: c + a.lo * b.lo + a.hi * b.hi on packed unsigned 16-bit
   pairs (v_dot2_u32_u16), c + a * b for a, b < 2^24 (v_mad_u32_u24), and the signed v_mad_i32_i24 */
#ifdef SIMT_EMU
static inline unsigned d_te_udot2(unsigned a, unsigned b, unsigned c) { return c + (a & 0xFFFFu) * (b & 0xFFFFu) + (a >> 16) * (b >> 16); }
static inline unsigned d_te_umad24(unsigned a, unsigned b, unsigned c) { return c + a * b; }
static inline int d_te_mad24(int a, int b, int c) { return (int)((unsigned)a * (unsigned)b + (unsigned)c); }
#else
__device__ __forceinline__ unsigned d_te_udot2(unsigned a, unsigned b, unsigned c)
{
  return __builtin_amdgcn_udot2(__builtin_bit_cast(m355_ushort2, a), __builtin_bit_cast(m355_ushort2, b), c, false);
}
__device__ __forceinline__ unsigned d_te_umad24(unsigned a, unsigned b, unsigned c) { return __umul24(a, b) + c; }
__device__ __forceinline__ int d_te_mad24(int a, int b, int c) { return (int)((unsigned)__mul24(a, b) + (unsigned)c); }
#endif

/* sample e of the 16-byte vectors of two rows as one 16-bit pair (row ra in the low half) */
template <int SB> __device__ __forceinline__ unsigned d_te_pair(const unsigned* ra, const unsigned* rb, int e)
{
  if (SB == 1) return d_perm(rb[e >> 2], ra[e >> 2], 0x0c000c00u | (unsigned)(e & 3) | ((unsigned)(4 + (e & 3)) << 16));
  return (e & 1) ? d_pack_hi16(ra[e >> 1], rb[e >> 1]) : d_pack_lo16(ra[e >> 1], rb[e >> 1]);
}

/* rows b .. b + 7 of a filter row of vn source rows, 16 bytes each from s (rows behind the vn-th: zeros) */
#define TE_LOAD_BATCH(s, b, vn, pitch) \
  _Pragma("unroll") for (int r_ = 0; r_ < 8; r_++) { \
    if ((b) + r_ < (vn)) d_ldg16((s) + (size_t)((b) + r_) * (size_t)(pitch), raw[r_]); \
    else raw[r_][0] = raw[r_][1] = raw[r_][2] = raw[r_][3] = 0; \
  }

/* A pass covers nseg <= 4 SEGMENTS: rows_pp consecutive output rows x nplanes planes (Cb and Cr), each with the span's nvec vectors; segment
   g = row * nplanes + plane has the lane-vectors g * nvec .. (g + 1) * nvec - 1 and its t row at trow[g * seglen].  Where lane-vector vv reads
   (without its source row), and what it belongs to: */
struct TeWhere { const M355_GLOBAL uint8_t* p; uint32_t seg, v, row; };
template <int SB>
__device__ __forceinline__ TeWhere d_te_where(const M355_GLOBAL uint8_t* src0, const M355_GLOBAL uint8_t* src1, int32_t span0, uint32_t nvec, uint32_t nplanes, uint32_t vv)
{
  TeWhere w;
  w.seg = (vv >= nvec ? 1u : 0u) + (vv >= 2u * nvec ? 1u : 0u) + (vv >= 3u * nvec ? 1u : 0u);
  w.v = vv - w.seg * nvec;
  w.row = nplanes == 2u ? w.seg >> 1 : w.seg;
  w.p = ((nplanes == 2u && (w.seg & 1u)) ? src1 : src0) + ((size_t)span0 + (size_t)w.v * (16 / SB)) * SB;
  return w;
}

/* The vertical pass of the segments of one pass and its rounding to t (steps 1 and 2 of k_export_resized.hip): a lane owns one 16-byte vector of
   the span of each source row of its segment's filter row vy[row] = {first source row, number of rows, coefficients} (LDS); rows_left: the rows
   from vy[0] to the tile's end.  The first batch of rows of this lane's first vector is in raw already (loaded a pass ahead). */
template <int SB>
__device__ __forceinline__ void d_te_vertical(const M355_GLOBAL uint8_t* src0, const M355_GLOBAL uint8_t* src1, uint32_t pitch, int32_t span0, uint32_t nvec,
                                              uint32_t nplanes, uint32_t nseg, uint32_t seglen, const int32_t (*vy)[2 + M355_RESIZE_MAX_TAPS], uint32_t rows_left,
                                              int tsh, unsigned* trow, uint32_t tid, unsigned (&raw)[8][4])
{
  constexpr int S = 16 / SB;
  for (uint32_t vv = tid; vv < nseg * nvec; vv += 256u) {
    const TeWhere w = d_te_where<SB>(src0, src1, span0, nvec, nplanes, vv);
    if (w.row >= rows_left) continue;
    const int32_t* const q = vy[w.row];
    const int vfirst = q[0], vn = q[1];
    const M355_GLOBAL uint8_t* s = w.p + (size_t)vfirst * (size_t)pitch;
    unsigned u[S];
#pragma unroll
    for (int e = 0; e < S; e++) u[e] = 0;
#pragma unroll
    for (int b = 0; b < M355_RESIZE_MAX_TAPS; b += 8) {
      if (b < vn) {
        if (b != 0 || vv != tid) { TE_LOAD_BATCH(s, b, vn, pitch) }          /* (else: loaded ahead) */
#pragma unroll
        for (int r = 0; r < 8; r += 2) {
          if (b + r < vn) {
            const unsigned q2 = (unsigned)(q[2 + b + r] | (q[3 + b + r] << 16));  /* (the same in every lane of a segment) */
#pragma unroll
            for (int e = 0; e < S; e++) u[e] = d_te_udot2(d_te_pair<SB>(raw[r], raw[r + 1], e), q2, u[e]);
          }
        }
      }
    }
    unsigned* const t = trow + w.seg * seglen + w.v * S;
#pragma unroll
    for (int e = 0; e < S; e++) t[e] = (u[e] + (1u << (tsh - 1))) >> tsh;
  }
}

/* The horizontal pass of one output sample (step 3) and its rounding to a sample of bd bits (osh = 31 - bd): hq = the lane's coefficients, hofs =
   where its first one lies in the t row of lim entries */
__device__ __forceinline__ unsigned d_te_horizontal(const unsigned* hq, const unsigned* trow, int32_t lim, int32_t hofs, int hmax, int osh)
{
  unsigned v = 0;
#pragma unroll
  for (int k = 0; k < M355_RESIZE_MAX_TAPS; k++) {
    if (k >= hmax) break;
    const int32_t x = hofs + k;
    v = d_te_umad24(hq[k], trow[x < lim ? x : lim - 1], v);     /* (behind the row's last coefficient: 0 times an entry of the row) */
  }
  return ((v >> 1) + (1u << (osh - 1))) >> osh;
}

/* The kernel's arguments: ROI = false the batch's geometry (m355_frames_export_tensor), ROI = true a geometry per slice
   (m355_frames_export_tensor_rois).  TE_GEOM(field) reads a field of the source's geometry from the slice's record or from the batch, at the place
   where the kernel reads the batch's. */
template <bool ROI> struct TeArgs { typedef ExportTensorArgs T; };
template <> struct TeArgs<true> { typedef ExportTensorRoisArgs T; };
#define TE_GEOM(field) ({ uint32_t g_; if constexpr (ROI) g_ = fr.field; else g_ = a.field; g_; })

template <int SB, int EB, bool ROI>
__global__ void __launch_bounds__(256) k_export_tensor(typename TeArgs<ROI>::T a)
{
  constexpr int S = 16 / SB;
  constexpr uint32_t OB = TE_TW * 3 * EB;                       /* bytes of a staged output row: 256 pixels x 3 channels x EB bytes */
  uint32_t slice;                                               /* (wave-uniform: the frame's record comes by scalar loads) */
  if constexpr (ROI) slice = blockIdx.y; else slice = blockIdx.x / a.units;
  if (slice >= a.n) return;
  const auto& fr = a.fr[slice];
  M355_GATE(fr);
  if constexpr (ROI) { if (blockIdx.x >= fr.units) return; }    /* (the grid is as wide as the slice with the most units) */
  __shared__ unsigned s_t[2][TE_SPAN];                          /* [pass & 1]: the t rows of the pass's segments; in the prologue: the lanes' horizontal rows */
  __shared__ int32_t s_vy[2][TE_TH][2 + M355_RESIZE_MAX_TAPS];  /* [luma, chroma] per output row of the tile: first source row, number of rows, coefficients */
  __shared__ int32_t s_span[2][2];                              /* [luma, chroma] first and last source column of the tile */
  __shared__ unsigned short s_c[2][TE_TH][TE_CW];               /* the resized Cb and Cr samples the tile's pixels need */
  __shared__ __attribute__((aligned(16))) uint8_t s_o[2][2][OB];  /* [pass & 1][row of the pass]: the staged output rows */
  uint32_t unit;
  if constexpr (ROI) unit = blockIdx.x; else unit = blockIdx.x - slice * a.units;
  const uint32_t tid = threadIdx.x;
  const uint32_t run = unit / TE_GEOM(tiles_x), tile = unit - run * TE_GEOM(tiles_x);
  const uint32_t tw = TE_GEOM(tile_w), c0 = tile * tw, j0 = run * TE_TH;
  const uint32_t dnx = a.dn_x[0], dny = a.dn_y[0], cdx = a.dn_x[1], cdy = a.dn_y[1];
  const uint32_t ncols = dnx - c0 < tw ? dnx - c0 : tw, nrows = dny - j0 < (uint32_t)TE_TH ? dny - j0 : (uint32_t)TE_TH;
  const int cf = a.cf;
  const bool planar = a.nhwc == 0;                             /* NCHW: three staged segments, as the planar R'G'B' layout */
  const uint32_t swl = (cf == 1 || cf == 2) ? 1u : 0u, shl = cf == 1 ? 1u : 0u;
  /* the chroma tile: columns cc0 .. cc1 and rows cj0 .. cj1 of the resized chroma planes */
  uint32_t cc0 = 0, ncc = 0, cj0 = 0, ncr = 0;
  if (cf != 0) {
    cc0 = c0 >> swl;
    uint32_t cc1 = ((c0 + ncols - 1) >> swl) + swl;
    if (cc1 > cdx - 1) cc1 = cdx - 1;
    cj0 = j0;
    uint32_t cj1 = j0 + nrows - 1;
    if (shl) { cj0 = (j0 >> 1) ? (j0 >> 1) - 1 : 0u; cj1 = ((j0 + nrows - 1) >> 1) + 1; }
    if (cj1 > cdy - 1) cj1 = cdy - 1;
    ncc = cc1 - cc0 + 1; ncr = cj1 - cj0 + 1;
  }

  /* prologue: the filter rows of this tile */
  int32_t* hrow = (int32_t*)&s_t[0][0];                        /* coefficient k of lane i at [k * TE_TW + i] */
  int32_t hfirst = 0, cfirst = 0;
  if (tid < ncc) {
    const int hn = m355_resize_row(TE_GEOM(sn_x[1]), cdx, (int)swl, cc0 + tid, &cfirst, hrow + tid, TE_TW);
    if (tid == 0) s_span[1][0] = cfirst;
    if (tid == ncc - 1) s_span[1][1] = cfirst + hn - 1;
  }
  if (tid >= 256u - TE_TH && tid - (256u - TE_TH) < nrows) {
    const uint32_t jj = tid - (256u - TE_TH);
    s_vy[0][jj][1] = m355_resize_row(TE_GEOM(sn_y[0]), dny, 0, j0 + jj, &s_vy[0][jj][0], &s_vy[0][jj][2], 1);
  }
  if (tid >= 256u - 2 * TE_TH && tid - (256u - 2 * TE_TH) < ncr) {
    const uint32_t jj = tid - (256u - 2 * TE_TH);
    s_vy[1][jj][1] = m355_resize_row(TE_GEOM(sn_y[1]), cdy, 0, cj0 + jj, &s_vy[1][jj][0], &s_vy[1][jj][2], 1);
  }
  __syncthreads();

  unsigned raw[8][4];
  uint32_t par = 0;
  /* the chroma phase: row by row into s_c, Cb and Cr in one pass where both t rows fit one row of s_t (4:2:0 / 4:2:2), else one after the other */
  if (cf != 0) {
    unsigned cq[M355_RESIZE_MAX_TAPS];
#pragma unroll
    for (int k = 0; k < M355_RESIZE_MAX_TAPS; k++) cq[k] = tid < ncc ? (unsigned)hrow[k * TE_TW + tid] : 0u;
    __syncthreads();                                           /* (the lanes' rows are read: s_t is free) */
    const int32_t span0 = s_span[1][0];
    uint32_t nvec = (uint32_t)(s_span[1][1] - span0 + S) / S;
    if (nvec > (uint32_t)(TE_SPAN / S)) nvec = TE_SPAN / S;
    /* segments per pass: Cb and Cr side by side where two spans fit a row of s_t and their vectors the workgroup's lanes (a lane with a second
       vector would load it behind the first, not ahead), and two rows of each where four fit */
    const uint32_t cap = (nvec * S <= (uint32_t)(TE_SPAN / 4) && 4u * nvec <= 256u) ? 4u : ((nvec * S <= (uint32_t)(TE_SPAN / 2) && 2u * nvec <= 256u) ? 2u : 1u);
    const uint32_t npl = cap >= 2u ? 2u : 1u, rpp = cap / npl, nseg = cap, seglen = TE_SPAN / cap;
    const int hmax = m355_resize_max_taps(TE_GEOM(sn_x[1]), cdx);
    const int32_t hofs = cfirst - span0, lim = (int32_t)seglen;
    const uint32_t pitch = (uint32_t)fr.src_pitch[1];
    const int tsh = a.bdc - 4, osh = 31 - a.bdc;
    for (uint32_t c = 0; c < 2; c += npl) {
      const M355_GLOBAL uint8_t* const src0 = (const M355_GLOBAL uint8_t*)(c ? fr.src[2] : fr.src[1]);
      const M355_GLOBAL uint8_t* const src1 = (const M355_GLOBAL uint8_t*)fr.src[2];
      const TeWhere me = d_te_where<SB>(src0, src1, span0, nvec, npl, tid);
      const bool active = tid < nseg * nvec;
      if (active && me.row < ncr) {
        const int vfirst = s_vy[1][me.row][0], vn = s_vy[1][me.row][1];
        TE_LOAD_BATCH(me.p + (size_t)vfirst * (size_t)pitch, 0, vn, pitch)
      }
      for (uint32_t r = 0; r < ncr; r += rpp, par ^= 1u) {
        d_te_vertical<SB>(src0, src1, pitch, span0, nvec, npl, nseg, seglen, &s_vy[1][r], ncr - r, tsh, s_t[par], tid, raw);
        if (active && r + rpp + me.row < ncr) {                /* the next pass's first batch, in flight across the horizontal pass */
          const int nfirst = s_vy[1][r + rpp + me.row][0], nn = s_vy[1][r + rpp + me.row][1];
          TE_LOAD_BATCH(me.p + (size_t)nfirst * (size_t)pitch, 0, nn, pitch)
        }
        __syncthreads();
        if (tid < ncc) {
          for (uint32_t i = 0; i < rpp && r + i < ncr; i++)
            for (uint32_t pl = 0; pl < npl; pl++)
              s_c[c + pl][r + i][tid] = (unsigned short)d_te_horizontal(cq, s_t[par] + (i * npl + pl) * seglen, lim, hofs, hmax, osh);
        }
        /* (no second barrier: the next pass's t goes to the other half of s_t, and the pass after it is written behind the next barrier) */
      }
    }
    __syncthreads();                                           /* (the last t row is read: s_t is free for the luma rows of the lanes) */
  }
  /* the horizontal rows of the tile's luma columns, derived here so that their registers are not held across the chroma phase */
  unsigned hq[M355_RESIZE_MAX_TAPS];
  if (tid < ncols) {
    const int hn = m355_resize_row(TE_GEOM(sn_x[0]), dnx, 0, c0 + tid, &hfirst, hrow + tid, TE_TW);
    if (tid == 0) s_span[0][0] = hfirst;
    if (tid == ncols - 1) s_span[0][1] = hfirst + hn - 1;
  }
#pragma unroll
  for (int k = 0; k < M355_RESIZE_MAX_TAPS; k++) hq[k] = tid < ncols ? (unsigned)hrow[k * TE_TW + tid] : 0u;
  __syncthreads();

  /* the luma phase */
  const int32_t span0 = s_span[0][0];
  uint32_t nvec = (uint32_t)(s_span[0][1] - span0 + S) / S;
  if (nvec > (uint32_t)(TE_SPAN / S)) nvec = TE_SPAN / S;
  const uint32_t rpp = (nvec * S <= (uint32_t)(TE_SPAN / 2) && 2u * nvec <= 256u) ? 2u : 1u, seglen = TE_SPAN / rpp;   /* two output rows per pass where two spans fit a row of s_t and the lanes */
  const int hmax = m355_resize_max_taps(TE_GEOM(sn_x[0]), dnx);
  const int32_t hofs = hfirst - span0;
  const uint32_t pitch = (uint32_t)fr.src_pitch[0];             /* (a frame's rows are far below 4 GiB) */
  const int tsh = a.bdl - 4, osh = 31 - a.bdl;
  const M355_GLOBAL uint8_t* const srcy = (const M355_GLOBAL uint8_t*)fr.src[0];
  const TeWhere me = d_te_where<SB>(srcy, srcy, span0, nvec, 1u, tid);
  const bool active = tid < rpp * nvec;
  /* the constants of the launch (scalar): the rounding term and the luma offset in one, c0 folded into the chroma filter's rounding constants */
  const int F = a.k.F, ky = (int)((1u << (F - 1)) - (unsigned)a.k.cy * (unsigned)a.k.y0);
  const int cy = a.k.cy, crv = a.k.crv, ncgu = -a.k.cgu, ncgv = -a.k.cgv, cbu = a.k.cbu, kc0 = a.k.c0;
  /* this lane's columns of the chroma tile: column i of its pixel and the clamped neighbour to the right */
  const uint32_t X = c0 + tid;
  uint32_t ci = 0, cin = 0;
  if (cf != 0 && tid < ncols) {
    const uint32_t i = X >> swl, in = i + 1 < cdx ? i + 1 : cdx - 1;
    ci = i - cc0; cin = swl ? in - cc0 : ci;
  }
  const bool odd = swl && (X & 1u);
  /* the float stage of the launch (scalar): the clip of the integer stage, the element format, scale and bias per channel */
  const int M = a.u16 ? 65535 : 255;
  const uint32_t bf16_mask = a.bf16 ? 0xFFFFFFFFu : 0u;
  const float sc[3] = {a.scale[0], a.scale[1], a.scale[2]}, bi[3] = {a.bias[0], a.bias[1], a.bias[2]};
  /* where the staged row's bytes go: NHWC one segment of up to 192 * EB dwords, NCHW three of up to SEGW = 64 * EB (the planes of the slice) */
  constexpr uint32_t SEGW = TE_TW * EB / 4, SEGSH = EB == 4 ? 8 : 7;
  const uint32_t seg_bytes = ncols * (uint32_t)EB * (planar ? 1u : 3u);
  /* a mirrored slice: the lane of tile column t stages its pixel at position ncols - 1 - t, and the tile's first destination column is
     out_width - c0 - ncols; the stores themselves do not change */
  bool mirror = false;
  if constexpr (ROI) mirror = (fr.flags & M355_ROI_MIRROR) != 0;
  const uint32_t pos = mirror ? ncols - 1u - tid : tid, col0 = mirror ? dnx - c0 - ncols : c0;
  M355_GLOBAL uint8_t* const dst0 = (M355_GLOBAL uint8_t*)a.dst + (size_t)slice * (size_t)a.stride_n + (size_t)col0 * (size_t)EB * (planar ? 1u : 3u);
  const size_t stride_c = (size_t)a.stride_c, stride_h = (size_t)a.stride_h;

#define TE_STORE_ROW(buf, row) \
  for (uint32_t q = tid; q < OB / 4u; q += 256u) { \
    const uint32_t seg = planar ? q >> SEGSH : 0u, w = planar ? q & (SEGW - 1u) : q; \
    if (4u * w < seg_bytes) { \
      M355_GLOBAL uint8_t* d = dst0 + (size_t)seg * stride_c + (size_t)(row) * stride_h + 4u * w; \
      unsigned val; \
      __builtin_memcpy(&val, (buf) + 4u * q, 4); \
      if (4u * w + 4u <= seg_bytes) d_stg4(d, val); \
      else { const unsigned short h_ = (unsigned short)val; *(M355_GLOBAL unsigned short*)d = h_; }   /* (EB = 2 only: the row's last element) */ \
    } \
  }

  if (active && me.row < nrows) {
    const int vfirst = s_vy[0][me.row][0], vn = s_vy[0][me.row][1];
    TE_LOAD_BATCH(me.p + (size_t)vfirst * (size_t)pitch, 0, vn, pitch)
  }
  uint32_t staged = 0, staged_j = 0;                           /* the rows staged by the pass before, and the first of them */
  for (uint32_t jp = 0; jp < nrows; jp += rpp, par ^= 1u) {
    d_te_vertical<SB>(srcy, srcy, pitch, span0, nvec, 1u, rpp, seglen, &s_vy[0][jp], nrows - jp, tsh, s_t[par], tid, raw);
    if (active && jp + rpp + me.row < nrows) {                 /* the next pass's first batch, in flight across the horizontal pass */
      const int nfirst = s_vy[0][jp + rpp + me.row][0], nn = s_vy[0][jp + rpp + me.row][1];
      TE_LOAD_BATCH(me.p + (size_t)nfirst * (size_t)pitch, 0, nn, pitch)
    }
    __syncthreads();
    for (uint32_t i = 0; i < staged; i++) { TE_STORE_ROW(s_o[par ^ 1u][i], j0 + staged_j + i) }   /* the rows staged before this barrier */
    staged = nrows - jp < rpp ? nrows - jp : rpp; staged_j = jp;
    for (uint32_t ri = 0; ri < staged; ri++) {
      const uint32_t jj = jp + ri;
      if (tid < ncols) {
        const int y = (int)d_te_horizontal(hq, s_t[par] + ri * seglen, (int32_t)seglen, hofs, hmax, osh);
        const int base = d_te_mad24(cy, y, ky);
        int r = base, g = base, b = base;
        if (cf != 0) {
          int uv[2];
          if (cf == 1) {
            const uint32_t Y = j0 + jj, j = Y >> 1, jn = (Y & 1u) ? (j + 1 < cdy ? j + 1 : cdy - 1) : (j ? j - 1 : 0u);
            const uint32_t rj = j - cj0, rn = jn - cj0;
#pragma unroll
            for (int c = 0; c < 2; c++) {
              const int t0 = 3 * (int)s_c[c][rj][ci] + (int)s_c[c][rn][ci], t1 = 3 * (int)s_c[c][rj][cin] + (int)s_c[c][rn][cin];
              uv[c] = odd ? (t0 + t1 + 4 - 8 * kc0) >> 3 : (t0 + 2 - 4 * kc0) >> 2;
            }
          } else {
#pragma unroll
            for (int c = 0; c < 2; c++) {
              const int t0 = (int)s_c[c][jj][ci], t1 = (int)s_c[c][jj][cin];
              uv[c] = odd ? (t0 + t1 + 1 - 2 * kc0) >> 1 : t0 - kc0;
            }
          }
          r = d_te_mad24(crv, uv[1], base);
          g = d_te_mad24(ncgv, uv[1], d_te_mad24(ncgu, uv[0], base));
          b = d_te_mad24(cbu, uv[0], base);
        }
        const unsigned e[3] = {(unsigned)d_clip3(0, M, r >> F), (unsigned)d_clip3(0, M, g >> F), (unsigned)d_clip3(0, M, b >> F)};
        uint8_t* o = s_o[par][ri];
#pragma unroll
        for (int c = 0; c < 3; c++) {
          const float f = m355_te_affine(e[c], sc[c], bi[c]);
          const uint32_t bits = EB == 4 ? m355_te_bits(f) : m355_te_half(f, bf16_mask);
          const uint32_t at = planar ? (uint32_t)c * (SEGW * 4u) + pos * (uint32_t)EB : (3u * pos + (uint32_t)c) * (uint32_t)EB;
          if (EB == 4) __builtin_memcpy(o + at, &bits, 4);
          else { const unsigned short h = (unsigned short)bits; __builtin_memcpy(o + at, &h, 2); }
        }
      }
    }
  }
  __syncthreads();
  for (uint32_t i = 0; i < staged; i++) { TE_STORE_ROW(s_o[par ^ 1u][i], j0 + staged_j + i) }
#undef TE_STORE_ROW
}
#undef TE_GEOM
#undef TE_LOAD_BATCH

void m355_launch_export_tensor(const ExportTensorArgs& a, int src_bytes, int elem_bytes, hipStream_t st)
{
  if (!a.units || !a.n) return;
  const dim3 grid(a.units * a.n), block(256);
#define M355_EXPORT_TENSOR_CASE(SB, EB) \
  if (src_bytes == SB && elem_bytes == EB) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_export_tensor<SB, EB, false>), grid, block, 0, st, a);
  M355_EXPORT_TENSOR_CASE(1, 2) M355_EXPORT_TENSOR_CASE(1, 4) M355_EXPORT_TENSOR_CASE(2, 2) M355_EXPORT_TENSOR_CASE(2, 4)
#undef M355_EXPORT_TENSOR_CASE
}

/* the batch of regions: blockIdx.y = slice, blockIdx.x = the unit inside it, up to the largest unit count of a slice */
void m355_launch_export_tensor_rois(const ExportTensorRoisArgs& a, int src_bytes, int elem_bytes, hipStream_t st)
{
  if (!a.max_units || !a.n) return;
  const dim3 grid(a.max_units, a.n), block(256);
#define M355_EXPORT_TENSOR_CASE(SB, EB) \
  if (src_bytes == SB && elem_bytes == EB) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_export_tensor<SB, EB, true>), grid, block, 0, st, a);
  M355_EXPORT_TENSOR_CASE(1, 2) M355_EXPORT_TENSOR_CASE(1, 4) M355_EXPORT_TENSOR_CASE(2, 2) M355_EXPORT_TENSOR_CASE(2, 4)
#undef M355_EXPORT_TENSOR_CASE
}
