/*
 * k_export_resized_rgb.hip — decoded frames (or a rectangle of each) RESIZED and converted to R'G'B' in one launch, in three modes:
 *   RR_FRAME  one frame, integer R'G'B' of EB = 1 or 2 bytes per channel (m355_frame_export_resized_rgb, include/de265_mi355x.h): the composition
 *             of m355_frame_export_resized (planar, NATIVE) and m355_frame_export_rgb of the resized picture, byte for byte, without a resized Y,
 *             Cb or Cr sample passing through global memory;
 *   RR_BATCH  n frames, one rectangle, as one float tensor of EB = 2 (F16 / BF16) or 4 (F32) bytes per element (m355_frames_export_tensor);
 *   RR_ROIS   n frames, a rectangle per slice, as one float tensor (m355_frames_export_tensor_rois).
 * No new arithmetic: the filter rows are those of resize_taps.h, the passes those of k_export_resized.hip, the chroma filter and the matrix those of
 * k_export_rgb.hip — for the chroma sample location types 1..3 of m355_export_opts the template parameter SITED is set and the type is a wave-uniform
 * kernel argument, which sets which chroma axes are co-sited and the weights of the chroma filter; type 0 runs the instantiations it always ran —, the float stage that of tensor_element.h.  The filter (M355_FILTER_TRIANGLE, or M355_FILTER_CUBIC of the _filtered entry points) is a
 * template parameter of the tile procedure — d_rr_row, d_rr_vertical, d_rr_horizontal — and so of every mode; the cubic passes are those of the cubic
 * k_export_resized: signed, 16 bits of fraction in t, luma and chroma clipped to a sample behind the horizontal pass.
 *
 * A workgroup of 256 lanes owns a tile of up to 256 luma output columns x 16 luma output rows (even width for 4:2:0 / 4:2:2, so that a tile's
 * first column is a chroma column).  Prologue: lane i derives the horizontal row of resized chroma column cc0 + i into registers (through LDS, as
 * in k_export_resized.hip), 16 + 16 lanes the vertical rows of the tile's luma and chroma rows into LDS; the horizontal row of luma column c0 + i
 * follows behind the chroma phase, so that the two sets of 16 coefficient registers are never held together.  Then:
 *   A PASS of the row procedure of k_export_resized.hip — lanes on the 16-byte vectors of the source span, the first batch of the next pass's
 *   loads in flight across the horizontal pass, two filter rows per v_dot2_u32_u16, the rounding to t in LDS, one barrier, the horizontal pass with
 *   v_mad_u32_u24 from coefficients in registers — covers up to four SEGMENTS, each a (row, plane) with the span's nvec vectors and a t row of its
 *   own inside one row of s_t: a workgroup's time follows its number of passes (each is a chain of load, LDS and barrier latencies), not the work
 *   in them.  Segments share a pass where their spans fit the row of s_t AND their vectors the 256 lanes (a lane with a second vector would load
 *   it behind the first instead of a pass ahead); the host picks the tile width so that they do (runtime.hip resize_rgb_tile_w).
 *   Chroma phase (not for monochrome): the resized chroma columns cc0 = c0 / SubWidthC (CENTRE: one more on the left) .. (c0 + ncols - 1) / SubWidthC + 1
 *   (4:4:4: the tile's own columns; subsampled: at most 128 + 2) and rows j0 / 2 - 1 (TOP: j0 / 2) .. (j0 + nrows - 1) / 2 + 1 (4:2:0: at most 10; else
 *   the tile's own 16), both clamped to the RESIZED plane, are
 *   produced and kept as NATIVE 16-bit entries in LDS (2 planes x 16 rows x 258 entries): two rows of Cb and of Cr per pass, or one row of both,
 *   or — where not even two spans fit — Cb's rows first, then Cr's.
 *   Luma phase: two output rows per pass where they fit, else one; the horizontal sum is rounded to a sample in a register; the lane's chroma comes
 *   from the LDS tile through the filter of the header (weights in quarters per axis, (sum + 8) >> 4, c0 folded into the rounding constant),
 *   then the five v_mad_i32_i24 of the matrix, the shift and the clip.
 *   Stores: a lane holds one pixel of each row of the pass; the rows' channels are staged in LDS as EB-byte elements (packed / NHWC: the three of a
 *   pixel side by side; planar / NCHW: three segments) and leave as dwords, a lane per dword of consecutive addresses; only the valid bytes at the
 *   end of the tile's row are stored.  The staged rows are stored behind the NEXT pass's barrier (two sets of staging rows alternate), so a pass
 *   costs one barrier.
 * What the modes differ in (`if constexpr`, at the place of the difference; a field that moves is read where it is used — RR_SRC, RR_PITCH, RR_GEOM —,
 * never through a reference to the slice's record, which costs the tensor instantiations some 200 instructions and an unrolled loop):
 *   Grid and gate.  RR_FRAME: blockIdx.x = the tile, one gate.  RR_BATCH: blockIdx.x runs over n * units, slice = blockIdx.x / units; RR_ROIS: slices
 *   have different unit counts, so blockIdx.y = slice and blockIdx.x = the unit inside it, as wide as the slice with the most units (a workgroup
 *   beyond its slice's count returns).  A slice picks its source pointers, two pitches, gate word and epoch from the per-slice array of the kernel
 *   arguments (a wave-uniform index: scalar loads), and a slice whose frame sits behind a rejected decode returns before it touches anything.
 *   RR_ROIS also reads the source size on both grids, the tile width and the tiles per row of tiles from the slice's record (the host derives
 *   each from the slice's own source size); output size, bit depths, chroma format and coefficients are the launch's in every mode.
 *   Epilogue.  RR_FRAME stages the clipped integers (clip by EB; a staged row is 1536 bytes, a planar segment 512, for both EB), stores the
 *   trailing bytes of a row singly and finds segment s at dst[s] + row * dst_pitch[s].  The tensor modes clip by the u16 argument, pass the integers
 *   through tensor_element.h (one multiplication, one addition, the conversion), stage rows of 768 * EB bytes, store a row's trailing half dword
 *   (EB = 2, an odd number of elements) as one element and find segment s at dst + slice * stride_n + s * stride_c + row * stride_h.  Static LDS:
 *   41 872 bytes, or 48 016 for EB = 4: three workgroups per CU in both (160 KiB of LDS).
 *   Mirror (RR_ROIS, M355_ROI_MIRROR) touches the epilogue only: the lane of tile column t stages its pixel at position ncols - 1 - t of the
 *   staged row (the channels of an NHWC pixel keep their order), and the tile's first destination column is out_width - c0 - ncols.
 * Layout, chroma format, F16 against BF16 and U8 against U16 of the tensors' integer stage are wave-uniform run-time switches (kernel arguments in
 * scalar registers): source sample bytes, element bytes, the mode, the filter, SITED and COLOUR are the template parameters, twelve instantiations per filter and
 * value of SITED and of COLOUR (off, tables, tables + tone: 144 in all).
 * COLOUR (m355_export_opts.colour; colour_transform.h, k_colour_dev.h) puts the colour transform stage between the clip and the staging: the launch's
 *   coefficients are then those of M355_RGB_U16 and the clip is to 65 535 whatever the samples; the pixel's three 16-bit values go through the input
 *   table (global memory, two neighbouring knots per channel in one load), the 3 x 3 matrix (wave-uniform kernel arguments, 24-bit multiplies) and the
 *   output table (LDS: 2 436 bytes more, filled behind the gate and ahead of the prologue's barrier), and the delivery the samples ask for (U8: one
 *   rounding division) hands the integer to the pack or to tensor_element.h as before.  COLOUR = off compiles none of it: those instantiations are
 *   what they were.  COLOUR = tone (an object of m355_colour_create_tone) puts step 2b between the matrix and the output table: one gain per pixel, looked
 *   up at the pixel's maxRGB or luminance (norm and the weights: wave-uniform kernel arguments) in the object's gain table (global memory, one gather of two
 *   neighbouring dwords: k_colour_dev.h bounds it) and multiplied into the three linear values in 64 bits.  COLOUR = tables is what COLOUR = true was.
 * PX (m355_frame_export_resized_pixels; pixel_pack.h; RR_FRAME only) replaces the staging of three elements by ONE pixel of bpp = 3 or 4 bytes at
 *   pos * bpp of the staged row — PX = 8-bit pixels: the three clipped (or delivered) bytes in the format's order and, bpp = 4, the alpha; PX = 10-bit
 *   pixels: the integer stage of EB = 2 (the coefficients of M355_RGB_U16, clip to 65 535; COLOUR: step 3's 16-bit result, not m355_ct_deliver's),
 *   then c10 per channel and the dword —, and RR_STORE_ROW's seg_bytes = ncols * bpp.  bpp, the channel order and the alpha in its place are
 *   wave-uniform kernel arguments, so the five formats are two values of PX; a staged row holds at most 256 * 4 = 1024 of its 1536 bytes, LDS and the
 *   two staging sets are what they were, and a 4-byte pixel row ends in whole dwords (BGR8: the byte tail of the 3-byte packed row).  PX = off
 *   compiles none of it: those 144 instantiations are what they were; 48 more (2 sample bytes x 2 PX x 2 filters x SITED x 3 COLOUR) make 192.
 *
 * Reads stay inside the planes' allocations, by the argument of k_export_resized.hip for every plane of every slice: the host admits a frame only
 * if it contains the slice's rectangle (export_plan per frame), whose size is the source size the slice's rows are derived from.  A filter row's
 * source indices are clamped to the rectangle on that plane's grid (resize_taps.h), so every row read — a luma row, or one of the chroma phase's
 * rows, whose output indices are clamped to the resized plane before their filter rows are derived — is a row of the rectangle; every vector starts
 * at a sample of the span, which runs from the first source column of the tile's first (chroma: cc0-th) column to the last source column of its
 * last one, both samples of the rectangle; a lane reads at most 16 bytes from there, i.e. less than 16 bytes beyond a sample inside a row of the
 * plane, and rows are padded to 128 bytes and a plane ends with a 256-byte tail (runtime_internal.h frame_alloc).  The slice index is below
 * n <= M355_TENSOR_MAX_FRAMES, the size of the per-slice array (checked first).  The t row holds RR_SPAN entries (256 columns advance by at most
 * 255 * 8 + 1 source samples, a row adds 16, the last vector 15); the vector count is clamped to the array all the same.  The chroma tile is
 * indexed by columns 0 .. cc1 - cc0 <= 256 and rows 0 .. cj1 - cj0 <= 15 only: the filter's neighbours are clamped to cc1 / cj0 / cj1, which the
 * clamp of the definition (the resized plane's last column and first / last row) never exceeds.  The staged row is indexed below its OB bytes
 * (position < ncols <= 256, channel < 3).
 * Writes: channel c of output pixel (row, column) of the slice only, with row < out_height and column < out_width (mirrored: the tile's columns
 * out_width - c0 - ncols .. out_width - c0 - 1); the host has checked that pitches and strides keep rows, planes and slices apart.
 * Arithmetic: the resize in unsigned 32 bits (cubic: signed) as in k_export_resized.hip; the conversion in signed 32 bits as in k_export_rgb.hip.
 */
#include "k_common.h"
#include "resize_taps.h"
#include "tensor_element.h"
#include "k_resize_dev.h"
#include "k_colour_dev.h"
#include "pixel_pack.h"

#define RR_TW M355_RESIZE_TILE_W
#define RR_TH M355_RESIZE_TILE_H
#define RR_SPAN 2112                /* >= 255 * 8 + 1 + 16 + 15 = 2072, and 2 * RR_SPAN >= 16 * RR_TW for the prologue's coefficient rows */
#define RR_CW 258                   /* entries of a row of the chroma tile: 4:4:4 256, 4:2:0 / 4:2:2 256 / 2 + 1 */

/* rows b .. b + 7 of a filter row of vn source rows, 16 bytes each from s (rows behind the vn-th: zeros) */
#define RR_LOAD_BATCH(s, b, vn, pitch) \
  _Pragma("unroll") for (int r_ = 0; r_ < 8; r_++) { \
    if ((b) + r_ < (vn)) d_ldg16((s) + (size_t)((b) + r_) * (size_t)(pitch), raw[r_]); \
    else raw[r_][0] = raw[r_][1] = raw[r_][2] = raw[r_][3] = 0; \
  }

/* A pass covers nseg <= 4 SEGMENTS: rows_pp consecutive output rows x nplanes planes (Cb and Cr), each with the span's nvec vectors; segment
   g = row * nplanes + plane has the lane-vectors g * nvec .. (g + 1) * nvec - 1 and its t row at trow[g * seglen].  Where lane-vector vv reads
   (without its source row), and what it belongs to: */
struct RrWhere { const M355_GLOBAL uint8_t* p; uint32_t seg, v, row; };
template <int SB>
__device__ __forceinline__ RrWhere d_rr_where(const M355_GLOBAL uint8_t* src0, const M355_GLOBAL uint8_t* src1, int32_t span0, uint32_t nvec, uint32_t nplanes, uint32_t vv)
{
  RrWhere w;
  w.seg = (vv >= nvec ? 1u : 0u) + (vv >= 2u * nvec ? 1u : 0u) + (vv >= 3u * nvec ? 1u : 0u);
  w.v = vv - w.seg * nvec;
  w.row = nplanes == 2u ? w.seg >> 1 : w.seg;
  w.p = ((nplanes == 2u && (w.seg & 1u)) ? src1 : src0) + ((size_t)span0 + (size_t)w.v * (16 / SB)) * SB;
  return w;
}

/* The vertical pass of the segments of one pass and its rounding to t (steps 1 and 2 of k_export_resized.hip): a lane owns one 16-byte vector of
   the span of each source row of its segment's filter row vy[row] = {first source row, number of rows, coefficients} (LDS); rows_left: the rows
   from vy[0] to the tile's end.  The first batch of rows of this lane's first vector is in raw already (loaded a pass ahead). */
template <int SB, int FILTER>
__device__ __forceinline__ void d_rr_vertical(const M355_GLOBAL uint8_t* src0, const M355_GLOBAL uint8_t* src1, uint32_t pitch, int32_t span0, uint32_t nvec,
                                              uint32_t nplanes, uint32_t nseg, uint32_t seglen, const int32_t (*vy)[2 + M355_RESIZE_MAX_TAPS], uint32_t rows_left,
                                              int tsh, unsigned* trow, uint32_t tid, unsigned (&raw)[8][4])
{
  constexpr int S = 16 / SB;
  constexpr bool CUBIC = FILTER == M355_FILTER_CUBIC;
  const unsigned sbias = CUBIC && SB == 2 && tsh == 14 ? 0x80008000u : 0u;     /* cubic (tsh = bd - 2): 16-bit samples are taken less 2^15 */
  for (uint32_t vv = tid; vv < nseg * nvec; vv += 256u) {
    const RrWhere w = d_rr_where<SB>(src0, src1, span0, nvec, nplanes, vv);
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
        if (b != 0 || vv != tid) { RR_LOAD_BATCH(s, b, vn, pitch) }          /* (else: loaded ahead) */
#pragma unroll
        for (int r = 0; r < 8; r += 2) {
          if (b + r < vn) {
            if constexpr (CUBIC) {
              const unsigned q2 = (unsigned)(q[2 + b + r] & 0xFFFF) | ((unsigned)q[3 + b + r] << 16);
#pragma unroll
              for (int e = 0; e < S; e++) u[e] = (unsigned)d_dot2(SB == 2 ? d_pair<SB>(raw[r], raw[r + 1], e) ^ sbias : d_pair<SB>(raw[r], raw[r + 1], e), q2, (int)u[e]);
            } else {
              const unsigned q2 = (unsigned)(q[2 + b + r] | (q[3 + b + r] << 16));  /* (the same in every lane of a segment) */
#pragma unroll
              for (int e = 0; e < S; e++) u[e] = d_udot2(d_pair<SB>(raw[r], raw[r + 1], e), q2, u[e]);
            }
          }
        }
      }
    }
    unsigned* const t = trow + w.seg * seglen + w.v * S;
#pragma unroll
    for (int e = 0; e < S; e++) {
      if constexpr (CUBIC) t[e] = (unsigned)(((int)u[e] + (sbias ? 1 << 29 : 0) + (1 << (tsh - 1))) >> tsh);   /* (2^15 * 2^14 back: a row sums to 1 << 14) */
      else t[e] = (u[e] + (1u << (tsh - 1))) >> tsh;
    }
  }
}

/* The horizontal pass of one output sample (step 3) and its rounding to a sample of bd bits (osh = 31 - bd): hq = the lane's coefficients, hofs =
   where its first one lies in the t row of lim entries.  Cubic: signed (v_mad_i32_i24: |t| < 2^18, |q| < 2^15), osh = 30 - bd, clipped to 0 .. top */
template <int FILTER>
__device__ __forceinline__ unsigned d_rr_horizontal(const unsigned* hq, const unsigned* trow, int32_t lim, int32_t hofs, int hmax, int osh, int top)
{
  unsigned v = 0;
#pragma unroll
  for (int k = 0; k < M355_RESIZE_MAX_TAPS; k++) {
    if (k >= hmax) break;
    const int32_t x = hofs + k;
    if constexpr (FILTER == M355_FILTER_CUBIC) v = (unsigned)d_mad24((int)hq[k], (int)trow[x < lim ? x : lim - 1], (int)v);
    else v = d_umad24(hq[k], trow[x < lim ? x : lim - 1], v);        /* (behind the row's last coefficient: 0 times an entry of the row) */
  }
  if constexpr (FILTER == M355_FILTER_CUBIC) return (unsigned)d_clip3(0, top, ((int)v + (1 << (osh - 1))) >> osh);
  else return ((v >> 1) + (1u << (osh - 1))) >> osh;
}
/* a row of resize_taps.h under the kernel's filter */
template <int FILTER>
__device__ __forceinline__ int d_rr_row(int64_t sn, int64_t dn, int cosited, int64_t i, int32_t* first, int32_t* coeff, int stride)
{
  if constexpr (FILTER == M355_FILTER_CUBIC) return m355_resize_row_cubic(sn, dn, cosited, i, first, coeff, stride);
  else return m355_resize_row(sn, dn, cosited, i, first, coeff, stride);
}

/* The modes and their kernel arguments.  RR_SRC(i) / RR_PITCH(i): plane i's first sample and pitch class i of the frame or of the slice's record;
   RR_GEOM(field): a field of the source's geometry, the slice's in RR_ROIS, else the launch's — each read at the place of its use. */
enum { RR_FRAME = 0, RR_BATCH = 1, RR_ROIS = 2 };
enum { RR_COLOUR_OFF = 0, RR_COLOUR_TABLES = 1, RR_COLOUR_TONE = 2 };   /* COLOUR: no stage, a plain object, a tone object */
enum { RR_PX_OFF = 0, RR_PX_8 = 1, RR_PX_10 = 2 };                      /* PX: R'G'B' elements, 8-bit pixels (3 or 4 bytes), 2:10:10:10 pixels */
template <int MODE> struct RrArgs { typedef ExportResizedRgbArgs T; };
template <> struct RrArgs<RR_BATCH> { typedef ExportTensorArgs T; };
template <> struct RrArgs<RR_ROIS> { typedef ExportTensorRoisArgs T; };
#define RR_SRC(i) ({ const M355_GLOBAL uint8_t* g_; if constexpr (MODE == RR_FRAME) g_ = (const M355_GLOBAL uint8_t*)a.src[i]; else g_ = (const M355_GLOBAL uint8_t*)a.fr[slice].src[i]; g_; })
#define RR_PITCH(i) ({ uint32_t g_; if constexpr (MODE == RR_FRAME) g_ = (uint32_t)a.src_pitch[i]; else g_ = (uint32_t)a.fr[slice].src_pitch[i]; g_; })
#define RR_GEOM(field) ({ uint32_t g_; if constexpr (MODE == RR_ROIS) g_ = a.fr[slice].field; else g_ = a.field; g_; })

template <int SB, int EB, int MODE, int FILTER, bool SITED, int COLOUR, int PX>
__global__ void __launch_bounds__(256) k_export_resized_rgb(typename RrArgs<MODE>::T a)
{
  static_assert(PX == RR_PX_OFF || (MODE == RR_FRAME && EB == (PX == RR_PX_10 ? 2 : 1)), "pixel formats: RR_FRAME, with the integer stage of their channel bits");
  constexpr bool CUBIC = FILTER == M355_FILTER_CUBIC;
  constexpr int S = 16 / SB;
  constexpr uint32_t OB = RR_TW * 3 * (MODE == RR_FRAME ? 2 : EB);   /* bytes of a staged output row: 256 pixels x 3 channels x 2 (tensors: EB) bytes */
  uint32_t slice = 0;                                           /* (wave-uniform: the slice's record comes by scalar loads) */
  if constexpr (MODE == RR_FRAME) M355_GATE(a);
  else {
    if constexpr (MODE == RR_ROIS) slice = blockIdx.y; else slice = blockIdx.x / a.units;
    if (slice >= a.n) return;
    M355_GATE(a.fr[slice]);
  }
  if constexpr (MODE == RR_ROIS) { if (blockIdx.x >= a.fr[slice].units) return; }   /* (the grid is as wide as the slice with the most units) */
  __shared__ unsigned s_t[2][RR_SPAN];                          /* [pass & 1]: the t rows of the pass's segments; in the prologue: the lanes' horizontal rows */
  __shared__ int32_t s_vy[2][RR_TH][2 + M355_RESIZE_MAX_TAPS];  /* [luma, chroma] per output row of the tile: first source row, number of rows, coefficients */
  __shared__ int32_t s_span[2][2];                              /* [luma, chroma] first and last source column of the tile */
  __shared__ unsigned short s_c[2][RR_TH][RR_CW];               /* the resized Cb and Cr samples the tile's pixels need */
  __shared__ __attribute__((aligned(16))) uint8_t s_o[2][2][OB];  /* [pass & 1][row of the pass]: the staged output rows */
  uint32_t unit = blockIdx.x;
  if constexpr (MODE == RR_FRAME) { if (unit >= a.units) return; }   /* (here, not beside the gate: there the two exits become one branch and the code another) */
  if constexpr (MODE == RR_BATCH) unit -= slice * a.units;
  const uint32_t tid = threadIdx.x;
  /* the colour transform stage (m355_export_opts.colour): its output table goes to LDS here, behind the gate and ahead of the prologue's barrier */
  const unsigned short* s_lo = nullptr;
  if constexpr (COLOUR != RR_COLOUR_OFF) {
    __shared__ unsigned s_lut[M355_COLOUR_LDS_DWORDS];
    d_colour_fill(a.colour.t, s_lut, tid);
    s_lo = (const unsigned short*)s_lut;
  }
  const uint32_t run = unit / RR_GEOM(tiles_x), tile = unit - run * RR_GEOM(tiles_x);
  const uint32_t tw = RR_GEOM(tile_w), c0 = tile * tw, j0 = run * RR_TH;
  const uint32_t dnx = a.dn_x[0], dny = a.dn_y[0], cdx = a.dn_x[1], cdy = a.dn_y[1];
  const uint32_t ncols = dnx - c0 < tw ? dnx - c0 : tw, nrows = dny - j0 < (uint32_t)RR_TH ? dny - j0 : (uint32_t)RR_TH;
  const int cf = a.cf;
  bool planar;                                                  /* planar R'G'B' / NCHW: three staged segments */
  if constexpr (PX != RR_PX_OFF) planar = false;              /* (a pixel is one element of the packed row) */
  else if constexpr (MODE == RR_FRAME) planar = a.planar != 0; else planar = a.nhwc == 0;
  const uint32_t swl = (cf == 1 || cf == 2) ? 1u : 0u, shl = cf == 1 ? 1u : 0u;
  /* the siting of 4:2:0 chroma (m355_export_opts; the host passes 0 for every other format): horizontally CENTRE, vertically TOP.  SITED = false is
     type 0, whose statements stand as they were in the other branch of each `if constexpr`: those instantiations are what they were before */
  bool centre = false, top_sited = false;
  if constexpr (SITED) { centre = (a.chroma_loc & 1) != 0; top_sited = (a.chroma_loc & 2) != 0; }
  /* the chroma tile: columns cc0 .. cc1 and rows cj0 .. cj1 of the resized chroma planes */
  uint32_t cc0 = 0, ncc = 0, cj0 = 0, ncr = 0;
  if (cf != 0) {
    cc0 = c0 >> swl;
    if constexpr (SITED) { if (centre && cc0) cc0--; }          /* CENTRE: the left neighbour of the tile's first column */
    uint32_t cc1 = ((c0 + ncols - 1) >> swl) + swl;
    if (cc1 > cdx - 1) cc1 = cdx - 1;
    cj0 = j0;
    uint32_t cj1 = j0 + nrows - 1;
    if (shl) { cj0 = (j0 >> 1) ? (j0 >> 1) - 1 : 0u; cj1 = ((j0 + nrows - 1) >> 1) + 1; }
    if constexpr (SITED) { if (shl && top_sited) cj0 = j0 >> 1; }   /* (TOP reads no row above j) */
    if (cj1 > cdy - 1) cj1 = cdy - 1;
    ncc = cc1 - cc0 + 1; ncr = cj1 - cj0 + 1;
  }

  /* prologue: the filter rows of this tile */
  int32_t* hrow = (int32_t*)&s_t[0][0];                        /* coefficient k of lane i at [k * RR_TW + i] */
  int32_t hfirst = 0, cfirst = 0;
  if (tid < ncc) {
    const int hn = d_rr_row<FILTER>(RR_GEOM(sn_x[1]), cdx, SITED && centre ? 0 : (int)swl, cc0 + tid, &cfirst, hrow + tid, RR_TW);
    if (tid == 0) s_span[1][0] = cfirst;
    if (tid == ncc - 1) s_span[1][1] = cfirst + hn - 1;
  }
  if (tid >= 256u - RR_TH && tid - (256u - RR_TH) < nrows) {
    const uint32_t jj = tid - (256u - RR_TH);
    s_vy[0][jj][1] = d_rr_row<FILTER>(RR_GEOM(sn_y[0]), dny, 0, j0 + jj, &s_vy[0][jj][0], &s_vy[0][jj][2], 1);
  }
  if (tid >= 256u - 2 * RR_TH && tid - (256u - 2 * RR_TH) < ncr) {
    const uint32_t jj = tid - (256u - 2 * RR_TH);
    s_vy[1][jj][1] = d_rr_row<FILTER>(RR_GEOM(sn_y[1]), cdy, SITED && top_sited ? 1 : 0, cj0 + jj, &s_vy[1][jj][0], &s_vy[1][jj][2], 1);
  }
  __syncthreads();

  unsigned raw[8][4];
  uint32_t par = 0;
  /* the chroma phase: row by row into s_c, Cb and Cr in one pass where both t rows fit one row of s_t (4:2:0 / 4:2:2), else one after the other */
  if (cf != 0) {
    unsigned cq[M355_RESIZE_MAX_TAPS];
#pragma unroll
    for (int k = 0; k < M355_RESIZE_MAX_TAPS; k++) cq[k] = tid < ncc ? (unsigned)hrow[k * RR_TW + tid] : 0u;
    __syncthreads();                                           /* (the lanes' rows are read: s_t is free) */
    const int32_t span0 = s_span[1][0];
    uint32_t nvec = (uint32_t)(s_span[1][1] - span0 + S) / S;
    if (nvec > (uint32_t)(RR_SPAN / S)) nvec = RR_SPAN / S;
    /* segments per pass: Cb and Cr side by side where two spans fit a row of s_t and their vectors the workgroup's lanes (a lane with a second
       vector would load it behind the first, not ahead), and two rows of each where four fit */
    const uint32_t cap = (nvec * S <= (uint32_t)(RR_SPAN / 4) && 4u * nvec <= 256u) ? 4u : ((nvec * S <= (uint32_t)(RR_SPAN / 2) && 2u * nvec <= 256u) ? 2u : 1u);
    const uint32_t npl = cap >= 2u ? 2u : 1u, rpp = cap / npl, nseg = cap, seglen = RR_SPAN / cap;
    const int hmax = m355_resize_max_taps_filtered(FILTER, RR_GEOM(sn_x[1]), cdx);
    const int32_t hofs = cfirst - span0, lim = (int32_t)seglen;
    const uint32_t pitch = RR_PITCH(1);
    const int tsh = a.bdc - (CUBIC ? 2 : 4), osh = (CUBIC ? 30 : 31) - a.bdc, top = (1 << a.bdc) - 1;
    for (uint32_t c = 0; c < 2; c += npl) {
      const M355_GLOBAL uint8_t* const src0 = c ? RR_SRC(2) : RR_SRC(1);
      const M355_GLOBAL uint8_t* const src1 = RR_SRC(2);
      const RrWhere me = d_rr_where<SB>(src0, src1, span0, nvec, npl, tid);
      const bool active = tid < nseg * nvec;
      if (active && me.row < ncr) {
        const int vfirst = s_vy[1][me.row][0], vn = s_vy[1][me.row][1];
        RR_LOAD_BATCH(me.p + (size_t)vfirst * (size_t)pitch, 0, vn, pitch)
      }
      for (uint32_t r = 0; r < ncr; r += rpp, par ^= 1u) {
        d_rr_vertical<SB, FILTER>(src0, src1, pitch, span0, nvec, npl, nseg, seglen, &s_vy[1][r], ncr - r, tsh, s_t[par], tid, raw);
        if (active && r + rpp + me.row < ncr) {                /* the next pass's first batch, in flight across the horizontal pass */
          const int nfirst = s_vy[1][r + rpp + me.row][0], nn = s_vy[1][r + rpp + me.row][1];
          RR_LOAD_BATCH(me.p + (size_t)nfirst * (size_t)pitch, 0, nn, pitch)
        }
        __syncthreads();
        if (tid < ncc) {
          for (uint32_t i = 0; i < rpp && r + i < ncr; i++)
            for (uint32_t pl = 0; pl < npl; pl++)
              s_c[c + pl][r + i][tid] = (unsigned short)d_rr_horizontal<FILTER>(cq, s_t[par] + (i * npl + pl) * seglen, lim, hofs, hmax, osh, top);
        }
        /* (no second barrier: the next pass's t goes to the other half of s_t, and the pass after it is written behind the next barrier) */
      }
    }
    __syncthreads();                                           /* (the last t row is read: s_t is free for the luma rows of the lanes) */
  }
  /* the horizontal rows of the tile's luma columns, derived here so that their registers are not held across the chroma phase */
  unsigned hq[M355_RESIZE_MAX_TAPS];
  if (tid < ncols) {
    const int hn = d_rr_row<FILTER>(RR_GEOM(sn_x[0]), dnx, 0, c0 + tid, &hfirst, hrow + tid, RR_TW);
    if (tid == 0) s_span[0][0] = hfirst;
    if (tid == ncols - 1) s_span[0][1] = hfirst + hn - 1;
  }
#pragma unroll
  for (int k = 0; k < M355_RESIZE_MAX_TAPS; k++) hq[k] = tid < ncols ? (unsigned)hrow[k * RR_TW + tid] : 0u;
  __syncthreads();

  /* the luma phase */
  const int32_t span0 = s_span[0][0];
  uint32_t nvec = (uint32_t)(s_span[0][1] - span0 + S) / S;
  if (nvec > (uint32_t)(RR_SPAN / S)) nvec = RR_SPAN / S;
  const uint32_t rpp = (nvec * S <= (uint32_t)(RR_SPAN / 2) && 2u * nvec <= 256u) ? 2u : 1u, seglen = RR_SPAN / rpp;   /* two output rows per pass where two spans fit a row of s_t and the lanes */
  const int hmax = m355_resize_max_taps_filtered(FILTER, RR_GEOM(sn_x[0]), dnx);
  const int32_t hofs = hfirst - span0;
  const uint32_t pitch = RR_PITCH(0);                           /* (a frame's rows are far below 4 GiB) */
  const int tsh = a.bdl - (CUBIC ? 2 : 4), osh = (CUBIC ? 30 : 31) - a.bdl, top = (1 << a.bdl) - 1;
  const M355_GLOBAL uint8_t* const srcy = RR_SRC(0);
  const RrWhere me = d_rr_where<SB>(srcy, srcy, span0, nvec, 1u, tid);
  const bool active = tid < rpp * nvec;
  /* the constants of the launch (scalar): the rounding term and the luma offset in one, c0 folded into the chroma filter's rounding constants */
  const int F = a.k.F, ky = (int)((1u << (F - 1)) - (unsigned)a.k.cy * (unsigned)a.k.y0);
  const int cy = a.k.cy, crv = a.k.crv, ncgu = -a.k.cgu, ncgv = -a.k.cgv, cbu = a.k.cbu, kc0 = a.k.c0;
  /* this lane's columns of the chroma tile: column i of its pixel and the clamped neighbour to the right.  SITED: the neighbour is to the left for an
     even luma column under CENTRE (LEFT: none, weight 0), and wh0, 4 - wh0 are the two columns' weights in quarters */
  const uint32_t X = c0 + tid;
  uint32_t ci = 0, cin = 0;
  if (cf != 0 && tid < ncols) {
    const uint32_t i = X >> swl;
    uint32_t in = i + 1 < cdx ? i + 1 : cdx - 1;
    if constexpr (SITED) { if (centre && !(X & 1u)) in = i ? i - 1 : 0u; }
    ci = i - cc0; cin = swl ? in - cc0 : ci;
  }
  const bool odd = swl && (X & 1u);
  /* the epilogue of the launch (scalar): the clip of the integer stage; tensors: the element format, scale and bias per channel (RR_TE: 0 for a frame) */
#define RR_TE(T, expr) ({ T g_ = 0; if constexpr (MODE != RR_FRAME) g_ = (expr); g_; })
  const int M = COLOUR != RR_COLOUR_OFF ? 65535 : (MODE == RR_FRAME ? (EB == 1 ? 255 : 65535) : (RR_TE(int, a.u16) ? 65535 : 255));   /* (COLOUR: k is the U16 set) */
  const bool deliver_u8 = MODE == RR_FRAME ? EB == 1 : !RR_TE(int, a.u16);   /* COLOUR: step 4 of colour_transform.h */
  const uint32_t bf16_mask = RR_TE(int, a.bf16) ? 0xFFFFFFFFu : 0u;
  const float sc[3] = {RR_TE(float, a.scale[0]), RR_TE(float, a.scale[1]), RR_TE(float, a.scale[2])};
  const float bi[3] = {RR_TE(float, a.bias[0]), RR_TE(float, a.bias[1]), RR_TE(float, a.bias[2])};
  /* where the staged row's bytes go: packed / NHWC one segment of up to OB / 4 dwords, planar / NCHW three of up to SEGW (512 or 1024 bytes apart) */
  constexpr uint32_t SEGW = OB / 12u, SEGSH = SEGW == 256u ? 8 : 7;
  /* PX: bytes per pixel (3: BGR8, else 4), the channel order and the alpha in its place — wave-uniform kernel arguments (pixel_pack.h) */
  uint32_t px_bytes = 0, px_alpha = 0;
  bool px_swapped = false;
  if constexpr (PX != RR_PX_OFF) { px_bytes = a.px_bytes; px_alpha = a.px_alpha_bits; px_swapped = a.px_swapped != 0; }
  uint32_t seg_bytes = ncols * (uint32_t)EB * (planar ? 1u : 3u);
  if constexpr (PX != RR_PX_OFF) seg_bytes = ncols * px_bytes;
  /* a mirrored slice: the lane of tile column t stages its pixel at position ncols - 1 - t, and the tile's first destination column is
     out_width - c0 - ncols; the stores themselves do not change */
  bool mirror = false;
  if constexpr (MODE == RR_ROIS) mirror = (a.fr[slice].flags & M355_ROI_MIRROR) != 0;
  const uint32_t pos = mirror ? ncols - 1u - tid : tid, col0 = mirror ? dnx - c0 - ncols : c0;
  /* the first byte of the tile's row of segment seg (RR_DST): in the frame's planes, or in the slice's place in the tensor */
  size_t col_bytes = 0, stride_c = 0, stride_h = 0;
  M355_GLOBAL uint8_t* dst0 = nullptr;
  if constexpr (PX != RR_PX_OFF) col_bytes = (size_t)col0 * px_bytes;
  else if constexpr (MODE == RR_FRAME) col_bytes = (size_t)col0 * (size_t)EB * (planar ? 1u : 3u);
  else {
    dst0 = (M355_GLOBAL uint8_t*)a.dst + (size_t)slice * (size_t)a.stride_n + (size_t)col0 * (size_t)EB * (planar ? 1u : 3u);
    stride_c = (size_t)a.stride_c; stride_h = (size_t)a.stride_h;
  }
#define RR_DST(seg, row) ({ \
    M355_GLOBAL uint8_t* d_; \
    if constexpr (MODE == RR_FRAME) \
      d_ = (M355_GLOBAL uint8_t*)(seg == 0 ? a.dst[0] : (seg == 1 ? a.dst[1] : a.dst[2])) + \
           (size_t)(row) * (size_t)(seg == 0 ? a.dst_pitch[0] : (seg == 1 ? a.dst_pitch[1] : a.dst_pitch[2])) + col_bytes; \
    else d_ = dst0 + (size_t)seg * stride_c + (size_t)(row) * stride_h; \
    d_; })
#define RR_STORE_ROW(buf, row) \
  for (uint32_t q = tid; q < OB / 4u; q += 256u) { \
    const uint32_t seg = planar ? q >> SEGSH : 0u, w = planar ? q & (SEGW - 1u) : q; \
    if (4u * w < seg_bytes) { \
      M355_GLOBAL uint8_t* d = RR_DST(seg, row) + 4u * w; \
      unsigned val; \
      __builtin_memcpy(&val, (buf) + 4u * q, 4); \
      if (4u * w + 4u <= seg_bytes) d_stg4(d, val); \
      else if constexpr (MODE == RR_FRAME) { for (uint32_t k = 0; k < 3; k++) if (4u * w + k < seg_bytes) d[k] = (uint8_t)(val >> (8 * k)); } \
      else d_stg2(d, val);                                     /* (EB = 2 only: the row's last element) */ \
    } \
  }

  if (active && me.row < nrows) {
    const int vfirst = s_vy[0][me.row][0], vn = s_vy[0][me.row][1];
    RR_LOAD_BATCH(me.p + (size_t)vfirst * (size_t)pitch, 0, vn, pitch)
  }
  uint32_t staged = 0, staged_j = 0;                           /* the rows staged by the pass before, and the first of them */
  for (uint32_t jp = 0; jp < nrows; jp += rpp, par ^= 1u) {
    d_rr_vertical<SB, FILTER>(srcy, srcy, pitch, span0, nvec, 1u, rpp, seglen, &s_vy[0][jp], nrows - jp, tsh, s_t[par], tid, raw);
    if (active && jp + rpp + me.row < nrows) {                 /* the next pass's first batch, in flight across the horizontal pass */
      const int nfirst = s_vy[0][jp + rpp + me.row][0], nn = s_vy[0][jp + rpp + me.row][1];
      RR_LOAD_BATCH(me.p + (size_t)nfirst * (size_t)pitch, 0, nn, pitch)
    }
    __syncthreads();
    for (uint32_t i = 0; i < staged; i++) { RR_STORE_ROW(s_o[par ^ 1u][i], j0 + staged_j + i) }   /* the rows staged before this barrier */
    staged = nrows - jp < rpp ? nrows - jp : rpp; staged_j = jp;
    for (uint32_t ri = 0; ri < staged; ri++) {
      const uint32_t jj = jp + ri;
      if (tid < ncols) {
        const int y = (int)d_rr_horizontal<FILTER>(hq, s_t[par] + ri * seglen, (int32_t)seglen, hofs, hmax, osh, top);
        const int base = d_mad24(cy, y, ky);
        int r = base, g = base, b = base;
        if (cf != 0) {
          int uv[2];
          if constexpr (SITED) {
            /* types 1..3 (4:2:0): the reconstruction filter of the header with weights in quarters per axis, one rounding, c0 folded into its
               constant.  The rows and their weights are wave-uniform: MID {j: 3, j -+ 1: 1}, TOP {j: 4} on even and {j: 2, j + 1: 2} on odd luma rows */
            const uint32_t Y = j0 + jj, j = Y >> 1, jn = ((Y & 1u) || top_sited) ? (j + 1 < cdy ? j + 1 : cdy - 1) : (j ? j - 1 : 0u);
            const uint32_t rj = j - cj0, rn = jn - cj0;
            const int wv0 = top_sited ? ((Y & 1u) ? 2 : 4) : 3, wh0 = centre ? 3 : (odd ? 2 : 4), wh1 = 4 - wh0;
            if (wv0 != 4) {
#pragma unroll
              for (int c = 0; c < 2; c++) {
                const int t0 = wv0 * (int)s_c[c][rj][ci] + (4 - wv0) * (int)s_c[c][rn][ci], t1 = wv0 * (int)s_c[c][rj][cin] + (4 - wv0) * (int)s_c[c][rn][cin];
                uv[c] = (wh0 * t0 + wh1 * t1 + 8 - 16 * kc0) >> 4;
              }
            } else {
#pragma unroll
              for (int c = 0; c < 2; c++) uv[c] = (4 * (wh0 * (int)s_c[c][rj][ci] + wh1 * (int)s_c[c][rj][cin]) + 8 - 16 * kc0) >> 4;
            }
          } else if (cf == 1) {
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
          r = d_mad24(crv, uv[1], base);
          g = d_mad24(ncgv, uv[1], d_mad24(ncgu, uv[0], base));
          b = d_mad24(cbu, uv[0], base);
        }
        unsigned e[3] = {(unsigned)d_clip3(0, M, r >> F), (unsigned)d_clip3(0, M, g >> F), (unsigned)d_clip3(0, M, b >> F)};
        if constexpr (COLOUR != RR_COLOUR_OFF) {               /* table, matrix, (tone: the gain,) table on the 16-bit R'G'B', then the delivery the samples ask for */
          if constexpr (COLOUR == RR_COLOUR_TONE) d_colour_pixel_tone(a.colour.t, s_lo, a.colour.m, a.colour.g, a.colour.norm, a.colour.w, e);
          else d_colour_pixel(a.colour.t, s_lo, a.colour.m, e);
#pragma unroll
          for (int c = 0; c < 3; c++) e[c] = m355_ct_deliver(e[c], deliver_u8);
        }
        uint8_t* o = s_o[par][ri];
        if constexpr (PX != RR_PX_OFF) {                       /* the pixel's dword (10-bit: c10 of each 16-bit value), bpp bytes at pos * bpp */
          const uint32_t dw = m355_pp_pixel(PX == RR_PX_10, px_swapped, e, px_alpha);
          if (px_bytes == 4u) __builtin_memcpy(o + 4u * pos, &dw, 4);
          else { o[3u * pos] = (uint8_t)dw; o[3u * pos + 1u] = (uint8_t)(dw >> 8); o[3u * pos + 2u] = (uint8_t)(dw >> 16); }
        } else {
#pragma unroll
          for (int c = 0; c < 3; c++) {
            uint32_t bits = e[c];                              /* a frame: the clipped integer; a tensor: through the float stage */
            if constexpr (MODE != RR_FRAME) {
              const float f = m355_te_affine(e[c], sc[c], bi[c]);
              bits = EB == 4 ? m355_te_bits(f) : m355_te_half(f, bf16_mask);
            }
            const uint32_t at = planar ? (uint32_t)c * (SEGW * 4u) + pos * (uint32_t)EB : (3u * pos + (uint32_t)c) * (uint32_t)EB;
            if (EB == 4) __builtin_memcpy(o + at, &bits, 4);
            else if (EB == 1) o[at] = (uint8_t)bits;
            else { const unsigned short h = (unsigned short)bits; __builtin_memcpy(o + at, &h, 2); }
          }
        }
      }
    }
  }
  __syncthreads();
  for (uint32_t i = 0; i < staged; i++) { RR_STORE_ROW(s_o[par ^ 1u][i], j0 + staged_j + i) }
#undef RR_STORE_ROW
#undef RR_DST
#undef RR_TE
}
#undef RR_GEOM
#undef RR_PITCH
#undef RR_SRC
#undef RR_LOAD_BATCH

/* src_bytes: 1 or 2 per sample; elem_bytes: 1 or 2 per channel of a frame, 2 or 4 per element of a tensor */
#define RR_LAUNCH_C(MODE, B0, B1, F, S, C) \
  if (src_bytes == 1 && elem_bytes == B0) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_export_resized_rgb<1, B0, MODE, F, S, C, RR_PX_OFF>), g_, block, 0, st, a); \
  if (src_bytes == 1 && elem_bytes == B1) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_export_resized_rgb<1, B1, MODE, F, S, C, RR_PX_OFF>), g_, block, 0, st, a); \
  if (src_bytes == 2 && elem_bytes == B0) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_export_resized_rgb<2, B0, MODE, F, S, C, RR_PX_OFF>), g_, block, 0, st, a); \
  if (src_bytes == 2 && elem_bytes == B1) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_export_resized_rgb<2, B1, MODE, F, S, C, RR_PX_OFF>), g_, block, 0, st, a);
/* the pixel formats (RR_FRAME only): element bytes 1 / 2 stand for PX = 8-bit / 10-bit pixels, whose integer stage has those element bytes */
#define RR_LAUNCH_PX(MODE, B0, B1, F, S, C) \
  if (src_bytes == 1 && elem_bytes == 1) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_export_resized_rgb<1, 1, RR_FRAME, F, S, C, RR_PX_8>), g_, block, 0, st, a); \
  if (src_bytes == 1 && elem_bytes == 2) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_export_resized_rgb<1, 2, RR_FRAME, F, S, C, RR_PX_10>), g_, block, 0, st, a); \
  if (src_bytes == 2 && elem_bytes == 1) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_export_resized_rgb<2, 1, RR_FRAME, F, S, C, RR_PX_8>), g_, block, 0, st, a); \
  if (src_bytes == 2 && elem_bytes == 2) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_export_resized_rgb<2, 2, RR_FRAME, F, S, C, RR_PX_10>), g_, block, 0, st, a);
#define RR_LAUNCH_S(L, MODE, B0, B1, F, S) \
  if (a.colour.t && a.colour.g) { L(MODE, B0, B1, F, S, RR_COLOUR_TONE) } \
  else if (a.colour.t) { L(MODE, B0, B1, F, S, RR_COLOUR_TABLES) } \
  else { L(MODE, B0, B1, F, S, RR_COLOUR_OFF) }
#define RR_LAUNCH_F(L, MODE, B0, B1, F) \
  if (a.chroma_loc != 0) { RR_LAUNCH_S(L, MODE, B0, B1, F, true) } \
  else { RR_LAUNCH_S(L, MODE, B0, B1, F, false) }
#define RR_LAUNCH_WITH(L, MODE, B0, B1, grid) \
  const dim3 g_ grid, block(256); \
  if (filter == M355_FILTER_CUBIC) { RR_LAUNCH_F(L, MODE, B0, B1, M355_FILTER_CUBIC) } \
  else { RR_LAUNCH_F(L, MODE, B0, B1, M355_FILTER_TRIANGLE) }
#define RR_LAUNCH(MODE, B0, B1, grid) RR_LAUNCH_WITH(RR_LAUNCH_C, MODE, B0, B1, grid)
void m355_launch_export_resized_rgb(const ExportResizedRgbArgs& a, int src_bytes, int elem_bytes, int filter, hipStream_t st)
{
  if (!a.units) return;
  RR_LAUNCH(RR_FRAME, 1, 2, (a.units))
}
/* the same frame as pixels of a.px_bytes bytes (m355_frame_export_resized_pixels): ten = a 2:10:10:10 format */
void m355_launch_export_resized_pixels(const ExportResizedRgbArgs& a, int src_bytes, bool ten, int filter, hipStream_t st)
{
  if (!a.units) return;
  const int elem_bytes = ten ? 2 : 1;
  RR_LAUNCH_WITH(RR_LAUNCH_PX, RR_FRAME, 1, 2, (a.units))
}
void m355_launch_export_tensor(const ExportTensorArgs& a, int src_bytes, int elem_bytes, int filter, hipStream_t st)
{
  if (!a.units || !a.n) return;
  RR_LAUNCH(RR_BATCH, 2, 4, (a.units * a.n))
}
/* the batch of regions: blockIdx.y = slice, blockIdx.x = the unit inside it, up to the largest unit count of a slice */
void m355_launch_export_tensor_rois(const ExportTensorRoisArgs& a, int src_bytes, int elem_bytes, int filter, hipStream_t st)
{
  if (!a.max_units || !a.n) return;
  RR_LAUNCH(RR_ROIS, 2, 4, (a.max_units, a.n))
}
#undef RR_LAUNCH
#undef RR_LAUNCH_WITH
#undef RR_LAUNCH_PX
#undef RR_LAUNCH_F
#undef RR_LAUNCH_S
#undef RR_LAUNCH_C
