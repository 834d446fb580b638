/* map_element.h — the side maps of a picture (m355_picture_maps_async, include/de265_mi355x.h), ONE definition for the kernels (k_maps.hip) and the
 * host helper m355_maps_unit (runtime_maps.hip): which records count, what a record covers, what an element holds, what the summary counts.
 * Plain C++ apart from the qualifier, like record_checks.h, whose predicates decide which records are skipped.
 *
 * A unit takes its value at a luma position P whose coordinates are multiples of 4 (units are 4 .. 64 samples wide), so a record matters only through
 * the points of the 4x4 grid its rectangle contains: cells c0 .. c1 - 1 per axis, c0 = ceil(x / 4), c1 = ceil((x + n) / 4), cut to the picture.  That
 * holds for ANY x and n — an unaligned record of an unvalidated list paints exactly the points it contains, and a record that ends beyond the picture
 * (a CU or TU of a CTB that hangs over the edge) is clipped. */
#ifndef M355_MAP_ELEMENT_H
#define M355_MAP_ELEMENT_H
#include "record_checks.h"
#define M355_ME_FN M355_RC_FN

#define M355_ME_NONE_CU    0xFFFFFFFFu
#define M355_ME_NONE_QP    (-128)
#define M355_ME_NONE_TU    0u
#define M355_ME_NONE_INTRA 255u
#define M355_ME_NONE_REF   0x0000FFFFu   /* bytes FF FF 00 00 */

/* bytes of an element of each map */
M355_ME_FN int m355_me_elem_size(int map) { return map == M355_MAP_CU || map == M355_MAP_REF ? 4 : (map == M355_MAP_MV ? 8 : (map == M355_MAP_SLICE ? 2 : 1)); }

/* the unit grid and the 4x4 grid of one picture */
struct M355MapGrid {
  int32_t log2_unit, units_w, units_h;   /* U = 1 << log2_unit */
  int32_t w4, h4;                        /* points of the 4x4 grid inside the picture: ceil(width / 4), ceil(height / 4) */
  int32_t log2_ctb, ctbW;
};
M355_ME_FN M355MapGrid m355_me_grid(int width, int height, int log2_ctb, int log2_unit)
{
  M355MapGrid g;
  const int U = 1 << log2_unit;
  g.log2_unit = log2_unit; g.units_w = (width + U - 1) >> log2_unit; g.units_h = (height + U - 1) >> log2_unit;
  g.w4 = (width + 3) >> 2; g.h4 = (height + 3) >> 2;
  g.log2_ctb = log2_ctb; g.ctbW = (width + (1 << log2_ctb) - 1) >> log2_ctb;
  return g;
}
/* what the geometry clauses are checked against (the fields the other clauses read stay 0: they do not decide here) */
M355_ME_FN M355RecLimits m355_me_limits(int width, int height, int chroma_format_idc, int log2_min_cb_size, int log2_ctb_size)
{
  M355RecLimits L = {width, height, (chroma_format_idc == 1 || chroma_format_idc == 2) ? 2 : 1, chroma_format_idc == 1 ? 2 : 1,
                     chroma_format_idc, log2_min_cb_size, log2_ctb_size, 0, 0u, 0u, 0u, 0u, 0u};
  return L;
}

/* a record is read (1) or skipped and counted (0): the geometry clause of its record check — `malformed` is the first clause of each predicate, so
   "the predicate does not answer malformed" is "the clause holds" whatever the later clauses say */
M355_ME_FN int m355_me_cu_ok(const m355_cu& cu, const M355RecLimits& L) { return m355_check_cu(cu, L) != M355_RC_MALFORMED; }
M355_ME_FN int m355_me_tu_ok(const m355_tu& tu, const M355RecLimits& L) { return m355_check_tu(tu, L) != M355_RC_MALFORMED; }
M355_ME_FN int m355_me_pb_ok(const m355_pb& pb, const M355RecLimits& L) { return m355_check_pb_geometry(pb, L) == 0; }
M355_ME_FN int m355_me_ib_ok(const m355_ib& ib, const M355RecLimits& L) { return m355_check_ib(ib, L) != M355_RC_MALFORMED; }
/* an intra block that MAP_INTRA shows: luma, not PCM (the others cover nothing on that map) */
M355_ME_FN int m355_me_ib_shown(const m355_ib& ib) { return ib.cidx == 0 && !(ib.flags & M355_IBF_PCM); }

/* points of the 4x4 grid along one axis inside x .. x + n: [*c0, *c1), cut to `limit` points (empty: *c1 <= *c0) */
M355_ME_FN void m355_me_cells(int x, int n, int limit, int* c0, int* c1)
{
  *c0 = (x + 3) >> 2;
  const int e = (x + n + 3) >> 2;
  *c1 = e < limit ? e : limit;
}
M355_ME_FN int m355_me_covers(int x, int n, int p) { return p >= x && p < x + n; }

/* the elements */
M355_ME_FN uint32_t m355_me_cu(const m355_cu& cu) { return (uint32_t)cu.pred_mode | (uint32_t)cu.part_mode << 8 | (uint32_t)cu.log2_size << 16 | (uint32_t)cu.flags << 24; }
M355_ME_FN uint32_t m355_me_tu(const m355_tu& tu) { return (uint32_t)tu.log2_size | ((tu.flags & M355_TUF_NONZERO_COEFF) ? 0x80u : 0u); }
/* the four 16-bit values as two little-endian words: [0] = L0's pair, [1] = L1's */
M355_ME_FN void m355_me_mv(const m355_pb& pb, uint32_t w[2])
{
  for (int l = 0; l < 2; l++)
    w[l] = (pb.flags & (M355_PBF_PRED_L0 << l)) ? ((uint32_t)(uint16_t)pb.mv[l][0] | (uint32_t)(uint16_t)pb.mv[l][1] << 16) : 0u;
}
M355_ME_FN uint32_t m355_me_ref(const m355_pb& pb)
{
  const uint32_t r0 = (pb.flags & M355_PBF_PRED_L0) ? (uint32_t)(uint8_t)pb.ref_slot[0] : 0xFFu;
  const uint32_t r1 = (pb.flags & M355_PBF_PRED_L1) ? (uint32_t)(uint8_t)pb.ref_slot[1] : 0xFFu;
  return r0 | r1 << 8 | (uint32_t)pb.flags << 16;
}

/* what the summary reads off the elements: the class of a MAP_CU element (0 intra, 1 inter, 2 skip; -1: not covered) and "both PRED flags" of a
   MAP_REF element */
M355_ME_FN int m355_me_cu_class(uint32_t cu_element) { return cu_element == M355_ME_NONE_CU ? -1 : (int)(cu_element & 0xFFu); }
M355_ME_FN int m355_me_ref_bipred(uint32_t ref_element) { return ((ref_element >> 16) & (M355_PBF_PRED_L0 | M355_PBF_PRED_L1)) == (M355_PBF_PRED_L0 | M355_PBF_PRED_L1); }
#endif
