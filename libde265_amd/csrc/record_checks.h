/* record_checks.h — the record checks of the work lists, ONE definition for the host's validate() (runtime_upload.hip: lists that are
 * copied) and the device's k_validate (k_meta.hip: lists recorded in place).  Every later kernel takes its bounds from them, so a clause
 * lives here or nowhere.  A predicate returns 0 or the reason the host prints (the device only asks "non-zero"); a record with several
 * faults reports the first clause in the order written here; a field is bounded before anything shifts by it or indexes with it.
 * Plain C++ apart from the qualifier: a program without any HIP header can call them. */
#ifndef M355_RECORD_CHECKS_H
#define M355_RECORD_CHECKS_H
#include <stdint.h>
#include "de265_mi355x.h"
#ifdef __HIPCC__
#define M355_RC_FN __host__ __device__ inline
#else
#define M355_RC_FN inline
#endif

/* what the records are checked against: built once per picture, from m355_picture on the host and from DevPic on the device */
struct M355RecLimits {
  int32_t  width, height, sw, sh;   /* luma size; SubWidthC, SubHeightC */
  int32_t  chroma_format_idc, log2_min_cb_size, log2_ctb_size, n_wts;
  uint32_t pic_flags, n_coeffs, res_len, n_pcm;
  uint32_t ref_mask;                /* bit s: ref_frames[s] is a frame */
};
enum M355RecReason {
  M355_RC_OK = 0, M355_RC_MALFORMED, M355_RC_GEOMETRY, M355_RC_NO_LIST, M355_RC_REF_SLOT, M355_RC_WEIGHT_INDEX, M355_RC_LOG2WD,
  M355_RC_COEFF_RANGE, M355_RC_RES_RANGE, M355_RC_PCM_RANGE, M355_RC_MATRIX_ID, M355_RC_DST_SIZE, M355_RC_N_REASONS
};
static const char* const m355_rc_text[M355_RC_N_REASONS] = {      /* (host) the message of each reason */
  nullptr, "malformed", "geometry", "no list selected", "reference slot invalid", "weight index", "log2WD out of range",
  "coefficient range", "residual range", "pcm range", "matrix id", "DST only exists for 4x4"};

M355_RC_FN int m355_check_cu(const m355_cu& cu, const M355RecLimits& L)
{
  return (cu.log2_size < L.log2_min_cb_size || cu.log2_size > L.log2_ctb_size || cu.x >= L.width || cu.y >= L.height || cu.pred_mode > 2 || cu.part_mode > 7) ? M355_RC_MALFORMED : 0;
}
M355_RC_FN int m355_check_tu(const m355_tu& tu, const M355RecLimits& L) { return (tu.log2_size < 2 || tu.log2_size > 6 || tu.x >= L.width || tu.y >= L.height) ? M355_RC_MALFORMED : 0; }
/* the geometry clause of a prediction block alone: all that a reader of the motion field needs (map_element.h), whatever the reference slots hold */
M355_RC_FN int m355_check_pb_geometry(const m355_pb& pb, const M355RecLimits& L)
{
  return (pb.w < 4 || pb.h < 4 || pb.w > 64 || pb.h > 64 || (pb.w & 3) || (pb.h & 3) || pb.x + pb.w > L.width || pb.y + pb.h > L.height) ? M355_RC_GEOMETRY : 0;
}
M355_RC_FN int m355_check_pb(const m355_pb& pb, const M355RecLimits& L)
{
  if (m355_check_pb_geometry(pb, L)) return M355_RC_GEOMETRY;
  if (!(pb.flags & (M355_PBF_MC_L0 | M355_PBF_MC_L1))) return M355_RC_NO_LIST;
  for (int l = 0; l < 2; l++) {
    if (!(pb.flags & (M355_PBF_MC_L0 << l))) continue;
    if (!(pb.flags & (M355_PBF_FILL_L0 << l)) && (pb.ref_slot[l] < 0 || pb.ref_slot[l] >= M355_MAX_REF_FRAMES || !((L.ref_mask >> pb.ref_slot[l]) & 1u))) return M355_RC_REF_SLOT;
    if ((pb.flags & M355_PBF_WEIGHTED) && pb.wt_idx[l] >= L.n_wts) return M355_RC_WEIGHT_INDEX;
  }
  return 0;
}
M355_RC_FN int m355_check_wt(const m355_wt& wt, const M355RecLimits& L)
{
  return (wt.log2wd_luma < 1 || wt.log2wd_luma > 31 || (L.chroma_format_idc && (wt.log2wd_chroma < 1 || wt.log2wd_chroma > 31))) ? M355_RC_LOG2WD : 0;
}
/* bin: the size bin the record sits in (0..3 = 4x4 .. 32x32) */
M355_RC_FN int m355_check_rb(const m355_rb& rb, int bin, const M355RecLimits& L)
{
  const int n = 1 << (bin + 2);
  const int W = rb.cidx ? L.width / L.sw : L.width, H = rb.cidx ? L.height / L.sh : L.height;
  if (rb.log2_size != bin + 2 || rb.cidx > 2 || rb.kind > 3 || rb.x + n > W || rb.y + n > H) return M355_RC_MALFORMED;
  /* (words, not entries: a narrow block holds two entries per word) */
  if ((uint64_t)rb.coeff_ofs + ((rb.flags & M355_RBF_NARROW) ? (rb.ncoeff + 1u) / 2 : rb.ncoeff) > L.n_coeffs) return M355_RC_COEFF_RANGE;
  if ((rb.flags & M355_RBF_DEFERRED) && (uint64_t)rb.res_ofs + (uint32_t)(n * n) > L.res_len) return M355_RC_RES_RANGE;
  if ((L.pic_flags & M355_PF_SCALING_LIST) && (rb.matrix_id & 7) > 5) return M355_RC_MATRIX_ID;
  return (rb.kind == M355_RK_DST && bin != 0) ? M355_RC_DST_SIZE : 0;
}
M355_RC_FN int m355_check_ib(const m355_ib& ib, const M355RecLimits& L)
{
  if (ib.log2_size < 2 || ib.log2_size > 5 || ib.cidx > 2 || ib.mode > 34) return M355_RC_MALFORMED;
  const int n = 1 << ib.log2_size;                          /* (bounded above: 4..32) */
  const int W = ib.cidx ? L.width / L.sw : L.width, H = ib.cidx ? L.height / L.sh : L.height;
  if (ib.x + n > W || ib.y + n > H) return M355_RC_MALFORMED;
  if ((ib.flags & M355_IBF_HAS_RESIDUAL) && (uint64_t)ib.res_ofs + (uint32_t)(n * n) > L.res_len) return M355_RC_RES_RANGE;
  return ((ib.flags & M355_IBF_PCM) && (uint64_t)ib.res_ofs + (uint32_t)(n * n) > L.n_pcm) ? M355_RC_PCM_RANGE : 0;
}
#endif
