/*
 * de265_mi355x.h — C ABI of the MI355X (gfx950 / CDNA4) HEVC pixel-reconstruction backend.
 *
 * This is the drop-in boundary for the ONE hot path of strukturag/libde265 that this project
 * accelerates: everything behind `struct acceleration_functions` (libde265/acceleration.h:29-231)
 * plus the two in-loop filter drivers that bypass that table (libde265/deblock.cc:908-946,
 * libde265/sao.cc:327-382).  Two layers are exported, both `extern "C"`, plain pointers/sizes only:
 *
 *  (1) SLOT LAYER  — `init_acceleration_functions_mi355x()` fills a table with the EXACT layout and
 *      signatures of the reference's `struct acceleration_functions` (cf. the reference's own
 *      `init_acceleration_functions_fallback` libde265/fallback.cc:28 and `_sse` x86/sse.cc:46).
 *      Every slot is synchronous, takes host pointers, and runs the HIP kernel for one block.
 *      It exists for parity (the tests drive it exactly like dev-tools/test-*.cc drive the SIMD
 *      tables) and as the trivially-correct entry; it is NOT the fast path (one PCIe round trip
 *      per block).  `m355_*_batch()` variants run N blocks per launch.
 *
 *  (2) PICTURE LAYER — the deferred reconstruction executor.  The host parser (the reference's own
 *      slice.cc / motion.cc glue) RECORDS per-picture work lists instead of
 *      calling slots per block; `m355_submit_picture()` uploads them and runs
 *         inter prediction → residual (dequant + IDCT/IDST/skip/bypass) → intra wavefront →
 *         deblock V → deblock H → SAO
 *      on the device, against reference frames that stay resident in HBM.
 *
 * All structs are plain little-endian PODs shared by the HIP library, the reference-side glue that
 * records them inside the reference's decoder (glue/m355_glue.cc), the CPU oracle
 * (oracle/hevc_oracle.c) and the Python test layer (numpy dtypes in libde265_amd/worklist.py mirror
 * them field by field; tests/test_abi_layout.py checks sizes).
 */
#ifndef DE265_MI355X_H
#define DE265_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define M355_API __attribute__((visibility("default")))

/* ------------------------------------------------------------------------------------------------
 * Error codes (the reference's slots return void and have no error channel, acceleration.h:29-231;
 * the picture layer can fail on resources, so it reports).
 * ---------------------------------------------------------------------------------------------- */
enum {
  M355_OK = 0,
  M355_ERR_NO_DEVICE = 1,     /* no HIP device / runtime failure at init            */
  M355_ERR_HIP = 2,           /* a HIP call failed; m355_last_error() has the text   */
  M355_ERR_INVALID = 3,       /* malformed work list / bad argument                  */
  M355_ERR_NOMEM = 4,
  M355_ERR_TIMEOUT = 5,       /* intra wavefront spin bound exceeded (device flag)   */
  M355_ERR_BUSY = 6,          /* m355_decode_status: the decode has not finished yet */
  M355_ERR_STALE = 7          /* m355_decode_status: the serial is older than the status ring (its outcome is no longer kept) */
};

M355_API const char* m355_last_error(void);
M355_API int m355_device_count(void);
M355_API const char* m355_version(void);

/* ================================================================================================
 * (1) SLOT LAYER — same member order as libde265/acceleration.h:29-231 (94 pointers, 752 bytes on
 * x86-64; the reference struct's inline wrapper methods/templates occupy no storage).
 * ============================================================================================== */

struct m355_acceleration_functions {
  /* weighted prediction write-back, 8 bit (acceleration.h:31-47) */
  void (*put_weighted_pred_avg_8)(uint8_t* dst, ptrdiff_t dststride, const int16_t* src1,
                                  const int16_t* src2, ptrdiff_t srcstride, int width, int height);
  void (*put_unweighted_pred_8)(uint8_t* dst, ptrdiff_t dststride, const int16_t* src,
                                ptrdiff_t srcstride, int width, int height);
  void (*put_weighted_pred_8)(uint8_t* dst, ptrdiff_t dststride, const int16_t* src,
                              ptrdiff_t srcstride, int width, int height, int w, int o, int log2WD);
  void (*put_weighted_bipred_8)(uint8_t* dst, ptrdiff_t dststride, const int16_t* src1,
                                const int16_t* src2, ptrdiff_t srcstride, int width, int height,
                                int w1, int o1, int w2, int o2, int log2WD);
  /* 9-16 bit (acceleration.h:50-64) */
  void (*put_weighted_pred_avg_16)(uint16_t* dst, ptrdiff_t dststride, const int16_t* src1,
                                   const int16_t* src2, ptrdiff_t srcstride, int width, int height,
                                   int bit_depth);
  void (*put_unweighted_pred_16)(uint16_t* dst, ptrdiff_t dststride, const int16_t* src,
                                 ptrdiff_t srcstride, int width, int height, int bit_depth);
  void (*put_weighted_pred_16)(uint16_t* dst, ptrdiff_t dststride, const int16_t* src,
                               ptrdiff_t srcstride, int width, int height, int w, int o, int log2WD,
                               int bit_depth);
  void (*put_weighted_bipred_16)(uint16_t* dst, ptrdiff_t dststride, const int16_t* src1,
                                 const int16_t* src2, ptrdiff_t srcstride, int width, int height,
                                 int w1, int o1, int w2, int o2, int log2WD, int bit_depth);

  /* chroma (epel) and luma (qpel) interpolation, 8 bit (acceleration.h:87-102).
     NOTE: as in the reference, put_hevc_epel_8 has NO bit_depth argument, the others do. */
  void (*put_hevc_epel_8)(int16_t* dst, ptrdiff_t dststride, const uint8_t* src, ptrdiff_t srcstride,
                          int width, int height, int mx, int my, int16_t* mcbuffer);
  void (*put_hevc_epel_h_8)(int16_t* dst, ptrdiff_t dststride, const uint8_t* src,
                            ptrdiff_t srcstride, int width, int height, int mx, int my,
                            int16_t* mcbuffer, int bit_depth);
  void (*put_hevc_epel_v_8)(int16_t* dst, ptrdiff_t dststride, const uint8_t* src,
                            ptrdiff_t srcstride, int width, int height, int mx, int my,
                            int16_t* mcbuffer, int bit_depth);
  void (*put_hevc_epel_hv_8)(int16_t* dst, ptrdiff_t dststride, const uint8_t* src,
                             ptrdiff_t srcstride, int width, int height, int mx, int my,
                             int16_t* mcbuffer, int bit_depth);
  void (*put_hevc_qpel_8[4][4])(int16_t* dst, ptrdiff_t dststride, const uint8_t* src,
                                ptrdiff_t srcstride, int width, int height, int16_t* mcbuffer);
  /* 9-16 bit (acceleration.h:105-120) */
  void (*put_hevc_epel_16)(int16_t* dst, ptrdiff_t dststride, const uint16_t* src,
                           ptrdiff_t srcstride, int width, int height, int mx, int my,
                           int16_t* mcbuffer, int bit_depth);
  void (*put_hevc_epel_h_16)(int16_t* dst, ptrdiff_t dststride, const uint16_t* src,
                             ptrdiff_t srcstride, int width, int height, int mx, int my,
                             int16_t* mcbuffer, int bit_depth);
  void (*put_hevc_epel_v_16)(int16_t* dst, ptrdiff_t dststride, const uint16_t* src,
                             ptrdiff_t srcstride, int width, int height, int mx, int my,
                             int16_t* mcbuffer, int bit_depth);
  void (*put_hevc_epel_hv_16)(int16_t* dst, ptrdiff_t dststride, const uint16_t* src,
                              ptrdiff_t srcstride, int width, int height, int mx, int my,
                              int16_t* mcbuffer, int bit_depth);
  void (*put_hevc_qpel_16[4][4])(int16_t* dst, ptrdiff_t dststride, const uint16_t* src,
                                 ptrdiff_t srcstride, int width, int height, int16_t* mcbuffer,
                                 int bit_depth);

  /* inverse transforms (acceleration.h:143-170) */
  void (*transform_bypass)(int32_t* residual, const int16_t* coeffs, int nT);
  void (*transform_bypass_rdpcm_v)(int32_t* r, const int16_t* coeffs, int nT);
  void (*transform_bypass_rdpcm_h)(int32_t* r, const int16_t* coeffs, int nT);
  void (*transform_skip_8)(uint8_t* dst, const int16_t* coeffs, ptrdiff_t stride);          /* dead slot in the reference (fallback-dct.cc:52) */
  void (*transform_skip_rdpcm_v_8)(uint8_t* dst, const int16_t* coeffs, int nT, ptrdiff_t stride);
  void (*transform_skip_rdpcm_h_8)(uint8_t* dst, const int16_t* coeffs, int nT, ptrdiff_t stride);
  void (*transform_4x4_dst_add_8)(uint8_t* dst, const int16_t* coeffs, ptrdiff_t stride);
  void (*transform_add_8[4])(uint8_t* dst, const int16_t* coeffs, ptrdiff_t stride);
  void (*transform_skip_16)(uint16_t* dst, const int16_t* coeffs, ptrdiff_t stride, int bit_depth); /* dead slot (fallback-dct.cc:69) */
  void (*transform_4x4_dst_add_16)(uint16_t* dst, const int16_t* coeffs, ptrdiff_t stride,
                                   int bit_depth);
  void (*transform_add_16[4])(uint16_t* dst, const int16_t* coeffs, ptrdiff_t stride, int bit_depth);
  void (*rotate_coefficients)(int16_t* coeff, int nT);
  void (*transform_idst_4x4)(int32_t* dst, const int16_t* coeffs, int bdShift, int max_coeff_bits);
  void (*transform_idct_4x4)(int32_t* dst, const int16_t* coeffs, int bdShift, int max_coeff_bits);
  void (*transform_idct_8x8)(int32_t* dst, const int16_t* coeffs, int bdShift, int max_coeff_bits);
  void (*transform_idct_16x16)(int32_t* dst, const int16_t* coeffs, int bdShift, int max_coeff_bits);
  void (*transform_idct_32x32)(int32_t* dst, const int16_t* coeffs, int bdShift, int max_coeff_bits);
  void (*add_residual_8)(uint8_t* dst, ptrdiff_t stride, const int32_t* r, int nT, int bit_depth);
  void (*add_residual_16)(uint16_t* dst, ptrdiff_t stride, const int32_t* r, int nT, int bit_depth);

  /* dequantisation (acceleration.h:175-181) */
  void (*dequant_coeff_block)(int16_t* coeffBuf, const int16_t* coeffList, const int16_t* coeffPos,
                              int nCoeff, int32_t fact, int32_t offset, int32_t bdShift);

  /* deblocking, one 4-line edge segment (acceleration.h:184-187) */
  void (*deblock_luma_8)(uint8_t* ptr, ptrdiff_t stride, int vertical, int dE, int dEp, int dEq,
                         int tc, int filterP, int filterQ);
  void (*deblock_chroma_8)(uint8_t* ptr, ptrdiff_t stride, int vertical, int tc, int filterP,
                           int filterQ);

  /* (R)DPCM / transform skip residuals (acceleration.h:189-193) */
  void (*rdpcm_v)(int32_t* residual, const int16_t* coeffs, int nT, int tsShift, int bdShift);
  void (*rdpcm_h)(int32_t* residual, const int16_t* coeffs, int nT, int tsShift, int bdShift);
  void (*transform_skip_residual)(int32_t* residual, const int16_t* coeffs, int nT, int tsShift,
                                  int bdShift);

  /* intra prediction from a prepared border[-2nT..2nT] (acceleration.h:205-212) */
  void (*intra_pred_dc_8)(uint8_t* dst, ptrdiff_t stride, int nT, int cIdx, const uint8_t* border);
  void (*intra_pred_dc_16)(uint16_t* dst, ptrdiff_t stride, int nT, int cIdx, const uint16_t* border);
  void (*intra_pred_planar_8)(uint8_t* dst, ptrdiff_t stride, int nT, int cIdx,
                              const uint8_t* border);
  void (*intra_pred_planar_16)(uint16_t* dst, ptrdiff_t stride, int nT, int cIdx,
                               const uint16_t* border);
  void (*intra_pred_angular_8)(uint8_t* dst, ptrdiff_t stride, int bit_depth,
                               int disableBoundaryFilter, int xB0, int yB0, int mode, int nT,
                               int cIdx, const uint8_t* border);
  void (*intra_pred_angular_16)(uint16_t* dst, ptrdiff_t stride, int bit_depth,
                                int disableBoundaryFilter, int xB0, int yB0, int mode, int nT,
                                int cIdx, const uint16_t* border);

  /* forward transforms — encoder only (acceleration.h:222-230); OUT OF SCOPE: left untouched
     (the fallback's pointers stay in place when the table was pre-filled, NULL otherwise). */
  void (*fwd_transform_4x4_dst_8)(int16_t* coeffs, const int16_t* src, ptrdiff_t stride);
  void (*fwd_transform_8[4])(int16_t* coeffs, const int16_t* src, ptrdiff_t stride);
  void (*hadamard_transform_8[4])(int16_t* coeffs, const int16_t* src, ptrdiff_t stride);
};

/* Replaces: init_acceleration_functions_sse/_avx2/_avx512 (libde265/x86/sse.cc:46-171) at the call
 * site libde265/decctx.cc:239-270 — call it AFTER init_acceleration_functions_fallback(); it
 * overrides every decoder slot and leaves the encoder-only forward transforms untouched.
 * `accel` must point to a `struct acceleration_functions` (identical layout). Returns M355_OK, or
 * M355_ERR_NO_DEVICE without touching the table (fail loudly; there is no CPU fallback here). */
M355_API int init_acceleration_functions_mi355x(void* accel);

/* ------------------------------------------------------------------------------------------------
 * Batched slot entry points: N independent blocks per launch, host pointers.
 * ---------------------------------------------------------------------------------------------- */

/* kind: 0 = IDCT (transform_add[log2-2]), 1 = 4x4 IDST (transform_4x4_dst_add). dst blocks live in
 * one host buffer `dst_base` (byte size dst_bytes) at sample offsets dst_off[i], row stride in
 * samples; coeffs are dense nT*nT int16 per block, consecutive. pixel_bytes 1 (8 bit) or 2. */
M355_API int m355_transform_add_batch(int n, int log2_nT, int kind, int bit_depth,
                                      void* dst_base, size_t dst_bytes, const int64_t* dst_off,
                                      ptrdiff_t stride, const int16_t* coeffs);

/* ================================================================================================
 * (2) PICTURE LAYER — work lists.
 * ============================================================================================== */

#define M355_MAX_TILE_COLS 20   /* DE265_MAX_TILE_COLUMNS, libde265/pps.h:30 */
#define M355_MAX_TILE_ROWS 22   /* DE265_MAX_TILE_ROWS,    libde265/pps.h:31 */
#define M355_MAX_REF_FRAMES 32  /* DPB slots addressable by one picture      */

/* picture-level flags (pic_params.flags) */
enum {
  M355_PF_CONSTRAINED_INTRA_PRED   = 1 << 0,  /* pps.constrained_intra_pred_flag (intrapred.h:546)      */
  M355_PF_STRONG_INTRA_SMOOTHING   = 1 << 1,  /* sps.strong_intra_smoothing_enable_flag (intrapred.h:216)*/
  M355_PF_PCM_LOOP_FILTER_DISABLE  = 1 << 2,  /* sps.pcm_loop_filter_disable_flag (deblock.cc:578)       */
  M355_PF_LF_ACROSS_TILES          = 1 << 3,  /* pps.loop_filter_across_tiles_enabled_flag               */
  M355_PF_SAO_ENABLED              = 1 << 4,  /* sps.sample_adaptive_offset_enabled_flag && !DISABLE_SAO */
  M355_PF_INTRA_SMOOTHING_DISABLED = 1 << 5,  /* sps.range_extension.intra_smoothing_disabled_flag       */
  M355_PF_IMPLICIT_RDPCM           = 1 << 6,  /* sps.range_extension.implicit_rdpcm_enabled_flag         */
  M355_PF_SCALING_LIST             = 1 << 7,  /* sps.scaling_list_enable_flag (transform.cc:461)         */
  M355_PF_DEBLOCK_ENABLED          = 1 << 8,  /* !DE265_DECODER_PARAM_DISABLE_DEBLOCKING (de265.h:409)   */
  M355_PF_CROSS_COMPONENT_PRED     = 1 << 9,  /* pps.range_extension.cross_component_prediction_enabled_flag
                                                 (4:4:4 only, transform.cc:244-260): chroma blocks may carry a
                                                 ResScaleVal in m355_rb.matrix_id (see there)            */
  M355_PF_TRANSFORM_SKIP_ROTATION  = 1 << 10, /* sps.range_extension.transform_skip_rotation_enabled_flag (transform.cc:400-402);
                                                 informative: the kernels follow the per-block M355_RBF_ROTATE */
  M355_PF_CLEAR_DST                = 1 << 11  /* zero the picture before reconstructing it, as the reference's allocator does for
                                                 every new picture (image.cc:164): only matters when the lists do not cover the
                                                 whole picture (damaged streams: missing slices, PBs without a usable list) */
};

typedef struct m355_pic_params {
  int32_t  width, height;          /* pic_width/height_in_luma_samples                      */
  uint8_t  chroma_format_idc;      /* 0 mono, 1 4:2:0, 2 4:2:2, 3 4:4:4                     */
  uint8_t  bit_depth_luma, bit_depth_chroma;
  uint8_t  log2_ctb_size;          /* Log2CtbSizeY                                          */
  uint8_t  log2_min_tb_size;       /* Log2MinTrafoSize (z-scan granularity, pps.cc:608-623) */
  uint8_t  log2_min_cb_size;       /* Log2MinCbSizeY                                        */
  int8_t   pic_cb_qp_offset, pic_cr_qp_offset;   /* deblock.cc:666-668                      */
  uint32_t flags;                  /* M355_PF_*                                             */
  uint8_t  num_tile_cols, num_tile_rows;         /* 1,1 when tiles are off                  */
  uint16_t col_bd[M355_MAX_TILE_COLS + 1];       /* pps.colBd, in CTBs                      */
  uint16_t row_bd[M355_MAX_TILE_ROWS + 1];       /* pps.rowBd                               */
  uint16_t reserved;
} m355_pic_params;                 /* 112 bytes */

/* slice (segment) header fields the pixel path reads */
enum {
  M355_SF_DEBLOCK_DISABLED = 1 << 0,  /* slice_deblocking_filter_disabled_flag (deblock.cc:216)        */
  M355_SF_LF_ACROSS_SLICES = 1 << 1,  /* slice_loop_filter_across_slices_enabled_flag                  */
  M355_SF_SAO_LUMA         = 1 << 2,  /* slice_sao_luma_flag (sao.cc:367)                              */
  M355_SF_SAO_CHROMA       = 1 << 3   /* slice_sao_chroma_flag                                         */
};
typedef struct m355_slice {
  int32_t slice_addr_rs;           /* SliceAddrRS */
  int8_t  beta_offset, tc_offset;  /* slice_beta_offset, slice_tc_offset (deblock.cc:521-523) */
  uint8_t flags;                   /* M355_SF_* */
  uint8_t reserved;
} m355_slice;                      /* 8 bytes */

enum { M355_CTBF_HAS_PCM_OR_BYPASS = 1 << 0 };  /* image.h get_CTB_has_pcm_or_cu_transquant_bypass */
typedef struct m355_ctb {
  uint16_t slice_idx;              /* index into slices[] (ctb_info.SliceHeaderIndex)              */
  uint8_t  sao_type;               /* sao_info.SaoTypeIdx  — 2 bits per cIdx (slice.h:271)         */
  uint8_t  sao_eo_class;           /* sao_info.SaoEoClass  — 2 bits per cIdx                       */
  uint8_t  sao_band_pos[3];        /* sao_info.sao_band_position                                   */
  uint8_t  flags;                  /* M355_CTBF_*                                                  */
  int8_t   sao_offset[3][4];       /* sao_info.saoOffsetVal                                        */
  uint32_t ib_start, ib_count;     /* this CTB's range in ibs[] (decode order)                     */
} m355_ctb;                        /* 28 bytes */

/* coding unit: rasterised on the device into the per-min-CB plane (image.h:173-195 CB_ref_info) */
enum { M355_CUF_PCM = 1 << 0, M355_CUF_TRANSQUANT_BYPASS = 1 << 1 };
typedef struct m355_cu {
  uint16_t x, y;                   /* luma position */
  uint8_t  log2_size;
  uint8_t  pred_mode;              /* 0 MODE_INTRA, 1 MODE_INTER, 2 MODE_SKIP (slice.h:87-90) */
  uint8_t  part_mode;              /* PartMode (slice.h:72-82) */
  int8_t   qp_y;                   /* QP_Y (transform.cc:199) */
  uint8_t  flags;                  /* M355_CUF_* */
  uint8_t  reserved[3];
} m355_cu;                         /* 12 bytes */

/* transform-tree leaf (luma geometry): transform edges + cbf_luma for deblocking
 * (deblock.cc:33-63 markTransformBlockBoundary, slice.cc:2958-2960 set_nonzero_coefficient) */
enum { M355_TUF_NONZERO_COEFF = 1 << 0 };
typedef struct m355_tu {
  uint16_t x, y;
  uint8_t  log2_size;
  uint8_t  flags;
  uint16_t reserved;
} m355_tu;                         /* 8 bytes */

/* explicit weighted-prediction entry: one (list, refIdx) of one slice (motion.cc:520-529) */
typedef struct m355_wt {
  int16_t w[3];                    /* LumaWeight / ChromaWeight[..][0] / [..][1]                      */
  int16_t o[3];                    /* offsets already << WpOffsetBdShift (motion.cc:524)              */
  uint8_t log2wd_luma;             /* luma_log2_weight_denom + shift1_L (motion.cc:520)               */
  uint8_t log2wd_chroma;
  uint16_t reserved;
} m355_wt;                         /* 16 bytes */

/* prediction block (motion.cc:288 generate_inter_prediction_samples, one call) */
enum {
  M355_PBF_PRED_L0   = 1 << 0,     /* PBMotion.predFlag[0] as stored (used by deblock bS)         */
  M355_PBF_PRED_L1   = 1 << 1,
  M355_PBF_MC_L0     = 1 << 2,     /* list actually interpolated (after motion.cc:348-357 demotion) */
  M355_PBF_MC_L1     = 1 << 3,
  M355_PBF_WEIGHTED  = 1 << 4,     /* explicit weights (motion.cc:508,571,633) */
  M355_PBF_FILL_L0   = 1 << 5,     /* reference missing → predSamples = 1<<13 (motion.cc:362-376) */
  M355_PBF_FILL_L1   = 1 << 6
};
typedef struct m355_pb {
  uint16_t x, y;                   /* luma position xP,yP */
  uint8_t  w, h;                   /* nPbW, nPbH (luma) */
  uint8_t  flags;                  /* M355_PBF_* */
  uint8_t  reserved;
  int8_t   ref_slot[2];            /* index into m355_picture.ref_frames (DPB identity), -1 none */
  int16_t  mv[2][2];               /* [list][x,y] quarter-pel */
  uint16_t wt_idx[2];              /* index into wts[] per list (valid when WEIGHTED) */
  uint16_t reserved2;
} m355_pb;                         /* 24 bytes */

/* residual block: one scale_coefficients() call (transform.cc:645 / :361-642) */
enum {
  M355_RK_DCT = 0, M355_RK_DST = 1, M355_RK_SKIP = 2, M355_RK_BYPASS = 3
};
enum {
  M355_RBF_DEFERRED  = 1 << 0,     /* intra block: store residual to the residual buffer (res_ofs)
                                      instead of adding it to the picture                         */
  M355_RBF_RDPCM_H   = 1 << 1,     /* rdpcmMode 1 */
  M355_RBF_RDPCM_V   = 1 << 2,     /* rdpcmMode 2 */
  M355_RBF_ROTATE    = 1 << 3,     /* transform_skip_rotation (transform.cc:400-402) */
  M355_RBF_DEQUANTIZED = 1 << 4,   /* coeffs[] levels are already scaled (what the table slots
                                      transform_add / transform_skip_residual receive): skip dequant */
  M355_RBF_NARROW    = 1 << 5      /* the block's entries are 16-bit: pos:u8 | level:i8 << 8, two per word of coeffs[], low half
                                      first — (ncoeff + 1) / 2 words from coeff_ofs (m355_picture below, m355_pack_narrow) */
};
typedef struct m355_rb {
  uint16_t x, y;                   /* position in component samples */
  uint8_t  cidx;
  uint8_t  log2_size;              /* 2..5 */
  uint8_t  kind;                   /* M355_RK_* */
  uint8_t  flags;                  /* M355_RBF_* */
  uint8_t  qp;                     /* qPYPrime / qPCbPrime / qPCrPrime (transform.cc:371-377) */
  uint8_t  matrix_id;              /* bits 0-2: scaling-list matrixID (transform.cc:493-502), unused if no list.
                                      Cross-component prediction (M355_PF_CROSS_COMPONENT_PRED, chroma blocks): bits 4-6 =
                                      log2_res_scale_abs_plus1 (0 = none), bit 7 = sign -> ResScaleVal = +-(1 << (v-1))
                                      (slice.cc:3721-3760); bit 3 = the TU's luma block is rbs[i-2] (else rbs[i-1]): the
                                      three blocks of a 4:4:4 transform unit have one size, so they sit next to each other
                                      in their size bin.  A chroma block with cbf 0 but ResScaleVal != 0 is listed with
                                      ncoeff 0 (slice.cc:3512-3523). */
  uint16_t ncoeff;                 /* entries; they occupy ncoeff words of coeffs[], (ncoeff + 1) / 2 with M355_RBF_NARROW */
  uint32_t coeff_ofs;              /* first word of the block in coeffs[] (a word offset, whatever the entry width) */
  uint32_t res_ofs;                /* int16 offset in the residual buffer (DEFERRED) */
} m355_rb;                         /* 20 bytes */

/* intra block: one decode_intra_prediction() call (intrapred.cc:321), in decode order */
enum {
  M355_IBF_HAS_RESIDUAL            = 1 << 0,
  M355_IBF_DISABLE_BOUNDARY_FILTER = 1 << 1,  /* intrapred.cc:306-308 */
  M355_IBF_PCM                     = 1 << 2   /* raw block (slice.cc:4211-4255): res_ofs indexes pcm[] */
};
typedef struct m355_ib {
  uint16_t x, y;                   /* position in component samples */
  uint8_t  cidx;
  uint8_t  log2_size;              /* 2..5 (PCM: up to 5) */
  uint8_t  mode;                   /* IntraPredMode 0..34 */
  uint8_t  flags;                  /* M355_IBF_* */
  uint32_t res_ofs;                /* residual buffer offset (int16 units) / pcm[] offset */
} m355_ib;                         /* 12 bytes */

/* One picture's complete work description. All pointers are HOST pointers owned by the caller;
 * m355_submit_picture() copies what it needs before returning. Lists:
 *   coeffs[i] = (uint16 pos) | (int16 level << 16)  with pos = xC + yC*nT (slice.cc:3441-3447)
 *     A block with M355_RBF_NARROW packs two entries per word instead: entry k is the 16-bit half (k & 1) of word
 *     coeff_ofs + k / 2, low half first, each (uint8 pos) | (int8 level << 8), the level sign-extended.  The spare half of a
 *     block with an odd count is never read.  Only blocks whose positions are all < 256 and whose levels all fit 8 bits can
 *     take the form; narrow and wide blocks mix freely in one picture and one size bin.  n_coeffs and coeff_ofs count words:
 *     a block must satisfy coeff_ofs + words <= n_coeffs, words = ncoeff or (ncoeff + 1) / 2.
 *   rbs[] is grouped by log2_size: rb_count[s] entries of size (s+2), concatenated 4x4,8x8,16,32.
 *   scaling_factors: [sizeId 0..3][matrixID 0..5][y][x] uint8 (sps.h:61-64), 6*(16+64+256+1024) B. */
typedef struct m355_picture {
  m355_pic_params pp;
  int32_t dst_frame;                         /* frame handle receiving the decoded picture  */
  int32_t ref_frames[M355_MAX_REF_FRAMES];   /* frame handles, indexed by m355_pb.ref_slot  */
  int32_t n_slices, n_ctbs, n_cus, n_tus, n_pbs, n_wts, n_ibs;
  int32_t rb_count[4];
  uint32_t n_coeffs, n_pcm, res_len;
  const m355_slice* slices;
  const m355_ctb*   ctbs;                    /* raster order, PicSizeInCtbsY entries */
  const m355_cu*    cus;
  const m355_tu*    tus;
  const m355_pb*    pbs;
  const m355_wt*    wts;
  const m355_rb*    rbs;
  const m355_ib*    ibs;
  const uint32_t*   coeffs;
  const uint16_t*   pcm;
  const uint8_t*    scaling_factors;         /* NULL unless M355_PF_SCALING_LIST */
} m355_picture;

/* ------------------------------------------------------------------------------------------------
 * Context, frames (device-resident DPB), submission.
 * ---------------------------------------------------------------------------------------------- */
typedef struct m355_ctx m355_ctx;

M355_API int  m355_create(int device, m355_ctx** out);
M355_API void m355_destroy(m355_ctx* ctx);

/* Frames: planes of uint8 (bit depth 8) or uint16 (9..16), exactly the reference's plane element
 * types (image.h:295-301). Returns handle >= 0 or a negative M355_ERR_*. */
M355_API int m355_frame_create(m355_ctx* ctx, int width, int height, int chroma_format_idc,
                               int bit_depth_luma, int bit_depth_chroma);
M355_API int m355_frame_destroy(m355_ctx* ctx, int frame);
/* stride in SAMPLES, as everywhere in the reference (acceleration.h: "Strides are in samples").  Both calls block until the plane has arrived; src / dst may be
 * any host memory: the library stages the plane in a pinned buffer of the context and queues the copy on one of its own streams (the frame's last writer's for a
 * download) — a blocking hipMemcpy2D on pageable memory was measured to deliver stale rows when many processes share the GPU. */
M355_API int m355_frame_upload(m355_ctx* ctx, int frame, int cidx, const void* src, ptrdiff_t stride);
M355_API int m355_frame_download(m355_ctx* ctx, int frame, int cidx, void* dst, ptrdiff_t stride);
/* The same for all planes of the frame, asynchronous (picture output, de265_get_next_picture / de265_get_image_plane: image.h's planes
 * are the destination): the copies are queued right behind the decode that writes the frame, on that lane's stream — beside the
 * host and the other lanes' decodes; a later picture decoded into the frame waits for them.  dst[c] / stride[c] (in samples) per plane
 * (unused planes of a monochrome frame are ignored); use m355_host_alloc'ed planes.  m355_frame_download_wait blocks until THIS
 * frame's copy has landed (m355_wait also waits for every copy). */
M355_API int m355_frame_download_async(m355_ctx* ctx, int frame, void* const dst[3], const ptrdiff_t stride[3]);
M355_API int m355_frame_download_wait(m355_ctx* ctx, int frame);
M355_API int m355_frame_fill(m355_ctx* ctx, int frame, int value_luma, int value_chroma);

/* Export into DEVICE memory, for a consumer on the same GPU (an encoder, a renderer, an inference pipeline): the frame's conformance
 * window — any rectangle — instead of the coded-size planes with their 128-byte pitch, planar or semi-planar (NV12 / NV16 / NV24 shapes,
 * P010 / P016 with M355_EXPORT_MSB16), optionally rounded to 8 bits.  One kernel for all planes, integer-exact: no colour conversion, no
 * scaling.  What lands is a closed-form function of the samples m355_frame_download returns:
 *   rectangle   luma samples [x0, x0 + width) x [y0, y0 + height), chroma the same divided by SubWidthC / SubHeightC
 *   NATIVE      s            MSB16  (uint16)(s << (16 - bit_depth))            U8  bit_depth 8: s, else min(255, (s + (1 << (bit_depth - 9))) >> (bit_depth - 8))
 * with the bit depth of the plane (bit_depth_luma / bit_depth_chroma).  A monochrome frame exports luma only (dst[1], dst[2] and their
 * pitches are ignored in both layouts).  Destination bytes of a row beyond the exported row are never written.
 * M355_ERR_INVALID (nothing is enqueued, no destination byte written): a rectangle that leaves the frame or is not aligned to the chroma
 * grid, a null destination for a plane that exists, a pitch below the row's bytes, unknown layout / samples values.
 * Asynchronous, and a READER of the frame: the kernel is queued behind the decode that writes the frame (on that lane's stream, beside the
 * host and the other lanes' decodes), and a later picture decoded into the frame waits for it in front of its first write.  An export
 * behind a decode whose lists were rejected writes nothing, like that decode (m355_decode_status).  The destination stays the caller's:
 * the library never frees it and does not track the consumer's reads.
 *   m355_frame_export_wait    the host blocks until this frame's last export has landed (m355_wait also waits for every export)
 *   m355_frame_export_order   the consumer's stream waits for it instead; the host does not.  m355_stream() cannot stand for this:
 *                             consecutive pictures go round several lanes, each with streams of its own */
#define M355_EXPORT_PLANAR      0   /* dst[0..2] = Y, Cb, Cr */
#define M355_EXPORT_SEMIPLANAR  1   /* dst[0] = Y, dst[1] = Cb,Cr interleaved (NV12/NV16/NV24 shapes by chroma format) */
#define M355_EXPORT_NATIVE      0   /* element type and values of the frame (u8, or u16 LSB-aligned) */
#define M355_EXPORT_MSB16       1   /* u16, value << (16 - bit_depth)  (P010/P016 convention; 8-bit sources too) */
#define M355_EXPORT_U8          2   /* u8: bit_depth 8 -> s; else min(255, (s + (1 << (bd-9))) >> (bd-8)) */
typedef struct m355_export_desc {
  int32_t layout, samples;
  int32_t x0, y0, width, height;    /* luma rectangle; width == 0: the whole frame. Multiples of SubWidthC / SubHeightC */
  void*   dst[3];                   /* device memory, or m355_host_alloc memory (device-addressable) */
  int64_t pitch[3];                 /* BYTES per destination row, >= the row's bytes */
} m355_export_desc;
M355_API int   m355_frame_export(m355_ctx* ctx, int frame, const m355_export_desc* desc);       /* asynchronous */
/* The same export, downscaled on the device by f = 1 << log2_scale in both directions, every plane on its own grid: an exact integer box average.
 * log2_scale 0 is m355_frame_export itself; 1, 2 and 3 take a kernel of their own (k_export_scaled.hip); anything else is M355_ERR_INVALID.
 * desc keeps its meaning.  In addition to the rules above, the rectangle's width must be a multiple of f * SubWidthC and its height a multiple
 * of f * SubHeightC (monochrome: f and f); a whole-frame request (width == 0) on a frame whose size is no such multiple is M355_ERR_INVALID like
 * any other misfit: nothing is cropped implicitly.  Plane p of the rectangle, pw x ph samples, becomes pw / f x ph / f samples; a semi-planar
 * chroma row interleaves the scaled Cb and Cr samples; a pitch is checked against the SCALED row's bytes, and bytes beyond a scaled row are never
 * written.  With k = log2_scale, n = f * f, bd the plane's bit depth and S(x, y) the sum of the f x f source block of output sample (x, y):
 *   NATIVE      a = (S + n / 2) >> 2k, in the frame's element type
 *   MSB16       (uint16)(a << (16 - bd))
 *   U8          min(255, (S + (1 << (2k + bd - 9))) >> (2k + bd - 8))     — ONE rounding from the sum, not a rounding of a; for bd = 8 it equals a
 * Siting: an output sample sits at the centre of its block, on each plane's own grid — for 4:2:0 content with left-sited chroma the scaled chroma
 * therefore lies (f - 1) / (2f) output luma samples off its nominal position; there is no siting correction and no other filter.
 * Errors, ordering and the gate are those of m355_frame_export: a rejected call enqueues nothing and writes nothing; the call is asynchronous and a
 * reader of the frame of the same kind, so m355_frame_export_wait and m355_frame_export_order cover it. */
M355_API int   m355_frame_export_scaled(m355_ctx* ctx, int frame, const m355_export_desc* desc, int log2_scale);   /* asynchronous */
/* The frame, or a rectangle of it, as R'G'B' (k_export_rgb.hip): for a model or a compositor on the same GPU.  Integer arithmetic only, so that
 * what lands is a closed-form function of the samples m355_frame_download returns, the same on every build.  m355_rgb_coefficients is the one
 * place the constants are made (the runtime calls it for the launch); with 64-bit integers, rdiv(a, b) = (2a + b) / (2b), D = 8 or 16 (samples),
 * M = 2^D - 1, F = 29 - D, Kr / Kb of the matrix in 1/10000, Kg = 10000 - Kr - Kb, bdY / bdC the bit depths:
 *   limited range  y0 = 16 << (bdY - 8)   ys = 219 << (bdY - 8)   cs = 224 << (bdC - 8)
 *   full range     y0 = 0                 ys = 2^bdY - 1          cs = 2^bdC - 1                  c0 = 1 << (bdC - 1) in both
 *   cy  = rdiv(M << F, ys)
 *   crv = rdiv(2 (10000 - Kr) (M << F), 10000 cs)             cbu = rdiv(2 (10000 - Kb) (M << F), 10000 cs)
 *   cgu = rdiv(2 Kb (10000 - Kb) (M << F), 10000 Kg cs)       cgv = rdiv(2 Kr (10000 - Kr) (M << F), 10000 Kg cs)
 * Per pixel, y = Y - y0, u = Cb' - c0, v = Cr' - c0, H = 1 << (F - 1), sums in signed 32 bits, >> an arithmetic shift:
 *   R = clip(0, M, (cy y + crv v + H) >> F)    G = clip(0, M, (cy y - cgu u - cgv v + H) >> F)    B = clip(0, M, (cy y + cbu u + H) >> F)
 * (within 0.5 + 0.5 (|y| + |u| + |v|) / 2^F output LSB of the real-valued conversion: below 1 LSB for 8..12-bit sources, up to 3.2 at 16 -> U16).
 * A monochrome frame has u = v = 0.  M355_RGB_U16 is full scale 0..65535, not the frame's bit depth MSB-aligned.
 * Cb', Cr' are the chroma samples AT THE LUMA POSITION.  There is ONE reconstruction filter, the bilinear one for chroma sample location type 0
 * (horizontally co-sited, vertically midway); types 1..3 are chosen through m355_export_opts (the _opts entry points below).  It works on the FRAME's chroma plane C of CW x CH samples with indices
 * clamped to that plane — samples outside the rectangle but inside the frame are read as they are, so an exported rectangle equals the same
 * rectangle cut from a whole-frame export — and its result is a sample of the chroma bit depth, rounded BEFORE the matrix.  For luma (X, Y):
 *   4:4:4  C[Y][X]
 *   4:2:2  i = X >> 1;  X even: C[Y][i];  X odd: (C[Y][i] + C[Y][min(i + 1, CW - 1)] + 1) >> 1
 *   4:2:0  j = Y >> 1, jn = max(j - 1, 0) for even Y, min(j + 1, CH - 1) for odd Y, T[i] = 3 C[j][i] + C[jn][i];
 *          X even: (T[i] + 2) >> 2;  X odd: (T[i] + T[min(i + 1, CW - 1)] + 4) >> 3
 * M355_ERR_INVALID (nothing is enqueued, no destination byte written): whatever m355_frame_export rejects for the frame handle and the rectangle;
 * an unknown layout, samples or matrix value, full_range not 0 or 1; a null dst for a plane the layout uses; a pitch below the row's bytes (width * 3 *
 * element bytes packed, width * element bytes planar); for U16 a pointer or a pitch that is no multiple of 2.  m355_rgb_coefficients rejects the same
 * matrix / full_range / samples values, bit depths outside 8..16 and a null `out`.
 * Ordering, the gate and sharded contexts are those of m355_frame_export: asynchronous, a reader of the frame of the same kind — m355_frame_export_wait
 * and m355_frame_export_order cover it, the next decode into the frame waits for it —, nothing is written behind a rejected decode, and destination
 * bytes beyond a row are never written. */
#define M355_RGB_PACKED  0   /* dst[0]: R,G,B,R,G,B,... three elements per pixel */
#define M355_RGB_PLANAR  1   /* dst[0..2] = R, G, B planes (CHW) */
#define M355_RGB_U8      0   /* D = 8 */
#define M355_RGB_U16     1   /* D = 16, full scale 0..65535 (not MSB-aligned bit-depth samples) */
#define M355_MATRIX_BT601 0  /* Kr, Kb = 2990, 1140 (in 1/10000) */
#define M355_MATRIX_BT709 1  /*          2126,  722 */
#define M355_MATRIX_BT2020 2 /*          2627,  593  (non-constant luminance) */
typedef struct m355_rgb_desc {
  int32_t layout, samples, matrix, full_range;
  int32_t x0, y0, width, height;    /* as m355_export_desc: luma rectangle, width == 0 = whole frame, multiples of SubWidthC / SubHeightC */
  void*   dst[3];                   /* device memory, or m355_host_alloc memory; PACKED uses [0] only */
  int64_t pitch[3];                 /* BYTES per destination row, >= the row's bytes */
} m355_rgb_desc;
M355_API int   m355_frame_export_rgb(m355_ctx* ctx, int frame, const m355_rgb_desc* desc);      /* asynchronous */
typedef struct m355_rgb_coeffs { int32_t F, y0, c0, cy, crv, cgu, cgv, cbu; } m355_rgb_coeffs;
M355_API int   m355_rgb_coefficients(int matrix, int full_range, int bit_depth_luma, int bit_depth_chroma, int samples, m355_rgb_coeffs* out);
/* The frame's rectangle RESIZED to out_width x out_height luma samples (k_export_resized.hip): every plane is resampled on its own grid — chroma to
 * out_width / SubWidthC x out_height / SubHeightC — and goes to the caller's memory in the layouts and sample formats of m355_frame_export.  The
 * filter of this call (M355_FILTER_TRIANGLE; the cubic one follows below): a separable triangle, widened by the downscale ratio — an antialiased
 * bilinear filter when downscaling, plain bilinear when upscaling.
 * Integer arithmetic only: what lands is a closed-form function of the samples m355_frame_download returns, the same on every build.
 * One axis of one plane maps sn source samples (the rectangle's, on that plane's grid) to dn output samples.  With 64-bit integers and
 * rdiv(a, b) = (2a + b) / (2b), for output index i:
 *   M = 2 max(sn, dn);   C = (2i + 1) sn - dn on a centre-aligned grid, C = 2 i sn on a co-sited grid
 *   for every integer k with |2 dn k - C| < M (at most 16 inside the ratio limit):  n_k = M - |2 dn k - C|
 *   N = sum n_k,  P_k = the prefix sum of n over increasing k (0 before the first),  q_k = rdiv(P_k << 14, N) - rdiv(P_(k-1) << 14, N)
 * so that every q_k >= 0 and the q_k sum to exactly 1 << 14.  k is then clamped to [0, sn - 1] — the RECTANGLE, not the frame: a rectangle's resize
 * equals the resize of a frame that holds only that rectangle — and coefficients that land on the same index are added.  m355_resize_taps returns this
 * folded row, which is contiguous (libde265_amd/csrc/resize_taps.h: the one definition, which the kernel calls too).
 * Grids: luma and every vertical axis are centre-aligned; the horizontal chroma axis of 4:2:0 and 4:2:2 is co-sited (chroma sample location type 0,
 * the siting m355_frame_export_rgb assumes), so resized chroma stays where type 0 puts it.  Types 1..3: m355_export_opts below.
 * Per plane, bd its bit depth, S the rectangle's samples, qy_j / qx_i the rows of the vertical / horizontal axis: the VERTICAL pass first, ONE
 * rounding to an 18-bit intermediate, then the horizontal pass, everything unsigned:
 *   u(x, j) = sum_k qy_j[k] S[k][x]                      < 2^(bd + 14)
 *   t(x, j) = (u + (1 << (bd - 5))) >> (bd - 4)          < 2^18
 *   v(i, j) = sum_k qx_i[k] t(k, j)                      < 2^32
 *   NATIVE  a = (v + (1 << (31 - bd))) >> (32 - bd)      (the sum still fits 32 bits)
 *   MSB16   (uint16)(a << (16 - bd))
 *   U8      min(255, (v + (1 << 23)) >> 24)              — ONE rounding from v, not a rounding of a; the sum needs 33 bits,
 *                                                          ((v >> 1) + (1 << 22)) >> 23 is the same value in 32
 * A constant plane stays constant; out_width == width && out_height == height delivers what m355_frame_export delivers, byte for byte.
 * M355_ERR_INVALID (nothing is enqueued, no destination byte written): whatever m355_frame_export rejects for the frame handle, the rectangle, the
 * layout and the samples; out_width not positive or no multiple of SubWidthC, out_height not positive or no multiple of SubHeightC (monochrome: 1
 * and 1); a ratio outside src <= 8 * out && out <= 8 * src on either axis (at most 8x down or 8x up: it bounds a row at 16 coefficients); a null dst
 * for a plane that exists; a pitch below the OUTPUT row's bytes.  A monochrome frame exports luma only; bytes beyond an output row are never written.
 * Ordering, the gate and sharded contexts are those of m355_frame_export: asynchronous, a reader of the frame of the same kind — m355_frame_export_wait
 * and m355_frame_export_order cover it, the next decode into the frame waits for it —, and nothing is written behind a rejected decode.
 * A SECOND FILTER, M355_FILTER_CUBIC (the _filtered entry points below; M355_FILTER_TRIANGLE = 0 is the filter above, and with it every _filtered
 * entry point IS the plain one): Catmull-Rom — Keys' cubic with a = -1/2, the kernel of an antialiased "bicubic" resize —, widened by the downscale
 * ratio like the triangle, defined in integers in the same notation.  With D = 2 dn, M and C as above, for every integer k with d = |D k - C| < 2 M:
 *   n_k = 3 d^3 - 5 M d^2 + 2 M^3                    for d <= M
 *   n_k = -d^3 + 5 M d^2 - 8 M^2 d + 4 M^3           for M < d < 2 M           (2 M^3 w(d / M) with the Catmull-Rom w; negative in this lobe)
 * N = sum n_k > 0, and P_k, q_k and rdiv — floor((2a + b) / (2b)) on SIGNED values — as above: the q_k sum to exactly 1 << 14 but may be negative; the
 * clamp of k to the rectangle and the folding are the triangle's.  N has up to 48 bits; m355_resize_taps_filtered returns the exact row all the same.
 * Limits: 16 coefficients per row need sn <= 4 dn, so the cubic filter takes at most 4x DOWN and, as the triangle, at most 8x up on either axis, and
 * sn and dn at most M355_RESIZE_CUBIC_MAX_N = 16384 on every axis resized with it; outside: M355_ERR_INVALID, nothing enqueued.
 * Passes, per plane, everything in SIGNED 32 bits, >> arithmetic; the intermediate keeps 16 bits of fraction so that the horizontal sum with its
 * overshoot fits (a row's sum of |q_k| is at most 20 788, reached at 13 -> 12 co-sited; 4 * 23000^2 + 2^21 < 2^31):
 *   u = sum_k qy[k] S[k][x]                            |u| < 2^31
 *   t = (u + (1 << (bd - 3))) >> (bd - 2)              not clipped: about -0.27 * 2^16 .. 1.27 * 2^16
 *   v = sum_k qx[k] t[k]                               |v| + 2^21 < 2^31
 *   NATIVE  a = clip(0, 2^bd - 1, (v + (1 << (29 - bd))) >> (30 - bd))
 *   MSB16   (uint16)(a << (16 - bd))
 *   U8      clip(0, 255, (v + (1 << 21)) >> 22)        — ONE rounding from v, not a rounding of a
 * A constant plane stays constant; out == rectangle gives the rows {0, 1 << 14, 0} and delivers what m355_frame_export delivers, byte for byte; a
 * rectangle's resize equals the resize of a frame that holds only the rectangle.  The three composed exports below keep their definitions word for
 * word, "the resized export" meaning the resized export with this filter: chroma is resized on its own grid with the SAME filter, rounded and clipped
 * to a sample (a above), reconstructed by the bilinear filter of m355_frame_export_rgb, then the matrix, then m355_tensor_element.
 * An unknown filter is M355_ERR_INVALID (m355_resize_taps_filtered: < 0); m355_frames_export_tensor_rois_filtered checks the filter's ratio and size
 * limit per entry.
 * Not offered: Lanczos, a selectable a, the cubic filter beyond 4x down (32 coefficients per row), sizes above 16384 per axis with it, a filter per
 * slice, ratios beyond 8, the bottom-sited chroma sample location types 4 and 5, a siting per slice, siting for 4:2:2, resizing into a
 * frame of the decoder; and of m355_frame_export_resized_rgb and m355_frames_export_tensor below: BGR order, chroma resampled
 * straight onto the luma grid (it is resized on its own grid, then reconstructed), per-frame output sizes within a batch (per-frame rectangles:
 * m355_frames_export_tensor_rois, which rejects a region smaller than an eighth of the output and does not clamp it), writing into a tensor owned by
 * a second HIP runtime without m355_frame_export_order. */
#define M355_RESIZE_MAX_TAPS 16
#define M355_FILTER_TRIANGLE 0          /* the separable triangle: antialiased bilinear */
#define M355_FILTER_CUBIC    1          /* Catmull-Rom: antialiased bicubic, at most 4x down */
#define M355_RESIZE_CUBIC_MAX_N 16384   /* samples of an axis, source or output, under M355_FILTER_CUBIC */
typedef struct m355_resize_desc {
  int32_t layout, samples;          /* M355_EXPORT_PLANAR / _SEMIPLANAR, M355_EXPORT_NATIVE / _MSB16 / _U8 */
  int32_t x0, y0, width, height;    /* source luma rectangle, exactly as in m355_export_desc (width == 0: whole frame) */
  int32_t out_width, out_height;    /* luma size of the result */
  void*   dst[3];
  int64_t pitch[3];                 /* bytes per destination row, >= the OUTPUT row's bytes */
} m355_resize_desc;
M355_API int   m355_frame_export_resized(m355_ctx* ctx, int frame, const m355_resize_desc* desc);   /* asynchronous */
M355_API int   m355_frame_export_resized_filtered(m355_ctx* ctx, int frame, const m355_resize_desc* desc, int filter);   /* M355_FILTER_*; asynchronous */
/* row i of one axis' filter: returns the number of coefficients (1..16), *first = source index of coeff[0]; < 0 on bad arguments (a size below 1,
 * a ratio outside the limit, i outside [0, dst_n), cosited not 0 or 1, a null pointer) */
M355_API int   m355_resize_taps(int src_n, int dst_n, int cosited, int i, int32_t* first, int32_t coeff[M355_RESIZE_MAX_TAPS]);
/* the same for M355_FILTER_*: also < 0 for an unknown filter and, under M355_FILTER_CUBIC, beyond 4x down or a size above M355_RESIZE_CUBIC_MAX_N */
M355_API int   m355_resize_taps_filtered(int filter, int src_n, int dst_n, int cosited, int i, int32_t* first, int32_t coeff[M355_RESIZE_MAX_TAPS]);
/* The frame's rectangle RESIZED to out_width x out_height luma samples AND converted to R'G'B', in one launch (k_export_resized_rgb.hip): what a model
 * (its input size) or a compositor (its window's size) on the same GPU takes.  The definition is a COMPOSITION and adds no arithmetic, constant or
 * siting rule of its own:
 *   let R be the planes m355_frame_export_resized delivers for this rectangle and this output size with M355_EXPORT_PLANAR, M355_EXPORT_NATIVE, and F'
 *   a frame of out_width x out_height with the source frame's chroma format and bit depths whose samples are R;
 *   the call delivers, byte for byte, what m355_frame_export_rgb delivers for the whole of F' with the same layout, samples, matrix and full_range.
 * Spelled out: every plane is resampled on its own grid by the one triangle filter above; each output sample is rounded to a sample of the plane's
 * bit depth, a = (v + (1 << (31 - bd))) >> (32 - bd); chroma is then brought to the luma positions by the one bilinear filter of m355_frame_export_rgb,
 * its indices clamped to the RESIZED chroma plane (out_width / SubWidthC x out_height / SubHeightC); then the eight integers of m355_rgb_coefficients are
 * applied as defined there.  No resized Y, Cb or Cr sample passes through memory.  Consequences:
 *   out == rectangle == whole frame: the call equals m355_frame_export_rgb of the whole frame;
 *   a sub-rectangle: it equals the R'G'B' export of a frame that holds only that rectangle — the resize clamps AND the chroma filter's clamps go to the
 *   rectangle, whereas m355_frame_export_rgb of a rectangle reads the frame's samples outside it, so the two differ at the rectangle's rim;
 *   a monochrome frame has u = v = 0; a constant frame gives a constant picture.
 * M355_ERR_INVALID (nothing is enqueued, no destination byte written): whatever m355_frame_export_resized rejects for the frame handle, the rectangle,
 * the output size and the ratio; whatever m355_frame_export_rgb rejects for layout, samples, matrix and full_range; a null dst for a plane the layout
 * uses; a pitch below the OUTPUT row's bytes (out_width * 3 * element bytes packed, out_width * element bytes planar); for U16 a pointer or a pitch
 * that is no multiple of 2; a null descriptor.
 * Ordering, the gate and sharded contexts are those of m355_frame_export: asynchronous, a reader of the frame of the same kind — m355_frame_export_wait
 * and m355_frame_export_order cover it, the next decode into the frame waits for it —, nothing is written behind a rejected decode, and destination
 * bytes beyond an output row are never written. */
typedef struct m355_resize_rgb_desc {
  int32_t layout, samples, matrix, full_range;   /* M355_RGB_PACKED / _PLANAR, M355_RGB_U8 / _U16, M355_MATRIX_*, 0 / 1: as m355_rgb_desc */
  int32_t x0, y0, width, height;    /* source luma rectangle, as m355_export_desc (width == 0: whole frame) */
  int32_t out_width, out_height;    /* luma size of the result */
  void*   dst[3];                   /* PACKED uses [0] only */
  int64_t pitch[3];                 /* bytes per destination row, >= the OUTPUT row's bytes */
} m355_resize_rgb_desc;             /* (LP64: 88 bytes) */
M355_API int   m355_frame_export_resized_rgb(m355_ctx* ctx, int frame, const m355_resize_rgb_desc* desc);   /* asynchronous */
M355_API int   m355_frame_export_resized_rgb_filtered(m355_ctx* ctx, int frame, const m355_resize_rgb_desc* desc, int filter);   /* M355_FILTER_* */
/* A BATCH of frames, each resized and converted to R'G'B' as above, NORMALISED and delivered as ONE float tensor in one launch (k_export_resized_rgb.hip):
 * the input of a model on the same GPU.  The definition is again a composition:
 *   channel c (0 = R, 1 = G, 2 = B) of pixel (x, y) of slice i starts as the integer v that m355_frame_export_resized_rgb delivers for frames[i]
 *   with this rectangle, this output size and the descriptor's samples (M355_RGB_U8: 0..255, M355_RGB_U16: 0..65535), matrix and full_range;
 *   the element is m355_tensor_element(v, scale[c], bias[c], dtype), which is (libde265_amd/csrc/tensor_element.h: the one definition, compiled
 *   into the kernel and into the host function):
 *     p = (float)v                     exact
 *     t = p * scale                    ONE binary32 multiplication, round to nearest even
 *     r = t + bias                     ONE binary32 addition, round to nearest even — two roundings, NOT a fused multiply-add
 *     M355_TENSOR_F32   r
 *     M355_TENSOR_F16   r converted to IEEE binary16, round to nearest even; underflow is gradual (binary16 subnormals are produced), overflow
 *                       gives infinity
 *     M355_TENSOR_BF16  r converted to bfloat16, round to nearest even: (bits + 0x7FFF + ((bits >> 16) & 1)) >> 16 on r's binary32 bit pattern
 *   *bits receives the element's bit pattern in the low 32 (F32) or 16 bits; the call returns M355_ERR_INVALID for an unknown dtype, a scale or bias
 *   that is not finite, or a null `bits`, and is host only.
 * A monochrome frame gives three equal channels before normalisation.  Cases in which t or r is a NONZERO binary32 SUBNORMAL are outside the
 * contract (the device may flush them to zero); v = 0 and bias = 0 give an exact zero and are inside it.
 * Where the elements go (eb = 4 for F32, else 2; strides in BYTES):
 *   M355_TENSOR_NCHW   element (n, c, y, x) at dst + n * stride_n + c * stride_c + y * stride_h + x * eb
 *   M355_TENSOR_NHWC   element (n, y, x, c) at dst + n * stride_n + y * stride_h + (3 * x + c) * eb       (stride_c is not used)
 * Bytes that are no element of the tensor — row padding, gaps between planes and between slices — are never written.  The same frame may appear
 * more than once in `frames`.
 * M355_ERR_INVALID (nothing is enqueued, no destination byte written): n outside 1..M355_TENSOR_MAX_FRAMES, null `frames`, null descriptor, a bad
 * handle; frames whose chroma format, bit depths or element size differ from frames[0]'s; a frame that does not contain the rectangle — with
 * width == 0 (the whole frame) every frame must have frames[0]'s size —; whatever m355_frame_export_resized_rgb rejects for the rectangle, the output
 * size, the ratio, samples, matrix and full_range; an unknown layout or dtype; a scale or bias that is not finite; a null dst; a dst or a USED
 * stride (stride_h; stride_c for NCHW; stride_n for n > 1) that is no multiple of eb; stride_h below the row's bytes (row = out_width * eb for NCHW,
 * 3 * out_width * eb for NHWC); strides that make planes or slices overlap — with E = (out_height - 1) * stride_h + row:
 *   NCHW  stride_c >= E, and for n > 1  stride_n >= 2 * stride_c + E            NHWC  for n > 1  stride_n >= E.
 * Ordering and the gate: asynchronous, and a reader of the kind of m355_frame_export of EVERY frame of the batch.  The launch is queued on the
 * stream of frames[0]'s last writer, which first continues behind the last writer and the earlier export of every other frame of the batch; ONE
 * mark behind the launch is kept by every frame, so m355_frame_export_wait / m355_frame_export_order on ANY frame of the batch cover the whole
 * tensor, and the next decode into any of those frames waits for it.  Every frame carries its own gate: a slice whose frame sits behind a rejected
 * decode is not written, the other slices are.  Tile-sharded contexts: as m355_frame_export_resized_rgb. */
#define M355_TENSOR_MAX_FRAMES 32
#define M355_TENSOR_NCHW 0
#define M355_TENSOR_NHWC 1
#define M355_TENSOR_F32  0
#define M355_TENSOR_F16  1   /* IEEE binary16 */
#define M355_TENSOR_BF16 2
typedef struct m355_tensor_desc {
  int32_t layout, dtype;                 /* M355_TENSOR_NCHW / _NHWC, M355_TENSOR_F32 / _F16 / _BF16 */
  int32_t samples, matrix, full_range;   /* the INTEGER stage: M355_RGB_U8 / _U16, M355_MATRIX_*, 0 / 1, as m355_rgb_desc */
  int32_t x0, y0, width, height;         /* source luma rectangle, the same in every frame (width == 0: the whole frame) */
  int32_t out_width, out_height;         /* luma size of every slice */
  float   scale[3], bias[3];             /* per channel R, G, B */
  void*   dst;                           /* device memory, or m355_host_alloc memory */
  int64_t stride_n, stride_c, stride_h;  /* BYTES */
} m355_tensor_desc;                      /* (LP64: 104 bytes) */
M355_API int   m355_frames_export_tensor(m355_ctx* ctx, const int* frames, int n, const m355_tensor_desc* desc);   /* asynchronous */
M355_API int   m355_frames_export_tensor_filtered(m355_ctx* ctx, const int* frames, int n, const m355_tensor_desc* desc, int filter);   /* M355_FILTER_* */
M355_API int   m355_tensor_element(uint32_t v, float scale, float bias, int dtype, uint32_t* bits);                 /* host only */
/* A batch of REGIONS as one float tensor in one launch: as m355_frames_export_tensor, but with ONE RECTANGLE PER SLICE — the boxes of a detector in
 * one frame, each resized to a classifier's input; the random crops and flips of a training loader; whole frames of different sizes.  The definition
 * is a composition and adds no arithmetic, constant or siting rule:
 *   let T_i be what m355_frames_export_tensor delivers for n = 1, frames = {frames[i]}, this descriptor with its rectangle replaced by rois[i] and
 *   dst replaced by dst + i * stride_n;
 *   without M355_ROI_MIRROR in rois[i].flags, slice i is T_i, byte for byte;
 *   with it, element (c, y, x) of slice i is element (c, y, out_width - 1 - x) of T_i: the pixels of a row are reversed, the three channels of an
 *   NHWC pixel keep their order.
 * rois[i].width == 0 means the whole of frames[i], by the rule of m355_export_desc, so frames of different SIZES may share a tensor (chroma format,
 * bit depths and element size must still be frames[0]'s).  The same frame may appear any number of times.  Bytes that are no element of the tensor
 * are never written.
 * M355_ERR_INVALID (nothing is enqueued, no destination byte written; m355_last_error names the entry): whatever m355_frames_export_tensor rejects for
 * n, the handles, chroma format, bit depths and element size against frames[0], the output size, samples, matrix, full_range, layout, dtype, scale,
 * bias, dst and the strides; null `rois`; a descriptor whose x0, y0, width, height are not all 0 (the rectangles are the entries'); a flag bit other
 * than M355_ROI_MIRROR; for ANY entry i: a rectangle that leaves frames[i], is off the chroma grid or has a negative size, or a ratio outside
 * src <= 8 * out && out <= 8 * src on either axis for THAT entry — a region smaller than an eighth of the output is rejected, not clamped.
 * Ordering, the gate, sharded contexts, m355_frame_export_wait and m355_frame_export_order: exactly those of m355_frames_export_tensor — one mark kept
 * by every distinct frame, each slice behind its own frame's gate: the slices of a frame behind a rejected decode are skipped, the others written.
 * Not offered: an output size per slice, a filter per slice, ratios beyond 8 (M355_FILTER_CUBIC: beyond 4 down), regions off the chroma grid,
 * a siting per slice. */
#define M355_ROI_MIRROR 1                /* flags: the slice's columns in reverse order */
typedef struct m355_tensor_roi {
  int32_t x0, y0, width, height;         /* source luma rectangle in frames[i], as in m355_export_desc (width == 0: the whole frame) */
  int32_t flags;                         /* 0 or M355_ROI_MIRROR */
} m355_tensor_roi;                       /* (20 bytes) */
M355_API int   m355_frames_export_tensor_rois(m355_ctx* ctx, const int* frames, const m355_tensor_roi* rois, int n,
                                              const m355_tensor_desc* desc);   /* asynchronous */
M355_API int   m355_frames_export_tensor_rois_filtered(m355_ctx* ctx, const int* frames, const m355_tensor_roi* rois, int n,
                                                       const m355_tensor_desc* desc, int filter);   /* M355_FILTER_*; its limits per entry */
/* OPTIONS of the five exports that bring chroma to the luma grid or resize it: the filter of the _filtered entry points and the CHROMA SAMPLE
 * LOCATION TYPE of the 4:2:0 source (H.265 Figure E.1, chroma_sample_loc_type; HDR / BT.2020 streams signal type 2).  One structure, so that the
 * chain of suffixes ends here: every plain and every _filtered call IS its _opts call with chroma_loc = 0 (and the triangle filter), and a NULL
 * `opts` means {M355_FILTER_TRIANGLE, 0}.  chroma_loc = 0..3 is two independent positions:
 *                 horizontal hx = chroma_loc & 1                          vertical vy = chroma_loc >> 1
 *   0   LEFT:   chroma column i sits on luma column 2i                    MID: chroma row j sits midway between luma rows 2j and 2j + 1
 *   1   CENTRE: chroma column i sits midway between columns 2i, 2i + 1    TOP: chroma row j sits on luma row 2j
 * so type 0 = (LEFT, MID), 1 = (CENTRE, MID), 2 = (LEFT, TOP), 3 = (CENTRE, TOP).
 * The RECONSTRUCTION FILTER for luma (X, Y) is bilinear with weights in quarters per axis and ONE rounding.  i = X >> 1, j = Y >> 1, indices
 * clamped to the plane the filter reads (the FRAME's in m355_frame_export_rgb, the RESIZED plane in the composed exports), {index: weight}:
 *   LEFT    X even {i: 4}             X odd {i: 2, i + 1: 2}          MID   Y even {j: 3, j - 1: 1}     Y odd {j: 3, j + 1: 1}
 *   CENTRE  X even {i: 3, i - 1: 1}   X odd {i: 3, i + 1: 1}          TOP   Y even {j: 4}               Y odd {j: 2, j + 1: 2}
 *   C' = (sum over rows and columns of wv * wh * C[row][col] + 8) >> 4        a sample of the chroma bit depth, rounded BEFORE the matrix; the
 *                                                                             sum stays below 2^20
 * For type 0 this is the filter stated at m355_frame_export_rgb bit for bit: (4 T + 8) >> 4 = (T + 2) >> 2 and (2 T + 2 T' + 8) >> 4 =
 * (T + T' + 4) >> 3 with T = 3 C[j] + C[jn].
 * RESIZE GRIDS keep the siting: planes are still resized each on its own grid; the horizontal chroma axis is co-sited iff LEFT (CENTRE: centre-
 * aligned), the vertical chroma axis is co-sited iff TOP (MID: centre-aligned); a co-sited axis has C = 2 i sn, the rows m355_resize_taps returns for
 * cosited = 1.  Luma, both filters, every rounding, the clamp to the rectangle and all limits are unchanged, and the composed exports remain
 * compositions: resize every plane on these grids, reconstruct on the resized chroma with the filter above, then the matrix / m355_tensor_element.
 * For a batch chroma_loc is the batch's, like the filter.
 * M355_ERR_INVALID (nothing is enqueued, no destination byte written) beyond what the plain call rejects: a non-zero `reserved` entry — reserved[0] is
 * `colour`, for which the rule reads: any value that is not 0 or a live colour transform of this context in a call that has the stage (COLOUR TRANSFORM below); an unknown
 * filter, and for m355_frame_export_rgb_opts, which resizes nothing, any filter but 0; chroma_loc outside 0..3 (4 and 5, bottom-sited, included);
 * a non-zero chroma_loc for a frame that is not 4:2:0 (the standard defines the field for 4:2:0 alone).
 * m355_frame_export, m355_frame_export_scaled (a box average without siting correction), the hashes, the measurements and the downloads deliver
 * samples on their own grids and know no siting.
 * Not offered: the bottom-sited types 4 and 5, a siting per slice, siting for 4:2:2. */
typedef struct m355_export_opts {
  int32_t filter;                        /* M355_FILTER_* */
  int32_t chroma_loc;                    /* chroma sample location type of the 4:2:0 source, 0..3 */
  union {
    int32_t reserved[6];                 /* 0, but for reserved[0], which IS `colour` */
    int32_t colour;                      /* 0: none; else a handle of m355_colour_create of THIS context (COLOUR TRANSFORM below) */
  };
} m355_export_opts;                      /* (32 bytes) */
M355_API int   m355_frame_export_rgb_opts(m355_ctx* ctx, int frame, const m355_rgb_desc* desc, const m355_export_opts* opts);
M355_API int   m355_frame_export_resized_opts(m355_ctx* ctx, int frame, const m355_resize_desc* desc, const m355_export_opts* opts);
M355_API int   m355_frame_export_resized_rgb_opts(m355_ctx* ctx, int frame, const m355_resize_rgb_desc* desc, const m355_export_opts* opts);
M355_API int   m355_frames_export_tensor_opts(m355_ctx* ctx, const int* frames, int n, const m355_tensor_desc* desc, const m355_export_opts* opts);
M355_API int   m355_frames_export_tensor_rois_opts(m355_ctx* ctx, const int* frames, const m355_tensor_roi* rois, int n,
                                                   const m355_tensor_desc* desc, const m355_export_opts* opts);
/* COLOUR TRANSFORM of the composed exports: a stage between the YCbCr -> R'G'B' matrix and the output of m355_frame_export_resized_rgb_opts,
 * m355_frames_export_tensor_opts and m355_frames_export_tensor_rois_opts — 1-D table -> 3x3 matrix -> 1-D table (shaper / matrix / shaper), in integers —
 * which maps, e.g., PQ or HLG code values in BT.2020 primaries to BT.709 / sRGB values for an SDR consumer.  m355_export_opts.colour = 0 is every
 * call as it is without the stage, byte for byte.
 * PER PIXEL (m355_colour_pixel; host only; csrc/colour_transform.h is the one definition, compiled into the kernel too).  rgb16 = the clipped 16-bit
 * full-scale R'G'B' of the pixel, 0..65535:
 *   1. linearise, per channel, k = v >> 6, f = v & 63:  L = (lut_in[k] (64 - f) + lut_in[k + 1] f + 32) >> 6.  Knot k stands for v = 64 k; knot
 *      1024 is reached only as the upper neighbour.  L <= M355_COLOUR_ONE.
 *   2. matrix, per output channel c, in exact integers (>> arithmetic):
 *      P_c = clip(0, ONE, (m[c][0] L_r + m[c][1] L_g + m[c][2] L_b + (1 << 13)) >> 14).
 *   3. encode, per channel, through a table indexed like a small float (accurate at the black end, where an inverse gamma is steep):
 *      P < 64: idx = P, fr = 0.  Otherwise e = floor(log2 P) (6..24), n = P << (24 - e), idx = 64 (e - 5) + ((n >> 18) & 63), fr = (n >> 10) & 255;
 *      P = ONE gives idx = 1216, fr = 0.  Knot idx stands for P = idx below 64 and for (64 + idx % 64) << (idx / 64 - 1) from 64 up.
 *      o = (lut_out[idx] (256 - fr) + lut_out[min(idx + 1, 1216)] fr + 128) >> 8.
 *   4. deliver.  M355_RGB_U16: o.  M355_RGB_U8: (2 o + 257) / 514, which is o / 257 rounded.
 * THE COMPOSED EXPORTS WITH A COLOUR TRANSFORM: for each pixel, the (R, G, B) the same call delivers with samples = M355_RGB_U16 and no colour
 * transform goes through m355_colour_pixel with the descriptor's `samples` — the matrix coefficients are those of m355_rgb_coefficients(...,
 * M355_RGB_U16, ...) whatever `samples` says, which only picks step 4.  Resize, siting, filter, mirror, m355_tensor_element, layouts, strides,
 * ordering and gates are unchanged.  A monochrome frame, or neutral chroma, gives three equal channels whenever every matrix row sums to 1 << 14.
 * out size == rectangle of m355_frame_export_resized_rgb_opts is the unresized R'G'B' export with colour: m355_frame_export_rgb_opts and
 * m355_frame_export_resized_opts reject a non-zero colour (M355_ERR_INVALID, nothing enqueued).
 * OBJECTS.  m355_colour_create checks the bounds stated at the fields and pad == 0 (else M355_ERR_INVALID, as for null pointers), copies the tables
 * into device memory the context owns and returns a handle >= 0x100 in *handle; at most M355_COLOUR_OBJECTS objects live per context (one more:
 * M355_ERR_BUSY).  A value that is not a live handle of THIS context — a destroyed one, another context's, 1 — is M355_ERR_INVALID in every export.
 * m355_colour_destroy waits for the context's work first, as m355_device_free does, so it may follow an export directly.
 * PRESETS (m355_colour_preset; host only, no context, double arithmetic).  Transfers and primaries are the H.265 code points of Tables E.3 / E.4; code
 * 2, unspecified, counts as 1.  white = white_nits, or 203 for 0.
 *   lut_in[k], E = min(64 k, 65535) / 65535 -> nits:  in_transfer 1 / 6 / 14 / 15: white E^2.4;  13: white * inverse sRGB;  8: white E;
 *     16: 10000 * ST 2084 EOTF;  18: 1000 * (inverse HLG OETF)^1.2 — the HLG OOTF per channel with gamma 1.2, a stated simplification.
 *     S = the nits at E = 1; the entry is min(ONE, floor(nits / S * ONE + 0.5)).
 *   matrix: RGB -> XYZ of in_primaries, then XYZ -> RGB of out_primaries; primaries 1, 5, 6 and 9, white D65 (0.3127, 0.3290), from the xy
 *     chromaticities of Table E.3.  Each coefficient is floor(c * 16384 + 0.5); then the largest-magnitude entry of each row is adjusted so that the
 *     row sums to exactly 1 << 14.  Equal primaries give the exact identity.
 *   lut_out[i]: nits = knot(i) / ONE * S, x = nits / white, peak = peak_nits or S for 0, w = max(1, peak / white);
 *     M355_TONE_CLIP y = min(1, x);  M355_TONE_REINHARD y = min(1, x (1 + x / w^2) / (1 + x));
 *     the inverse of out_transfer: 1 / 6 / 14 / 15 y^(1 / 2.4), 13 sRGB, 8 y; the entry is floor(y' * 65535 + 0.5).
 *   M355_ERR_INVALID: any other code point; out_transfer 16 or 18; a non-zero `reserved`; negative nits; peak < white when given; null pointers.
 * TONE OBJECTS (m355_colour_create_tone): tables plus a m355_colour_tone.  The tone curve of a plain object is baked into lut_out and so acts per
 * channel, which changes R : G : B above SDR white: saturated highlights shift in hue and desaturate.  A tone object looks ONE gain per pixel up, at
 * the pixel's maxRGB or luminance, and multiplies it into the three linear channels (BT.2390's advice).  Per pixel (m355_colour_pixel_tone; host only)
 * steps 1 and 2 run unchanged and give P_r, P_g, P_b in 0..ONE; then
 *   2b. n = max(P_r, P_g, P_b) for M355_NORM_MAXRGB; for M355_NORM_LUMA n = clip(0, ONE, (w[0] P_r + w[1] P_g + w[2] P_b + (1 << 13)) >> 14), the
 *       arithmetic of step 2 with `weights` as the row.  (idx, fr) from n as in step 3;
 *       g = (gain[idx] (256 - fr) + gain[min(idx + 1, 1216)] fr + 128) >> 8  (Q24, <= M355_TONE_GAIN_ONE);
 *       P'_c = (P_c g + (1 << 23)) >> 24 in exact integers (49 bits), so P'_c <= ONE, and P'_a P_b and P'_b P_a differ by at most (P_a + P_b) / 2:
 *       the ratios are kept to the one rounding.
 *   Steps 3 and 4 run unchanged on P'.  With every gain = M355_TONE_GAIN_ONE a tone object delivers what the plain object of the same tables does.
 * m355_colour_create_tone shares the handle space, the limit of M355_COLOUR_OBJECTS and m355_colour_destroy with m355_colour_create; its handle goes
 * wherever `colour` does.  M355_ERR_INVALID, nothing allocated: whatever m355_colour_create rejects; a null tone; an unknown norm; a gain above
 * M355_TONE_GAIN_ONE; a weight outside -65535..65535; a non-zero weight with M355_NORM_MAXRGB; a non-zero `reserved`.
 * m355_colour_preset_tone (host only, doubles) takes the descriptor of m355_colour_preset and a norm: lut_in and matrix are those of m355_colour_preset
 *   byte for byte; lut_out is that of M355_TONE_CLIP (the inverse of out_transfer on min(1, x)); weights = the Y row of RGB -> XYZ of out_primaries,
 *   Q14 rounded, the largest entry adjusted so that the row sums to 1 << 14 (all 0 for M355_NORM_MAXRGB); gain[0] = M355_TONE_GAIN_ONE and
 *   gain[i] = floor(min(1, y(x) / x) 2^24 + 0.5) at x = knot(i) / ONE * S / white, with y the curve of `tone`: M355_TONE_CLIP y = min(1, x), a
 *   hue-preserving clip; M355_TONE_REINHARD as above; M355_TONE_BT2390 the EETF of BT.2390 in the PQ domain with black 0: L_w = peak (or S),
 *   maxLum = PQ^-1(white) / PQ^-1(L_w), KS = 1.5 maxLum - 0.5, E1 = PQ^-1(x white) / PQ^-1(L_w), E2 = E1 below KS and the Hermite spline
 *   (2 t^3 - 3 t^2 + 1) KS + (t^3 - 2 t^2 + t) (1 - KS) + (-2 t^3 + 3 t^2) maxLum with t = (E1 - KS) / (1 - KS) above, clamped to 0..1,
 *   y = PQ(E2 PQ^-1(L_w)) / white.  maxLum >= 1 is the identity; KS < 0 (a peak too far above white for the spline) is M355_ERR_INVALID, like
 *   everything m355_colour_preset rejects and an unknown norm.  M355_TONE_BT2390 is the new call's alone: m355_colour_preset rejects it.
 * Not offered: HDR outputs (PQ / HLG out, linear above SDR white); a gain above 1; the luminance-dependent HLG OOTF; 3-D
 * LUTs; dynamic metadata; colour in m355_frame_export_rgb_opts; a transform per slice. */
#define M355_COLOUR_ONE        (1 << 24)     /* linear light, full scale */
#define M355_COLOUR_IN_KNOTS   1025
#define M355_COLOUR_OUT_KNOTS  1217
#define M355_COLOUR_OBJECTS    16
#define M355_TONE_CLIP         0
#define M355_TONE_REINHARD     1
#define M355_TONE_BT2390       2             /* m355_colour_preset_tone only */
#define M355_TONE_GAIN_ONE     (1 << 24)     /* a gain of 1, Q24 */
#define M355_NORM_MAXRGB       0
#define M355_NORM_LUMA         1
typedef struct m355_colour_tables {
  uint32_t lut_in[M355_COLOUR_IN_KNOTS];     /* every entry <= M355_COLOUR_ONE */
  int32_t  matrix[9];                        /* row-major, Q14, every |entry| <= 65535 */
  uint16_t lut_out[M355_COLOUR_OUT_KNOTS];
  uint16_t pad;                              /* 0 */
} m355_colour_tables;                        /* (6572 bytes) */
typedef struct m355_colour_preset_desc {
  int32_t in_transfer, in_primaries, out_transfer, out_primaries, tone, white_nits, peak_nits, reserved;
} m355_colour_preset_desc;
typedef struct m355_colour_tone {
  int32_t  norm;                             /* M355_NORM_* */
  int32_t  weights[3];                       /* M355_NORM_LUMA: Q14 row, every |entry| <= 65535; M355_NORM_MAXRGB: 0 */
  uint32_t gain[M355_COLOUR_OUT_KNOTS];      /* Q24, every entry <= M355_TONE_GAIN_ONE; indexed like lut_out */
  uint32_t reserved[3];                      /* 0 */
} m355_colour_tone;                          /* (4896 bytes) */
M355_API int   m355_colour_create_tone(m355_ctx* ctx, const m355_colour_tables* tables, const m355_colour_tone* tone, int* handle);
M355_API int   m355_colour_preset_tone(const m355_colour_preset_desc* desc, int norm, m355_colour_tables* tables_out, m355_colour_tone* tone_out);
M355_API int   m355_colour_pixel_tone(const m355_colour_tables* tables, const m355_colour_tone* tone, const uint32_t rgb16[3], int samples, uint32_t out[3]);
M355_API int   m355_colour_create(m355_ctx* ctx, const m355_colour_tables* tables, int* handle);
M355_API int   m355_colour_destroy(m355_ctx* ctx, int handle);
M355_API int   m355_colour_preset(const m355_colour_preset_desc* desc, m355_colour_tables* out);
M355_API int   m355_colour_pixel(const m355_colour_tables* tables, const uint32_t rgb16[3], int samples, uint32_t out[3]);
/* PIXEL FORMATS: the last stage of the export line for a compositor on the same GPU — a swap chain, a Vulkan or GL image, a DRM plane, a HIP texture —,
 * which takes B8G8R8A8, R8G8B8A8 or a 2:10:10:10 dword and no 24-bit texel, and for consumers that want B, G, R order (k_export_rgb.hip,
 * k_export_resized_rgb.hip RR_FRAME).  The definition is a COMPOSITION and adds one formula:
 *   1. S(format) = M355_RGB_U8 for RGBA8, BGRA8 and BGR8, M355_RGB_U16 for the two 10-bit formats;
 *   2. (R, G, B) of a pixel are the three values the existing call delivers with M355_RGB_PACKED, samples S(format) and the same matrix, range,
 *      rectangle, output size and options: m355_frame_export_rgb_opts for m355_frame_export_pixels, m355_frame_export_resized_rgb_opts — with its
 *      filter, chroma siting and colour / tone object — for m355_frame_export_resized_pixels;
 *   3. the pixel's bytes are m355_pixel_pack(format, {R, G, B}, alpha) (host only; csrc/pixel_pack.h is the one definition, compiled into the kernels
 *      too).  8-bit formats: the values as they are, in the byte order below.  10-bit formats: each channel first becomes
 *      c10 = (2046 c + 65535) / 131070 in unsigned 32-bit arithmetic = round(c * 1023 / 65535), the 10-bit sibling of step 4 of m355_colour_pixel,
 *      then the dword below, stored little-endian.  With a colour object the 10-bit delivery is therefore c10 of step 3's 16-bit result.
 * Every rule of the call underneath carries over: the whole-frame and sub-rectangle rim rules of the two calls as stated above; the colour stage exists
 * in the resized call only (a non-zero `colour` in m355_frame_export_pixels is M355_ERR_INVALID, as in m355_frame_export_rgb_opts), and
 * m355_frame_export_resized_pixels with the output size equal to the rectangle is the way to tone-map without resizing.
 * M355_ERR_INVALID (nothing is enqueued, no destination byte written): whatever the call underneath rejects for the frame handle, the rectangle, the
 * output size, the ratio, matrix, full_range and the options; an unknown format; alpha outside the format's range; a null descriptor or a null dst;
 * a pitch below width * bytes per pixel (the resized call: out_width * bytes per pixel); for the 4-byte formats a dst or a pitch that is no multiple
 * of 4; for m355_frame_export_pixels a non-zero out_width or out_height.  m355_pixel_pack rejects an unknown format, a channel above 255 (8-bit
 * formats) or 65535 (10-bit formats), alpha outside the range and null pointers; *n_bytes = the bytes written to out (3 or 4).
 * Ordering, the gate behind a rejected decode, reader marks, m355_frame_export_wait and m355_frame_export_order, and sharded contexts are exactly
 * those of m355_frame_export_rgb, and destination bytes beyond a row are never written.
 * Not offered: 16-bit and half-float four-channel pixels (the composed kernel's staged row has 1536 bytes for 256 columns); ARGB and ABGR byte orders;
 * an alpha plane taken from a picture; pixel formats in the tensor exports; premultiplication. */
#define M355_PIXEL_RGBA8        0   /* 4 bytes per pixel: R, G, B, A */
#define M355_PIXEL_BGRA8        1   /* 4 bytes per pixel: B, G, R, A */
#define M355_PIXEL_BGR8         2   /* 3 bytes per pixel: B, G, R */
#define M355_PIXEL_A2B10G10R10  3   /* one little-endian dword: R | G << 10 | B << 20 | A << 30 */
#define M355_PIXEL_A2R10G10B10  4   /* one little-endian dword: B | G << 10 | R << 20 | A << 30 */
typedef struct m355_pixel_desc {
  int32_t format, alpha;            /* M355_PIXEL_*; A: 0..255 (RGBA8 / BGRA8), 0..3 (2:10:10:10), 0 (BGR8) */
  int32_t matrix, full_range;       /* as m355_rgb_desc */
  int32_t x0, y0, width, height;    /* source luma rectangle, as m355_export_desc (width == 0: whole frame) */
  int32_t out_width, out_height;    /* m355_frame_export_resized_pixels: luma size of the result; m355_frame_export_pixels: both 0 */
  void*   dst;                      /* device memory or m355_host_alloc memory */
  int64_t pitch;                    /* BYTES per destination row */
} m355_pixel_desc;                  /* LP64: 56 bytes */
M355_API int   m355_frame_export_pixels(m355_ctx* ctx, int frame, const m355_pixel_desc* desc, const m355_export_opts* opts);           /* asynchronous */
M355_API int   m355_frame_export_resized_pixels(m355_ctx* ctx, int frame, const m355_pixel_desc* desc, const m355_export_opts* opts);   /* asynchronous */
M355_API int   m355_pixel_pack(int format, const uint32_t rgb[3], uint32_t alpha, uint8_t out[4], int* n_bytes);   /* host only */
/* ORIENTATION — m355_frame_export and m355_frame_export_pixels with the picture turned in the same launch: a phone's portrait video (landscape samples
 * plus a 90 degree flag in the container), the irot / imir of a HEIF still, HEVC's display orientation SEI.  The source is read once and the
 * destination written once (k_export_oriented.hip); csrc/orientation.h is the one definition, compiled into the kernels too.
 * An orientation o is 0..7, three bits: TRANSPOSE is applied FIRST, then FLIP, then MIRROR.  A source rectangle S of w columns and h rows of ELEMENTS
 * becomes D of W' x H' = h x w with TRANSPOSE, else w x h, and for every (X, Y)
 *   u = MIRROR ? W' - 1 - X : X      v = FLIP ? H' - 1 - Y : Y      D[Y][X] = TRANSPOSE ? S[u][v] : S[v][u]        (S[row][column])
 * — numpy: T = S.T if o & 4 else S; T = T[::-1] if o & 2 else T; T = T[:, ::-1] if o & 1 else T.  0 identity, 1 mirror, 2 flip, 3 rotation by 180
 * degrees, 4 transpose, 5 rotation by 90 degrees clockwise (np.rot90(S, -1)), 6 by 90 degrees anticlockwise (np.rot90(S, 1)), 7 anti-transpose.
 *   m355_orientation_compose    *out = the one orientation equal to `first` and then `then` (an irot followed by an imir, a container matrix on top of
 *                               an SEI); M355_ERR_INVALID for a value outside 0..7 or a null result
 *   m355_orientation_from_exif  *out = the orientation that brings a picture stored with EXIF / TIFF Orientation 1..8 upright: 1 -> 0, 2 -> 1, 3 -> 3,
 *                               4 -> 2, 5 -> 4, 6 -> 5, 7 -> 7, 8 -> 6; anything else is M355_ERR_INVALID
 * m355_frame_export_oriented is m355_frame_export with every plane of the rectangle oriented ON ITS OWN GRID.  desc keeps its meaning: the layout, the
 * samples with the formulas above, the crop, the caller's pitches.  An element is one converted sample; for the interleaved chroma plane of the
 * semi-planar layout it is the (Cb, Cr) pair, which moves as a unit.  With TRANSPOSE plane p of pw x ph elements becomes ph x pw, and its pitch is
 * checked against the ORIENTED row's bytes; bytes beyond an oriented row are never written.  Orientation 0 IS m355_frame_export: the call dispatches
 * to it.  Like m355_frame_export this call moves samples and knows no siting: the chroma samples keep their values, so what a 4:2:0 siting becomes is
 * the consumer's to note.  An axis with chroma MIDWAY between two luma samples (horizontally types 1, 3, 5; vertically
 * types 0, 1) stays midway when it is reversed.  Reversing an axis on which chroma is CO-SITED with the even luma samples puts it on the ODD ones:
 * vertically that exchanges the top-sited types 2, 3 with the bottom-sited 4, 5; horizontally (types 0, 2, 4 under MIRROR) it LEAVES the types 0..5,
 * none of which has chroma on odd luma columns.  TRANSPOSE exchanges the two axes' sitings (type 0 becomes 3, 3 becomes 0, 1 and 2 stay; 4 and 5 leave
 * the types).  A consumer that needs R'G'B' takes m355_frame_export_pixels_oriented, which reconstructs chroma BEFORE the picture is turned.
 * M355_ERR_INVALID (nothing is enqueued, no destination byte written): whatever m355_frame_export rejects; an orientation outside 0..7; TRANSPOSE on a
 * 4:2:2 frame (the result would be 4:4:0, which no layout here describes).
 * m355_frame_export_pixels_oriented is a COMPOSITION: the pixels m355_frame_export_pixels delivers for the same arguments, permuted as whole pixels by
 * the definition above — chroma reconstruction, chroma_loc and the matrix happen in the SOURCE's orientation.  The four-byte formats RGBA8, BGRA8 and
 * both 2:10:10:10; with TRANSPOSE the pitch is checked against height * 4.  Orientation 0 dispatches to m355_frame_export_pixels.  M355_ERR_INVALID:
 * whatever that call rejects, an orientation outside 0..7, M355_PIXEL_BGR8 with an orientation other than 0.
 * Ordering, the gate behind a rejected decode, reader marks, m355_frame_export_wait and m355_frame_export_order, and sharded contexts are exactly those
 * of m355_frame_export.
 * Not offered: orientation in the resized, colour / tone and tensor exports (the composed kernel of k_export_resized_rgb.hip, which stores rows as it
 * filters them); M355_PIXEL_BGR8 (a three-byte element in the transposing tile, whose elements are 1, 2 or 4 bytes); planar R'G'B'
 * (m355_frame_export_rgb); arbitrary angles (a resampling, not a permutation). */
#define M355_ORIENT_MIRROR        1   /* columns reversed */
#define M355_ORIENT_FLIP          2   /* rows reversed */
#define M355_ORIENT_TRANSPOSE     4   /* rows and columns exchanged (applied FIRST) */
#define M355_ORIENT_ROTATE_0      0
#define M355_ORIENT_ROTATE_180    3   /* MIRROR | FLIP */
#define M355_ORIENT_ROTATE_90_CW  5   /* TRANSPOSE | MIRROR */
#define M355_ORIENT_ROTATE_90_CCW 6   /* TRANSPOSE | FLIP */
M355_API int   m355_orientation_compose(int first, int then, int* out);                /* host only */
M355_API int   m355_orientation_from_exif(int exif_1_to_8, int* out);                  /* host only */
M355_API int   m355_frame_export_oriented(m355_ctx* ctx, int frame, const m355_export_desc* desc, int orientation);   /* asynchronous */
M355_API int   m355_frame_export_pixels_oriented(m355_ctx* ctx, int frame, const m355_pixel_desc* desc, const m355_export_opts* opts, int orientation);   /* asynchronous */
M355_API int   m355_frame_export_wait(m355_ctx* ctx, int frame);
M355_API int   m355_frame_export_order(m355_ctx* ctx, int frame, void* consumer_hipStream);
/* Device memory for export destinations and blocking copies out of / into it, for applications (and the tests) that keep a second HIP
 * runtime out of the process.  m355_device_alloc: NULL on failure, contents undefined;
 * m355_device_free waits for the context's work first.  m355_device_read / _write block until all work of the context (exports included) has
 * finished and copy through the context's pinned staging buffer. */
M355_API void* m355_device_alloc(m355_ctx* ctx, size_t bytes);
M355_API void  m355_device_free(m355_ctx* ctx, void* p);
M355_API int   m355_device_read(m355_ctx* ctx, const void* dev_src, void* host_dst, size_t bytes);
M355_API int   m355_device_write(m355_ctx* ctx, void* dev_dst, const void* host_src, size_t bytes);

/* Diagnostic (bench.py's roofline): the device-to-device copy rate this box reaches — `bytes` read + `bytes` written per launch of a float4 copy
 * kernel, the median of `iters` launches timed with events on the context's stream, in GB/s (read + written bytes / time).  The achievable
 * ceiling next to the 8 TB/s specification ("measure the real ceiling with a device-to-device copy kernel on the box"). */
M355_API int m355_measure_copy_rate(m355_ctx* ctx, size_t bytes, int iters, double* gbps);

/* Pinned host memory for the planes an application reads decoded pictures from: what a get_buffer callback registered
 * with de265_set_image_allocation_functions (de265.h:350-368; default allocator image.cc:110-184) hands out, so that
 * m355_frame_download runs at full PCIe rate.  NULL on failure. */
M355_API void* m355_host_alloc(size_t bytes);
M355_API void  m355_host_free(void* p);

/* SEI decoded picture hash of a device frame, computed where the frame lives.
 * Replaces compute_MD5 / compute_CRC_8bit_fast / compute_checksum (sei.cc:161-258) as called by
 * process_sei_decoded_picture_hash (sei.cc:276-356); hash_type and the result fields are those of
 * sei_decoded_picture_hash (sei.h:57-70).  Only the field of the requested type is written, for plane 0 (monochrome)
 * or planes 0..2.  Synchronous: waits for the pictures in flight — for EVERY picture on every lane, not only for the frame's own:
 * a caller that hashes every picture decodes one picture at a time, whatever m355_set_pipeline_depth says (m355_frame_hash_async
 * below does not).  CRC and checksum run on the device (the frame is not
 * copied back); MD5 is one serial chain per plane, so the planes are downloaded and hashed on host threads. */
#define M355_HASH_MD5      0
#define M355_HASH_CRC      1
#define M355_HASH_CHECKSUM 2
typedef struct m355_picture_hash {
  uint8_t  md5[3][16];
  uint16_t crc[3];
  uint32_t checksum[3];
} m355_picture_hash;
M355_API int m355_frame_hash(m355_ctx* ctx, int frame, int hash_type, m355_picture_hash* out);
/* The same hash as a REQUEST queued behind the frame's decode: m355_frame_hash_async enqueues the hash of the frame as its last writer
 * leaves it and returns without waiting for anything; the pictures in flight on the other lanes go on.  The request is a reader of the
 * frame, like m355_frame_export: it runs on the stream of the decode that wrote the frame, and the next decode INTO the frame waits
 * for it in front of its first write — hash a frame, then decode the next picture into it, and the value is the earlier picture's.
 * CRC / checksum: one kernel launch that reduces the planes and writes the values into pinned memory of the request.  MD5: the planes
 * are copied into pinned planes of the request behind the decode and hashed on host threads when the result is collected.
 * *ticket counts 1, 2, ... per context.  At most M355_HASH_REQUESTS requests may be outstanding (enqueued and not yet collected):
 * one more returns M355_ERR_BUSY and enqueues nothing.  M355_ERR_INVALID (nothing enqueued): bad frame handle, bad hash type, null
 * ticket, or a tile-sharded context (its frames are complete only behind the gather).
 * m355_frame_hash_result collects a request and frees its slot: block = 0 -> M355_ERR_BUSY while the request has not finished
 * (nothing is waited for, the request stays), block = 1 -> the host waits for THAT request only.  M355_OK: the field of the requested
 * type is filled as by m355_frame_hash, bit for bit.  M355_ERR_INVALID: an unknown or already collected ticket; or — the request is
 * collected all the same — a hash queued behind a decode whose lists were rejected on the device (m355_decode_status): like an
 * export behind such a decode it has produced nothing.  m355_wait completes every request and collects none; a frame may be
 * destroyed with requests pending (they are completed first and stay collectable). */
#define M355_HASH_REQUESTS 16
M355_API int m355_frame_hash_async(m355_ctx* ctx, int frame, int hash_type, unsigned long long* ticket);
M355_API int m355_frame_hash_result(m355_ctx* ctx, unsigned long long ticket, int block, m355_picture_hash* out);

/* A frame COMPARED with another picture where both lie — what libde265/quality.cc (SSD, SAD, MSE) computes on host planes and `dec265 -m`
 * prints per picture, without either side crossing PCIe — as a request queued behind the frame's decode, under the contract of
 * m355_frame_hash_async.  The other picture is a frame of the same context (ref_frame >= 0) or planes in memory of the caller (ref_frame == -1).
 * Per plane of the rectangle, with a = the frame's element values as stored, b = the reference's, d = a - b:
 *   row_ssd[y] = sum_x d^2    ssd = sum_y row_ssd[y]    sad = sum |d|    n_diff = #{d != 0}    max_abs = max |d|
 *   first_x, first_y = the first sample with d != 0 in raster order, in PLANE COORDINATES OF THE FRAME (-1, -1: none)
 *   mse = MSE() of quality.cc:71-95 — from 0.0, plus (double)row_ssd[y] / width for each row in row order, then divided by height, in IEEE
 *         double (the host does this sum at collection, from per-row sums the kernel left in pinned memory).
 * All but mse are exact integers; PSNR stays with the caller (the peak value is the caller's: the reference's PSNR() hard-codes 255).
 * Planes a monochrome frame does not have read 0 / -1 / 0.0.  ref_frame == frame is legal (all zero).
 * The request is a READER of the frame, and of ref_frame when given: queued on the stream of the frame's last writer, ordered behind
 * ref_frame's last writer the way a decode waits for the writers of its reference frames, and a later decode into either frame waits for it
 * in front of its first write; the host waits for nothing at enqueue.  ref[] memory must be complete when the call is made: ordering
 * against a producer's stream is not provided.  *ticket counts 1, 2, ... per context (a count of its own, not the hash requests'); at most
 * M355_MEASURE_REQUESTS requests may be outstanding: one more returns M355_ERR_BUSY and enqueues nothing.
 * M355_ERR_INVALID, nothing enqueued: bad handles, null descriptor or ticket; a rectangle that leaves the frame or is not aligned to the
 * chroma grid (the rules of m355_export_desc); a ref_frame whose chroma format, bit depths or element size differ or which does not contain
 * the rectangle; a null ref[p] for a plane that exists, a pitch below the row's bytes, a pointer or pitch that is no multiple of the element
 * size; a tile-sharded context.
 * m355_frame_measure_result collects a request and frees its slot: block = 0 -> M355_ERR_BUSY while it runs (the request stays), block = 1 ->
 * the host waits for THAT request only.  M355_ERR_INVALID: an unknown or collected ticket; or — the request is collected all the same — a
 * request queued behind a decode whose lists were rejected, for either frame: it has read nothing.  (The gate is the lane's: a request whose
 * ref_frame was written on another lane sees that decode's verdict as long as no LATER decode of that lane has been rejected meanwhile:
 * then it returns M355_OK with values of the frame's older content — DESIGN.md section 3 states this limit of the per-lane gate.)
 * m355_wait completes every request and collects none; a frame may be destroyed with requests pending. */
#define M355_MEASURE_REQUESTS 16
typedef struct m355_measure_desc {
  int32_t     ref_frame;              /* >= 0: compare with this frame of the same context; -1: with ref[] below */
  int32_t     x0, y0, width, height;  /* luma rectangle, rules of m355_export_desc (width == 0: whole frame; chroma-grid aligned) */
  const void* ref[3];                 /* ref_frame == -1: the RECTANGLE's planes, planar, element type of the frame's plane
                                         (u8, or u16 LSB-aligned), device memory or m355_host_alloc memory */
  int64_t     pitch[3];               /* BYTES per row of ref[]; >= the row's bytes; pointer and pitch multiples of the element size */
} m355_measure_desc;
typedef struct m355_measure {
  uint64_t ssd[3], sad[3], n_diff[3];
  uint32_t max_abs[3];
  int32_t  first_x[3], first_y[3];    /* plane coordinates IN THE FRAME of the first differing sample in raster order; -1, -1: none */
  double   mse[3];
} m355_measure;
M355_API int m355_frame_measure_async(m355_ctx* ctx, int frame, const m355_measure_desc* desc, unsigned long long* ticket);
M355_API int m355_frame_measure_result(m355_ctx* ctx, unsigned long long ticket, int block, m355_measure* out);

/* The SSIM of a frame against another picture where both lie — the second number `dec265 -m` prints per picture (dec265.cc:423-504, there behind
 * libvideogfx's float Gaussian) — per plane, as a request queued behind the frame's decode like m355_frame_measure_async.  No float code is the
 * reference here: THE DEFINITION IS INTEGER-EXACT and this library's own (csrc/ssim_window.h is the one statement of it; the kernel and the host
 * helpers below run that code).
 * WEIGHTS.  The 11-tap Gaussian with sigma = 1.5 in 14 bits, w = {17, 124, 590, 1792, 3490, 4358, 3490, 1792, 590, 124, 17}: exp(-(i - 5)^2 / 4.5)
 * normalised, times 16384, rounded half up; they sum to exactly 16384 (m355_ssim_weights).
 * WINDOWS.  Each measured plane on its own grid, valid windows only: a plane of the rectangle with pw x ph samples has (pw - 10) x (ph - 10) windows,
 * window (i, j) covers the samples [i, i + 10] x [j, j + 10] with weights w[dx] w[dy] (total 2^28).  With a = the frame's sample values as stored and
 * b = the reference's, five unsigned 64-bit sums, exact:
 *   MA = sum w a    MB = sum w b    SAA = sum w a^2    SBB = sum w b^2    SAB = sum w a b
 * POINT.  In IEEE double, each operation rounded by itself in exactly this order (no fused multiply-add), peak = 2^bd - 1 with bd the PLANE's bit depth:
 *   c1 = (double)(peak peak) 2^56 / 10000.0        c2 = (double)(9 peak peak) 2^56 / 10000.0                    (K1 = 0.01, K2 = 0.03)
 *   fa = (double)MA, fb = (double)MB;  ab = fa fb, aa = fa fa, bb = fb fb
 *   cov = 2^28 (double)SAB - ab,  va = 2^28 (double)SAA - aa,  vb = 2^28 (double)SBB - bb
 *   s = ((2.0 ab + c1) (2.0 cov + c2)) / (((aa + bb) + c1) ((va + vb) + c2))
 *   q = clamp((int64)floor(s 2^30 + 0.5), -2^30, 2^30)                                                          (Q30; m355_ssim_window)
 * RESULT per measured plane: sum_q = the sum of q over the plane's windows (exact, independent of order; it can be negative), n = the number of
 * windows, min_q = the worst window, ssim = (double)sum_q / ((double)n 2^30), computed by the host at collection.  Planes that are not selected or
 * that the frame does not have read 0 in every field.  Identical planes give q = 2^30 in every window and ssim = 1.0 exactly.
 * MAP (optional, per measured plane): q of every window as int32 in device memory, (pw - 10) elements per row, (ph - 10) rows map_pitch bytes apart;
 * bytes of a row beyond its elements are not written.  The map is complete when the request has been collected, or behind m355_wait.
 * ORDERING AND VERDICTS are those of m355_frame_measure_async: a READER of the frame and of ref_frame (a kind of its own), queued on the stream of the
 * frame's last writer behind ref_frame's last writer; a later decode into either frame waits for it; the host waits for nothing at enqueue.  *ticket
 * counts 1, 2, ... per context (a count of its own); at most M355_SSIM_REQUESTS requests may be outstanding: one more returns M355_ERR_BUSY and
 * enqueues nothing.  The slots are separate from the comparison, statistics and hash slots.
 * M355_ERR_INVALID, nothing enqueued: everything m355_frame_measure_async rejects (handles, null pointers, the rectangle, ref_frame, ref[] and pitch[]
 * of every plane the frame has, a tile-sharded context); a selected plane of the rectangle narrower or lower than 11 samples; a `planes` bit for a
 * plane the frame does not have, or bits above 2; a non-zero `reserved`; a map pointer or pitch that is no multiple of 4, or a pitch below
 * 4 (pw - 10); a map for a plane that is not selected.
 * m355_frame_ssim_result collects a request and frees its slot: block = 0 -> M355_ERR_BUSY while it runs (the request stays), block = 1 -> the host
 * waits for THAT request only.  M355_ERR_INVALID: an unknown or collected ticket; or — the request is collected all the same — a request queued
 * behind a decode whose lists were rejected, for either frame (the limit of the per-lane gate stated at m355_frame_measure_async holds): it has read
 * nothing and written no map element.  m355_wait completes every request and collects none; a frame may be destroyed with requests pending.
 * HOST-ONLY HELPERS (exact, no context): m355_ssim_weights fills w[11]; m355_ssim_window computes q from sums = {MA, MB, SAA, SBB, SAB} for a bit
 * depth 1..16 (the point above).  M355_ERR_INVALID: null pointers, a bit depth outside 1..16.
 * Not offered: other window sizes or K1 / K2, border padding, a batch of frames in one launch, sharded contexts.  (Downscaled levels and their
 * combination: m355_frame_msssim_async below.) */
#define M355_SSIM_REQUESTS 16
typedef struct m355_ssim_desc {
  int32_t     ref_frame;              /* as m355_measure_desc */
  int32_t     x0, y0, width, height;  /* as m355_measure_desc */
  const void* ref[3];                 /* as m355_measure_desc */
  int64_t     pitch[3];               /* as m355_measure_desc */
  int32_t     planes;                 /* bit p = measure plane p; 0 = every plane the frame has */
  int32_t     reserved[7];            /* 0 */
  void*       map[3];                 /* optional, device memory: int32 q per window, (pw - 10) per row, (ph - 10) rows; null = none */
  int64_t     map_pitch[3];           /* BYTES per row of map[]; a multiple of 4, >= 4 (pw - 10) */
} m355_ssim_desc;
typedef struct m355_ssim {
  int64_t  sum_q[3];
  uint64_t n[3];
  int32_t  min_q[3];
  double   ssim[3];
} m355_ssim;
M355_API int m355_frame_ssim_async(m355_ctx* ctx, int frame, const m355_ssim_desc* desc, unsigned long long* ticket);
M355_API int m355_frame_ssim_result(m355_ctx* ctx, unsigned long long ticket, int block, m355_ssim* out);
M355_API int m355_ssim_window(const uint64_t sums[5], int bit_depth, int32_t* q);   /* host only */
M355_API int m355_ssim_weights(int32_t w[11]);                                      /* host only */

/* MULTI-SCALE SSIM (Wang, Simoncelli, Bovik 2003) of a frame against another picture where both lie, per plane, on up to five levels, as a request
 * queued behind the frame's decode like m355_frame_ssim_async.  The definition is integer-exact and this library's own; it is stated here once.
 * PLANES, RECTANGLE, REFERENCE, a AND b are exactly those of m355_frame_ssim_async: each measured plane on its own grid, with the plane's own bit depth.
 * LEVELS.  levels = L, 1 .. M355_MSSSIM_LEVELS.  Level j (j = 0 .. L - 1) of a plane of the rectangle with pw x ph samples has (pw >> j) x (ph >> j)
 * samples.  Level 0 is the plane itself.  For j >= 1, with f = 1 << j and S(x, y) the sum of the f x f block of ORIGINAL samples whose first sample is
 * (f x, f y) relative to the rectangle's first sample:  a_j(x, y) = (S + f f / 2) >> 2j  — one rounding from the exact sum, the NATIVE formula of
 * m355_frame_export_scaled continued to j = 4, NOT a rounding of the level above.  Samples of the rectangle beyond f (pw >> j) columns or f (ph >> j)
 * rows do not take part in level j.  The same for b.  A level is a picture of the plane's bit depth.
 * PER LEVEL.  Valid windows only, ((pw >> j) - 10) x ((ph >> j) - 10) of them; weights and the five exact sums as at m355_frame_ssim_async; two points
 * per window from the same sums and the same intermediates, every double operation rounded by itself in the written order (no fused multiply-add):
 *   q   as at m355_frame_ssim_async (m355_ssim_window)
 *   cs = (2.0 cov + c2) / ((va + vb) + c2),   qc = clamp((int64)floor(cs 2^30 + 0.5), -2^30, 2^30)              (Q30; m355_ssim_window_cs)
 * RESULT per measured plane p and level j: sum_q[p][j], sum_cs[p][j] (exact, independent of order; either can be negative) and n[p][j], the number of
 * windows.  Levels >= L, planes that are not selected and planes the frame does not have read 0 in every field.
 * THE NUMBER is the host's, at collection, in IEEE double:  m_j = (double)sum_cs[p][j] / ((double)n[p][j] 2^30) for j < L - 1,
 * m_{L-1} = (double)sum_q[p][L-1] / ((double)n[p][L-1] 2^30);  m355_msssim_combine(m, L, weight, &out) multiplies, in level order from 1.0,
 * pow(max(m_j, 0.0), weight[j]).  weight == NULL stands for Wang's {0.0448, 0.2856, 0.3001, 0.2363, 0.1333} and is accepted for L == 5 only; they sum to
 * 1.0001 and are used as published.  msssim[p] is that value for L == 5 and 0.0 for fewer levels, which the caller combines with weights of their own.
 * Identical planes give exactly 1.0; a level whose mean is negative gives exactly 0.0.  The integers are the contract: msssim goes through the C library's
 * pow and may differ from another C library's by a few units in the last place.
 * ORDERING, VERDICTS AND COLLECTION are those of m355_frame_ssim_async: a READER of the frame and of ref_frame (a kind of its own), queued on the stream of
 * the frame's last writer behind ref_frame's last writer; a later decode into either frame waits for it; the host waits for nothing at enqueue, with the
 * one exception under SCRATCH.  *ticket counts 1, 2, ... per context (a count of its own); at most M355_MSSSIM_REQUESTS requests may be outstanding: one
 * more returns M355_ERR_BUSY and enqueues nothing.  m355_frame_msssim_result collects a request and frees its slot: block = 0 -> M355_ERR_BUSY while it
 * runs (the request stays), block = 1 -> the host waits for THAT request only.  M355_ERR_INVALID: an unknown or collected ticket; or — the request is
 * collected all the same — a request queued behind a decode whose lists were rejected, for either frame: it has read nothing.  m355_wait completes every
 * request and collects none; a frame may be destroyed with requests pending.
 * M355_ERR_INVALID, nothing enqueued: everything m355_frame_ssim_async rejects for handles, pointers, the rectangle, ref_frame, ref[] / pitch[], planes,
 * reserved and a tile-sharded context; levels outside 1 .. 5; a selected plane with (pw >> (levels - 1)) < 11 or (ph >> (levels - 1)) < 11.
 * SCRATCH.  The levels 1 .. L - 1 of both sides pass through device memory of the request's slot, in the frame's element type: a third of the pair's
 * bytes at most (66 MB for an 8K 10-bit 4:2:0 pair).  A slot's scratch is allocated when a request needs more than the slot holds, and kept: it grows
 * only and is freed with the context.  Such a request pays an allocation at enqueue, and where it replaces a smaller one, a free, which waits for the
 * device's queued work.  No sample of any level is produced or touched by the host; the originals are read from memory once per request.
 * HOST-ONLY HELPERS (exact, no context): m355_ssim_window_cs computes qc from sums = {MA, MB, SAA, SBB, SAB} for a bit depth 1..16;
 * m355_msssim_combine as above, from mean[0 .. levels - 1].  M355_ERR_INVALID: null pointers, a bit depth outside 1..16, levels outside 1..5, weight ==
 * NULL with levels != 5, a mean that is NaN, a weight that is negative or not finite.
 * Not offered: maps per level, other weights inside the call, more than five levels, border padding, a batch of frames, sharded contexts. */
#define M355_MSSSIM_REQUESTS 4
#define M355_MSSSIM_LEVELS   5
typedef struct m355_msssim_desc {
  int32_t     ref_frame;              /* as m355_ssim_desc */
  int32_t     x0, y0, width, height;  /* as m355_ssim_desc */
  const void* ref[3];                 /* as m355_ssim_desc */
  int64_t     pitch[3];               /* as m355_ssim_desc */
  int32_t     planes;                 /* as m355_ssim_desc */
  int32_t     levels;                 /* 1..5 */
  int32_t     reserved[6];            /* 0 */
} m355_msssim_desc;
typedef struct m355_msssim {
  int64_t  sum_q[3][M355_MSSSIM_LEVELS];
  int64_t  sum_cs[3][M355_MSSSIM_LEVELS];
  uint64_t n[3][M355_MSSSIM_LEVELS];
  double   msssim[3];
} m355_msssim;
M355_API int m355_frame_msssim_async(m355_ctx* ctx, int frame, const m355_msssim_desc* desc, unsigned long long* ticket);
M355_API int m355_frame_msssim_result(m355_ctx* ctx, unsigned long long ticket, int block, m355_msssim* out);
M355_API int m355_ssim_window_cs(const uint64_t sums[5], int bit_depth, int32_t* qc);                     /* host only */
M355_API int m355_msssim_combine(const double mean[5], int levels, const double* weight, double* out);   /* host only */

/* What is IN a frame, measured where it lies: histograms, the active area, the light level — what a tone mapper without metadata (a high percentile
 * of max(R, G, B)), a crop detector (the box of the content in letterboxed material) and a scene-cut / fade / black-frame detector (luma histograms and
 * means) need of every picture, in one pass over the planes and without a download.  A request queued behind the frame's decode, like
 * m355_frame_measure_async.  EVERYTHING IS AN INTEGER AND EXACT.
 * PLANES.  For each plane the frame has, over the samples s of the rectangle on THAT PLANE'S OWN GRID (no siting is known or needed):
 *   hist[p][b] = #{s : (s >> (bd - 8)) == b}, bd the PLANE's bit depth      min[p], max[p]      sum[p] = sum s      sum_sq[p] = sum s * s
 * A plane a monochrome frame does not have reads 0 in all of its fields.
 * ACTIVE AREA.  box = {x0, y0, x1, y1}, inclusive, in luma coordinates OF THE FRAME, around the luma samples of the rectangle that are > black;
 * n_active = how many there are; none: box = {-1, -1, -1, -1}, n_active = 0.
 * LIGHT (light == 1).  For every luma position of the rectangle, (R, G, B) is BY DEFINITION what m355_frame_export_rgb_opts delivers for that pixel
 * with samples = M355_RGB_U16, this matrix and full_range, and opts.chroma_loc = chroma_loc: the integers of m355_rgb_coefficients(..., M355_RGB_U16,
 * ...), the bilinear chroma reconstruction with indices clamped to the FRAME — a rectangle's values are those of the same rectangle of a whole-frame
 * request: its rim reads chroma outside the rectangle.  m = max(R, G, B); a monochrome frame gives m = R.
 *   light_hist[b] = #{pixels : (m >> 8) == b}      light_min, light_max = min m, max m      light_sum = sum m
 * No R'G'B' sample passes through memory.  With light == 0 these fields read 0.  Linear light is the host's: m355_stats_quantile on light_hist,
 * then m355_colour_linear on the bin's upper edge (below).
 * COUNT RANGE.  Counts are 32-bit: the largest frame, 16384 x 16384, has 2^28 samples per plane.
 * ORDERING AND VERDICTS are those of m355_frame_measure_async.  The request is a READER of the frame (a kind of its own): it runs on the stream of the
 * frame's last writer, and a later decode into the frame waits for it in front of its first write; the host waits for nothing at enqueue.  *ticket
 * counts 1, 2, ... per context (a count of its own); at most M355_STATS_REQUESTS requests may be outstanding: one more returns M355_ERR_BUSY and
 * enqueues nothing.  The slots are separate from the comparison and hash slots.
 * M355_ERR_INVALID, nothing enqueued: what m355_frame_measure_async rejects for the frame and the rectangle (bad handle; a rectangle that leaves the
 * frame or is off the chroma grid); a tile-sharded context; black outside 0 .. 2^bdl - 1; light not 0 or 1; with light == 1 an unknown matrix or
 * range, chroma_loc outside 0..3 or non-zero for a frame that is not 4:2:0; with light == 0 a non-zero matrix, full_range or chroma_loc; a non-zero
 * `reserved`; null pointers.
 * m355_frame_stats_result collects a request and frees its slot: block = 0 -> M355_ERR_BUSY while it runs (the request stays), block = 1 -> the
 * host waits for THAT request only.  M355_ERR_INVALID: an unknown or collected ticket; or — the request is collected all the same — a request
 * queued behind a decode whose lists were rejected: it has read nothing.  m355_wait completes every request and collects none; a frame may be
 * destroyed with requests pending.
 * HOST-ONLY HELPERS (exact, no context; csrc/stats_quantile.h and csrc/colour_transform.h are the one definition of each).
 *   m355_stats_quantile: the smallest bin b with den * (hist[0] + ... + hist[b]) >= num * total, total = the sum of all bins, in 64-bit arithmetic;
 *     0 < num <= den <= 1 << 20.  M355_ERR_INVALID: total == 0, num or den outside that, null pointers.
 *   m355_colour_linear: step 1 of m355_colour_pixel for one value — k = v16 >> 6, f = v16 & 63, *L = (lut_in[k] (64 - f) + lut_in[k + 1] f + 32) >> 6,
 *     the code m355_colour_pixel runs.  M355_ERR_INVALID: v16 > 65535, null pointers, tables outside their bounds.
 * Not offered: statistics in linear light on the device, per-channel R, G, B histograms, more than 256 bins, row and column profiles, a batch of
 * frames or several rectangles in one launch, sharded contexts. */
#define M355_STATS_REQUESTS 16
#define M355_STATS_BINS     256
typedef struct m355_stats_desc {
  int32_t x0, y0, width, height;   /* luma rectangle, rules of m355_measure_desc (width == 0: whole frame; on the chroma grid) */
  int32_t black;                   /* active area: luma samples > black count as content (sample units of the luma bit depth; 0 .. 2^bdl - 1) */
  int32_t light;                   /* 0: planes only; 1: also the R'G'B' light level */
  int32_t matrix, full_range;      /* light == 1: as in m355_rgb_desc; light == 0: must be 0 */
  int32_t chroma_loc;              /* light == 1: as in m355_export_opts (0..3, non-zero for 4:2:0 only); light == 0: must be 0 */
  int32_t reserved[7];             /* 0 */
} m355_stats_desc;
typedef struct m355_stats {
  uint32_t hist[3][M355_STATS_BINS];   /* per plane: samples with (s >> (bd - 8)) == bin, bd the PLANE's bit depth */
  uint32_t min[3], max[3];             /* sample values; a plane that does not exist: all of its fields 0 */
  uint64_t sum[3], sum_sq[3];          /* sum of s, sum of s * s */
  int32_t  box[4];                     /* x0, y0, x1, y1 (inclusive, luma coordinates IN THE FRAME) around the rectangle's luma samples > black; -1 x 4: none */
  uint64_t n_active;                   /* how many such samples */
  uint32_t light_hist[M355_STATS_BINS];/* light == 1: pixels with (m >> 8) == bin, m = max(R, G, B) of the pixel's 16-bit R'G'B'; else 0 */
  uint32_t light_min, light_max;       /* of m */
  uint64_t light_sum;                  /* sum of m */
} m355_stats;
M355_API int m355_frame_stats_async(m355_ctx* ctx, int frame, const m355_stats_desc* desc, unsigned long long* ticket);
M355_API int m355_frame_stats_result(m355_ctx* ctx, unsigned long long ticket, int block, m355_stats* out);
M355_API int m355_stats_quantile(const uint32_t hist[M355_STATS_BINS], uint32_t num, uint32_t den, int* bin);   /* host only */
M355_API int m355_colour_linear(const m355_colour_tables* tables, uint32_t v16, uint32_t* L);                    /* host only */

/* HOW a picture was coded, as dense maps in the caller's device memory: where the coding units are, which are intra, inter or skipped, the QP, the
 * transform tree, the intra modes, the motion field with its reference slots, the slices — what the reference shows through its per-picture arrays
 * (image.h get_pred_mode / get_QPY / get_mv_info ...) and a compressed-domain model, a quality-aware filter, a transcoder or a scene-cut detector
 * wants without a round trip over the host.  The request reads the work LISTS of one picture (cus, tus, pbs, ibs, ctbs), not a frame; no decode is
 * needed.  csrc/map_element.h is the one statement of the definition, for the kernels and for m355_maps_unit.  EVERYTHING IS AN INTEGER AND EXACT.
 * UNIT GRID.  U = 1 << log2_unit (2..6); units_w = ceil(pp.width / U), units_h = ceil(pp.height / U) (the coded size).  Unit (ux, uy) takes its
 * value at the luma position P = (ux * U, uy * U), which always lies inside the picture.  "The record covering P" is the record whose luma rectangle
 * contains P: x .. x + size for a CU, a TU and a luma intra block, x .. x + w, y .. y + h for a prediction block.  Every map is computed from its own
 * list only.  Elements are little-endian, a row is units_w elements, rows are pitch[m] bytes apart:
 *   M355_MAP_CU     u32     pred_mode | part_mode << 8 | log2_size << 16 | flags << 24 of the CU          no covering record: 0xFFFFFFFF
 *   M355_MAP_QP     i8      cu.qp_y                                                                        -128
 *   M355_MAP_TU     u8      tu.log2_size | 0x80 if M355_TUF_NONZERO_COEFF                                  0
 *   M355_MAP_INTRA  u8      ib.mode of the luma (cidx == 0) intra block without M355_IBF_PCM               255 (inter, PCM, uncovered)
 *   M355_MAP_MV     i16[4]  mv[0][0], mv[0][1], mv[1][0], mv[1][1]; a list's pair is 0, 0 unless its M355_PBF_PRED_Lx is set     all 0
 *   M355_MAP_REF    u8[4]   (u8)ref_slot[0] if M355_PBF_PRED_L0 else 0xFF; the same for L1; pb.flags; 0    FF FF 00 00
 *   M355_MAP_SLICE  u16     ctbs[CTB of P].slice_idx                                                       (always defined)
 * SKIPPED RECORDS.  The lists need not have been validated (lists recorded in place are checked on the device, by the decode).  A record that fails
 * the geometry clause of its record check (csrc/record_checks.h) is skipped and counted in skipped[]: for a CU, a TU and an intra block (of any
 * component) the whole `malformed` clause, for a prediction block m355_check_pb_geometry alone — reference slots do not matter here.  Positions need
 * not be aligned: a record covers exactly the positions P its rectangle contains.  Where valid records of one list overlap, a unit gets the value of
 * one of them, unspecified which.
 * SUMMARY (m355_maps_info).  units_w, units_h; from MAP_CU the units by pred_mode — n_intra, n_inter, n_skip — and covered, their sum; from MAP_QP
 * qp_sum, qp_min, qp_max over the covered units (none: 0, 127, -128); from MAP_REF n_bipred, the units whose prediction block has both PRED flags;
 * skipped[4], the cu, tu, pb and ib records skipped, counted for the lists the request read.  A field whose map was not requested reads as its empty
 * value.
 * THE REQUEST.  `handle` is a resident picture (m355_picture_upload / _replace) or M355_PICTURE_LAST, the lists of this context's most recent
 * m355_submit_picture.  dst[m] == NULL: map m is not wanted.  dst[m] is device memory or m355_host_alloc memory; pointer and pitch are multiples of
 * the element size (4, 1, 1, 1, 8, 4, 2) and need no more alignment; the pitch is at least the row's bytes.  Bytes beyond a row and rows beyond
 * units_h are never written.
 * ORDERING.  The host waits for nothing at enqueue.  All map requests of a context run in order on one stream of their own, behind the upload of
 * their lists; they delay no decode and none delays them (decodes only read the lists too).  m355_picture_replace, m355_picture_release, the reuse of
 * a submit arena (three rotate) and m355_destroy wait for the requests that read the lists they overwrite.  *ticket counts 1, 2, ... per context (a
 * count of its own); at most M355_MAPS_REQUESTS requests may be outstanding: one more returns M355_ERR_BUSY and enqueues nothing.
 * M355_ERR_INVALID, nothing enqueued, no slot taken, no byte written: a bad handle, M355_PICTURE_LAST before any submit, a tile-sharded context;
 * null desc or ticket, log2_unit outside 2..6, reserved != 0; all dst null, a pitch below the row, a misaligned pointer or pitch.
 * m355_picture_maps_result collects a request and frees its slot: block = 0 -> M355_ERR_BUSY while it runs (the request stays), block = 1 -> the host
 * waits for THAT request only; an unknown or collected ticket: M355_ERR_INVALID.  m355_picture_maps_order makes the consumer's stream wait for the
 * request instead of the host (the request stays to be collected).  m355_wait completes every request and collects none.
 * m355_maps_unit (host only, no context): element (ux, uy) of map `map` from HOST lists by a linear search — the same definition through the same
 * header; `element` receives the element's bytes (4, 1, 1, 1, 8, 4, 2).  M355_ERR_INVALID: null pointers, map or log2_unit out of range, a unit
 * outside the grid. */
#define M355_N_MAPS        7
#define M355_MAPS_REQUESTS 16
#define M355_PICTURE_LAST  (-1)   /* the lists of this context's most recent m355_submit_picture */
enum { M355_MAP_CU = 0, M355_MAP_QP = 1, M355_MAP_TU = 2, M355_MAP_INTRA = 3, M355_MAP_MV = 4, M355_MAP_REF = 5, M355_MAP_SLICE = 6 };
typedef struct m355_maps_desc {
  int32_t log2_unit, reserved;     /* 2..6; 0 */
  void*   dst[M355_N_MAPS];        /* device memory, or m355_host_alloc memory; NULL: not wanted */
  int64_t pitch[M355_N_MAPS];      /* bytes between rows */
} m355_maps_desc;                  /* (LP64: 120 bytes) */
typedef struct m355_maps_info {
  int32_t  units_w, units_h;
  uint32_t covered, n_intra, n_inter, n_skip;   /* MAP_CU: units by pred_mode, and their sum */
  int64_t  qp_sum;                              /* MAP_QP, over covered units */
  int32_t  qp_min, qp_max;                      /* none covered: 127, -128 */
  uint32_t n_bipred;                            /* MAP_REF: units whose prediction block has both PRED flags */
  uint32_t skipped[4];                          /* cu, tu, pb, ib records skipped (of the lists the request read) */
} m355_maps_info;                              /* (64 bytes) */
M355_API int m355_picture_maps_async(m355_ctx* ctx, int handle, const m355_maps_desc* desc, unsigned long long* ticket);
M355_API int m355_picture_maps_result(m355_ctx* ctx, unsigned long long ticket, int block, m355_maps_info* out);
M355_API int m355_picture_maps_order(m355_ctx* ctx, unsigned long long ticket, void* consumer_hipStream);
M355_API int m355_maps_unit(const m355_picture* pic, int map, int log2_unit, int ux, int uy, void* element);   /* host only */

/* Replaces (deferred): decode_TU (slice.cc:3460), decode_prediction_unit (motion.cc:2190) and
 * run_postprocessing_filters_sequential/_parallel (decctx.cc:1783/1811) for one picture. Asynchronous:
 * returns after the work is enqueued on the context's stream. */
M355_API int m355_submit_picture(m355_ctx* ctx, const m355_picture* pic);
/* Lists recorded IN PLACE: m355_arena_begin hands out, for the NEXT m355_submit_picture on this context, host pointers into
 * the context's pinned staging arena with room for `caps` entries per list (the caller sizes them from the previous
 * picture, say).  The parser's recorder threads write the lists there; the submitted m355_picture carries exactly those
 * pointers (pic->rbs = the 4x4 bin's region; the four size bins live in their own regions caps->rb_bin[0..3], filled in by
 * the call) and its real counts (<= the capacities): the submit then validates, derives its schedules and starts the
 * host-to-device copy without copying a byte on the host.  It waits for the picture that used this arena last (three arenas
 * rotate — measured: a longer ring gains nothing, the submitting thread is the bound).  dst_frame / ref_frames / pp / counts are the caller's to fill in. */
typedef struct m355_arena_caps {
  int32_t n_slices, n_ctbs, n_cus, n_tus, n_pbs, n_wts, n_ibs;
  int32_t n_rbs[4];
  uint32_t n_coeffs, n_pcm;
  int32_t scaling;                 /* 1: room for the scaling-factor tables */
  m355_rb* rb_bin[4];              /* out: where the residual blocks of each size go */
} m355_arena_caps;
M355_API int m355_arena_begin(m355_ctx* ctx, m355_arena_caps* caps, m355_picture* pic);
/* Host only (no GPU call, no context): a copy of the residual records and their coefficient list in which every block that can
 * take the 16-bit form has it (M355_RBF_NARROW: all positions < 256, all levels in [-128, 127]) and the others are copied as they
 * are.  A block without entries stays wide; a block that is already narrow is copied unchanged.
 * The list is compacted: each block's own range is copied, the blocks in the order they have in coeffs_in (equal offsets: the
 * order of the records).  The records are binned by size while the list is in decode order, so this order is what makes widening
 * the result again give coeffs_in back word for word.  The luma block a cross-component chroma block re-reads keeps its own range
 * and flag.
 * coeffs_out needs room for n_coeffs_in words and must not be coeffs_in; rbs_out may be rbs_in.  *n_coeffs_out = the words written.
 * M355_ERR_INVALID when a block's range leaves coeffs_in, or when blocks overlap so far that the copies of their ranges would
 * outgrow n_coeffs_in. */
M355_API int m355_pack_narrow(const m355_rb* rbs_in, int n_rbs, const uint32_t* coeffs_in, uint32_t n_coeffs_in,
                              m355_rb* rbs_out, uint32_t* coeffs_out, uint32_t* n_coeffs_out);
/* Blocks until all submitted work finished; returns M355_ERR_TIMEOUT if a device spin bound hit, M355_ERR_INVALID if a picture
 * recorded in place was rejected by the device-side list validation (the message names the picture's serial and the record; the
 * next call reports the next rejected picture, if any). */
M355_API int m355_wait(m355_ctx* ctx);
/* Per-picture outcome of asynchronous submits.  The record checks of lists recorded in place (m355_arena_begin) run on the device,
 * ahead of the picture's kernels: m355_submit_picture has returned M355_OK long before a rejection is known.  Every decode gets
 * a serial (1, 2, ...); m355_decode_status(serial) is non-blocking: M355_ERR_BUSY while the decode runs, M355_OK when it finished,
 * M355_ERR_INVALID when its lists were rejected — none of its kernels acted on them, the destination frame was NOT written
 * (m355_last_error names the record: the same checks and list names as for lists the library copies, which
 * m355_submit_picture rejects itself.  Two lists are numbered differently on the two paths: a residual block rejected at the submit is
 * numbered across the four size bins concatenated, one rejected on the device inside its own bin; and the device checks its sorted copy of
 * ibs, so an intra block's number there need not be the caller's).  Kept for the last 64 decodes (an older serial: M355_ERR_STALE — distinct from a rejection, which M355_ERR_INVALID stays for; a
 * rejection that left the ring unreported is still reported by the next m355_wait).  The caller marks the picture and whatever references it
 * as damaged (the reference does the same bookkeeping with de265_image::integrity, image.h:347). */
M355_API unsigned long long m355_last_serial(m355_ctx* ctx);      /* of the decode the last submit / decode call enqueued */
M355_API int m355_decode_status(m355_ctx* ctx, unsigned long long serial);

/* Resident work lists (benchmarks, replay): upload once, decode many times. */
M355_API int m355_picture_upload(m355_ctx* ctx, const m355_picture* pic);   /* -> handle >= 0 */
M355_API int m355_picture_release(m355_ctx* ctx, int handle);
/* other lists into an uploaded picture's arenas: waits for that handle's last decode only (no allocation when they fit) */
M355_API int m355_picture_replace(m355_ctx* ctx, int handle, const m355_picture* pic);
/* m355_arena_begin for the arenas of a RESIDENT picture: list pointers into the pinned arena of `handle` (-1: a new handle) with room
 * for `caps` entries; returns the handle (>= 0) or -error.  The recorder threads write the lists there and
 * m355_picture_replace(ctx, handle, pic) takes them over without copying a byte on the host (same rules as m355_submit_picture on
 * in-place lists).  This is the in-place path of a TILE-SHARDED context (m355_shard_set / m355_group_*), whose pictures are decoded
 * from handles; there `pp` — the picture's parameters, known before its lists are recorded — sizes the room for the border units
 * of the other ranks behind cus[] / pbs[] (unsharded contexts ignore it; the lists of a sharded picture are checked on the host). */
M355_API int m355_picture_arena_begin(m355_ctx* ctx, int handle, m355_arena_caps* caps, const m355_pic_params* pp, m355_picture* pic);
M355_API int m355_decode_resident(m355_ctx* ctx, int handle);
/* n independent INTRA pictures (n <= pipeline depth, distinct destination frames, one chroma format and sample type) with ONE intra
 * stage: each picture's residuals / border plans and its filters run on a lane of its own as for n m355_decode_resident calls, the
 * CTB wavefronts of all n run interleaved inside one k_intra launch — the way all-intra material (the reference's decode_CTB loop
 * over intra slices, slice.cc:4375 read_coding_tree_unit -> intrapred.cc:279 decode_intra_prediction, one picture at a time) fills
 * the GPU without one hardware queue per picture.  The pictures get consecutive serials (m355_last_serial = the last one's);
 * results are those of n single decodes, bit for bit.  Not stage-timed (m355_timing_collect sees single decodes only). */
M355_API int m355_decode_batch(m355_ctx* ctx, const int* handles, int n);
/* stage mask for m355_set_stages: run only part of the chain (stage-isolated parity, like
 * DE265_DECODER_PARAM_DISABLE_DEBLOCKING / _DISABLE_SAO, de265.h:409-410) */
enum { M355_STAGE_INTER = 1, M355_STAGE_RESIDUAL = 2, M355_STAGE_INTRA = 4, M355_STAGE_DEBLOCK = 8,
       M355_STAGE_SAO = 16, M355_STAGE_ALL = 31 };
M355_API int m355_set_stages(m355_ctx* ctx, int stage_mask);
/* Pictures in flight (1..32): 1 (default) = one after the other on the context's stream; n = consecutive decodes go
 * round n lanes (own streams, working planes, scratch) and overlap wherever the frames they touch allow: a decode
 * waits for the last writer of each reference frame it reads and, right before its own first write, for the last writer
 * and the readers of its destination frame.  (The reference decodes independent pictures concurrently too: frame-parallel
 * image units, decctx.cc:605-630.)  Three is the sweet spot for inter pictures; an all-intra stream (dependency-bound k_intra,
 * a fraction of the GPU per picture) gains up to nine: intra pictures on lanes 3.. run on streams of other priority classes, which
 * the HIP runtime gives hardware queues of their own (M355_LANE_PRIORITIES=0 turns that off). */
M355_API int m355_set_pipeline_depth(m355_ctx* ctx, int depth);

/* ------------------------------------------------------------------------------------------------
 * Tile sharding across GPUs (one process per GPU).  Tiles are independent for
 * prediction (intrapred.h:499-508 stops availability at tile borders) but coupled by the in-loop
 * filters when pps.loop_filter_across_tiles_enabled_flag is set (deblock.cc:191-209, sao.cc:158-163)
 * and by motion vectors that reach into other tiles of the reference pictures.  A sharded context
 * owns the tiles t (tile-scan order) with  t * nranks / n_tiles == rank  and is given work lists
 * that hold ONLY its tiles' CUs / TUs / PBs / residual / intra blocks (slices[] and ctbs[] stay
 * picture-wide: the filters read the neighbours' slice flags).  One picture then runs as five phases
 * with an exchange between them; the exchange buffers are CALLER-owned device memory (so the host
 * layer can hand them to RCCL / torch.distributed), all 32-bit-word arrays in a canonical,
 * rank-independent layout in which every element is produced by exactly one rank and is ZERO on all
 * others — an integer SUM all-reduce (or any owner -> neighbour point-to-point copy) completes them:
 *
 *   phase 0  k_meta, k_inter, k_residual, k_intra on the own tiles;
 *            pack X0 = border-unit metadata (QP_Y, PredMode, pcm/bypass, PBMotion, edge + cbf flags of
 *            every 4x4 unit next to an interior tile boundary) + the 4-luma / 2-chroma-sample column
 *            strips either side of every vertical tile boundary, PRE-deblock        -> exchange X0
 *   phase 1  unpack X0 (foreign units appear as local metadata), deblock vertical edges (a boundary edge
 *            is computed by both owners, each writes only its own side); pack X1 = row strips either
 *            side of every horizontal tile boundary, post-vertical-pass             -> exchange X1
 *   phase 2  unpack X1, deblock horizontal edges; pack X2 = column + row strips, deblocked (the
 *            1-sample ring incl. corners that SAO edge classes read)                -> exchange X2
 *   phase 3  unpack X2, SAO into the destination frame (own tiles); pack X3[rank] = own tiles of the
 *            destination frame                                                      -> all-gather X3
 *   phase 4  unpack X3: the destination frame is complete on every rank (reference for later pictures).
 * ---------------------------------------------------------------------------------------------- */
M355_API int m355_shard_set(m355_ctx* ctx, int rank, int nranks);      /* nranks == 0: sharding off (default) */
/* rank owning tile t (tile-scan order) — pure function, the partition rule above */
M355_API int m355_shard_owner_of_tile(int tile, int n_tiles, int nranks);
/* byte size of exchange buffer `which` (0..3) for a resident picture; X3 = nranks equal slots
 * (this rank's slot is [rank*bytes/nranks, (rank+1)*bytes/nranks)).  Multiples of 4. */
M355_API int64_t m355_shard_xbuf_bytes(m355_ctx* ctx, int handle, int which);
/* run one phase (0..4) of a resident picture; xbuf = the buffer the phase packs into (phases 0..3) —
 * the buffer it unpacks is the one passed to the previous phase, which must still be valid and hold
 * the exchanged contents.  Asynchronous.  With m355_set_pipeline_depth(ctx, n >= 2) consecutive pictures run on n lanes: phase 0
 * takes the next lane, the later phases of a picture follow it there, frame hazards are ordered as for m355_decode_resident —
 * the exchanges and filter phases of one picture overlap the prediction phase of the next.  After every call m355_stream() is
 * the stream of the picture's lane: order the exchange that follows on it.
 * A REFERENCE picture is complete only after phase 4 (phase 3 marks the destination frame written with the own tiles only): issue
 * its phase 4 before phase 0 of any picture that reads it — m355_decode_sharded and libde265_amd/shard.py do, they issue a picture's
 * phases back to back. */
M355_API int m355_decode_phase(m355_ctx* ctx, int handle, int phase, void* xbuf);

/* The whole sharded picture in ONE call: the five phases with the exchanges between them, issued from the library (C++; no
 * interpreter between the launches).  The exchange buffers live in the library; the exchanges go through a small callback table,
 * each called in issue order with the stream of the picture's lane (whatever it enqueues on that stream is ordered between the
 * phase that packed the buffer and the phase that unpacks it):
 *   halo_sum    buf holds this rank's elements of X0 / X1 / X2 (zero elsewhere): make it the SUM over this rank and `peers` — the
 *               ranks that own a tile touching one of this rank's (edge or corner; the only producers of what this rank reads,
 *               deblock.cc:191-209, sao.cc:158-163); scratch = room for one buffer per peer
 *   all_gather  X3: nranks slots of slot_bytes, slot `rank` filled -> all slots
 * m355_shard_rccl_init installs the built-in RCCL implementation (librccl is loaded at that moment; neighbour ncclSend / ncclRecv
 * in one group + one add kernel, ncclAllGather in place): one process per GPU, the unique id travels over the application's own
 * bootstrap channel.  Tests install callbacks over another transport (gloo).  gather = 0: a non-reference picture (no X3). */
typedef struct m355_comm {
  void* user;
  int (*halo_sum)(void* user, void* buf, size_t bytes, const int* peers, int n_peers, void* scratch, void* stream);
  int (*all_gather)(void* user, void* buf, size_t slot_bytes, int rank, int nranks, void* stream);
} m355_comm;
M355_API int m355_shard_set_comm(m355_ctx* ctx, const m355_comm* comm);
M355_API int m355_decode_sharded(m355_ctx* ctx, int handle, int gather);
M355_API int m355_rccl_unique_id(void* out128);                                  /* rank 0: ncclGetUniqueId (128 bytes) */
M355_API int m355_shard_rccl_init(m355_ctx* ctx, const void* id128, int rank, int nranks);   /* m355_shard_set + an RCCL communicator on the context's device */
/* The same exchanges between the rank PROCESSES of one node without a collective library (csrc/runtime_ipc.hip): every rank's exchange buffers are
 * exported with hipIpcGetMemHandle through a POSIX shared-memory segment named after `name` (a job-unique string, the same on every rank; rank 0
 * creates the segment) and mapped by their readers — X0..X2: a rank fetches its neighbours' buffers and adds; X3: a rank copies every other rank's
 * finished tiles straight out of that rank's gather buffer (N - 1 concurrent peer reads, one per xGMI link) — ordered by interprocess events
 * (M355_IPC_HOST_SYNC=1: by draining the recording stream instead) and per-rank sequence words in the segment.  Every rank must decode the same
 * pictures in the same order with the same handle numbers (at most 32 handles with exchange buffers, 16 ranks).  m355_shard_set + the callbacks
 * of m355_decode_sharded; needs HSA_ENABLE_IPC_MODE_LEGACY=0 where the driver only has dmabuf IPC.  M355_IPC_TIMEOUT=<seconds> (default 30)
 * bounds every wait for another rank. */
M355_API int m355_shard_ipc_init(m355_ctx* ctx, const char* name, int rank, int nranks);
M355_API int m355_shard_ipc_close(m355_ctx* ctx);
/* collective self-test of that transport: `words` 32-bit words through the halo exchange (every other rank as peer; a lone rank
 * sends to itself) and the all-gather, verified on the host */
M355_API int m355_shard_rccl_selftest(m355_ctx* ctx, size_t words);
/* Tile sharding inside ONE process (no collective library): a group of contexts — one per device, or several on one device —
 * decodes one picture; rank r = position in `ctxs`.  Each context gets its share of the picture with m355_picture_upload (after
 * m355_group_create, which calls m355_shard_set(ctx, r, n)); m355_group_decode(handles[r]) issues every rank's phases and moves
 * the halo buffers / finished tiles between the contexts with hipMemcpyPeerAsync ordered by events on their own streams.
 * Asynchronous like m355_decode_sharded; m355_wait on every context to finish.  This is what a decoder that parses one
 * bitstream with a thread per tile uses to spread the tiles over the GPUs of a node (deblock.cc:191-209, sao.cc:158-163 are
 * the couplings the exchanges carry). */
typedef struct m355_group m355_group;
M355_API int m355_group_create(m355_ctx* const* ctxs, int n, m355_group** out);
M355_API void m355_group_destroy(m355_group* group);
M355_API int m355_group_decode(m355_group* group, const int* handles, int gather);
/* device time (ms) of exchange `which` (0..3) of a sharded picture's buffers over the installed transport, averaged over `iters` runs;
 * collective: every rank calls it alike, after at least one m355_decode_sharded of the picture */
M355_API int m355_shard_time_exchange(m355_ctx* ctx, int handle, int which, int iters, float* ms_each);
/* the ranks `rank` exchanges halos with for these picture parameters (-> count, peers[] filled up to max_peers) */
M355_API int m355_shard_peers(const m355_pic_params* pp, int rank, int nranks, int* peers, int max_peers);

/* Per-stage device timing from HIP events recorded on the context's OWN stream around every decode
 * enqueued between m355_timing_reset() and m355_timing_collect(): averages in milliseconds, stage order
 * [meta, inter, residual, intra, deblock, sao]. m355_timing_collect() waits for the work and ends the window: decodes outside a
 * window record no stage events (seven event packets per picture are a diagnostic, not part of the decode). */
M355_API int m355_timing_reset(m355_ctx* ctx);
M355_API int m355_timing_collect(m355_ctx* ctx, int* n_decodes, float* total_ms, float stage_ms[6]);
M355_API void* m355_stream(m355_ctx* ctx);   /* hipStream_t of the context's active lane (the lane of the last decode / phase call) */

#ifdef __cplusplus
}
#endif
#endif /* DE265_MI355X_H */
