/* k_maps.h — arguments of the side-map kernels (k_maps.hip), shared with runtime_maps.hip */
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <hip/hip_runtime.h>
#include "de265_mi355x.h"
#include "map_element.h"

#define MAPS_RASTER_BLOCK 256 /* threads of a workgroup of the raster pass: four wavefronts, 64 records each */
#define MAPS_BLOCK 1024       /* threads of a workgroup of the gather pass: sixteen wavefronts share one summary record and one arrival ticket */
#define MAPS_WAVES (MAPS_BLOCK / 64)
#define MAPS_PART_WORDS 12    /* words of a workgroup's summary record (MAPS_COVERED .. MAPS_BIPRED, padded: the 64-bit sum stays 8-byte aligned) */

/* The summary as 32-bit words: a workgroup's record (MAPS_PART_WORDS of them, in MapsArgs::part) and the slot's pinned record.  Every encoding's
   neutral value is 0:
     MAPS_QP_MIN  128 - min qp_y (1 .. 256), gathered with max      MAPS_QP_MAX  max qp_y + 129 (1 .. 256)      0: no unit covered
   The pinned record: [MAPS_ARRIVED] = 1 when the request's values are in, [MAPS_ARRIVED + 1] its sequence number.  The slot's DEVICE record uses
   MAPS_SKIPPED (added by the raster pass) and MAPS_ARRIVED (the gather pass's arrival counter) only; the kernels leave it zero. */
enum {
  MAPS_COVERED = 0, MAPS_INTRA = 1, MAPS_INTER = 2, MAPS_SKIP = 3,
  MAPS_QP_SUM = 4,              /* 64 bit, two's complement */
  MAPS_QP_MIN = 6, MAPS_QP_MAX = 7, MAPS_BIPRED = 8,
  MAPS_SKIPPED = 9,             /* 4: cu, tu, pb, ib */
  MAPS_VALUES = 13,             /* what the last workgroup moves */
  MAPS_ARRIVED = 13,
  MAPS_REC_WORDS = 16
};

/* The scratch of a request: planes on the 4x4 grid of the picture, rows of `sp` cells (w4 rounded up to 4, so that a lane's four cells are one aligned
   16-byte load), zero before the raster pass.  A plane the request does not need is null. */
struct MapsArgs {
  M355MapGrid g;
  M355RecLimits lim;
  int32_t sp;                   /* cells per scratch row */
  uint32_t* s_cu;               /* CU index + 1 */
  uint32_t* s_pb;               /* PB index + 1 */
  uint8_t* s_tu;                /* the MAP_TU element */
  uint8_t* s_ib;                /* mode + 1 of the luma intra block that is shown */
  const m355_cu* cus; const m355_tu* tus; const m355_pb* pbs; const m355_ib* ibs; const m355_ctb* ctbs;
  int32_t n_cus, n_tus, n_pbs, n_ibs;          /* of the lists the request reads (0: not read) */
  uint32_t wg_end[4];           /* raster pass: the workgroups of the cu, tu, pb, ib lists end here (one wavefront per 64 records) */
  uint8_t* dst[M355_N_MAPS];    /* null: not wanted */
  long long pitch[M355_N_MAPS];
  uint32_t quads;               /* gather pass: lanes per row of units = ceil(units_w / 4) */
  uint32_t n_wg;                /* gather pass: workgroups; each draws one arrival ticket */
  uint32_t* part;               /* gather pass: n_wg summary records, one per workgroup (scratch; every workgroup writes all of its own) */
  uint32_t* rec;                /* the slot's device record */
  uint32_t* res;                /* the slot's pinned record */
  uint32_t seq;
};

/* both passes of one request, behind each other on `st` (the scratch is zero when the first starts) */
void m355_launch_maps(const MapsArgs& a, hipStream_t st);
