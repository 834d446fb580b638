/* k_msssim.h — arguments of the MS-SSIM kernels (k_msssim.hip), shared with runtime_msssim.hip.  Tiles and workgroups are those of k_ssim.h. */
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <hip/hip_runtime.h>
#include "k_ssim.h"

#define MSSSIM_LEVELS 5       /* M355_MSSSIM_LEVELS */

/* LAUNCH 1, one measured plane of the rectangle: level 0 is measured, and levels 1 .. levels - 1 of both sides are written to the slot's scratch.
   a1 .. a4 / b1 .. b4: level 1 .. 4, (pw >> j) elements per row, rows packed ((pw >> j) * sizeof(element) bytes apart), (ph >> j) rows. */
struct MsssimPlane {
  const uint8_t* a;
  const uint8_t* b;
  long long pitch_a, pitch_b;   /* bytes between rows */
  int pw, ph;                   /* samples of the rectangle on this plane */
  int tiles_x;                  /* tiles per row of tiles, by SAMPLES: ceil(pw / SSIM_TILE_W); 0: not measured */
  int acc;                      /* the plane's first accumulator: MSSSIM_LEVELS * p */
  double c1, c2;
  uint8_t *a1, *a2, *a3, *a4;   /* (members, not arrays: the kernel picks the plane by a computed index and keeps the copy in registers) */
  uint8_t *b1, *b2, *b3, *b4;
};
struct MsssimArgs {
  MsssimPlane pl[3];
  int first[4];                 /* first workgroup of plane 0,1,2 and the launch's total */
  int levels;
  int arrivals;                 /* workgroups of BOTH launches: who draws the last ticket moves the record */
};

/* LAUNCH 2, one (plane, level >= 1): two packed pictures in scratch, tiles by WINDOWS as in k_ssim.hip */
struct MsssimLevel {
  const uint8_t* a;
  const uint8_t* b;
  int pw, ph;                   /* samples of the level; the pitch is pw elements */
  int tiles_x;
  int acc;                      /* MSSSIM_LEVELS * p + j */
  double c1, c2;
};
#define MSSSIM_ENTRIES (3 * (MSSSIM_LEVELS - 1))
struct MsssimLevelArgs {
  MsssimLevel lv[MSSSIM_ENTRIES];
  int first[MSSSIM_ENTRIES + 1];   /* first workgroup of entry 0 .. n - 1, and the launch's total at [n] */
  int n;
  int arrivals;
};

/* One REQUEST (m355_frame_msssim_async), shaped like an SSIM request: 64-bit words, two's complement sums, neutral value 0.
   Device record: [MSSSIM_Q + 5 p + j] the sum of q, [MSSSIM_CS + 5 p + j] the sum of qc, [31] the arrival counter of both launches.
   Pinned record: the thirty values, [30] MSSSIM_RES_* state, [31] the request's sequence number. */
enum { MSSSIM_Q = 0, MSSSIM_CS = 3 * MSSSIM_LEVELS, MSSSIM_VALUES = 6 * MSSSIM_LEVELS };
#define MSSSIM_REC_WORDS 32
enum { MSSSIM_RES_NONE = 0, MSSSIM_RES_VALID = 1, MSSSIM_RES_GATED = 2 };
struct MsssimReq {
  unsigned long long* rec;
  unsigned long long* res;
  const uint32_t* timeout[2];   /* as SsimReq */
  uint32_t epoch[2];
  uint32_t seq;
};

/* bytes_per_sample: 1 or 2.  lv.n == 0 (levels == 1): one launch */
void m355_launch_msssim(const MsssimArgs& a, const MsssimLevelArgs& lv, const MsssimReq& q, int bytes_per_sample, hipStream_t st);
