/* k_ssim.h — arguments of the SSIM kernel (k_ssim.hip), shared with runtime_ssim.hip */
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <hip/hip_runtime.h>

#define SSIM_TILE_W 32        /* windows of one workgroup: SSIM_TILE_W x SSIM_TILE_H, from (SSIM_TILE_W + 10) x (SSIM_TILE_H + 10) samples of either side */
#define SSIM_TILE_H 32
#define SSIM_BLOCK 1024       /* threads of a workgroup: sixteen wavefronts share one tile's LDS (measured against 256 and 512: profiles/ssim_bench.txt) */

/* one plane of the rectangle: `a` the frame's samples, `b` the reference's, both at the rectangle's first sample.  tiles_x == 0: not measured */
struct SsimPlane {
  const uint8_t* a;
  const uint8_t* b;
  long long pitch_a, pitch_b;   /* bytes between rows */
  int pw, ph;                   /* samples of the rectangle on this plane: (pw - 10) x (ph - 10) windows */
  int tiles_x;                  /* tiles per row of tiles */
  double c1, c2;                /* m355_ssim_c1 / m355_ssim_c2 of the plane's bit depth (ssim_window.h) */
  uint8_t* map;                 /* null, or int32 q per window: row j at map + j * map_pitch */
  long long map_pitch;
};
struct SsimArgs {
  SsimPlane pl[3];
  int first[4];                 /* first workgroup of plane 0,1,2 and the total (= the number of arrivals) */
};

/* One REQUEST (m355_frame_ssim_async), shaped like a comparison request (k_measure.h): the launch reduces into the request slot's device record, the
   workgroup that arrives last moves the values into the slot's pinned record and leaves the device record zero.  64-bit words.  Every encoding's
   neutral value is 0: the sums are added as two's complement, and the worst window is kept as max (2^30 - q), 0 .. 2^31. */
enum { SSIM_SUM = 0, SSIM_WORST = 3, SSIM_VALUES = 6 };   /* [SSIM_SUM + p], [SSIM_WORST + p] of plane p */
#define SSIM_REC_WORDS 8      /* device record: the six values, [7] the arrival counter.  Pinned record: the six values, [6] SSIM_RES_* state, [7] the request's sequence number */
enum { SSIM_RES_NONE = 0, SSIM_RES_VALID = 1, SSIM_RES_GATED = 2 };
struct SsimReq {
  unsigned long long* rec;
  unsigned long long* res;
  const uint32_t* timeout[2];  /* the gates of the decodes that wrote the frame and the reference frame (M355_GATE): a gated request writes SSIM_RES_GATED, nothing else */
  uint32_t epoch[2];
  uint32_t seq;
};

/* bytes_per_sample: 1 or 2 (of every plane of the frame) */
void m355_launch_ssim(const SsimArgs& a, const SsimReq& q, int bytes_per_sample, hipStream_t st);
