/* k_stats.h — arguments of the frame-statistics kernel (k_stats.hip), shared with runtime_stats.hip */
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <hip/hip_runtime.h>
#include "de265_mi355x.h"

#define STATS_BLOCK 1024      /* threads of a workgroup: 16 wavefronts, each with histograms of its own in LDS */
#define STATS_WAVES (STATS_BLOCK / 64)
#define STATS_LIGHT_WEIGHT 3      /* a LIGHT unit loads a luma vector and up to four chroma vectors and converts every pixel: about three PLANES units */
#define STATS_TARGET_WAVES 4096   /* wavefronts a launch is cut into at most (plus idle ones that fill a part's last workgroup): one workgroup per CU of 256 */

/* A PART of a launch is what whole workgroups work on: the rectangle on one plane's grid (PLANES), or the rectangle's luma positions with the
   chroma around them (LIGHT, which takes plane 0's statistics along: it holds every luma vector anyway).  A part is cut into UNITS — one
   64-lane chunk (1 KB) of one row — and a wavefront takes `units_per_wave` consecutive ones (a LIGHT unit counts as STATS_LIGHT_WEIGHT units when the wavefronts are shared out). */
struct StatsPart {
  const uint8_t* p;             /* PLANES: the rectangle's first sample on this plane (LIGHT reads through StatsArgs::src) */
  long long pitch;              /* bytes between rows */
  uint32_t row_bytes, rows;     /* of the rectangle on this plane; rows == 0: the part does not exist */
  uint32_t chunks, units;       /* chunks per row, chunks * rows */
  uint32_t units_per_wave;      /* consecutive units a wavefront of this part takes */
  uint32_t first_wg;            /* the part's first workgroup */
  uint32_t shift;               /* bit depth of the plane - 8: bin = sample >> shift */
};
struct StatsArgs {
  StatsPart part[3];            /* plane 0 (with light == 1: the LIGHT part), 1, 2 */
  uint32_t n_wg;                /* workgroups of the launch; each draws one arrival ticket */
  uint32_t px, py;              /* the rectangle's first luma sample IN THE FRAME: what the box is reported in */
  uint32_t black;               /* luma samples > black count as content */
  /* LIGHT (the member names d_rgb_load of k_rgb_dev.h reads): the FRAME's planes, pitches in bytes, the chroma plane's size */
  const uint8_t* src[3];
  long long src_pitch[2];
  uint32_t cw, ch;
  uint32_t x0, y0, width, height;
  m355_rgb_coeffs k;            /* m355_rgb_coefficients(..., M355_RGB_U16, ...) */
};

/* One REQUEST (m355_frame_stats_async), shaped like a comparison request (k_measure.h): the launch reduces into the slot's device record, the
   workgroup that arrives last moves it into the slot's pinned record and leaves the device record zero.  32-bit words; the 64-bit sums lie on
   even word indices and are added as 64-bit words.  Every encoding's neutral value is 0:
     STATS_MIN  ~min (a sample is below 2^16: ~s is never 0)        STATS_MAX  max        [3] of both: of the light values m
     STATS_BOX  ~x0, ~y0, x1 + 1, y1 + 1, each gathered with max     0: no sample above `black` */
enum {
  STATS_HIST = 0,               /* 4 x 256: planes 0..2, light */
  STATS_SUM = 1024,             /* 4 x 64 bit: planes 0..2, light */
  STATS_SQ = 1032,              /* 3 x 64 bit */
  STATS_NACT = 1038,            /* 64 bit */
  STATS_MIN = 1040,             /* 4 */
  STATS_MAX = 1044,             /* 4 */
  STATS_BOX = 1048,             /* 4 */
  STATS_VALUES = 1052,          /* what the last wavefront moves */
  STATS_ARRIVED = 1052,         /* device record: the arrival counter.  Pinned record: [1052] STATS_RES_* state, [1053] the request's sequence number */
  STATS_REC_WORDS = 1056
};
enum { STATS_RES_NONE = 0, STATS_RES_VALID = 1, STATS_RES_GATED = 2 };
struct StatsReq {
  uint32_t* rec;
  uint32_t* res;
  const uint32_t* timeout;      /* the gate of the decode that wrote the frame (M355_GATE): a gated request writes STATS_RES_GATED, nothing else */
  uint32_t epoch;
  uint32_t seq;
};

/* bytes_per_sample: 1 or 2 (of every plane of the frame); light: 0 / 1; chroma_format 0..3 and chroma_loc 0..3 (4:2:0 only) matter with light == 1 */
void m355_launch_stats(const StatsArgs& a, const StatsReq& q, int bytes_per_sample, int light, int chroma_format, int chroma_loc, hipStream_t st);
