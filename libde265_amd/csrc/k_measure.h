/* k_measure.h — arguments of the frame-comparison kernel (k_measure.hip), shared with runtime.hip */
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <hip/hip_runtime.h>

/* one plane of the rectangle: `a` the frame's samples, `b` the reference's, both at the rectangle's first sample */
struct MeasPlane {
  const uint8_t* a;
  const uint8_t* b;
  long long pitch_a, pitch_b;   /* bytes between rows */
  int row_bytes;                /* bytes of a row of the rectangle: width * bytes per sample */
  int h;                        /* rows of the rectangle */
  int px, py;                   /* the rectangle's first sample in plane coordinates of the frame (m355_measure::first_x / first_y) */
  int row0;                     /* this plane's first entry of the request's row array */
};
struct MeasArgs {
  MeasPlane pl[3];
  int first[4];                 /* first wave of plane 0,1,2 and the total (= the number of arrivals) */
  int rows_per_wave;
};

/* One REQUEST (m355_frame_measure_async), shaped like a hash request (k_hash.h): the launch reduces into the request slot's device record, the
   wavefront that arrives last moves the values into the slot's pinned record and leaves the device record zero.  64-bit words. */
enum { MEAS_SSD = 0, MEAS_SAD, MEAS_NDIFF, MEAS_MAX, MEAS_FIRST, MEAS_PER_PLANE };   /* MEAS_FIRST: ~(y << 32 | x) of the raster-first differing sample, 0: none */
#define MEAS_REC_WORDS 16     /* device record: MEAS_PER_PLANE words of planes 0..2, arrival counter */
#define MEAS_RES_WORDS 24     /* pinned record: the same 15 values, [15] MEAS_RES_* state, [16] the request's sequence number */
enum { MEAS_RES_NONE = 0, MEAS_RES_VALID = 1, MEAS_RES_GATED = 2 };
struct MeasReq {
  unsigned long long* rec;
  unsigned long long* res;
  unsigned long long* rows;    /* pinned: per row of every plane the row's sum of squared differences (MeasPlane::row0 + y) */
  const uint32_t* timeout[2];  /* the gates of the decodes that wrote the frame and the reference frame (M355_GATE): a gated request writes MEAS_RES_GATED, nothing else */
  uint32_t epoch[2];
  uint32_t seq;
};

void m355_launch_measure(const MeasArgs& a, const MeasReq& q, int bytes_per_sample, hipStream_t st);
