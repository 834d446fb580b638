/* k_hash.h — arguments of the picture-hash kernels (k_hash.hip), shared with runtime.hip */
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <hip/hip_runtime.h>

struct HashPlane {
  const uint8_t* base;
  size_t pitch;        /* bytes between rows */
  int row_bytes;       /* message bytes per row: width * bytes per sample */
  int h;
  int bpp;             /* bytes per sample (1 or 2) */
};
struct HashArgs {
  HashPlane pl[3];
  int first[4];        /* first wave of plane 0,1,2 and the total */
  int rows_per_wave;
  uint32_t* out;       /* 3 accumulators, zeroed by the caller on the same stream */
};

/* One hash REQUEST (m355_frame_hash_async): the launch reduces into the request slot's own device record, the wavefront that arrives
   last moves the values into the slot's pinned record and leaves the device record zero — no fill before, no copy after. */
#define HASH_REC_WORDS 4     /* device record: accumulators of planes 0..2, arrival counter */
#define HASH_RES_WORDS 8     /* pinned record: values of planes 0..2, HASH_RES_* state, the request's sequence number */
enum { HASH_RES_NONE = 0, HASH_RES_VALID = 1, HASH_RES_GATED = 2 };
struct HashReq {
  uint32_t* rec;             /* HashArgs::out of the launch points at the same record */
  uint32_t* res;
  const uint32_t* timeout;   /* the gate of the decode that wrote the frame (M355_GATE): a gated request writes HASH_RES_GATED, nothing else */
  uint32_t epoch;
  uint32_t seq;
};

void m355_launch_frame_hash(const HashArgs& a, int type, hipStream_t st);
void m355_launch_frame_hash_req(const HashArgs& a, const HashReq& q, int type, hipStream_t st);   /* type M355_HASH_MD5: the gate's verdict only */
uint32_t m355_crc_init_term(uint64_t nbytes);     /* init * x^(8 nbytes): what the host XORs onto the device accumulator */
void m355_md5_rows(const uint8_t* data, size_t pitch, int row_bytes, int h, uint8_t out[16]);
