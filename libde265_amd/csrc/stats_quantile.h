/*
 * stats_quantile.h — the ONE definition of m355_stats_quantile (include/de265_mi355x.h): the smallest bin b of a 256-bin histogram with
 * den * (hist[0] + ... + hist[b]) >= num * total, in 64-bit integers (total < 2^32 * 256 = 2^40, num, den <= 2^20: products below 2^60).
 * Plain C++, compiled into the library (runtime_stats.hip) and into whatever host code wants the same answer without it, as resize_taps.h and
 * colour_transform.h are.
 */
#ifndef M355_STATS_QUANTILE_H
#define M355_STATS_QUANTILE_H

#include <stdint.h>

/* -> the bin, or -1: null histogram, total == 0, or not 0 < num <= den <= 1 << 20 */
static inline int m355_sq_quantile(const uint32_t* hist, uint32_t num, uint32_t den)
{
  if (!hist || num == 0 || num > den || den > (1u << 20)) return -1;
  uint64_t total = 0;
  for (int b = 0; b < 256; b++) total += hist[b];
  if (!total) return -1;
  uint64_t run = 0;
  for (int b = 0; b < 256; b++) {
    run += hist[b];
    if ((uint64_t)den * run >= (uint64_t)num * total) return b;
  }
  return 255;   /* (not reached: run == total at b = 255 and num <= den) */
}

#endif
