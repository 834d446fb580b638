/*
 * orientation.h — the ONE definition of the orientations of m355_frame_export_oriented and m355_frame_export_pixels_oriented (include/de265_mi355x.h,
 * M355_ORIENT_*), for the kernels (k_export_oriented.hip), their SIMT-interpreter build and the host (runtime_export.hip: the argument checks,
 * m355_orientation_compose, m355_orientation_from_exif).  Plain C++ apart from the qualifier, like pixel_pack.h and map_element.h.
 *
 * An orientation o is 0..7, three bits: TRANSPOSE (rows and columns exchanged) is applied FIRST, then FLIP (rows reversed), then MIRROR (columns
 * reversed).  A source rectangle S of w columns and h rows of elements becomes D of W' x H' = h x w with TRANSPOSE, else w x h, and for every (X, Y)
 *   u = MIRROR ? W' - 1 - X : X      v = FLIP ? H' - 1 - Y : Y      D[Y][X] = TRANSPOSE ? S[u][v] : S[v][u]        (S[row][column])
 * which is m355_or_source below.  An element is whatever moves as a unit: a sample, the (Cb, Cr) pair of an interleaved row, a pixel.
 */
#ifndef M355_ORIENTATION_H
#define M355_ORIENTATION_H

#include <stdint.h>
#include "de265_mi355x.h"

#ifdef __HIPCC__
#define M355_OR_FN __host__ __device__ static inline
#else
#define M355_OR_FN static inline
#endif

M355_OR_FN bool m355_or_known(int o) { return o >= 0 && o <= 7; }
M355_OR_FN bool m355_or_mirror(int o) { return (o & M355_ORIENT_MIRROR) != 0; }
M355_OR_FN bool m355_or_flip(int o) { return (o & M355_ORIENT_FLIP) != 0; }
M355_OR_FN bool m355_or_transpose(int o) { return (o & M355_ORIENT_TRANSPOSE) != 0; }

/* the size of the result of a w x h source */
M355_OR_FN int64_t m355_or_width(int o, int64_t w, int64_t h) { return m355_or_transpose(o) ? h : w; }
M355_OR_FN int64_t m355_or_height(int o, int64_t w, int64_t h) { return m355_or_transpose(o) ? w : h; }

/* D[Y][X] = S[*row][*col] for a source of w columns and h rows */
M355_OR_FN void m355_or_source(int o, int64_t w, int64_t h, int64_t X, int64_t Y, int64_t* row, int64_t* col)
{
  const int64_t u = m355_or_mirror(o) ? m355_or_width(o, w, h) - 1 - X : X, v = m355_or_flip(o) ? m355_or_height(o, w, h) - 1 - Y : Y;
  *row = m355_or_transpose(o) ? u : v;
  *col = m355_or_transpose(o) ? v : u;
}

/* The one orientation equal to `first` and then `then`.  Write an orientation as the operator m^M f^F t^T (t applied first).  f and m commute, and a
 * transpose behind a flip is a mirror behind the transpose (t f = m t, t m = f t), so a TRANSPOSE in `then` exchanges the two reversals of `first`
 * on its way to the right: m^M2 f^F2 t m^M1 f^F1 t^T1 = m^(M2 ^ F1) f^(F2 ^ M1) t^(1 ^ T1). */
M355_OR_FN int m355_or_compose(int first, int then)
{
  const int m1 = first & 1, f1 = (first >> 1) & 1, m2 = then & 1, f2 = (then >> 1) & 1;
  const int m = m355_or_transpose(then) ? m2 ^ f1 : m2 ^ m1, f = m355_or_transpose(then) ? f2 ^ m1 : f2 ^ f1;
  return m | (f << 1) | ((first ^ then) & M355_ORIENT_TRANSPOSE);
}

/* The orientation that brings a picture stored with EXIF / TIFF Orientation 1..8 upright; -1 for any other value.  Orientation names the visual side
 * the stored row 0 and the stored column 0 lie on: 1 top / left, 2 top / right, 3 bottom / right, 4 bottom / left, 5 left / top, 6 right / top,
 * 7 right / bottom, 8 left / bottom.  2..4 reverse the columns, both or the rows; 5..8 exchange rows and columns first: 5 needs nothing more, 6 (a
 * phone held upright: its row 0 is the right side) the columns reversed behind the transpose = 90 degrees clockwise, 8 the rows = 90 degrees
 * anticlockwise, 7 both. */
M355_OR_FN int m355_or_from_exif(int exif)
{
  switch (exif) {
    case 1: return 0;
    case 2: return M355_ORIENT_MIRROR;
    case 3: return M355_ORIENT_ROTATE_180;
    case 4: return M355_ORIENT_FLIP;
    case 5: return M355_ORIENT_TRANSPOSE;
    case 6: return M355_ORIENT_ROTATE_90_CW;
    case 7: return M355_ORIENT_TRANSPOSE | M355_ORIENT_FLIP | M355_ORIENT_MIRROR;
    case 8: return M355_ORIENT_ROTATE_90_CCW;
    default: return -1;
  }
}

#endif
