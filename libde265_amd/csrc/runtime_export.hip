/*
 * runtime_export.hip — host side of the exports (runtime_internal.h lists the parts): a decoded frame, or a rectangle of it, converted into memory of
 * the caller — as it is, downscaled, resized, as R'G'B', or a batch of frames / regions as one float tensor — and what goes with them: the integers of
 * the conversion, the rows of the resize filter, the colour transform objects, the float stage of one tensor element, the wait for an export and the
 * order of a consumer's stream behind it.
 *
 * Every entry point runs the same stages in the same order, and the first failing check is the one reported: the PLAN (export_plan: frame handle,
 * descriptor, layout, samples, rectangle), the OPTIONS (opts_check), the RESIZE CHECK (resize_check: filter, output size, ratio), the DESCRIPTOR CHECK
 * (rgb_desc_check / tensor_desc_check / the destinations: dst_check), the colour step (colour_apply), then the launch as a READER of the frame
 * (export_launch / batch_launch).  tests/test_export_rejections_emu.py pins every message and every winner.
 */
#include "runtime_internal.h"
#include "resize_taps.h"
#include "tensor_element.h"
#include "colour_transform.h"
#include "colour_preset.h"
#include "pixel_pack.h"
#include "orientation.h"
#include <utility>

namespace {
/* What the exports share per plane of the launch (semi-planar: plane 1 = Cb and Cr interleaved): where the rectangle starts in the frame, its size and
 * where it goes. */
struct ExportPlane {
  const uint8_t* src[2];            /* the rectangle's first sample (src[1]: the Cr plane of an interleaved row) */
  uint8_t* dst;
  long long src_pitch, dst_pitch;   /* bytes */
  int pw, ph, bd, sb, db;           /* the rectangle on this plane (source samples), bit depth, bytes per source / destination sample */
  int64_t row_bytes;                /* of a destination row */
};
struct ExportPlan { Frame* f; int np; bool semi; ExportPlane p[3]; };

/* the luma samples one chroma sample of the frame spans, across and down (4:0:0: 1 x 1) */
struct ChromaStep { int sw, sh; };
ChromaStep chroma_step(const Frame* f) { return {(f->cf == 1 || f->cf == 2) ? 2 : 1, f->cf == 1 ? 2 : 1}; }

/* One destination plane: it is there, its pitch holds a row of row_bytes and — eb == 2: the R'G'B' exports, which store 16-bit elements whole — its
 * address and pitch are even.  (The YUV exports pass eb = 1: they take 16-bit planes at any address.) */
int dst_check(const char* who, int p, const void* dst, int64_t pitch, int64_t row_bytes, int eb)
{
  if (!dst) return fail(M355_ERR_INVALID, "%s: no destination for plane %d", who, p);
  if (pitch < row_bytes) return fail(M355_ERR_INVALID, "%s: pitch %lld of plane %d is below its row of %lld bytes", who, (long long)pitch, p, (long long)row_bytes);
  if (eb == 2 && (((uintptr_t)dst | (uint64_t)pitch) & 1)) return fail(M355_ERR_INVALID, "%s: 16-bit plane %d at an odd address or pitch", who, p);
  return M355_OK;
}
/* The plan of m355_frame_export, m355_frame_export_scaled and m355_frame_export_oriented: the argument checks and the planes.  log2_scale = k: the
 * rectangle must divide into blocks of 1 << k samples on every plane's grid, and row_bytes / the pitch check are those of the SCALED row; transposed:
 * those of a row of the plane's ph elements. */
int export_plan(m355_ctx* c, int h, const m355_export_desc* e, int k, const char* who, ExportPlan& P, bool transposed = false)
{
  Frame* f = get_frame(c, h);
  if (!f || !e) return fail(M355_ERR_INVALID, "bad frame handle %d / null descriptor", h);
  if (e->layout != M355_EXPORT_PLANAR && e->layout != M355_EXPORT_SEMIPLANAR) return fail(M355_ERR_INVALID, "%s: unknown layout %d", who, e->layout);
  if (e->samples != M355_EXPORT_NATIVE && e->samples != M355_EXPORT_MSB16 && e->samples != M355_EXPORT_U8) return fail(M355_ERR_INVALID, "%s: unknown sample format %d", who, e->samples);
  const auto [sw, sh] = chroma_step(f);
  const int fs = 1 << k;
  int x0 = 0, y0 = 0, w = f->w, hgt = f->h;
  if (e->width != 0) {
    x0 = e->x0; y0 = e->y0; w = e->width; hgt = e->height;
    if (x0 < 0 || y0 < 0 || w <= 0 || hgt <= 0 || x0 > f->w - w || y0 > f->h - hgt) return fail(M355_ERR_INVALID, "%s: rectangle %d,%d %dx%d leaves the %dx%d frame", who, x0, y0, w, hgt, f->w, f->h);
    if (f->cf && ((x0 | w) % sw || (y0 | hgt) % sh)) return fail(M355_ERR_INVALID, "%s: rectangle %d,%d %dx%d is not aligned to the chroma grid (%dx%d luma samples)", who, x0, y0, w, hgt, sw, sh);
  }
  if (k && (w % (fs * sw) || hgt % (fs * sh))) return fail(M355_ERR_INVALID, "%s: %dx%d is no multiple of %dx%d luma samples (scale %d on every plane)", who, w, hgt, fs * sw, fs * sh, fs);
  P.f = f;
  P.semi = e->layout == M355_EXPORT_SEMIPLANAR && f->cf != 0;
  P.np = f->cf == 0 ? 1 : (P.semi ? 2 : 3);
  for (int p = 0; p < P.np; p++) {
    ExportPlane& q = P.p[p];
    q.bd = p ? f->bdc : f->bdl; q.sb = f->bpp[p];
    q.db = e->samples == M355_EXPORT_NATIVE ? q.sb : (e->samples == M355_EXPORT_MSB16 ? 2 : 1);
    q.pw = p ? w / sw : w; q.ph = p ? hgt / sh : hgt;
    const int px = p ? x0 / sw : x0, py = p ? y0 / sh : y0;
    q.row_bytes = (int64_t)((transposed ? q.ph : q.pw) >> k) * q.db * (P.semi && p ? 2 : 1);
    const int rc = dst_check(who, p, e->dst[p], e->pitch[p], q.row_bytes, 1);
    if (rc) return rc;
    q.dst = (uint8_t*)e->dst[p]; q.dst_pitch = e->pitch[p];
    q.src_pitch = (long long)f->stride[p] * q.sb;
    for (int j = 0; j < (P.semi && p ? 2 : 1); j++) q.src[j] = (const uint8_t*)f->plane[p + j] + (size_t)py * q.src_pitch + (size_t)px * q.sb;
  }
  return M355_OK;
}
/* export_plan for the calls that check their destinations themselves: r = what holds the rectangle (a descriptor or a region; null: no descriptor),
 * planned as an export of `layout` / `samples` whose destinations — `dst` for every plane, with a pitch no row exceeds — cannot fail unless dst is null */
template <class R>
int export_plan_rect(m355_ctx* c, int h, const R* r, const void* dst, const char* who, ExportPlan& P, int layout = M355_EXPORT_PLANAR, int samples = M355_EXPORT_NATIVE)
{
  m355_export_desc yuv = {};
  if (r) {
    yuv.layout = layout; yuv.samples = samples;
    yuv.x0 = r->x0; yuv.y0 = r->y0; yuv.width = r->width; yuv.height = r->height;
    for (int p = 0; p < 3; p++) { yuv.dst[p] = (void*)dst; yuv.pitch[p] = INT64_MAX; }
  }
  return export_plan(c, h, r ? &yuv : nullptr, 0, who, P);
}
/* Plane p of a plan into the kernel arguments of the three YUV exports: the source pointers (an interleaved plane: Cb in src[p], Cr in src[2]), the
 * source pitch, the destination and its pitch.  Shifts, chunks and units are each export's own. */
template <class A> void plane_fill(const ExportPlan& P, int p, uint8_t* dst, long long dst_pitch, A& a)
{
  const ExportPlane& q = P.p[p];
  a.src[p] = q.src[0];
  if (P.semi && p) a.src[2] = q.src[1];
  a.src_pitch[p] = q.src_pitch;
  a.dst[p] = dst; a.dst_pitch[p] = dst_pitch;
}
/* The launch of a single-frame export: a READER of the frame of the kind RD_EXPORT (reader_begin, which hands the gate to a.timeout / a.epoch) — the mark
 * behind it is what the next decode into the frame waits for (dst_hazards), what m355_frame_export_wait blocks on and what m355_frame_export_order makes a
 * consumer's stream wait for.  launch(stream) enqueues the kernel. */
template <class A, class L> int export_launch(m355_ctx* c, Frame* f, A& a, L launch)
{
  hipSetDevice(c->device);
  const hipStream_t cs = reader_begin(c, f, RD_EXPORT, &a.timeout, &a.epoch);
  launch(cs);
  HIPCHK(hipGetLastError());
  return reader_end(c, f, RD_EXPORT, cs);
}
/* The checks of the R'G'B' descriptors (m355_rgb_desc, m355_resize_rgb_desc) behind the plan: the layout, the conversion (into a.k) and the destinations
 * of rows of `width` pixels (into a.dst / a.dst_pitch) */
template <class D, class A>
int rgb_desc_check(const char* who, const D* e, const Frame* f, int64_t width, A& a, bool* planar_out, int* db_out)
{
  if (e->layout != M355_RGB_PACKED && e->layout != M355_RGB_PLANAR) return fail(M355_ERR_INVALID, "%s: unknown layout %d", who, e->layout);
  int rc = m355_rgb_coefficients(e->matrix, e->full_range, f->bdl, f->bdc, e->samples, &a.k);
  if (rc) return rc;
  const bool planar = e->layout == M355_RGB_PLANAR;
  const int db = e->samples == M355_RGB_U16 ? 2 : 1;
  const int64_t row_bytes = width * db * (planar ? 1 : 3);
  for (int p = 0; p < (planar ? 3 : 1); p++) {
    if ((rc = dst_check(who, p, e->dst[p], e->pitch[p], row_bytes, db)) != 0) return rc;
    a.dst[p] = (uint8_t*)e->dst[p]; a.dst_pitch[p] = e->pitch[p];
  }
  *planar_out = planar; *db_out = db;
  return M355_OK;
}
/* m355_export_opts behind the plan of a frame like f (a batch: frames[0], whose chroma format every frame shares): null = the defaults; the reserved
 * entries, the colour transform and the chroma sample location type, which is 4:2:0's alone.  The filter is checked where it is used (resize_check); resizes = false: the
 * call has no filter to choose. */
int opts_check(const char* who, m355_ctx* c, const m355_export_opts* o, const Frame* f, bool resizes, m355_export_opts& out, ColourArgs* colour = nullptr)
{
  out = m355_export_opts{};
  if (!o) return M355_OK;
  for (int i = 1; i < 6; i++) if (o->reserved[i]) return fail(M355_ERR_INVALID, "%s: reserved[%d] of the options is %d, not 0", who, i, o->reserved[i]);
  /* reserved[0] is the colour transform: a live object of this context, where the call has the stage (colour != null) */
  if (o->colour) {
    if (!colour) return fail(M355_ERR_INVALID, "%s: colour %d (reserved[0]) in a call without a colour transform stage", who, o->colour);
    const m355_ctx::ColourObj* obj = nullptr;
    for (const auto& q : c->colour) if (q.handle == o->colour) obj = &q;
    if (!obj) return fail(M355_ERR_INVALID, "%s: colour %d (reserved[0]) is no live colour transform of this context", who, o->colour);
    colour->t = obj->dev;
    for (int k = 0; k < 9; k++) colour->m[k] = obj->matrix[k];
    colour->g = obj->gain; colour->norm = obj->norm;
    for (int k = 0; k < 3; k++) colour->w[k] = obj->weights[k];
  }
  if (!resizes && o->filter != M355_FILTER_TRIANGLE) return fail(M355_ERR_INVALID, "%s: filter %d where nothing is resized", who, o->filter);
  if (o->chroma_loc < 0 || o->chroma_loc > 3) return fail(M355_ERR_INVALID, "%s: chroma sample location type %d is not 0..3", who, o->chroma_loc);
  if (o->chroma_loc && f->cf != 1) return fail(M355_ERR_INVALID, "%s: chroma sample location type %d for a frame that is not 4:2:0", who, o->chroma_loc);
  out = *o;
  return M355_OK;
}
/* the options of a _filtered call: that filter, chroma sample location type 0 */
m355_export_opts filter_opts(int filter) { m355_export_opts o = {}; o.filter = filter; return o; }

/* The width of k_export_resized's tiles on one plane: 256 output columns, or a few less where that saves a wavefront — the lanes of the vertical pass
 * own the 16-byte vectors of the tile's source span, and a span of 64 k + a few vectors (256 columns at ratio 4: 129) would run a wavefront for them. */
uint32_t resize_tile_w(int filter, int64_t sn, int64_t dn, int sb)
{
  const int64_t S = 16 / sb, T = m355_resize_max_taps_filtered(filter, sn, dn);
  const auto vectors = [&](int64_t w) { return ((w - 1) * sn / dn + 2 + T + S - 1) / S; };   /* (an upper bound of the span of w columns) */
  int64_t w = M355_RESIZE_TILE_W;
  const int64_t nv = vectors(w), k = nv / 64;
  if (k >= 1 && nv % 64 != 0 && nv % 64 <= 16) while (w > 1 && vectors(w) > 64 * k) w--;
  return (uint32_t)w;
}
/* What the resizing exports check behind their plans: the filter, the output size against the chroma grid, and the filter's limits — the ratio, and for
 * the cubic filter the sizes — of every plan (entries > 0: of every entry of a batch of regions, which the message then names).  The chroma planes'
 * ratios are the luma plane's and their sizes smaller. */
int resize_check(const char* who, const ExportPlan* P, int entries, int ow, int oh, int filter)
{
  if (filter != M355_FILTER_TRIANGLE && filter != M355_FILTER_CUBIC) return fail(M355_ERR_INVALID, "%s: unknown filter %d", who, filter);
  const auto [sw, sh] = chroma_step(P[0].f);
  if (ow <= 0 || oh <= 0 || ow % sw || oh % sh)
    return fail(M355_ERR_INVALID, "%s: output size %dx%d is not positive or no multiple of %dx%d luma samples", who, ow, oh, sw, sh);
  for (int i = 0; i < (entries ? entries : 1); i++) {
    const int pw = P[i].p[0].pw, ph = P[i].p[0].ph;
    if (m355_resize_ratio_ok_filtered(filter, pw, ow) && m355_resize_ratio_ok_filtered(filter, ph, oh)) continue;
    char entry[32] = "", limits[96] = "8x down or up";
    if (entries) snprintf(entry, sizeof(entry), "entry %d, ", i);
    if (filter == M355_FILTER_CUBIC) snprintf(limits, sizeof(limits), "4x down or 8x up, or a size above %d (cubic filter)", M355_RESIZE_CUBIC_MAX_N);
    return fail(M355_ERR_INVALID, "%s: %s%dx%d to %dx%d is more than %s", who, entry, pw, ph, ow, oh, limits);
  }
  return M355_OK;
}
/* The width of k_export_resized_rgb's tiles: a pass of that kernel takes two luma rows, or two rows of Cb and of Cr, where their source vectors fit
 * the workgroup's 256 lanes, and a workgroup's time follows its number of passes — so the widest width (even for 4:2:0 / 4:2:2: a tile's first column
 * is a chroma column) not above resize_tile_w's at which they fit, but at least 64 columns, then the narrowest one with the same number of tiles. */
uint32_t resize_rgb_tile_w(int filter, int64_t sn, int64_t dn, int64_t csn, int64_t cdn, int sb, int sw, int centre)
{
  const int64_t S = 16 / sb;
  const auto vectors = [&](int64_t w, int64_t s, int64_t d) { return ((w - 1) * s / d + 2 + m355_resize_max_taps_filtered(filter, s, d) + S - 1) / S; };   /* (an upper bound) */
  const auto fits = [&](int64_t w) { return 2 * vectors(w, sn, dn) <= 256 && (sw != 2 || 4 * vectors(w / 2 + 1 + centre, csn, cdn) <= 256); };   /* (CENTRE: a chroma column more) */
  int64_t w = resize_tile_w(filter, sn, dn, sb);
  if (sw == 2) w = w > 2 ? w & ~(int64_t)1 : 2;
  int64_t t = w;
  while (t > 64 && !fits(t)) t -= sw;
  if (fits(t)) w = t;
  const int64_t tiles = (dn + w - 1) / w;
  int64_t even = (dn + tiles - 1) / tiles;
  if (sw == 2) even = (even + 1) & ~(int64_t)1;
  return (uint32_t)(even < w ? even : w);
}
/* The colour transform stage of a composed export into its kernel arguments: the object's tables and matrix, and the coefficients of M355_RGB_U16
 * in place of the descriptor's samples', which then only pick the delivery (the kernel's element bytes, or the tensors' u16) */
template <class D, class A> int colour_apply(const ColourArgs& colour, const D* e, const Frame* f, A& a)
{
  if (!colour.t) return M355_OK;
  a.colour = colour;
  return m355_rgb_coefficients(e->matrix, e->full_range, f->bdl, f->bdc, M355_RGB_U16, &a.k);
}
/* What the kernel arguments of k_export_resized_rgb.hip take from a plan.  plan_sources: the rectangle's first samples and the two pitches, into the
 * launch's or the slice's record.  plan_geometry: the source size on both grids, the tile width, the tiles per row of tiles and the units into g (the
 * launch's or the slice's record), the output size on both grids into d (the launch's). */
template <class R> void plan_sources(const ExportPlan& Q, R& r)
{
  for (int p = 0; p < Q.np; p++) r.src[p] = Q.p[p].src[0];
  r.src_pitch[0] = Q.p[0].src_pitch; r.src_pitch[1] = Q.np > 1 ? Q.p[1].src_pitch : 0;
}
template <class G, class D> void plan_geometry(const ExportPlan& Q, int ow, int oh, int filter, int chroma_loc, G& g, D& d)
{
  const auto [sw, sh] = chroma_step(Q.f);
  g.sn_x[0] = (uint32_t)Q.p[0].pw; g.sn_y[0] = (uint32_t)Q.p[0].ph; d.dn_x[0] = (uint32_t)ow; d.dn_y[0] = (uint32_t)oh;
  if (Q.np > 1) { g.sn_x[1] = (uint32_t)Q.p[1].pw; g.sn_y[1] = (uint32_t)Q.p[1].ph; d.dn_x[1] = (uint32_t)(ow / sw); d.dn_y[1] = (uint32_t)(oh / sh); }
  g.tile_w = resize_rgb_tile_w(filter, Q.p[0].pw, ow, Q.np > 1 ? Q.p[1].pw : 0, ow / sw, Q.f->bpp[0], sw, chroma_loc & 1);
  g.tiles_x = ((uint32_t)ow + g.tile_w - 1) / g.tile_w;
  g.units = g.tiles_x * (((uint32_t)oh + M355_RESIZE_TILE_H - 1) / M355_RESIZE_TILE_H);
}
/* What the two tensor exports share (k_export_resized_rgb.hip, RR_BATCH and RR_ROIS).  batch_frame_check: frame i of the batch against frame 0 —
 * chroma format and bit depths, and the size where whole frames must agree. */
int batch_frame_check(const char* who, const int* frames, int i, const ExportPlan* P, bool same_size)
{
  const Frame *f = P[i].f, *f0 = P[0].f;
  if (f->cf != f0->cf || f->bdl != f0->bdl || f->bdc != f0->bdc || f->bpp[0] != f0->bpp[0])
    return fail(M355_ERR_INVALID, "%s: chroma format / bit depths of frame %d (entry %d) differ from those of frame %d", who, frames[i], i, frames[0]);
  if (same_size && (f->w != f0->w || f->h != f0->h))
    return fail(M355_ERR_INVALID, "%s: whole frames of different sizes (%dx%d, entry %d: %dx%d)", who, f0->w, f0->h, i, f->w, f->h);
  return M355_OK;
}
/* the tensor's descriptor for n slices of frames like f: layout, dtype, conversion, scale and bias, the destination and the strides, which must keep
 * rows, planes and slices apart; fills what the launch takes from them and *eb_out = the element's bytes */
template <class A>
int tensor_desc_check(const char* who, const m355_tensor_desc* e, int n, const Frame* f, A& a, int* eb_out)
{
  if (e->layout != M355_TENSOR_NCHW && e->layout != M355_TENSOR_NHWC) return fail(M355_ERR_INVALID, "%s: unknown layout %d", who, e->layout);
  if (e->dtype != M355_TENSOR_F32 && e->dtype != M355_TENSOR_F16 && e->dtype != M355_TENSOR_BF16) return fail(M355_ERR_INVALID, "%s: unknown dtype %d", who, e->dtype);
  int rc = m355_rgb_coefficients(e->matrix, e->full_range, f->bdl, f->bdc, e->samples, &a.k);
  if (rc) return rc;
  for (int k = 0; k < 3; k++) {
    if ((m355_te_bits(e->scale[k]) & 0x7F800000u) == 0x7F800000u || (m355_te_bits(e->bias[k]) & 0x7F800000u) == 0x7F800000u)
      return fail(M355_ERR_INVALID, "%s: scale / bias of channel %d is not finite", who, k);
    a.scale[k] = e->scale[k]; a.bias[k] = e->bias[k];
  }
  const bool nhwc = e->layout == M355_TENSOR_NHWC;
  const int eb = e->dtype == M355_TENSOR_F32 ? 4 : 2;
  const int64_t row = (int64_t)e->out_width * eb * (nhwc ? 3 : 1);
  if (!e->dst) return fail(M355_ERR_INVALID, "%s: no destination", who);
  if (((uintptr_t)e->dst | (uint64_t)e->stride_h | (nhwc ? 0u : (uint64_t)e->stride_c) | (n > 1 ? (uint64_t)e->stride_n : 0u)) & (uint64_t)(eb - 1))
    return fail(M355_ERR_INVALID, "%s: the destination or a stride is no multiple of the %d-byte element", who, eb);
  if (e->stride_h < row) return fail(M355_ERR_INVALID, "%s: stride_h %lld is below the row of %lld bytes", who, (long long)e->stride_h, (long long)row);
  const __int128 E = (__int128)(e->out_height - 1) * e->stride_h + row;              /* first byte behind a plane's (NHWC: a slice's) last row */
  if (!nhwc && (__int128)e->stride_c < E) return fail(M355_ERR_INVALID, "%s: stride_c %lld lets the planes overlap (%lld bytes each)", who, (long long)e->stride_c, (long long)E);
  if (n > 1 && (__int128)e->stride_n < (nhwc ? E : 2 * (__int128)e->stride_c + E))
    return fail(M355_ERR_INVALID, "%s: stride_n %lld lets the slices overlap", who, (long long)e->stride_n);
  a.dst = (uint8_t*)e->dst; a.stride_n = n > 1 ? e->stride_n : 0; a.stride_c = nhwc ? 0 : e->stride_c; a.stride_h = e->stride_h;
  a.n = (uint32_t)n;
  a.cf = f->cf; a.nhwc = nhwc; a.bf16 = e->dtype == M355_TENSOR_BF16; a.u16 = e->samples == M355_RGB_U16; a.bdl = f->bdl; a.bdc = f->bdc;
  *eb_out = eb;
  return M355_OK;
}
/* The launch as a reader of the kind RD_EXPORT of EVERY frame of the batch, as m355_frame_measure_async is of its two: it goes on the stream of
 * frames[0]'s writer, which first continues behind the writer and the earlier export of each other frame; the one mark behind the launch is kept by all
 * of them (batch_reader_end); each slice's record fr[i] gets the gate of its frame. */
template <class R>
hipStream_t batch_reader_begin(m355_ctx* c, const ExportPlan* P, int n, R* fr)
{
  const hipStream_t cs = reader_begin(c, P[0].f, RD_EXPORT, &fr[0].timeout, &fr[0].epoch);
  for (int i = 1; i < n; i++) {
    Frame* g = P[i].f;
    int first = 0;
    while (P[first].f != g) first++;
    if (first < i) { fr[i].timeout = fr[first].timeout; fr[i].epoch = fr[first].epoch; continue; }   /* the same frame again */
    ev_wait(c, cs, g->wr);                                  /* the frame's last writer (nothing to enqueue when that ran on `cs`) */
    ev_wait(c, cs, g->reader[RD_EXPORT]);                   /* ... and its earlier export on another stream: the one mark kept stands for both */
    if (g->wr_stream && g->wr_gate) { fr[i].timeout = g->wr_gate; fr[i].epoch = g->wr_epoch; }
    else {                                                  /* no decode to be gated by: an epoch of its own, which no gate word holds (reader_begin) */
      fr[i].timeout = lane(c).timeout; fr[i].epoch = ++c->epoch;
      if (fr[i].epoch == 0) fr[i].epoch = ++c->epoch;
    }
  }
  return cs;
}
int batch_reader_end(m355_ctx* c, const ExportPlan* P, int n, hipStream_t cs)
{
  Frame* f = P[0].f;
  int rc = reader_end(c, f, RD_EXPORT, cs);
  if (rc) return rc;
  for (int i = 1; i < n; i++) P[i].f->reader[RD_EXPORT] = f->reader[RD_EXPORT];
  return M355_OK;
}
/* the launch of a batch export between the two: launch(stream) enqueues the kernel */
template <class A, class L> int batch_launch(m355_ctx* c, const ExportPlan* P, int n, A& a, L launch)
{
  hipSetDevice(c->device);
  const hipStream_t cs = batch_reader_begin(c, P, n, a.fr);
  launch(cs);
  HIPCHK(hipGetLastError());
  return batch_reader_end(c, P, n, cs);
}
std::atomic<int> g_colour_handle{0x100};
}   /* namespace */

extern "C" {
/* The frame, or a rectangle of it, converted into memory of the caller (k_export.hip): one launch for all planes. */
int m355_frame_export(m355_ctx* c, int h, const m355_export_desc* e)
{
  ExportPlan P;
  int rc = export_plan(c, h, e, 0, "m355_frame_export", P);
  if (rc) return rc;
  ExportArgs a = {};
  uint32_t units = 0;
  for (int p = 0; p < 3; p++) {
    if (p < P.np) {
      const ExportPlane& q = P.p[p];
      plane_fill(P, p, q.dst, q.dst_pitch, a);
      a.row_bytes[p] = (uint32_t)q.row_bytes; a.chunks[p] = (uint32_t)((q.row_bytes + 1023) / 1024);
      a.shift[p] = e->samples == M355_EXPORT_MSB16 ? 16 - q.bd : (e->samples == M355_EXPORT_U8 ? q.bd - 8 : 0);
      units += a.chunks[p] * (uint32_t)q.ph;
    }
    a.unit_end[p] = units;
  }
  return export_launch(c, P.f, a, [&](hipStream_t cs) { m355_launch_export(a, P.f->bpp[0], P.p[0].db, P.semi, cs); });
}
/* The same with every plane of the rectangle oriented on its own grid (k_export_oriented.hip; orientation.h): the plan of m355_frame_export, its pitches
 * checked against the oriented rows.  Orientation 0 is m355_frame_export itself. */
int m355_frame_export_oriented(m355_ctx* c, int h, const m355_export_desc* e, int orientation)
{
  const char* who = "m355_frame_export_oriented";
  if (!m355_or_known(orientation)) return fail(M355_ERR_INVALID, "%s: orientation %d is not 0..7", who, orientation);
  if (orientation == 0) return m355_frame_export(c, h, e);
  const bool tr = m355_or_transpose(orientation);
  const Frame* g = get_frame(c, h);
  if (g && tr && g->cf == 2) return fail(M355_ERR_INVALID, "%s: a transposed 4:2:2 frame would be 4:4:0, which no layout describes", who);
  ExportPlan P;
  int rc = export_plan(c, h, e, 0, who, P, tr);
  if (rc) return rc;
  ExportOrientedArgs a = {};
  uint32_t units = 0;
  for (int p = 0; p < 3; p++) {
    if (p < P.np) {
      const ExportPlane& q = P.p[p];
      plane_fill(P, p, q.dst, q.dst_pitch, a);
      a.pw[p] = (uint32_t)q.pw; a.ph[p] = (uint32_t)q.ph;
      a.shift[p] = e->samples == M355_EXPORT_MSB16 ? 16 - q.bd : (e->samples == M355_EXPORT_U8 ? q.bd - 8 : 0);
      if (tr) {
        a.per_row[p] = (uint32_t)((q.pw + M355_ORIENT_TILE - 1) / M355_ORIENT_TILE);
        units += a.per_row[p] * (uint32_t)((q.ph + M355_ORIENT_TILE - 1) / M355_ORIENT_TILE);
      } else {
        a.per_row[p] = (uint32_t)((q.row_bytes + 1023) / 1024);
        units += a.per_row[p] * (uint32_t)q.ph;
      }
    }
    a.unit_end[p] = units;
  }
  a.mirror = m355_or_mirror(orientation); a.flip = m355_or_flip(orientation); a.transpose = tr;
  return export_launch(c, P.f, a, [&](hipStream_t cs) { m355_launch_export_oriented(a, P.f->bpp[0], P.p[0].db, P.semi, cs); });
}
int m355_orientation_compose(int first, int then, int* out)
{
  if (!out || !m355_or_known(first) || !m355_or_known(then)) return fail(M355_ERR_INVALID, "m355_orientation_compose: null result, or %d / %d is not 0..7", first, then);
  *out = m355_or_compose(first, then);
  return M355_OK;
}
int m355_orientation_from_exif(int exif, int* out)
{
  if (!out || m355_or_from_exif(exif) < 0) return fail(M355_ERR_INVALID, "m355_orientation_from_exif: null result, or %d is not 1..8", exif);
  *out = m355_or_from_exif(exif);
  return M355_OK;
}
/* The same, downscaled by 1 << log2_scale in both directions (k_export_scaled.hip): a reader of the same kind, so that m355_frame_export_wait and
 * m355_frame_export_order cover it and the next decode into the frame waits for it. */
int m355_frame_export_scaled(m355_ctx* c, int h, const m355_export_desc* e, int log2_scale)
{
  if (log2_scale == 0) return m355_frame_export(c, h, e);
  if (log2_scale < 0 || log2_scale > 3) return fail(M355_ERR_INVALID, "m355_frame_export_scaled: log2_scale %d is not 0..3", log2_scale);
  ExportPlan P;
  int rc = export_plan(c, h, e, log2_scale, "m355_frame_export_scaled", P);
  if (rc) return rc;
  ExportScaledArgs a = {};
  uint32_t units = 0;
  for (int p = 0; p < 3; p++) {
    if (p < P.np) {
      const ExportPlane& q = P.p[p];
      plane_fill(P, p, q.dst, q.dst_pitch, a);
      a.out_w[p] = (uint32_t)(q.pw >> log2_scale); a.chunks[p] = (uint32_t)(((int64_t)q.pw * q.sb + 1023) / 1024);
      a.rshift[p] = 2 * log2_scale + (e->samples == M355_EXPORT_U8 ? q.bd - 8 : 0);
      a.lshift[p] = e->samples == M355_EXPORT_MSB16 ? 16 - q.bd : 0;
      units += a.chunks[p] * (uint32_t)(q.ph >> log2_scale);
    }
    a.unit_end[p] = units;
  }
  return export_launch(c, P.f, a, [&](hipStream_t cs) { m355_launch_export_scaled(a, P.f->bpp[0], P.p[0].db, P.semi, log2_scale, cs); });
}
/* The integers of the R'G'B' conversion (de265_mi355x.h states the formulas): 64-bit integer arithmetic only, so every build makes the same ones */
int m355_rgb_coefficients(int matrix, int full_range, int bdl, int bdc, int samples, m355_rgb_coeffs* out)
{
  static const int64_t K[3][2] = {{2990, 1140}, {2126, 722}, {2627, 593}};
  if (!out) return fail(M355_ERR_INVALID, "m355_rgb_coefficients: null result");
  if (matrix < 0 || matrix > 2 || (full_range != 0 && full_range != 1) || (samples != M355_RGB_U8 && samples != M355_RGB_U16))
    return fail(M355_ERR_INVALID, "m355_rgb_coefficients: unknown matrix %d / full_range %d / samples %d", matrix, full_range, samples);
  if (bdl < 8 || bdl > 16 || bdc < 8 || bdc > 16) return fail(M355_ERR_INVALID, "m355_rgb_coefficients: bit depths %d / %d are not 8..16", bdl, bdc);
  const auto rdiv = [](int64_t a, int64_t b) { return (2 * a + b) / (2 * b); };
  const int D = samples == M355_RGB_U8 ? 8 : 16, F = 29 - D;
  const int64_t kr = K[matrix][0], kb = K[matrix][1], kg = 10000 - kr - kb, mf = (((int64_t)1 << D) - 1) << F;
  const int64_t ys = full_range ? ((int64_t)1 << bdl) - 1 : (int64_t)219 << (bdl - 8), cs = full_range ? ((int64_t)1 << bdc) - 1 : (int64_t)224 << (bdc - 8);
  out->F = F;
  out->y0 = full_range ? 0 : 16 << (bdl - 8);
  out->c0 = 1 << (bdc - 1);
  out->cy = (int32_t)rdiv(mf, ys);
  out->crv = (int32_t)rdiv(2 * (10000 - kr) * mf, 10000 * cs);
  out->cbu = (int32_t)rdiv(2 * (10000 - kb) * mf, 10000 * cs);
  out->cgu = (int32_t)rdiv(2 * kb * (10000 - kb) * mf, 10000 * kg * cs);
  out->cgv = (int32_t)rdiv(2 * kr * (10000 - kr) * mf, 10000 * kg * cs);
  return M355_OK;
}
/* The frame, or a rectangle of it, as R'G'B' (k_export_rgb.hip): the frame handle and the rectangle are checked by export_plan — as a planar NATIVE
 * export whose destinations cannot fail —, the destinations by rgb_desc_check. */
int m355_frame_export_rgb_opts(m355_ctx* c, int h, const m355_rgb_desc* e, const m355_export_opts* opts)
{
  const char* who = "m355_frame_export_rgb";
  ExportPlan P;
  int rc = export_plan_rect(c, h, e, e ? e->dst[0] : nullptr, who, P);
  if (rc) return rc;
  Frame* f = P.f;
  m355_export_opts o;
  rc = opts_check(who, c, opts, f, false, o);
  if (rc) return rc;
  ExportRgbArgs a = {};
  bool planar = false;
  int db = 1;
  const int sb = f->bpp[0];
  const int64_t w = P.p[0].pw;
  rc = rgb_desc_check(who, e, f, w, a, &planar, &db);
  if (rc) return rc;
  for (int p = 0; p < 3; p++) a.src[p] = (const uint8_t*)f->plane[p];
  a.src_pitch[0] = (long long)f->stride[0] * sb; a.src_pitch[1] = (long long)f->stride[1] * sb;
  a.x0 = e->width ? (uint32_t)e->x0 : 0u; a.y0 = e->width ? (uint32_t)e->y0 : 0u;
  a.width = (uint32_t)w; a.height = (uint32_t)P.p[0].ph;
  a.cw = (uint32_t)f->pw[1]; a.ch = (uint32_t)f->ph[1];
  const uint32_t per_chunk = 64u * 16u / (uint32_t)sb;
  a.chunks = (a.width + per_chunk - 1) / per_chunk;
  a.units = a.chunks * a.height;
  return export_launch(c, f, a, [&](hipStream_t cs) { m355_launch_export_rgb(a, sb, db, planar, f->cf, o.chroma_loc, cs); });
}
int m355_frame_export_rgb(m355_ctx* c, int h, const m355_rgb_desc* e) { return m355_frame_export_rgb_opts(c, h, e, nullptr); }
/* row i of one axis of the resize filter (resize_taps.h: the function k_export_resized.hip derives its rows with) */
int m355_resize_taps_filtered(int filter, int src_n, int dst_n, int cosited, int i, int32_t* first, int32_t coeff[M355_RESIZE_MAX_TAPS])
{
  if (!first || !coeff || (cosited != 0 && cosited != 1) || !m355_resize_ratio_ok_filtered(filter, src_n, dst_n) || i < 0 || i >= dst_n) return -1;
  return m355_resize_row_filtered(filter, src_n, dst_n, cosited, i, first, coeff, 1);
}
int m355_resize_taps(int src_n, int dst_n, int cosited, int i, int32_t* first, int32_t coeff[M355_RESIZE_MAX_TAPS])
{
  return m355_resize_taps_filtered(M355_FILTER_TRIANGLE, src_n, dst_n, cosited, i, first, coeff);
}
/* The frame, or a rectangle of it, resized to out_width x out_height luma samples (k_export_resized.hip): the frame handle, the rectangle, the layout and
 * the samples are checked by export_plan — with destinations that cannot fail, as for the R'G'B' export —, the output size, the ratio and the destinations
 * here. */
int m355_frame_export_resized_opts(m355_ctx* c, int h, const m355_resize_desc* e, const m355_export_opts* opts)
{
  const char* who = "m355_frame_export_resized";
  ExportPlan P;
  int rc = export_plan_rect(c, h, e, e, who, P, e ? e->layout : 0, e ? e->samples : 0);
  if (rc) return rc;
  Frame* f = P.f;
  m355_export_opts o;
  rc = opts_check(who, c, opts, f, true, o);
  if (rc) return rc;
  const int filter = o.filter;
  const auto [sw, sh] = chroma_step(f);
  rc = resize_check(who, &P, 0, e->out_width, e->out_height, filter);
  if (rc) return rc;
  const bool cubic = filter == M355_FILTER_CUBIC;               /* (its intermediate keeps 16 bits of fraction and its sums their sign: shifts 2 and 1 less) */
  ExportResizedArgs a = {};
  uint32_t units = 0;
  for (int p = 0; p < 3; p++) {
    if (p < P.np) {
      const ExportPlane& q = P.p[p];
      const int ow = p ? e->out_width / sw : e->out_width, oh = p ? e->out_height / sh : e->out_height;
      if ((rc = dst_check(who, p, e->dst[p], e->pitch[p], (int64_t)ow * q.db * (P.semi && p ? 2 : 1), 1)) != 0) return rc;
      plane_fill(P, p, (uint8_t*)e->dst[p], e->pitch[p], a);
      a.sn_x[p] = (uint32_t)q.pw; a.sn_y[p] = (uint32_t)q.ph; a.dn_x[p] = (uint32_t)ow; a.dn_y[p] = (uint32_t)oh;
      a.cosited[p] = p && sw == 2 && !(o.chroma_loc & 1);        /* chroma: horizontally co-sited iff LEFT, vertically iff TOP (4:2:0 only) */
      a.cosited_y[p] = p && (o.chroma_loc & 2);
      a.tile_w[p] = resize_tile_w(filter, q.pw, ow, q.sb);
      a.tiles_x[p] = ((uint32_t)ow + a.tile_w[p] - 1) / a.tile_w[p];
      a.tshift[p] = q.bd - (cubic ? 2 : 4);
      a.oshift[p] = (e->samples == M355_EXPORT_U8 ? 23 : 31 - q.bd) - (cubic ? 1 : 0);
      a.lshift[p] = e->samples == M355_EXPORT_MSB16 ? 16 - q.bd : 0;
      units += a.tiles_x[p] * (((uint32_t)oh + M355_RESIZE_TILE_H - 1) / M355_RESIZE_TILE_H);
    }
    a.unit_end[p] = units;
  }
  return export_launch(c, f, a, [&](hipStream_t cs) { m355_launch_export_resized(a, f->bpp[0], P.p[0].db, P.semi, filter, cs); });
}
int m355_frame_export_resized_filtered(m355_ctx* c, int h, const m355_resize_desc* e, int filter)
{
  const m355_export_opts o = filter_opts(filter);
  return m355_frame_export_resized_opts(c, h, e, &o);
}
int m355_frame_export_resized(m355_ctx* c, int h, const m355_resize_desc* e) { return m355_frame_export_resized_opts(c, h, e, nullptr); }
/* The colour transform objects (include/de265_mi355x.h, COLOUR TRANSFORM): the tables go to device memory of the context through its pinned staging
 * buffer and the active lane's stream, like m355_device_write's bytes; the exports find an object by its handle (opts_check). */
/* A tone object (q != null) is the same object with its gain table behind the tables in one allocation: M355_COLOUR_GAIN_DWORDS dwords at
 * M355_COLOUR_GAIN_OFFSET, the last entry repeated so that the kernel's idx + 1 needs no clamp. */
constexpr size_t M355_COLOUR_GAIN_OFFSET = (sizeof(m355_colour_tables) + 7) & ~(size_t)7, M355_COLOUR_GAIN_DWORDS = M355_COLOUR_OUT_KNOTS + 1;
static int colour_create(const char* who, m355_ctx* c, const m355_colour_tables* t, const m355_colour_tone* q, bool tone, int* handle)
{
  if (!c || !t || !handle || (tone && !q)) return fail(M355_ERR_INVALID, "%s: no context / tables / %shandle", who, tone ? "tone / " : "");
  const int bad = m355_ct_tables_check(t);
  if (bad) return fail(M355_ERR_INVALID, "%s: %s", who, bad == 1 ? "an entry of lut_in is above M355_COLOUR_ONE" : (bad == 2 ? "a matrix entry is outside -65535..65535" : "pad is not 0"));
  const int badq = tone ? m355_ct_tone_check(q) : 0;
  if (badq) return fail(M355_ERR_INVALID, "%s: %s", who, badq == 1 ? "unknown norm" : (badq == 2 ? "a weight is outside -65535..65535, or not 0 with M355_NORM_MAXRGB" :
                                                          (badq == 3 ? "a gain is above M355_TONE_GAIN_ONE" : "reserved is not 0")));
  m355_ctx::ColourObj* obj = nullptr;
  for (auto& o : c->colour) if (!o.handle && !obj) obj = &o;
  if (!obj) return fail(M355_ERR_BUSY, "%s: %d colour transforms live (destroy one: m355_colour_destroy)", who, M355_COLOUR_OBJECTS);
  hipSetDevice(c->device);
  const size_t bytes = tone ? M355_COLOUR_GAIN_OFFSET + 4 * M355_COLOUR_GAIN_DWORDS : sizeof(*t);
  int rc = stage_reserve(c, bytes);
  if (rc) return rc;
  uint8_t* dev = nullptr;
  if (hipMalloc(&dev, bytes) != hipSuccess) return fail(M355_ERR_NOMEM, "%s: hipMalloc(%zu) failed", who, bytes);
  memset(c->stage, 0, bytes);
  memcpy(c->stage, t, sizeof(*t));
  if (tone) {
    uint32_t* g = (uint32_t*)((uint8_t*)c->stage + M355_COLOUR_GAIN_OFFSET);
    memcpy(g, q->gain, sizeof(q->gain));
    g[M355_COLOUR_OUT_KNOTS] = q->gain[M355_COLOUR_OUT_KNOTS - 1];
  }
  const hipStream_t st = lane(c).stream;
  if (hipMemcpyAsync(dev, c->stage, bytes, hipMemcpyHostToDevice, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
    hipFree(dev);
    return fail(M355_ERR_HIP, "%s: the copy of the tables failed", who);
  }
  *obj = m355_ctx::ColourObj();
  obj->dev = dev;
  for (int k = 0; k < 9; k++) obj->matrix[k] = t->matrix[k];
  if (tone) {
    obj->gain = (uint32_t*)(dev + M355_COLOUR_GAIN_OFFSET); obj->norm = q->norm;
    for (int k = 0; k < 3; k++) obj->weights[k] = q->weights[k];
  }
  *handle = obj->handle = g_colour_handle.fetch_add(1);
  return M355_OK;
}
int m355_colour_create(m355_ctx* c, const m355_colour_tables* t, int* handle) { return colour_create("m355_colour_create", c, t, nullptr, false, handle); }
int m355_colour_create_tone(m355_ctx* c, const m355_colour_tables* t, const m355_colour_tone* q, int* handle)
{
  return colour_create("m355_colour_create_tone", c, t, q, true, handle);
}
int m355_colour_destroy(m355_ctx* c, int handle)
{
  if (!c) return fail(M355_ERR_INVALID, "m355_colour_destroy: no context");
  for (auto& q : c->colour) {
    if (!handle || q.handle != handle) continue;
    hipSetDevice(c->device);
    sync_all(c);                                              /* (an export may still be reading the tables) */
    hipFree(q.dev);
    q = m355_ctx::ColourObj();
    return M355_OK;
  }
  return fail(M355_ERR_INVALID, "m355_colour_destroy: %d is no live colour transform of this context", handle);
}
int m355_colour_preset(const m355_colour_preset_desc* d, m355_colour_tables* out)
{
  if (m355_cp_build(d, out)) return fail(M355_ERR_INVALID, "m355_colour_preset: null pointer, unknown code point, tone or reserved, negative nits, or peak below white");
  return M355_OK;
}
int m355_colour_pixel(const m355_colour_tables* t, const uint32_t rgb16[3], int samples, uint32_t out[3])
{
  if (!t || !rgb16 || !out || (samples != M355_RGB_U8 && samples != M355_RGB_U16) || m355_ct_tables_check(t))
    return fail(M355_ERR_INVALID, "m355_colour_pixel: null pointer, unknown samples %d, or tables outside their bounds", samples);
  m355_ct_pixel(t, rgb16, samples, out);
  return M355_OK;
}
int m355_colour_preset_tone(const m355_colour_preset_desc* d, int norm, m355_colour_tables* out, m355_colour_tone* tone)
{
  if (m355_cp_build_tone(d, norm, out, tone))
    return fail(M355_ERR_INVALID, "m355_colour_preset_tone: what m355_colour_preset rejects, an unknown tone or norm %d, or a peak so far above white that BT.2390's KS < 0", norm);
  return M355_OK;
}
int m355_colour_pixel_tone(const m355_colour_tables* t, const m355_colour_tone* q, const uint32_t rgb16[3], int samples, uint32_t out[3])
{
  if (!t || !q || !rgb16 || !out || (samples != M355_RGB_U8 && samples != M355_RGB_U16) || m355_ct_tables_check(t) || m355_ct_tone_check(q))
    return fail(M355_ERR_INVALID, "m355_colour_pixel_tone: null pointer, unknown samples %d, or tables / tone outside their bounds", samples);
  m355_ct_pixel_tone(t, q, rgb16, samples, out);
  return M355_OK;
}
/* The same resize with the R'G'B' conversion of the resized picture behind it, in one launch (k_export_resized_rgb.hip, RR_FRAME): the frame handle and
 * the rectangle are checked by export_plan — with destinations that cannot fail —, the output size and the ratio as for the resized export, the
 * conversion and the destinations as for the R'G'B' export, with the OUTPUT width. */
int m355_frame_export_resized_rgb_opts(m355_ctx* c, int h, const m355_resize_rgb_desc* e, const m355_export_opts* opts)
{
  const char* who = "m355_frame_export_resized_rgb";
  ExportPlan P;
  int rc = export_plan_rect(c, h, e, e, who, P);
  if (rc) return rc;
  Frame* f = P.f;
  m355_export_opts o;
  ColourArgs colour = {};
  rc = opts_check(who, c, opts, f, true, o, &colour);
  if (rc) return rc;
  const int filter = o.filter;
  rc = resize_check(who, &P, 0, e->out_width, e->out_height, filter);
  if (rc) return rc;
  ExportResizedRgbArgs a = {};
  bool planar = false;
  int db = 1;
  rc = rgb_desc_check(who, e, f, e->out_width, a, &planar, &db);
  if (rc) return rc;
  if ((rc = colour_apply(colour, e, f, a)) != 0) return rc;
  plan_sources(P, a);
  plan_geometry(P, e->out_width, e->out_height, filter, o.chroma_loc, a, a);
  a.cf = f->cf; a.planar = planar; a.bdl = f->bdl; a.bdc = f->bdc; a.chroma_loc = o.chroma_loc;
  return export_launch(c, f, a, [&](hipStream_t cs) { m355_launch_export_resized_rgb(a, f->bpp[0], db, filter, cs); });
}
int m355_frame_export_resized_rgb_filtered(m355_ctx* c, int h, const m355_resize_rgb_desc* e, int filter)
{
  const m355_export_opts o = filter_opts(filter);
  return m355_frame_export_resized_rgb_opts(c, h, e, &o);
}
int m355_frame_export_resized_rgb(m355_ctx* c, int h, const m355_resize_rgb_desc* e) { return m355_frame_export_resized_rgb_opts(c, h, e, nullptr); }
/* The pixel formats (pixel_pack.h): the two R'G'B' exports above with a pixel of 3 or 4 bytes in place of three elements.  The descriptor check behind
 * the plan, the options and (resized) the resize check: the format and its alpha, the conversion of the format's channel bits (into k), the destination
 * of rows of `width` pixels, whole dwords for the 4-byte formats. */
static int pixel_desc_check(const char* who, const m355_pixel_desc* e, const Frame* f, int64_t width, m355_rgb_coeffs* k)
{
  if (!m355_pp_known(e->format)) return fail(M355_ERR_INVALID, "%s: unknown pixel format %d", who, e->format);
  if (e->alpha < 0 || (uint32_t)e->alpha > m355_pp_alpha_max(e->format)) return fail(M355_ERR_INVALID, "%s: alpha %d is not 0..%u (format %d)", who, e->alpha, m355_pp_alpha_max(e->format), e->format);
  int rc = m355_rgb_coefficients(e->matrix, e->full_range, f->bdl, f->bdc, m355_pp_ten(e->format) ? M355_RGB_U16 : M355_RGB_U8, k);
  if (rc) return rc;
  const int bpp = m355_pp_bytes(e->format);
  if ((rc = dst_check(who, 0, e->dst, e->pitch, width * bpp, 1)) != 0) return rc;
  if (bpp == 4 && (((uintptr_t)e->dst | (uint64_t)e->pitch) & 3)) return fail(M355_ERR_INVALID, "%s: 4-byte pixels at an address or a pitch that is no multiple of 4", who);
  return M355_OK;
}
/* (k_export_rgb.hip: k_export_pixels for the 4-byte formats, the packed U8 path of k_export_rgb for BGR8.)  B, G, R order is R, G, B of the frame with
 * Cb and Cr and their coefficients exchanged — R = cy y + crv v and B = cy y + cbu u change places, G's sum keeps its terms —, so the kernels have
 * one channel order. */
static int pixels_plan(const char* who, m355_ctx* c, int h, const m355_pixel_desc* e, const m355_export_opts* opts, bool transposed, Frame** fo, ExportRgbArgs& a,
                       m355_export_opts& o)
{
  ExportPlan P;
  int rc = export_plan_rect(c, h, e, e ? e->dst : nullptr, who, P);
  if (rc) return rc;
  Frame* f = P.f;
  rc = opts_check(who, c, opts, f, false, o);
  if (rc) return rc;
  if (e->out_width || e->out_height) return fail(M355_ERR_INVALID, "%s: output size %dx%d in a call that resizes nothing", who, e->out_width, e->out_height);
  const int sb = f->bpp[0];
  const int64_t w = P.p[0].pw;
  rc = pixel_desc_check(who, e, f, transposed ? P.p[0].ph : w, &a.k);
  if (rc) return rc;
  a.dst[0] = (uint8_t*)e->dst; a.dst_pitch[0] = e->pitch;
  for (int p = 0; p < 3; p++) a.src[p] = (const uint8_t*)f->plane[p];
  if (m355_pp_swapped(e->format)) { std::swap(a.src[1], a.src[2]); std::swap(a.k.crv, a.k.cbu); std::swap(a.k.cgu, a.k.cgv); }
  a.src_pitch[0] = (long long)f->stride[0] * sb; a.src_pitch[1] = (long long)f->stride[1] * sb;
  a.x0 = e->width ? (uint32_t)e->x0 : 0u; a.y0 = e->width ? (uint32_t)e->y0 : 0u;
  a.width = (uint32_t)w; a.height = (uint32_t)P.p[0].ph;
  a.cw = (uint32_t)f->pw[1]; a.ch = (uint32_t)f->ph[1];
  const uint32_t per_chunk = 64u * 16u / (uint32_t)sb;
  a.chunks = (a.width + per_chunk - 1) / per_chunk;
  a.units = a.chunks * a.height;
  a.alpha_bits = m355_pp_alpha_bits(e->format, (uint32_t)e->alpha);
  *fo = f;
  return M355_OK;
}
int m355_frame_export_pixels(m355_ctx* c, int h, const m355_pixel_desc* e, const m355_export_opts* opts)
{
  Frame* f = nullptr;
  ExportRgbArgs a = {};
  m355_export_opts o;
  int rc = pixels_plan("m355_frame_export_pixels", c, h, e, opts, false, &f, a, o);
  if (rc) return rc;
  const int format = e->format, sb = f->bpp[0];
  return export_launch(c, f, a, [&](hipStream_t cs) {
    if (m355_pp_bytes(format) == 3) m355_launch_export_rgb(a, sb, 1, false, f->cf, o.chroma_loc, cs);
    else m355_launch_export_pixels(a, sb, m355_pp_ten(format), f->cf, o.chroma_loc, cs);
  });
}
/* The pixels of m355_frame_export_pixels permuted as whole pixels (k_export_oriented.hip): that call's plan — with TRANSPOSE the pitch checked against
 * height * 4 — and, with TRANSPOSE, tiles of the rectangle in place of its chunks.  Orientation 0 is m355_frame_export_pixels itself. */
int m355_frame_export_pixels_oriented(m355_ctx* c, int h, const m355_pixel_desc* e, const m355_export_opts* opts, int orientation)
{
  const char* who = "m355_frame_export_pixels_oriented";
  if (!m355_or_known(orientation)) return fail(M355_ERR_INVALID, "%s: orientation %d is not 0..7", who, orientation);
  if (orientation == 0) return m355_frame_export_pixels(c, h, e, opts);
  if (e && e->format == M355_PIXEL_BGR8) return fail(M355_ERR_INVALID, "%s: M355_PIXEL_BGR8 with an orientation (a 3-byte element)", who);
  Frame* f = nullptr;
  ExportPixelsOrientedArgs a = {};
  m355_export_opts o;
  const bool tr = m355_or_transpose(orientation);
  int rc = pixels_plan(who, c, h, e, opts, tr, &f, a.r, o);
  if (rc) return rc;
  if (tr) {
    a.r.chunks = (a.r.width + M355_ORIENT_TILE - 1) / M355_ORIENT_TILE;
    a.r.units = a.r.chunks * ((a.r.height + M355_ORIENT_TILE - 1) / M355_ORIENT_TILE);
  }
  a.mirror = m355_or_mirror(orientation); a.flip = m355_or_flip(orientation); a.transpose = tr;
  const bool ten = m355_pp_ten(e->format);
  return export_launch(c, f, a.r, [&](hipStream_t cs) { m355_launch_export_pixels_oriented(a, f->bpp[0], ten, f->cf, o.chroma_loc, cs); });
}
/* (k_export_resized_rgb.hip, RR_FRAME with PX: the colour stage sits between the matrix and the pack, so the channel order is the kernel's here.) */
int m355_frame_export_resized_pixels(m355_ctx* c, int h, const m355_pixel_desc* e, const m355_export_opts* opts)
{
  const char* who = "m355_frame_export_resized_pixels";
  ExportPlan P;
  int rc = export_plan_rect(c, h, e, e ? e->dst : nullptr, who, P);
  if (rc) return rc;
  Frame* f = P.f;
  m355_export_opts o;
  ColourArgs colour = {};
  rc = opts_check(who, c, opts, f, true, o, &colour);
  if (rc) return rc;
  const int filter = o.filter;
  rc = resize_check(who, &P, 0, e->out_width, e->out_height, filter);
  if (rc) return rc;
  ExportResizedRgbArgs a = {};
  rc = pixel_desc_check(who, e, f, e->out_width, &a.k);
  if (rc) return rc;
  a.dst[0] = (uint8_t*)e->dst; a.dst_pitch[0] = e->pitch;
  if ((rc = colour_apply(colour, e, f, a)) != 0) return rc;
  plan_sources(P, a);
  plan_geometry(P, e->out_width, e->out_height, filter, o.chroma_loc, a, a);
  a.cf = f->cf; a.planar = 0; a.bdl = f->bdl; a.bdc = f->bdc; a.chroma_loc = o.chroma_loc;
  a.px_bytes = (uint32_t)m355_pp_bytes(e->format); a.px_swapped = m355_pp_swapped(e->format) ? 1u : 0u;
  a.px_alpha_bits = m355_pp_alpha_bits(e->format, (uint32_t)e->alpha);
  const bool ten = m355_pp_ten(e->format);
  return export_launch(c, f, a, [&](hipStream_t cs) { m355_launch_export_resized_pixels(a, f->bpp[0], ten, filter, cs); });
}
/* one pixel's bytes (pixel_pack.h: the function the kernels call) */
int m355_pixel_pack(int format, const uint32_t rgb[3], uint32_t alpha, uint8_t out[4], int* n_bytes)
{
  if (!rgb || !out || !n_bytes || !m355_pp_known(format)) return fail(M355_ERR_INVALID, "m355_pixel_pack: null pointer / unknown format %d", format);
  const uint32_t top = m355_pp_channel_max(format);
  if (rgb[0] > top || rgb[1] > top || rgb[2] > top || alpha > m355_pp_alpha_max(format))
    return fail(M355_ERR_INVALID, "m355_pixel_pack: a channel above %u or alpha %u above %u (format %d)", top, alpha, m355_pp_alpha_max(format), format);
  const uint32_t dw = m355_pp_pixel(m355_pp_ten(format), m355_pp_swapped(format), rgb, m355_pp_alpha_bits(format, alpha));
  const int n = m355_pp_bytes(format);
  for (int i = 0; i < n; i++) out[i] = (uint8_t)(dw >> (8 * i));
  *n_bytes = n;
  return M355_OK;
}
/* the float stage of m355_frames_export_tensor for one value (tensor_element.h: the function the kernel calls) */
int m355_tensor_element(uint32_t v, float scale, float bias, int dtype, uint32_t* bits)
{
  const auto finite = [](float x) { return (m355_te_bits(x) & 0x7F800000u) != 0x7F800000u; };
  if (!bits || (dtype != M355_TENSOR_F32 && dtype != M355_TENSOR_F16 && dtype != M355_TENSOR_BF16) || !finite(scale) || !finite(bias))
    return fail(M355_ERR_INVALID, "m355_tensor_element: null result / unknown dtype %d / scale or bias not finite", dtype);
  *bits = m355_te_element(v, scale, bias, dtype);
  return M355_OK;
}
/* A batch of frames resized, converted, normalised and delivered as one float tensor in one launch (k_export_resized_rgb.hip, RR_BATCH).  Every frame's
 * handle and the rectangle in it are checked by export_plan — with destinations that cannot fail —, the output size, the ratio and the conversion as for
 * m355_frame_export_resized_rgb, the tensor's layout by tensor_desc_check. */
int m355_frames_export_tensor_opts(m355_ctx* c, const int* frames, int n, const m355_tensor_desc* e, const m355_export_opts* opts)
{
  const char* who = "m355_frames_export_tensor";
  if (!c || !frames || !e || n < 1 || n > M355_TENSOR_MAX_FRAMES) return fail(M355_ERR_INVALID, "%s: no context / frames / descriptor, or %d frames are not 1..%d", who, n, M355_TENSOR_MAX_FRAMES);
  ExportPlan P[M355_TENSOR_MAX_FRAMES];
  int rc, eb = 0;
  for (int i = 0; i < n; i++) {
    if ((rc = export_plan_rect(c, frames[i], e, e, who, P[i])) != 0) return rc;
    if ((rc = batch_frame_check(who, frames, i, P, e->width == 0)) != 0) return rc;
  }
  m355_export_opts o;
  ColourArgs colour = {};
  if ((rc = opts_check(who, c, opts, P[0].f, true, o, &colour)) != 0) return rc;
  const int filter = o.filter;
  if ((rc = resize_check(who, P, 0, e->out_width, e->out_height, filter)) != 0) return rc;
  ExportTensorArgs a = {};
  if ((rc = tensor_desc_check(who, e, n, P[0].f, a, &eb)) != 0) return rc;
  if ((rc = colour_apply(colour, e, P[0].f, a)) != 0) return rc;
  plan_geometry(P[0], e->out_width, e->out_height, filter, o.chroma_loc, a, a);
  a.chroma_loc = o.chroma_loc;
  for (int i = 0; i < n; i++) plan_sources(P[i], a.fr[i]);
  return batch_launch(c, P, n, a, [&](hipStream_t cs) { m355_launch_export_tensor(a, P[0].f->bpp[0], eb, filter, cs); });
}
int m355_frames_export_tensor_filtered(m355_ctx* c, const int* frames, int n, const m355_tensor_desc* e, int filter)
{
  const m355_export_opts o = filter_opts(filter);
  return m355_frames_export_tensor_opts(c, frames, n, e, &o);
}
int m355_frames_export_tensor(m355_ctx* c, const int* frames, int n, const m355_tensor_desc* e) { return m355_frames_export_tensor_opts(c, frames, n, e, nullptr); }
/* A batch of REGIONS, one rectangle per slice, as one float tensor in one launch (k_export_resized_rgb.hip, RR_ROIS): slice i is what
 * m355_frames_export_tensor delivers for frames[i] alone with rois[i] as the rectangle, its columns reversed under M355_ROI_MIRROR.  Every entry's
 * handle and rectangle are checked by export_plan against ITS frame, the ratio per entry; tile width, tiles and units are resize_rgb_tile_w's for the
 * entry's own source size. */
int m355_frames_export_tensor_rois_opts(m355_ctx* c, const int* frames, const m355_tensor_roi* rois, int n, const m355_tensor_desc* e, const m355_export_opts* opts)
{
  const char* who = "m355_frames_export_tensor_rois";
  if (!c || !frames || !rois || !e || n < 1 || n > M355_TENSOR_MAX_FRAMES)
    return fail(M355_ERR_INVALID, "%s: no context / frames / rois / descriptor, or %d entries are not 1..%d", who, n, M355_TENSOR_MAX_FRAMES);
  if (e->x0 || e->y0 || e->width || e->height)
    return fail(M355_ERR_INVALID, "%s: the descriptor's rectangle %d,%d %dx%d must be zero (the rectangles are the entries')", who, e->x0, e->y0, e->width, e->height);
  ExportPlan P[M355_TENSOR_MAX_FRAMES];
  int rc, eb = 0;
  for (int i = 0; i < n; i++) {
    if (rois[i].flags & ~M355_ROI_MIRROR) return fail(M355_ERR_INVALID, "%s: unknown flags 0x%x of entry %d", who, (unsigned)rois[i].flags, i);
    if ((rc = export_plan_rect(c, frames[i], &rois[i], e, who, P[i])) != 0) return rc;
    if ((rc = batch_frame_check(who, frames, i, P, false)) != 0) return rc;
  }
  m355_export_opts o;
  ColourArgs colour = {};
  if ((rc = opts_check(who, c, opts, P[0].f, true, o, &colour)) != 0) return rc;
  const int filter = o.filter;
  if ((rc = resize_check(who, P, n, e->out_width, e->out_height, filter)) != 0) return rc;
  ExportTensorRoisArgs a = {};
  if ((rc = tensor_desc_check(who, e, n, P[0].f, a, &eb)) != 0) return rc;
  if ((rc = colour_apply(colour, e, P[0].f, a)) != 0) return rc;
  a.chroma_loc = o.chroma_loc;
  for (int i = 0; i < n; i++) {
    ExportTensorRoi& r = a.fr[i];
    plan_sources(P[i], r);
    plan_geometry(P[i], e->out_width, e->out_height, filter, o.chroma_loc, r, a);
    r.flags = (uint32_t)rois[i].flags;
    if (r.units > a.max_units) a.max_units = r.units;
  }
  return batch_launch(c, P, n, a, [&](hipStream_t cs) { m355_launch_export_tensor_rois(a, P[0].f->bpp[0], eb, filter, cs); });
}
int m355_frames_export_tensor_rois_filtered(m355_ctx* c, const int* frames, const m355_tensor_roi* rois, int n, const m355_tensor_desc* e, int filter)
{
  const m355_export_opts o = filter_opts(filter);
  return m355_frames_export_tensor_rois_opts(c, frames, rois, n, e, &o);
}
int m355_frames_export_tensor_rois(m355_ctx* c, const int* frames, const m355_tensor_roi* rois, int n, const m355_tensor_desc* e)
{
  return m355_frames_export_tensor_rois_opts(c, frames, rois, n, e, nullptr);
}
/* the host waits until this frame's last export has landed */
int m355_frame_export_wait(m355_ctx* c, int h)
{
  Frame* f = get_frame(c, h);
  if (!f) return fail(M355_ERR_INVALID, "bad frame handle %d", h);
  hipSetDevice(c->device);
  HIPCHK(ev_sync(c, f->reader[RD_EXPORT]));
  f->reader[RD_EXPORT] = EvRef();
  return M355_OK;
}
/* the consumer's stream continues behind this frame's last export (nothing to enqueue when that has long passed: its mark has left the ring) */
int m355_frame_export_order(m355_ctx* c, int h, void* consumer)
{
  Frame* f = get_frame(c, h);
  if (!f) return fail(M355_ERR_INVALID, "bad frame handle %d", h);
  hipSetDevice(c->device);
  ev_wait(c, (hipStream_t)consumer, f->reader[RD_EXPORT]);
  return M355_OK;
}
} /* extern "C" */
