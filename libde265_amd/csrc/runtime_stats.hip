/*
 * runtime_stats.hip — host side of the statistics requests (m355_frame_stats_async / m355_frame_stats_result, include/de265_mi355x.h): the comparison
 * requests' machinery (runtime.hip) with another kernel (k_stats.hip), one frame to read, and slots, tickets and a reader kind (RD_STATS) of their own —
 * and the two host-only helpers that go with the result, m355_stats_quantile and m355_colour_linear.
 */
#include "runtime_internal.h"
#include "colour_transform.h"
#include "stats_quantile.h"

/* the slots: device records (zeroed here, once: every request leaves its record zero), pinned result records */
int stats_requests_create(m355_ctx* c)
{
  hipStream_t st = c->lanes[0].stream;
  HIPCHK(hipMalloc(&c->stats_rec, M355_STATS_REQUESTS * STATS_REC_WORDS * sizeof(uint32_t)));
  HIPCHK(hipMemsetAsync(c->stats_rec, 0, M355_STATS_REQUESTS * STATS_REC_WORDS * sizeof(uint32_t), st));
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipHostMalloc(&c->stats_res, M355_STATS_REQUESTS * STATS_REC_WORDS * sizeof(uint32_t), hipHostMallocDefault));
  memset(c->stats_res, 0, M355_STATS_REQUESTS * STATS_REC_WORDS * sizeof(uint32_t));
  return M355_OK;
}
/* (behind sync_all: nothing is in flight; requests nobody collected are dropped) */
void stats_requests_destroy(m355_ctx* c)
{
  for (auto& s : c->stats_slot) s = m355_ctx::StatsSlot();
  if (c->stats_rec) hipFree(c->stats_rec);
  if (c->stats_res) hipHostFree(c->stats_res);
  c->stats_rec = c->stats_res = nullptr;
}

static m355_ctx::StatsSlot* stats_slot_of(m355_ctx* c, unsigned long long ticket)
{
  if (ticket) for (auto& s : c->stats_slot) if (s.ticket == ticket) return &s;
  return nullptr;
}
/* collected behind its mark: the next decode into the frame has nothing to wait for, if the frame's mark is still this request's (meas_slot_free) */
static void stats_slot_free(m355_ctx* c, m355_ctx::StatsSlot& s)
{
  Frame* f = get_frame(c, s.frame);
  if (f && s.mark.ticket && f->reader[RD_STATS].ticket == s.mark.ticket) f->reader[RD_STATS] = EvRef();
  s = m355_ctx::StatsSlot();
}

/* Enqueue only: the host waits for nothing here.  A READER of the frame of the kind RD_STATS (reader_begin): the kernel runs on the stream of the frame's
   last writer, and the next decode into the frame waits for the request's mark, which the slot remembers for m355_frame_stats_result. */
int m355_frame_stats_async(m355_ctx* c, int h, const m355_stats_desc* e, unsigned long long* ticket)
{
  const char* who = "m355_frame_stats_async";
  Frame* f = c ? get_frame(c, h) : nullptr;
  if (!f || !e || !ticket) return fail(M355_ERR_INVALID, "%s: bad frame handle %d / null descriptor / null ticket", who, h);
  if (c->shard_n > 0) return fail(M355_ERR_INVALID, "%s: not on a tile-sharded context (its frames are complete only behind the gather)", who);
  const int sw = (f->cf == 1 || f->cf == 2) ? 2 : 1, sh = f->cf == 1 ? 2 : 1;
  int x0 = 0, y0 = 0, w = f->w, hgt = f->h;
  if (e->width != 0) {
    x0 = e->x0; y0 = e->y0; w = e->width; hgt = e->height;
    if (x0 < 0 || y0 < 0 || w <= 0 || hgt <= 0 || x0 > f->w - w || y0 > f->h - hgt) return fail(M355_ERR_INVALID, "%s: rectangle %d,%d %dx%d leaves the %dx%d frame", who, x0, y0, w, hgt, f->w, f->h);
    if (f->cf && ((x0 | w) % sw || (y0 | hgt) % sh)) return fail(M355_ERR_INVALID, "%s: rectangle %d,%d %dx%d is not aligned to the chroma grid (%dx%d luma samples)", who, x0, y0, w, hgt, sw, sh);
  }
  if (e->black < 0 || e->black > (1 << f->bdl) - 1) return fail(M355_ERR_INVALID, "%s: black %d is not a luma sample of %d bits", who, e->black, f->bdl);
  if (e->light != 0 && e->light != 1) return fail(M355_ERR_INVALID, "%s: light %d is not 0 or 1", who, e->light);
  for (int i = 0; i < 7; i++) if (e->reserved[i]) return fail(M355_ERR_INVALID, "%s: reserved[%d] is %d, not 0", who, i, e->reserved[i]);
  StatsArgs a = {};
  if (e->light) {
    if (e->chroma_loc < 0 || e->chroma_loc > 3) return fail(M355_ERR_INVALID, "%s: chroma sample location type %d is not 0..3", who, e->chroma_loc);
    if (e->chroma_loc && f->cf != 1) return fail(M355_ERR_INVALID, "%s: chroma sample location type %d for a frame that is not 4:2:0", who, e->chroma_loc);
    const int rc = m355_rgb_coefficients(e->matrix, e->full_range, f->bdl, f->cf ? f->bdc : f->bdl, M355_RGB_U16, &a.k);
    if (rc) return rc;
  } else if (e->matrix || e->full_range || e->chroma_loc)
    return fail(M355_ERR_INVALID, "%s: matrix %d / full_range %d / chroma_loc %d with light == 0", who, e->matrix, e->full_range, e->chroma_loc);
  const int np = f->cf == 0 ? 1 : 3, sb = f->bpp[0];
  uint64_t total = 0;
  for (int p = 0; p < np; p++) {
    StatsPart& t = a.part[p];
    const int pw = p ? w / sw : w, ph = p ? hgt / sh : hgt, px = p ? x0 / sw : x0, py = p ? y0 / sh : y0;
    t.pitch = (long long)f->stride[p] * sb;
    t.p = (const uint8_t*)f->plane[p] + (size_t)py * t.pitch + (size_t)px * sb;
    t.row_bytes = (uint32_t)(pw * sb); t.rows = (uint32_t)ph;
    t.chunks = (t.row_bytes + 1023u) / 1024u; t.units = t.chunks * t.rows;
    t.shift = (uint32_t)((p ? f->bdc : f->bdl) - 8);
    total += (uint64_t)t.units * (p == 0 && e->light ? STATS_LIGHT_WEIGHT : 1);
  }
  /* the wavefronts are shared out by weighted units, so that the parts end together */
  for (int p = 0; p < 3; p++) {
    StatsPart& t = a.part[p];
    t.first_wg = a.n_wg;
    if (p >= np) continue;
    const uint64_t weight = p == 0 && e->light ? STATS_LIGHT_WEIGHT : 1;
    const uint64_t waves = std::max<uint64_t>(1, std::min<uint64_t>(t.units, (uint64_t)STATS_TARGET_WAVES * t.units * weight / total));
    t.units_per_wave = (uint32_t)((t.units + waves - 1) / waves);
    a.n_wg += (uint32_t)(((t.units + t.units_per_wave - 1) / t.units_per_wave + STATS_WAVES - 1) / STATS_WAVES);
  }
  a.px = (uint32_t)x0; a.py = (uint32_t)y0; a.black = (uint32_t)e->black;
  for (int p = 0; p < 3; p++) a.src[p] = (const uint8_t*)f->plane[p];
  a.src_pitch[0] = (long long)f->stride[0] * sb; a.src_pitch[1] = (long long)f->stride[1] * sb;
  a.cw = (uint32_t)f->pw[1]; a.ch = (uint32_t)f->ph[1];
  a.x0 = (uint32_t)x0; a.y0 = (uint32_t)y0; a.width = (uint32_t)w; a.height = (uint32_t)hgt;
  m355_ctx::StatsSlot* s = nullptr;
  for (auto& x : c->stats_slot) if (!x.ticket) { s = &x; break; }
  if (!s) return fail(M355_ERR_BUSY, "%s: %d requests outstanding (collect one: m355_frame_stats_result)", who, M355_STATS_REQUESTS);
  const int slot = (int)(s - c->stats_slot);
  hipSetDevice(c->device);
  StatsReq q = {};
  q.rec = c->stats_rec + slot * STATS_REC_WORDS;
  q.res = c->stats_res + slot * STATS_REC_WORDS;
  q.seq = (uint32_t)(c->stats_ticket + 1);
  q.res[STATS_ARRIVED] = STATS_RES_NONE;                                        /* (the slot is idle: nothing in flight writes its record) */
  const hipStream_t cs = reader_begin(c, f, RD_STATS, &q.timeout, &q.epoch);
  m355_launch_stats(a, q, sb, e->light, f->cf, e->chroma_loc, cs);
  if (hipGetLastError() != hipSuccess || reader_end(c, f, RD_STATS, cs) != M355_OK) { stats_slot_free(c, *s); return fail(M355_ERR_HIP, "%s: launch failed", who); }
  s->mark = f->reader[RD_STATS]; s->frame = h; s->np = np; s->light = e->light;
  s->ticket = ++c->stats_ticket;
  *ticket = s->ticket;
  return M355_OK;
}

int m355_frame_stats_result(m355_ctx* c, unsigned long long ticket, int block, m355_stats* out)
{
  m355_ctx::StatsSlot* s = c ? stats_slot_of(c, ticket) : nullptr;
  if (!s) return fail(M355_ERR_INVALID, "m355_frame_stats_result: ticket %llu is unknown or was collected", ticket);
  if (!out) return fail(M355_ERR_INVALID, "m355_frame_stats_result: null result");
  hipSetDevice(c->device);
  if (block) HIPCHK(ev_sync(c, s->mark));                                       /* this request's mark only */
  else {
    const hipError_t e = ev_query(c, s->mark);
    if (e == hipErrorNotReady) return M355_ERR_BUSY;
    if (e != hipSuccess) return fail(M355_ERR_HIP, "hipEventQuery failed: %s", hipGetErrorString(e));
  }
  const uint32_t* res = c->stats_res + (s - c->stats_slot) * STATS_REC_WORDS;
  const uint32_t state = res[STATS_ARRIVED], seq = res[STATS_ARRIVED + 1];
  if (state == STATS_RES_GATED && seq == (uint32_t)ticket) {
    stats_slot_free(c, *s);
    return fail(M355_ERR_INVALID, "statistics request %llu was queued behind a decode whose lists were rejected: no value", ticket);
  }
  if (state != STATS_RES_VALID || seq != (uint32_t)ticket) {
    stats_slot_free(c, *s);
    return fail(M355_ERR_HIP, "statistics request %llu finished without a result (state %u, sequence %u)", ticket, state, seq);
  }
  const auto u64 = [&](int word) { return (uint64_t)res[word] | ((uint64_t)res[word + 1] << 32); };
  memset(out, 0, sizeof(*out));
  for (int p = 0; p < s->np; p++) {
    memcpy(out->hist[p], res + STATS_HIST + 256 * p, 256 * sizeof(uint32_t));
    out->min[p] = res[STATS_MIN + p] ? ~res[STATS_MIN + p] : 0u;                 /* (the record holds ~min; a rectangle has at least one sample) */
    out->max[p] = res[STATS_MAX + p];
    out->sum[p] = u64(STATS_SUM + 2 * p); out->sum_sq[p] = u64(STATS_SQ + 2 * p);
  }
  out->n_active = u64(STATS_NACT);
  for (int k = 0; k < 4; k++) out->box[k] = -1;
  if (out->n_active) {
    out->box[0] = (int32_t)~res[STATS_BOX + 0]; out->box[1] = (int32_t)~res[STATS_BOX + 1];
    out->box[2] = (int32_t)res[STATS_BOX + 2] - 1; out->box[3] = (int32_t)res[STATS_BOX + 3] - 1;
  }
  if (s->light) {
    memcpy(out->light_hist, res + STATS_HIST + 256 * 3, 256 * sizeof(uint32_t));
    out->light_min = res[STATS_MIN + 3] ? ~res[STATS_MIN + 3] : 0u;
    out->light_max = res[STATS_MAX + 3];
    out->light_sum = u64(STATS_SUM + 2 * 3);
  }
  stats_slot_free(c, *s);
  return M355_OK;
}

int m355_stats_quantile(const uint32_t hist[M355_STATS_BINS], uint32_t num, uint32_t den, int* bin)
{
  const int b = bin ? m355_sq_quantile(hist, num, den) : -1;
  if (b < 0) return fail(M355_ERR_INVALID, "m355_stats_quantile: null pointer, an empty histogram, or not 0 < num (%u) <= den (%u) <= 1 << 20", num, den);
  *bin = b;
  return M355_OK;
}

int m355_colour_linear(const m355_colour_tables* t, uint32_t v16, uint32_t* L)
{
  if (!t || !L || v16 > 65535u || m355_ct_tables_check(t)) return fail(M355_ERR_INVALID, "m355_colour_linear: null pointer, a value above 65535 (%u), or tables outside their bounds", v16);
  *L = m355_ct_linear_of(t, v16);
  return M355_OK;
}
