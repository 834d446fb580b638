/*
 * runtime_msssim.hip — host side of the MS-SSIM requests (m355_frame_msssim_async / m355_frame_msssim_result, include/de265_mi355x.h): the SSIM
 * requests' machinery (runtime_ssim.hip) with the two launches of k_msssim.hip, slots, tickets and a reader kind (RD_MSSSIM) of their own, the
 * slots' scratch for the levels between the launches — and the two host-only helpers, m355_ssim_window_cs (ssim_window.h) and
 * m355_msssim_combine, which collection itself uses for the number it reports.
 */
#include "runtime_internal.h"
#include "ssim_window.h"

#define MSSSIM_ALIGN 256   /* every level picture starts on a multiple of this in the slot's scratch */

int msssim_requests_create(m355_ctx* c)
{
  hipStream_t st = c->lanes[0].stream;
  const size_t bytes = M355_MSSSIM_REQUESTS * MSSSIM_REC_WORDS * sizeof(unsigned long long);
  HIPCHK(hipMalloc(&c->msssim_rec, bytes));
  HIPCHK(hipMemsetAsync(c->msssim_rec, 0, bytes, st));
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipHostMalloc(&c->msssim_res, bytes, hipHostMallocDefault));
  memset(c->msssim_res, 0, bytes);
  return M355_OK;
}
/* (behind sync_all: nothing is in flight; requests nobody collected are dropped) */
void msssim_requests_destroy(m355_ctx* c)
{
  for (auto& s : c->msssim_slot) s = m355_ctx::MsssimSlot();
  for (int k = 0; k < M355_MSSSIM_REQUESTS; k++) {
    if (c->msssim_scratch[k]) hipFree(c->msssim_scratch[k]);
    c->msssim_scratch[k] = nullptr; c->msssim_scratch_cap[k] = 0;
  }
  if (c->msssim_rec) hipFree(c->msssim_rec);
  if (c->msssim_res) hipHostFree(c->msssim_res);
  c->msssim_rec = c->msssim_res = nullptr;
}

static m355_ctx::MsssimSlot* msssim_slot_of(m355_ctx* c, unsigned long long ticket)
{
  if (ticket) for (auto& s : c->msssim_slot) if (s.ticket == ticket) return &s;
  return nullptr;
}
/* collected behind its mark: the next decode into either frame has nothing to wait for, if the frame's mark is still this request's (ssim_slot_free) */
static void msssim_slot_free(m355_ctx* c, m355_ctx::MsssimSlot& s)
{
  for (int k = 0; k < 2; k++) {
    Frame* f = get_frame(c, s.frame[k]);
    if (f && s.mark.ticket && f->reader[RD_MSSSIM].ticket == s.mark.ticket) f->reader[RD_MSSSIM] = EvRef();
  }
  s = m355_ctx::MsssimSlot();
}

/* Enqueue only, ordered as m355_frame_ssim_async orders its request; the two launches follow one another on the one stream, and ONE mark behind the
   second is kept by both frames and by the slot. */
int m355_frame_msssim_async(m355_ctx* c, int h, const m355_msssim_desc* e, unsigned long long* ticket)
{
  const char* who = "m355_frame_msssim_async";
  PairGeom g = {};
  const int grc = pair_geometry(c, who, h, e && ticket, e ? e->ref_frame : -1, e ? e->x0 : 0, e ? e->y0 : 0, e ? e->width : 0, e ? e->height : 0,
                                e ? e->ref : nullptr, e ? e->pitch : nullptr, &g);
  if (grc) return grc;
  Frame *f = g.f, *r = g.r;
  for (int i = 0; i < 6; i++) if (e->reserved[i]) return fail(M355_ERR_INVALID, "%s: reserved[%d] is %d, not 0", who, i, e->reserved[i]);
  if (e->planes < 0 || e->planes > 7) return fail(M355_ERR_INVALID, "%s: planes %d has bits above plane 2", who, e->planes);
  if (e->planes >> g.np) return fail(M355_ERR_INVALID, "%s: planes %d selects a plane the frame does not have", who, e->planes);
  if (e->levels < 1 || e->levels > M355_MSSSIM_LEVELS) return fail(M355_ERR_INVALID, "%s: levels %d is outside 1..%d", who, e->levels, M355_MSSSIM_LEVELS);
  const int sel = e->planes ? e->planes : (1 << g.np) - 1;
  const int L = e->levels, sb = f->bpp[0];
  MsssimArgs a = {};
  MsssimLevelArgs lv = {};
  uint64_t n[3][M355_MSSSIM_LEVELS] = {};
  size_t off[3][2][MSSSIM_LEVELS - 1] = {};    /* where level j of plane p, side s lies in the scratch */
  size_t need = 0;
  int nwg = 0, nwg2 = 0;
  for (int p = 0; p < 3; p++) {
    a.first[p] = nwg;
    if (!(p < g.np && ((sel >> p) & 1))) continue;
    const PairPlane& gp = g.pl[p];
    if ((gp.pw >> (L - 1)) < M355_SSIM_TAPS || (gp.ph >> (L - 1)) < M355_SSIM_TAPS)
      return fail(M355_ERR_INVALID, "%s: plane %d of the rectangle has %dx%d samples, which leaves %dx%d on level %d, below one 11x11 window", who, p, gp.pw, gp.ph,
                  gp.pw >> (L - 1), gp.ph >> (L - 1), L - 1);
    const double c1 = m355_ssim_c1(p ? f->bdc : f->bdl), c2 = m355_ssim_c2(p ? f->bdc : f->bdl);
    MsssimPlane& m = a.pl[p];
    m.a = gp.a; m.b = gp.b; m.pitch_a = gp.pitch_a; m.pitch_b = gp.pitch_b;
    m.pw = gp.pw; m.ph = gp.ph;
    m.tiles_x = (gp.pw + SSIM_TILE_W - 1) / SSIM_TILE_W;                        /* by samples: every tile owes the pyramid its block */
    m.acc = MSSSIM_LEVELS * p;
    m.c1 = c1; m.c2 = c2;
    n[p][0] = (uint64_t)(gp.pw - 10) * (gp.ph - 10);
    nwg += m.tiles_x * ((gp.ph + SSIM_TILE_H - 1) / SSIM_TILE_H);
    for (int j = 1; j < L; j++) {
      const int lw = gp.pw >> j, lh = gp.ph >> j;
      for (int s = 0; s < 2; s++) {
        off[p][s][j - 1] = need;
        need += ((size_t)lw * lh * sb + MSSSIM_ALIGN - 1) & ~(size_t)(MSSSIM_ALIGN - 1);
      }
      MsssimLevel& x = lv.lv[lv.n];
      x.pw = lw; x.ph = lh;
      x.tiles_x = (lw - 10 + SSIM_TILE_W - 1) / SSIM_TILE_W;
      x.acc = MSSSIM_LEVELS * p + j;
      x.c1 = c1; x.c2 = c2;
      n[p][j] = (uint64_t)(lw - 10) * (lh - 10);
      lv.first[lv.n++] = nwg2;
      nwg2 += x.tiles_x * ((lh - 10 + SSIM_TILE_H - 1) / SSIM_TILE_H);
    }
  }
  a.first[3] = nwg;
  lv.first[lv.n] = nwg2;
  a.levels = L;
  a.arrivals = lv.arrivals = nwg + nwg2;
  m355_ctx::MsssimSlot* s = nullptr;
  for (auto& x : c->msssim_slot) if (!x.ticket) { s = &x; break; }
  if (!s) return fail(M355_ERR_BUSY, "%s: %d requests outstanding (collect one: m355_frame_msssim_result)", who, M355_MSSSIM_REQUESTS);
  const int slot = (int)(s - c->msssim_slot);
  hipSetDevice(c->device);
  if (need > c->msssim_scratch_cap[slot]) {                                     /* (the slot is idle: nothing in flight uses its scratch) */
    if (c->msssim_scratch[slot]) hipFree(c->msssim_scratch[slot]);
    c->msssim_scratch[slot] = nullptr; c->msssim_scratch_cap[slot] = 0;
    HIPCHK(hipMalloc(&c->msssim_scratch[slot], need));
    c->msssim_scratch_cap[slot] = need;
  }
  for (int p = 0, k = 0; p < 3; p++) {
    if (!a.pl[p].tiles_x) continue;
    uint8_t** const la[MSSSIM_LEVELS - 1] = {&a.pl[p].a1, &a.pl[p].a2, &a.pl[p].a3, &a.pl[p].a4};
    uint8_t** const lb[MSSSIM_LEVELS - 1] = {&a.pl[p].b1, &a.pl[p].b2, &a.pl[p].b3, &a.pl[p].b4};
    for (int j = 1; j < L; j++, k++) {
      lv.lv[k].a = *la[j - 1] = c->msssim_scratch[slot] + off[p][0][j - 1];
      lv.lv[k].b = *lb[j - 1] = c->msssim_scratch[slot] + off[p][1][j - 1];
    }
  }
  MsssimReq q = {};
  q.rec = c->msssim_rec + slot * MSSSIM_REC_WORDS;
  q.res = c->msssim_res + slot * MSSSIM_REC_WORDS;
  q.seq = (uint32_t)(c->msssim_ticket + 1);
  q.res[MSSSIM_REC_WORDS - 2] = MSSSIM_RES_NONE;                                /* (the slot is idle: nothing in flight writes its record) */
  const hipStream_t cs = reader_begin(c, f, RD_MSSSIM, &q.timeout[0], &q.epoch[0]);
  q.timeout[1] = q.timeout[0]; q.epoch[1] = q.epoch[0];
  if (r && r != f) {
    ev_wait(c, cs, r->wr);                                                      /* the reference frame's last writer (nothing to enqueue when that ran on `cs`) */
    ev_wait(c, cs, r->reader[RD_MSSSIM]);                                       /* ... and its earlier MS-SSIM request on another stream: the one mark kept stands for both */
    if (r->wr_stream && r->wr_gate) { q.timeout[1] = r->wr_gate; q.epoch[1] = r->wr_epoch; }
  }
  m355_launch_msssim(a, lv, q, sb, cs);
  if (hipGetLastError() != hipSuccess || reader_end(c, f, RD_MSSSIM, cs) != M355_OK) { msssim_slot_free(c, *s); return fail(M355_ERR_HIP, "%s: launch failed", who); }
  s->mark = f->reader[RD_MSSSIM]; s->frame[0] = h; s->frame[1] = -1;
  if (r && r != f) { r->reader[RD_MSSSIM] = s->mark; s->frame[1] = e->ref_frame; }
  for (int p = 0; p < 3; p++) for (int j = 0; j < M355_MSSSIM_LEVELS; j++) s->n[p][j] = n[p][j];
  s->levels = L;
  s->ticket = ++c->msssim_ticket;
  *ticket = s->ticket;
  return M355_OK;
}

int m355_frame_msssim_result(m355_ctx* c, unsigned long long ticket, int block, m355_msssim* out)
{
  m355_ctx::MsssimSlot* s = c ? msssim_slot_of(c, ticket) : nullptr;
  if (!s) return fail(M355_ERR_INVALID, "m355_frame_msssim_result: ticket %llu is unknown or was collected", ticket);
  if (!out) return fail(M355_ERR_INVALID, "m355_frame_msssim_result: null result");
  hipSetDevice(c->device);
  if (block) HIPCHK(ev_sync(c, s->mark));                                       /* this request's mark only */
  else {
    const hipError_t e = ev_query(c, s->mark);
    if (e == hipErrorNotReady) return M355_ERR_BUSY;
    if (e != hipSuccess) return fail(M355_ERR_HIP, "hipEventQuery failed: %s", hipGetErrorString(e));
  }
  const unsigned long long* res = c->msssim_res + (s - c->msssim_slot) * MSSSIM_REC_WORDS;
  const unsigned long long state = res[MSSSIM_REC_WORDS - 2], seq = res[MSSSIM_REC_WORDS - 1];
  if (state == MSSSIM_RES_GATED && seq == (uint32_t)ticket) {
    msssim_slot_free(c, *s);
    return fail(M355_ERR_INVALID, "MS-SSIM request %llu was queued behind a decode whose lists were rejected: no value", ticket);
  }
  if (state != MSSSIM_RES_VALID || seq != (uint32_t)ticket) {
    msssim_slot_free(c, *s);
    return fail(M355_ERR_HIP, "MS-SSIM request %llu finished without a result (state %llu, sequence %llu)", ticket, state, seq);
  }
  memset(out, 0, sizeof(*out));
  const int L = s->levels;
  for (int p = 0; p < 3; p++) {
    if (!s->n[p][0]) continue;
    double mean[M355_MSSSIM_LEVELS] = {};
    for (int j = 0; j < L; j++) {
      out->sum_q[p][j] = (int64_t)res[MSSSIM_Q + MSSSIM_LEVELS * p + j];
      out->sum_cs[p][j] = (int64_t)res[MSSSIM_CS + MSSSIM_LEVELS * p + j];
      out->n[p][j] = s->n[p][j];
      mean[j] = (double)(j < L - 1 ? out->sum_cs[p][j] : out->sum_q[p][j]) / ((double)out->n[p][j] * 1073741824.0);
    }
    if (L == M355_MSSSIM_LEVELS) m355_msssim_combine(mean, L, nullptr, &out->msssim[p]);
  }
  msssim_slot_free(c, *s);
  return M355_OK;
}

int m355_ssim_window_cs(const uint64_t sums[5], int bit_depth, int32_t* qc)
{
  if (!sums || !qc || bit_depth < 1 || bit_depth > 16) return fail(M355_ERR_INVALID, "m355_ssim_window_cs: null pointer or a bit depth (%d) outside 1..16", bit_depth);
  *qc = m355_ssim_point_cs(sums[0], sums[1], sums[2], sums[3], sums[4], m355_ssim_c1(bit_depth), m355_ssim_c2(bit_depth));
  return M355_OK;
}

int m355_msssim_combine(const double mean[5], int levels, const double* weight, double* out)
{
  static const double wang[M355_MSSSIM_LEVELS] = {0.0448, 0.2856, 0.3001, 0.2363, 0.1333};
  if (!mean || !out) return fail(M355_ERR_INVALID, "m355_msssim_combine: null pointer");
  if (levels < 1 || levels > M355_MSSSIM_LEVELS) return fail(M355_ERR_INVALID, "m355_msssim_combine: levels %d is outside 1..%d", levels, M355_MSSSIM_LEVELS);
  if (!weight && levels != M355_MSSSIM_LEVELS) return fail(M355_ERR_INVALID, "m355_msssim_combine: the built-in weights are those of %d levels, not %d", M355_MSSSIM_LEVELS, levels);
  if (!weight) weight = wang;
  for (int j = 0; j < levels; j++) {
    if (mean[j] != mean[j]) return fail(M355_ERR_INVALID, "m355_msssim_combine: mean[%d] is not a number", j);
    if (!(weight[j] >= 0.0) || weight[j] > 1.79769313486231570815e308) return fail(M355_ERR_INVALID, "m355_msssim_combine: weight[%d] is negative or not finite", j);
  }
  double v = 1.0;
  for (int j = 0; j < levels; j++) v *= pow(mean[j] > 0.0 ? mean[j] : 0.0, weight[j]);
  *out = v;
  return M355_OK;
}
