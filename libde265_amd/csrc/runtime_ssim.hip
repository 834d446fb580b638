/*
 * runtime_ssim.hip — host side of the SSIM requests (m355_frame_ssim_async / m355_frame_ssim_result, include/de265_mi355x.h): the comparison requests'
 * machinery (runtime.hip) with another kernel (k_ssim.hip), the frame, rectangle and reference checked by the same code (pair_geometry,
 * runtime_internal.h), and slots, tickets and a reader kind (RD_SSIM) of their own — and the two host-only helpers that state the definition,
 * m355_ssim_window and m355_ssim_weights (ssim_window.h).
 */
#include "runtime_internal.h"
#include "ssim_window.h"

/* the slots: device records (zeroed here, once: every request leaves its record zero), pinned result records */
int ssim_requests_create(m355_ctx* c)
{
  hipStream_t st = c->lanes[0].stream;
  HIPCHK(hipMalloc(&c->ssim_rec, M355_SSIM_REQUESTS * SSIM_REC_WORDS * sizeof(unsigned long long)));
  HIPCHK(hipMemsetAsync(c->ssim_rec, 0, M355_SSIM_REQUESTS * SSIM_REC_WORDS * sizeof(unsigned long long), st));
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipHostMalloc(&c->ssim_res, M355_SSIM_REQUESTS * SSIM_REC_WORDS * sizeof(unsigned long long), hipHostMallocDefault));
  memset(c->ssim_res, 0, M355_SSIM_REQUESTS * SSIM_REC_WORDS * sizeof(unsigned long long));
  return M355_OK;
}
/* (behind sync_all: nothing is in flight; requests nobody collected are dropped) */
void ssim_requests_destroy(m355_ctx* c)
{
  for (auto& s : c->ssim_slot) s = m355_ctx::SsimSlot();
  if (c->ssim_rec) hipFree(c->ssim_rec);
  if (c->ssim_res) hipHostFree(c->ssim_res);
  c->ssim_rec = c->ssim_res = nullptr;
}

static m355_ctx::SsimSlot* ssim_slot_of(m355_ctx* c, unsigned long long ticket)
{
  if (ticket) for (auto& s : c->ssim_slot) if (s.ticket == ticket) return &s;
  return nullptr;
}
/* collected behind its mark: the next decode into either frame has nothing to wait for, if the frame's mark is still this request's (meas_slot_free) */
static void ssim_slot_free(m355_ctx* c, m355_ctx::SsimSlot& s)
{
  for (int k = 0; k < 2; k++) {
    Frame* f = get_frame(c, s.frame[k]);
    if (f && s.mark.ticket && f->reader[RD_SSIM].ticket == s.mark.ticket) f->reader[RD_SSIM] = EvRef();
  }
  s = m355_ctx::SsimSlot();
}

/* Enqueue only: the host waits for nothing here.  A READER of the frame and of the reference frame, ordered as m355_frame_measure_async orders its
   request: on the stream of the frame's last writer, behind the reference frame's last writer and that frame's earlier SSIM mark; ONE mark behind the
   launch is kept by both frames and by the slot. */
int m355_frame_ssim_async(m355_ctx* c, int h, const m355_ssim_desc* e, unsigned long long* ticket)
{
  const char* who = "m355_frame_ssim_async";
  PairGeom g = {};
  const int grc = pair_geometry(c, who, h, e && ticket, e ? e->ref_frame : -1, e ? e->x0 : 0, e ? e->y0 : 0, e ? e->width : 0, e ? e->height : 0,
                                e ? e->ref : nullptr, e ? e->pitch : nullptr, &g);
  if (grc) return grc;
  Frame *f = g.f, *r = g.r;
  for (int i = 0; i < 7; i++) if (e->reserved[i]) return fail(M355_ERR_INVALID, "%s: reserved[%d] is %d, not 0", who, i, e->reserved[i]);
  if (e->planes < 0 || e->planes > 7) return fail(M355_ERR_INVALID, "%s: planes %d has bits above plane 2", who, e->planes);
  if (e->planes >> g.np) return fail(M355_ERR_INVALID, "%s: planes %d selects a plane the frame does not have", who, e->planes);
  const int sel = e->planes ? e->planes : (1 << g.np) - 1;
  SsimArgs a = {};
  uint64_t n[3] = {0, 0, 0};
  int nwg = 0;
  for (int p = 0; p < 3; p++) {
    a.first[p] = nwg;
    const bool on = p < g.np && ((sel >> p) & 1);
    if (!on) {
      if (e->map[p]) return fail(M355_ERR_INVALID, "%s: a map for plane %d, which is not measured", who, p);
      continue;
    }
    const PairPlane& gp = g.pl[p];
    if (gp.pw < M355_SSIM_TAPS || gp.ph < M355_SSIM_TAPS) return fail(M355_ERR_INVALID, "%s: plane %d of the rectangle has %dx%d samples, below one 11x11 window", who, p, gp.pw, gp.ph);
    const int nwx = gp.pw - 10, nwy = gp.ph - 10;
    if (e->map[p]) {
      if (((uintptr_t)e->map[p] | (uintptr_t)e->map_pitch[p]) & 3u) return fail(M355_ERR_INVALID, "%s: map pointer / pitch of plane %d is no multiple of 4", who, p);
      if (e->map_pitch[p] < (int64_t)4 * nwx) return fail(M355_ERR_INVALID, "%s: map pitch %lld of plane %d is below its row of %lld bytes", who, (long long)e->map_pitch[p], p, (long long)4 * nwx);
    }
    SsimPlane& m = a.pl[p];
    m.a = gp.a; m.b = gp.b; m.pitch_a = gp.pitch_a; m.pitch_b = gp.pitch_b;
    m.pw = gp.pw; m.ph = gp.ph;
    m.tiles_x = (nwx + SSIM_TILE_W - 1) / SSIM_TILE_W;
    m.c1 = m355_ssim_c1(p ? f->bdc : f->bdl); m.c2 = m355_ssim_c2(p ? f->bdc : f->bdl);
    m.map = (uint8_t*)e->map[p]; m.map_pitch = e->map_pitch[p];
    n[p] = (uint64_t)nwx * nwy;
    nwg += m.tiles_x * ((nwy + SSIM_TILE_H - 1) / SSIM_TILE_H);
  }
  a.first[3] = nwg;
  m355_ctx::SsimSlot* s = nullptr;
  for (auto& x : c->ssim_slot) if (!x.ticket) { s = &x; break; }
  if (!s) return fail(M355_ERR_BUSY, "%s: %d requests outstanding (collect one: m355_frame_ssim_result)", who, M355_SSIM_REQUESTS);
  const int slot = (int)(s - c->ssim_slot);
  hipSetDevice(c->device);
  SsimReq q = {};
  q.rec = c->ssim_rec + slot * SSIM_REC_WORDS;
  q.res = c->ssim_res + slot * SSIM_REC_WORDS;
  q.seq = (uint32_t)(c->ssim_ticket + 1);
  q.res[6] = SSIM_RES_NONE;                                                     /* (the slot is idle: nothing in flight writes its record) */
  const hipStream_t cs = reader_begin(c, f, RD_SSIM, &q.timeout[0], &q.epoch[0]);
  q.timeout[1] = q.timeout[0]; q.epoch[1] = q.epoch[0];
  if (r && r != f) {
    ev_wait(c, cs, r->wr);                                                      /* the reference frame's last writer (nothing to enqueue when that ran on `cs`) */
    ev_wait(c, cs, r->reader[RD_SSIM]);                                         /* ... and its earlier SSIM request on another stream: the one mark kept stands for both */
    if (r->wr_stream && r->wr_gate) { q.timeout[1] = r->wr_gate; q.epoch[1] = r->wr_epoch; }
  }
  m355_launch_ssim(a, q, f->bpp[0], cs);
  if (hipGetLastError() != hipSuccess || reader_end(c, f, RD_SSIM, cs) != M355_OK) { ssim_slot_free(c, *s); return fail(M355_ERR_HIP, "%s: launch failed", who); }
  s->mark = f->reader[RD_SSIM]; s->frame[0] = h; s->frame[1] = -1;
  if (r && r != f) { r->reader[RD_SSIM] = s->mark; s->frame[1] = e->ref_frame; }
  for (int p = 0; p < 3; p++) s->n[p] = n[p];
  s->ticket = ++c->ssim_ticket;
  *ticket = s->ticket;
  return M355_OK;
}

int m355_frame_ssim_result(m355_ctx* c, unsigned long long ticket, int block, m355_ssim* out)
{
  m355_ctx::SsimSlot* s = c ? ssim_slot_of(c, ticket) : nullptr;
  if (!s) return fail(M355_ERR_INVALID, "m355_frame_ssim_result: ticket %llu is unknown or was collected", ticket);
  if (!out) return fail(M355_ERR_INVALID, "m355_frame_ssim_result: null result");
  hipSetDevice(c->device);
  if (block) HIPCHK(ev_sync(c, s->mark));                                       /* this request's mark only */
  else {
    const hipError_t e = ev_query(c, s->mark);
    if (e == hipErrorNotReady) return M355_ERR_BUSY;
    if (e != hipSuccess) return fail(M355_ERR_HIP, "hipEventQuery failed: %s", hipGetErrorString(e));
  }
  const unsigned long long* res = c->ssim_res + (s - c->ssim_slot) * SSIM_REC_WORDS;
  const unsigned long long state = res[6], seq = res[7];
  if (state == SSIM_RES_GATED && seq == (uint32_t)ticket) {
    ssim_slot_free(c, *s);
    return fail(M355_ERR_INVALID, "SSIM request %llu was queued behind a decode whose lists were rejected: no value", ticket);
  }
  if (state != SSIM_RES_VALID || seq != (uint32_t)ticket) {
    ssim_slot_free(c, *s);
    return fail(M355_ERR_HIP, "SSIM request %llu finished without a result (state %llu, sequence %llu)", ticket, state, seq);
  }
  memset(out, 0, sizeof(*out));
  for (int p = 0; p < 3; p++) {
    if (!s->n[p]) continue;
    out->sum_q[p] = (int64_t)res[SSIM_SUM + p];
    out->n[p] = s->n[p];
    out->min_q[p] = (int32_t)((int64_t)M355_SSIM_ONE - (int64_t)res[SSIM_WORST + p]);
    out->ssim[p] = (double)out->sum_q[p] / ((double)out->n[p] * 1073741824.0);
  }
  ssim_slot_free(c, *s);
  return M355_OK;
}

int m355_ssim_window(const uint64_t sums[5], int bit_depth, int32_t* q)
{
  if (!sums || !q || bit_depth < 1 || bit_depth > 16) return fail(M355_ERR_INVALID, "m355_ssim_window: null pointer or a bit depth (%d) outside 1..16", bit_depth);
  *q = m355_ssim_point(sums[0], sums[1], sums[2], sums[3], sums[4], m355_ssim_c1(bit_depth), m355_ssim_c2(bit_depth));
  return M355_OK;
}

int m355_ssim_weights(int32_t w[M355_SSIM_TAPS])
{
  if (!w) return fail(M355_ERR_INVALID, "m355_ssim_weights: null pointer");
  const int32_t t[M355_SSIM_TAPS] = M355_SSIM_WEIGHTS;
  for (int i = 0; i < M355_SSIM_TAPS; i++) w[i] = t[i];
  return M355_OK;
}
