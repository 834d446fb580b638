/*
 * runtime_maps.hip — host side of the side-map requests (m355_picture_maps_async / _result / _order, include/de265_mi355x.h) and the host-only
 * m355_maps_unit.  A request reads the LISTS of a resident picture, not a frame: it is ordered behind the upload of the lists (Resident::up) and
 * leaves a mark of its own on them (Resident::maps) beside the decodes' Resident::done — whoever overwrites the arenas waits for both.  All requests
 * of a context run in order on one stream of their own (made with the first request: a context that never asks for maps keeps the streams, and the
 * dealing of streams to hardware queues, it had) and share one scratch allocation, grown on demand.
 */
#include "runtime_internal.h"
#include "map_element.h"

extern "C" {
/* the slots: device records (zeroed here, once: every request leaves its record zero), pinned result records */
int maps_requests_create(m355_ctx* c)
{
  hipStream_t st = c->lanes[0].stream;
  HIPCHK(hipMalloc(&c->maps_rec, M355_MAPS_REQUESTS * MAPS_REC_WORDS * sizeof(uint32_t)));
  HIPCHK(hipMemsetAsync(c->maps_rec, 0, M355_MAPS_REQUESTS * MAPS_REC_WORDS * sizeof(uint32_t), st));
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipHostMalloc(&c->maps_res, M355_MAPS_REQUESTS * MAPS_REC_WORDS * sizeof(uint32_t), hipHostMallocDefault));
  memset(c->maps_res, 0, M355_MAPS_REQUESTS * MAPS_REC_WORDS * sizeof(uint32_t));
  /* M355_MAPS_STREAM_EAGER=1 (measurement only): the requests' stream is made HERE, in front of the streams of lanes 1.., which shifts the dealing of
     the lanes' streams to the hardware queues — what making it with the first request avoids (profiles/side_maps_bench.txt has the A/B) */
  if (getenv("M355_MAPS_STREAM_EAGER")) HIPCHK(hipStreamCreateWithFlags(&c->maps_stream, hipStreamNonBlocking));
  return M355_OK;
}
/* (behind sync_all, which waits for the requests' stream too: nothing is in flight; requests nobody collected are dropped) */
void maps_requests_destroy(m355_ctx* c)
{
  for (auto& s : c->maps_slot) s = m355_ctx::MapsSlot();
  if (c->maps_rec) hipFree(c->maps_rec);
  if (c->maps_res) hipHostFree(c->maps_res);
  if (c->maps_scratch) hipFree(c->maps_scratch);
  if (c->maps_stream) hipStreamDestroy(c->maps_stream);
  c->maps_rec = c->maps_res = nullptr; c->maps_scratch = nullptr; c->maps_scratch_cap = 0; c->maps_stream = nullptr;
}
/* the host waits for the requests that read the lists of `r` (in front of whatever overwrites its arenas) */
int maps_lists_idle(m355_ctx* c, Resident& r)
{
  if (!r.maps.ticket) return M355_OK;
  HIPCHK(ev_sync(c, r.maps));
  r.maps = EvRef();
  return M355_OK;
}
}

static m355_ctx::MapsSlot* maps_slot_of(m355_ctx* c, unsigned long long ticket)
{
  if (ticket) for (auto& s : c->maps_slot) if (s.ticket == ticket) return &s;
  return nullptr;
}

/* Enqueue only: the host waits for nothing here (but for the scratch to grow, when a larger picture than any before is mapped). */
int m355_picture_maps_async(m355_ctx* c, int h, const m355_maps_desc* e, unsigned long long* ticket)
{
  const char* who = "m355_picture_maps_async";
  if (!c || !e || !ticket) return fail(M355_ERR_INVALID, "%s: null context / descriptor / ticket", who);
  if (c->shard_n > 0) return fail(M355_ERR_INVALID, "%s: not on a tile-sharded context (its lists hold one rank's tiles)", who);
  Resident* r = nullptr;
  if (h == M355_PICTURE_LAST) {
    if (c->last_transient < 0) return fail(M355_ERR_INVALID, "%s: M355_PICTURE_LAST without a successful m355_submit_picture on this context", who);
    r = &c->transient[c->last_transient];
  } else if (h >= 0 && h < (int)c->resident.size() && c->resident[h].used) r = &c->resident[h];
  if (!r || !r->used) return fail(M355_ERR_INVALID, "%s: bad picture handle %d", who, h);
  if (r->sharded) return fail(M355_ERR_INVALID, "%s: the lists of picture %d were uploaded for tile sharding (they hold one rank's tiles)", who, h);
  if (e->log2_unit < 2 || e->log2_unit > 6) return fail(M355_ERR_INVALID, "%s: log2_unit %d is not 2..6", who, e->log2_unit);
  if (e->reserved) return fail(M355_ERR_INVALID, "%s: reserved is %d, not 0", who, e->reserved);
  const m355_pic_params& pp = r->hdr.pp;
  MapsArgs a;
  memset(&a, 0, sizeof(a));
  a.g = m355_me_grid(pp.width, pp.height, pp.log2_ctb_size, e->log2_unit);
  a.lim = m355_me_limits(pp.width, pp.height, pp.chroma_format_idc, pp.log2_min_cb_size, pp.log2_ctb_size);
  uint32_t want = 0;
  for (int m = 0; m < M355_N_MAPS; m++) {
    if (!e->dst[m]) continue;
    const int es = m355_me_elem_size(m);
    if (e->pitch[m] < (int64_t)a.g.units_w * es) return fail(M355_ERR_INVALID, "%s: pitch %lld of map %d is below its row of %lld bytes", who, (long long)e->pitch[m], m, (long long)a.g.units_w * es);
    if (((uintptr_t)e->dst[m] | (uintptr_t)e->pitch[m]) & (uintptr_t)(es - 1)) return fail(M355_ERR_INVALID, "%s: pointer / pitch of map %d is no multiple of the %d-byte element", who, m, es);
    a.dst[m] = (uint8_t*)e->dst[m]; a.pitch[m] = e->pitch[m];
    want |= 1u << m;
  }
  if (!want) return fail(M355_ERR_INVALID, "%s: no map wanted (every dst is null)", who);
  m355_ctx::MapsSlot* s = nullptr;
  for (auto& x : c->maps_slot) if (!x.ticket) { s = &x; break; }
  if (!s) return fail(M355_ERR_BUSY, "%s: %d requests outstanding (collect one: m355_picture_maps_result)", who, M355_MAPS_REQUESTS);
  const int slot = (int)(s - c->maps_slot);
  hipSetDevice(c->device);
  if (!c->maps_stream) HIPCHK(hipStreamCreateWithFlags(&c->maps_stream, hipStreamNonBlocking));
  const hipStream_t st = c->maps_stream;
  /* the lists read, the planes they are painted on: the 32-bit planes first, every plane a whole number of 16-byte groups of cells */
  const bool rd_cu = want & (1u << M355_MAP_CU | 1u << M355_MAP_QP), rd_pb = want & (1u << M355_MAP_MV | 1u << M355_MAP_REF);
  const bool rd_tu = want & (1u << M355_MAP_TU), rd_ib = want & (1u << M355_MAP_INTRA);
  a.sp = (a.g.w4 + 3) & ~3;
  const size_t cells = (size_t)a.sp * a.g.h4;
  const size_t bytes = (((rd_cu ? 4 : 0) + (rd_pb ? 4 : 0) + (rd_tu ? 1 : 0) + (rd_ib ? 1 : 0)) * cells + 15) & ~(size_t)15;
  a.quads = (uint32_t)((a.g.units_w + 3) / 4);
  a.n_wg = (uint32_t)(((size_t)a.quads * a.g.units_h + MAPS_BLOCK - 1) / MAPS_BLOCK);
  {
    /* behind the planes (which alone are zero-filled): the gather pass's table of one summary record per workgroup */
    const int rc = grow(&c->maps_scratch, &c->maps_scratch_cap, bytes + (size_t)a.n_wg * MAPS_PART_WORDS * sizeof(uint32_t), st, false);
    if (rc) return rc;
    a.part = (uint32_t*)(c->maps_scratch + bytes);
    uint8_t* p = c->maps_scratch;
    if (rd_cu) { a.s_cu = (uint32_t*)p; p += 4 * cells; }
    if (rd_pb) { a.s_pb = (uint32_t*)p; p += 4 * cells; }
    if (rd_tu) { a.s_tu = p; p += cells; }
    if (rd_ib) { a.s_ib = p; p += cells; }
  }
  const DevPic& d = r->dp;
  a.cus = d.cus; a.tus = d.tus; a.pbs = d.pbs; a.ibs = d.ibs; a.ctbs = d.ctbs;
  a.n_cus = rd_cu ? r->hdr.n_cus : 0; a.n_tus = rd_tu ? r->hdr.n_tus : 0; a.n_pbs = rd_pb ? r->hdr.n_pbs : 0; a.n_ibs = rd_ib ? r->hdr.n_ibs : 0;
  const int n[4] = {a.n_cus, a.n_tus, a.n_pbs, a.n_ibs};
  uint32_t end = 0;
  for (int l = 0; l < 4; l++) { end += (uint32_t)((n[l] + MAPS_RASTER_BLOCK - 1) / MAPS_RASTER_BLOCK); a.wg_end[l] = end; }
  a.rec = c->maps_rec + slot * MAPS_REC_WORDS;
  a.res = c->maps_res + slot * MAPS_REC_WORDS;
  a.seq = (uint32_t)(c->maps_ticket + 1);
  a.res[MAPS_ARRIVED] = 0u;                                                     /* (the slot is idle: nothing in flight writes its record) */
  ev_wait(c, st, r->up);                                                        /* behind the copy of the lists */
  if (bytes) HIPCHK(hipMemsetAsync(c->maps_scratch, 0, bytes, st));
  m355_launch_maps(a, st);
  EvRef mark;
  if (hipGetLastError() != hipSuccess || ev_mark(c, st, &mark) != M355_OK) return fail(M355_ERR_HIP, "%s: launch failed", who);
  r->maps = mark;                                                               /* (requests run in order: the last one's mark stands for all) */
  s->mark = mark; s->units_w = a.g.units_w; s->units_h = a.g.units_h; s->want = want;
  s->ticket = ++c->maps_ticket;
  *ticket = s->ticket;
  return M355_OK;
}

int m355_picture_maps_result(m355_ctx* c, unsigned long long ticket, int block, m355_maps_info* out)
{
  m355_ctx::MapsSlot* s = c ? maps_slot_of(c, ticket) : nullptr;
  if (!s) return fail(M355_ERR_INVALID, "m355_picture_maps_result: ticket %llu is unknown or was collected", ticket);
  if (!out) return fail(M355_ERR_INVALID, "m355_picture_maps_result: null result");
  hipSetDevice(c->device);
  if (block) HIPCHK(ev_sync(c, s->mark));                                       /* this request's mark only */
  else {
    const hipError_t e = ev_query(c, s->mark);
    if (e == hipErrorNotReady) return M355_ERR_BUSY;
    if (e != hipSuccess) return fail(M355_ERR_HIP, "hipEventQuery failed: %s", hipGetErrorString(e));
  }
  const uint32_t* res = c->maps_res + (s - c->maps_slot) * MAPS_REC_WORDS;
  const uint32_t state = res[MAPS_ARRIVED], seq = res[MAPS_ARRIVED + 1], want = s->want;
  memset(out, 0, sizeof(*out));
  out->units_w = s->units_w; out->units_h = s->units_h;
  *s = m355_ctx::MapsSlot();
  if (state != 1u || seq != (uint32_t)ticket) return fail(M355_ERR_HIP, "maps request %llu finished without a result (state %u, sequence %u)", ticket, state, seq);
  out->qp_min = 127; out->qp_max = -128;
  if (want & (1u << M355_MAP_CU)) { out->covered = res[MAPS_COVERED]; out->n_intra = res[MAPS_INTRA]; out->n_inter = res[MAPS_INTER]; out->n_skip = res[MAPS_SKIP]; }
  if (want & (1u << M355_MAP_QP)) {
    out->qp_sum = (int64_t)((uint64_t)res[MAPS_QP_SUM] | (uint64_t)res[MAPS_QP_SUM + 1] << 32);
    if (res[MAPS_QP_MIN]) out->qp_min = 128 - (int32_t)res[MAPS_QP_MIN];
    if (res[MAPS_QP_MAX]) out->qp_max = (int32_t)res[MAPS_QP_MAX] - 129;
  }
  if (want & (1u << M355_MAP_REF)) out->n_bipred = res[MAPS_BIPRED];
  for (int l = 0; l < 4; l++) out->skipped[l] = res[MAPS_SKIPPED + l];
  return M355_OK;
}

/* the consumer's stream continues behind the request (nothing to enqueue when it has long passed: its mark has left the ring) */
int m355_picture_maps_order(m355_ctx* c, unsigned long long ticket, void* consumer)
{
  m355_ctx::MapsSlot* s = c ? maps_slot_of(c, ticket) : nullptr;
  if (!s) return fail(M355_ERR_INVALID, "m355_picture_maps_order: ticket %llu is unknown or was collected", ticket);
  hipSetDevice(c->device);
  ev_wait(c, (hipStream_t)consumer, s->mark);
  return M355_OK;
}

/* host only: the definition of map_element.h by a linear search over host lists (the first record that counts and covers the position) */
int m355_maps_unit(const m355_picture* pic, int map, int log2_unit, int ux, int uy, void* element)
{
  if (!pic || !element || map < 0 || map >= M355_N_MAPS || log2_unit < 2 || log2_unit > 6) return fail(M355_ERR_INVALID, "m355_maps_unit: null pointer, map %d not 0..%d or log2_unit %d not 2..6", map, M355_N_MAPS - 1, log2_unit);
  const m355_pic_params& pp = pic->pp;
  if (pp.width <= 0 || pp.height <= 0 || pp.log2_ctb_size < 3 || pp.log2_ctb_size > 6) return fail(M355_ERR_INVALID, "m355_maps_unit: bad picture parameters");
  const M355MapGrid g = m355_me_grid(pp.width, pp.height, pp.log2_ctb_size, log2_unit);
  const M355RecLimits L = m355_me_limits(pp.width, pp.height, pp.chroma_format_idc, pp.log2_min_cb_size, pp.log2_ctb_size);
  if (ux < 0 || uy < 0 || ux >= g.units_w || uy >= g.units_h) return fail(M355_ERR_INVALID, "m355_maps_unit: unit %d,%d outside the %dx%d grid", ux, uy, g.units_w, g.units_h);
  const int px = ux << log2_unit, py = uy << log2_unit;
  if (map == M355_MAP_CU || map == M355_MAP_QP) {
    uint32_t v = M355_ME_NONE_CU; int8_t qp = M355_ME_NONE_QP;
    for (int i = 0; i < pic->n_cus; i++) {
      const m355_cu& cu = pic->cus[i];
      if (!m355_me_cu_ok(cu, L) || !m355_me_covers(cu.x, 1 << cu.log2_size, px) || !m355_me_covers(cu.y, 1 << cu.log2_size, py)) continue;
      v = m355_me_cu(cu); qp = cu.qp_y;
      break;
    }
    if (map == M355_MAP_CU) memcpy(element, &v, 4); else memcpy(element, &qp, 1);
  } else if (map == M355_MAP_TU) {
    uint8_t v = (uint8_t)M355_ME_NONE_TU;
    for (int i = 0; i < pic->n_tus; i++) {
      const m355_tu& tu = pic->tus[i];
      if (!m355_me_tu_ok(tu, L) || !m355_me_covers(tu.x, 1 << tu.log2_size, px) || !m355_me_covers(tu.y, 1 << tu.log2_size, py)) continue;
      v = (uint8_t)m355_me_tu(tu);
      break;
    }
    memcpy(element, &v, 1);
  } else if (map == M355_MAP_INTRA) {
    uint8_t v = (uint8_t)M355_ME_NONE_INTRA;
    for (int i = 0; i < pic->n_ibs; i++) {
      const m355_ib& ib = pic->ibs[i];
      if (!m355_me_ib_ok(ib, L) || !m355_me_ib_shown(ib) || !m355_me_covers(ib.x, 1 << ib.log2_size, px) || !m355_me_covers(ib.y, 1 << ib.log2_size, py)) continue;
      v = ib.mode;
      break;
    }
    memcpy(element, &v, 1);
  } else if (map == M355_MAP_MV || map == M355_MAP_REF) {
    uint32_t mv[2] = {0u, 0u}, ref = M355_ME_NONE_REF;
    for (int i = 0; i < pic->n_pbs; i++) {
      const m355_pb& pb = pic->pbs[i];
      if (!m355_me_pb_ok(pb, L) || !m355_me_covers(pb.x, pb.w, px) || !m355_me_covers(pb.y, pb.h, py)) continue;
      m355_me_mv(pb, mv); ref = m355_me_ref(pb);
      break;
    }
    if (map == M355_MAP_MV) memcpy(element, mv, 8); else memcpy(element, &ref, 4);
  } else {
    const int ctb = (py >> g.log2_ctb) * g.ctbW + (px >> g.log2_ctb);
    if (!pic->ctbs || ctb >= pic->n_ctbs) return fail(M355_ERR_INVALID, "m355_maps_unit: the CTB table has %d entries, the position lies in CTB %d", pic->n_ctbs, ctb);
    const uint16_t v = pic->ctbs[ctb].slice_idx;
    memcpy(element, &v, 2);
  }
  return M355_OK;
}
