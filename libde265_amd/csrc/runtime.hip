/*
 * runtime.hip — host side of the picture layer, part 1 of 4 (runtime_internal.h lists the parts): context, lanes, events,
 * device-resident frames (the DPB lives in HBM), arenas, submit / wait, timing.
 *
 * Per picture the executor enqueues, on the context's own HIP stream:
 *   H2D (one pinned arena copy)  ->  k_meta_*  ->  k_inter  ->  k_residual<2..5>  ->  k_intra
 *   ->  k_deblock<V>  ->  k_deblock<H>  ->  k_sao
 * which is the deferred form of decode_TU / decode_prediction_unit / run_postprocessing_filters_*
 * (slice.cc:3460, motion.cc:2190, decctx.cc:1783-1833).  Nothing here falls back to the CPU: if HIP
 * is unavailable every entry point fails with M355_ERR_NO_DEVICE.
 */
#include "runtime_internal.h"
#include "resize_taps.h"
#include "tensor_element.h"
#include "colour_transform.h"
#include "colour_preset.h"

thread_local std::string g_err;
int fail(int code, const char* fmt, ...)
{
  char buf[512];
  va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof(buf), fmt, ap); va_end(ap);
  g_err = buf;
  return code;
}

extern "C" {
/* mark the point the stream has reached (one event packet); -> *out */
int ev_mark(m355_ctx* c, hipStream_t st, EvRef* out) {
  const unsigned long long t = ++c->ev_ticket;
  m355_ctx::EvSlot& e = c->evring[t % M355_EV_RING];
  if (!e.ev) { if (hipEventCreateWithFlags(&e.ev, hipEventDisableTiming) != hipSuccess) return fail(M355_ERR_HIP, "hipEventCreate failed"); }
  else if (e.ticket) hipEventSynchronize(e.ev);            /* the slot's old mark, M355_EV_RING marks ago (passed long since: this is the ring's invariant, not a wait) */
  if (hipEventRecord(e.ev, st) != hipSuccess) return fail(M355_ERR_HIP, "hipEventRecord failed");
  e.ticket = t;
  out->ticket = t; out->stream = st;
  return M355_OK;
}
/* `st` continues behind the mark: nothing to enqueue when the mark has passed or lies on `st` itself (stream order) */
void ev_wait(m355_ctx* c, hipStream_t st, const EvRef& r) {
  if (!r.ticket || r.stream == st) return;
  const m355_ctx::EvSlot& e = c->evring[r.ticket % M355_EV_RING];
  if (e.ticket == r.ticket) hipStreamWaitEvent(st, e.ev, 0);
}
/* the host waits for the mark / asks whether it has passed */
hipError_t ev_sync(m355_ctx* c, const EvRef& r) {
  if (!r.ticket) return hipSuccess;
  const m355_ctx::EvSlot& e = c->evring[r.ticket % M355_EV_RING];
  return e.ticket == r.ticket ? hipEventSynchronize(e.ev) : hipSuccess;
}
hipError_t ev_query(m355_ctx* c, const EvRef& r) {
  if (!r.ticket) return hipSuccess;
  const m355_ctx::EvSlot& e = c->evring[r.ticket % M355_EV_RING];
  return e.ticket == r.ticket ? hipEventQuery(e.ev) : hipSuccess;
}

/* A READER of frame `f` (Frame::reader) is queued on the stream this returns: the stream of the decode that wrote the frame, right behind it — measured
 * (tests/test_gpu_pipeline.py, profiles/r03_y_*) a copy on a stream of its own, ordered behind the writer by an event (even with the host waiting for that event
 * first), now and then read a half-written picture: the writer's last stores were not yet visible to the copy engine; queued on the writer's own stream it never
 * did.  It still runs beside the host and beside the other lanes' decodes.  gate / epoch: what a gated kernel of the reader is launched with. */
hipStream_t reader_begin(m355_ctx* c, Frame* f, int kind, const uint32_t** gate, uint32_t* epoch) {
  const hipStream_t st = f->wr_stream ? f->wr_stream : lane(c).stream;
  if (!f->wr_stream) ev_wait(c, st, f->wr);                 /* no decode of this context wrote it (uploads and fills are synchronous): its zero fill at creation */
  ev_wait(c, st, f->reader[kind]);                          /* (an earlier reader of the kind on another stream: the one mark kept stands for both) */
  if (!gate) return st;
  if (f->wr_stream && f->wr_gate) { *gate = f->wr_gate; *epoch = f->wr_epoch; }
  else {                                                    /* no decode to be gated by: an epoch of its own, which no gate word holds */
    *gate = lane(c).timeout; *epoch = ++c->epoch;
    if (*epoch == 0) *epoch = ++c->epoch;
  }
  return st;
}
/* the mark behind the reader: what the next decode into the frame and the host's wait for this kind of reader go by */
int reader_end(m355_ctx* c, Frame* f, int kind, hipStream_t st) { return ev_mark(c, st, &f->reader[kind]); }
/* `st` (the next decode into the frame) continues behind the frame's readers */
void readers_wait(m355_ctx* c, hipStream_t st, const Frame* f) {
  for (const EvRef& m : f->reader) ev_wait(c, st, m);
}

/* The HIP runtime multiplexes its streams onto a few hardware queues PER STREAM PRIORITY (GPU_MAX_HW_QUEUES, default 4), and
 * kernels of different streams that share a hardware queue mostly run one after the other.  Three lanes (six streams) do well on
 * the default priority's queues.  Every further group of three lanes belongs to the next priority class, whose streams have
 * hardware queues of their own — used by INTRA PICTURES only (they keep to one stream, launch_prediction, and their k_intra is
 * what gains from more pictures in flight: 1080p, nine lanes 0.84 -> 0.334 ms per picture, profiles/r03_v_*, r03_x_c2_in_flight):
 * such a picture runs on its lane's stream_hi.  Inter pictures stay on the default-priority streams: every queue beyond the first
 * few slows their short kernels down (8K at depth 4: 0.436 -> 0.466 ms with all streams in classes).
 * M355_LANE_PRIORITIES=0: no classes at all; =1: ALL streams of lanes 3.. in their class (the measurement above). */
int lane_class_priority(int index) {
  static int lo = 0, hi = 0, probed = 0;
  if (!probed) { probed = 1; if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess) lo = hi = 0; }   /* (least, greatest) */
  const int cls = (index / 3) % 3;
  return cls == 0 ? 0 : (cls == 1 ? hi : lo);
}
int lane_priorities_mode() { return 2; }              /* 0 off, 1 every stream, 2 intra pictures only (what the measurements of round 3 left: profiles/r03_v_*) */
static int lane_priority(int index) { return lane_priorities_mode() == 1 ? lane_class_priority(index) : 0; }
/* (the ORDER in which the streams are created is load-bearing: the runtime deals its streams round its four hardware queues in creation order, kernels of streams
   that share a queue run one after the other, and which lanes share decides how three pictures' stages interleave — main, side, main, side, main, side (lanes 0 and 2 on
   one pair of queues, lane 1 on the other) is the second best of the 187 ways of dealing six streams to four queues, 1 % behind the best and up to 37 % ahead of the
   others at C5: tools/qmap_search.py, profiles/r06_v49_lane_stream_queue_mapping.txt) */
static int lane_create(m355_ctx* c, Lane& l, int index)
{
  HIPCHK(hipStreamCreateWithPriority(&l.stream, hipStreamNonBlocking, lane_priority(index)));
  HIPCHK(hipStreamCreateWithPriority(&l.stream2, hipStreamNonBlocking, lane_priority(index)));
  HIPCHK(hipEventCreateWithFlags(&l.ev_fork, hipEventDisableTiming));
  HIPCHK(hipEventCreateWithFlags(&l.ev_fork2, hipEventDisableTiming));
  HIPCHK(hipEventCreateWithFlags(&l.ev_join, hipEventDisableTiming));
  HIPCHK(hipMalloc(&l.ticket, 64));
  HIPCHK(hipMalloc(&l.timeout, 128));
  HIPCHK(hipMemsetAsync(l.ticket, 0, 64, l.stream));
  HIPCHK(hipMemsetAsync(l.timeout, 0, 128, l.stream));
  HIPCHK(hipMemsetAsync(l.timeout + 2, 0xFF, 8, l.stream));     /* rejected record of the latest rejected decode: none */
  HIPCHK(hipStreamSynchronize(l.stream));
  return M355_OK;
}
static void lane_destroy(Lane& l)
{
  if (l.stream) hipStreamSynchronize(l.stream);
  if (l.stream2) hipStreamSynchronize(l.stream2);
  if (l.work.used) frame_free(l.work);
  void* bufs[] = {l.pb_of, l.edge, l.ticket, l.timeout, l.edge_tu, l.cuf, l.resbuf, l.jobs, l.sao_nb, l.iplan, l.job_base};
  for (void* b : bufs) if (b) hipFree(b);
  if (l.ev_fork) hipEventDestroy(l.ev_fork);
  if (l.ev_fork2) hipEventDestroy(l.ev_fork2);
  if (l.ev_join) hipEventDestroy(l.ev_join);
  if (l.stream_hi) { hipStreamSynchronize(l.stream_hi); hipStreamDestroy(l.stream_hi); }
  if (l.stream2) hipStreamDestroy(l.stream2);
  if (l.stream) hipStreamDestroy(l.stream);
  l = Lane();
}
/* all work of the context, on every lane */
hipError_t sync_all(m355_ctx* c) {
  hipError_t e = hipSuccess;
  auto sync = [&](hipStream_t s) { if (s) { hipError_t e2 = hipStreamSynchronize(s); if (e == hipSuccess) e = e2; } };
  for (const Lane& l : c->lanes) { sync(l.stream); sync(l.stream_hi); }
  for (hipStream_t bs : c->batch_stream) sync(bs);
  return e;
}


static std::vector<TileRect> rank_tiles(const m355_pic_params& pp, int rank, int nranks)
{
  std::vector<TileRect> v;
  const int cs = 1 << pp.log2_ctb_size, n_tiles = pp.num_tile_cols * pp.num_tile_rows;
  for (int ty = 0, t = 0; ty < pp.num_tile_rows; ty++)
    for (int tx = 0; tx < pp.num_tile_cols; tx++, t++) {
      if (m355_shard_owner_of_tile(t, n_tiles, nranks) != rank) continue;
      TileRect r = {pp.col_bd[tx] * cs, pp.row_bd[ty] * cs, pp.col_bd[tx + 1] * cs, pp.row_bd[ty + 1] * cs};
      if (r.x1 > pp.width) r.x1 = pp.width;
      if (r.y1 > pp.height) r.y1 = pp.height;
      v.push_back(r);
    }
  return v;
}
static size_t tiles_bytes(const m355_pic_params& pp, const std::vector<TileRect>& v)
{
  const int cf = pp.chroma_format_idc;
  const int sw = (cf == 1 || cf == 2) ? 2 : 1, sh = cf == 1 ? 2 : 1;
  const size_t bl = pp.bit_depth_luma <= 8 ? 1 : 2, bc = pp.bit_depth_chroma <= 8 ? 1 : 2;
  size_t n = 0;
  for (const TileRect& r : v) {
    n += (size_t)(r.x1 - r.x0) * (r.y1 - r.y0) * bl;
    if (cf) n += 2 * (size_t)((r.x1 - r.x0) / sw) * ((r.y1 - r.y0) / sh) * bc;
  }
  return (n + 255) & ~(size_t)255;
}
size_t slot_bytes(const m355_pic_params& pp, int nranks) {
  size_t m = 0;
  for (int k = 0; k < nranks; k++) { const size_t b = tiles_bytes(pp, rank_tiles(pp, k, nranks)); if (b > m) m = b; }
  return m;
}
/* copy the tiles of ranks [k0, k1) except `skip` between the frame planes and their slots of the all-gather buffer (to_slot) or
   back: all rectangles in as few launches as the argument block allows */
int copy_tiles(m355_ctx* c, const m355_pic_params& pp, Frame* f, int k0, int k1, int skip, int nranks, char* xbuf, size_t slot, bool to_slot) {
  const int cf = pp.chroma_format_idc;
  const int sw = (cf == 1 || cf == 2) ? 2 : 1, sh = cf == 1 ? 2 : 1;
  TileCopyArgs a;
  for (int cc = 0; cc < 3; cc++) { a.plane[cc] = (char*)f->plane[cc]; a.pitch[cc] = (size_t)f->stride[cc] * f->bpp[cc]; }
  int n = 0;
  for (int k = k0; k < k1; k++) {
    if (k == skip) continue;
    size_t o = slot * (size_t)k;
    for (const TileRect& r : rank_tiles(pp, k, nranks))
      for (int cc = 0; cc < 3; cc++) {
        if (cc && !cf) continue;
        const int x = cc ? r.x0 / sw : r.x0, y = cc ? r.y0 / sh : r.y0;
        const int w = cc ? (r.x1 - r.x0) / sw : r.x1 - r.x0, h = cc ? (r.y1 - r.y0) / sh : r.y1 - r.y0;
        const size_t bpp = f->bpp[cc], wb = (size_t)w * bpp;
        if (w > 0 && h > 0) {
          if ((wb | (x * bpp)) & 3) return fail(M355_ERR_INVALID, "tile rectangle is not a whole number of 32-bit words");
          TileCopyRect& t = a.r[n++];
          t.plane = (uint32_t)cc; t.xb = (uint32_t)(x * bpp); t.y = (uint32_t)y; t.wb = (uint32_t)wb; t.h = (uint32_t)h; t.pad = 0; t.ofs = o;
          if (n == M355_TILE_COPY_RECTS) { m355_launch_tiles_copy(a, n, xbuf, to_slot, lane(c).stream); n = 0; }
        }
        o += wb * h;
      }
  }
  m355_launch_tiles_copy(a, n, xbuf, to_slot, lane(c).stream);
  return M355_OK;
}



const char* m355_last_error(void) { return g_err.c_str(); }
const char* m355_version(void) { return "libde265_mi355x 0.1 (gfx950)"; }
int m355_device_count(void)
{
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

/* the slots of m355_frame_hash_async: device records (zeroed here, once: every request leaves its record zero), pinned result records */
static int hash_requests_create(m355_ctx* c)
{
  hipStream_t st = c->lanes[0].stream;
  HIPCHK(hipMalloc(&c->hash_rec, M355_HASH_REQUESTS * HASH_REC_WORDS * sizeof(uint32_t)));
  HIPCHK(hipMemsetAsync(c->hash_rec, 0, M355_HASH_REQUESTS * HASH_REC_WORDS * sizeof(uint32_t), st));
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipHostMalloc(&c->hash_res, M355_HASH_REQUESTS * HASH_RES_WORDS * sizeof(uint32_t), hipHostMallocDefault));
  memset(c->hash_res, 0, M355_HASH_REQUESTS * HASH_RES_WORDS * sizeof(uint32_t));
  return M355_OK;
}
/* (behind sync_all: nothing is in flight; requests nobody collected are dropped) */
static void hash_requests_destroy(m355_ctx* c)
{
  for (auto& s : c->hash_slot) { if (s.planes) hipHostFree(s.planes); s = m355_ctx::HashSlot(); }
  for (auto& b : c->hash_pool) hipHostFree(b.first);
  c->hash_pool.clear();
  if (c->hash_rec) hipFree(c->hash_rec);
  if (c->hash_res) hipHostFree(c->hash_res);
  c->hash_rec = c->hash_res = nullptr;
}

/* the slots of m355_frame_measure_async: the same two kinds of record, 64-bit words */
static int measure_requests_create(m355_ctx* c)
{
  hipStream_t st = c->lanes[0].stream;
  HIPCHK(hipMalloc(&c->meas_rec, M355_MEASURE_REQUESTS * MEAS_REC_WORDS * sizeof(unsigned long long)));
  HIPCHK(hipMemsetAsync(c->meas_rec, 0, M355_MEASURE_REQUESTS * MEAS_REC_WORDS * sizeof(unsigned long long), st));
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipHostMalloc(&c->meas_res, M355_MEASURE_REQUESTS * MEAS_RES_WORDS * sizeof(unsigned long long), hipHostMallocDefault));
  memset(c->meas_res, 0, M355_MEASURE_REQUESTS * MEAS_RES_WORDS * sizeof(unsigned long long));
  return M355_OK;
}
static void measure_requests_destroy(m355_ctx* c)
{
  for (auto& s : c->meas_slot) { if (s.rows) hipHostFree(s.rows); s = m355_ctx::MeasSlot(); }
  for (auto& b : c->meas_pool) hipHostFree(b.first);
  c->meas_pool.clear();
  if (c->meas_rec) hipFree(c->meas_rec);
  if (c->meas_res) hipHostFree(c->meas_res);
  c->meas_rec = c->meas_res = nullptr;
}

int m355_create(int device, m355_ctx** out)
{
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(M355_ERR_NO_DEVICE, "no HIP device visible (the MI355X backend has no CPU fallback)");
  if (device < 0 || device >= n) return fail(M355_ERR_INVALID, "device %d out of range (0..%d)", device, n - 1);
  HIPCHK(hipSetDevice(device));
  m355_ctx* c = new m355_ctx;
  c->device = device;
  int rc = lane_create(c, c->lanes[0], 0);
  if (rc == M355_OK) rc = hash_requests_create(c);
  if (rc == M355_OK) rc = measure_requests_create(c);
  if (rc) { measure_requests_destroy(c); hash_requests_destroy(c); lane_destroy(c->lanes[0]); delete c; return rc; }
  *out = c;
  return M355_OK;
}

/* the exchange buffers of a sharded picture are read by the OTHER ranks' devices (m355_group_*: peer copies on their streams), which a hipFree on this
   device does not wait for: before they go, every device is drained (a rare path: teardown, or a handle re-used for another geometry) */
static void drain_all_devices(int keep_current)
{
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return;
  for (int d = 0; d < n; d++) if (hipSetDevice(d) == hipSuccess) hipDeviceSynchronize();
  hipSetDevice(keep_current);
}

static void resident_free(Resident& r)
{
  if (r.xb[0]) { int cur = 0; hipGetDevice(&cur); drain_all_devices(cur); }
  for (void* b : r.xb) if (b) hipFree(b);
  if (r.xscratch) hipFree(r.xscratch);
  for (hipEvent_t e : r.x3_read) if (e) hipEventDestroy(e);
  if (r.dev) hipFree(r.dev);
  if (r.host) hipHostFree(r.host);
  if (r.refs_dev) hipFree(r.refs_dev);
  if (r.refs_host) hipHostFree(r.refs_host);
  r = Resident();
}

void m355_destroy(m355_ctx* c)
{
  if (!c) return;
  hipSetDevice(c->device);
  sync_all(c);
  if (c->ipc) m355_shard_ipc_close(c);          /* (first: it waits for the other ranks' last reads of this rank's exchange buffers) */
  for (auto& f : c->frames) if (f.used) frame_free(f);
  for (auto& r : c->resident) if (r.used) resident_free(r);
  for (auto& t : c->transient) resident_free(t);
  for (hipEvent_t e : c->evs) hipEventDestroy(e);
  if (c->hash_acc) hipFree(c->hash_acc);
  hash_requests_destroy(c);
  measure_requests_destroy(c);
  for (auto& e : c->inter_tabs) hipFree(e.second);
  for (auto& b : c->batch) { if (b.host) hipHostFree(b.host); if (b.dev) hipFree(b.dev); if (b.ev) hipEventDestroy(b.ev); }
  for (hipEvent_t e : c->batch_ev_pre) if (e) hipEventDestroy(e);
  for (hipStream_t bs : c->batch_stream) if (bs) hipStreamDestroy(bs);
  if (c->rccl && g_rccl.CommDestroy) g_rccl.CommDestroy(c->rccl);
  for (auto& e_ : c->evring) if (e_.ev) hipEventDestroy(e_.ev);
  if (c->status_words) hipHostFree(c->status_words);
  for (auto& q : c->colour) if (q.dev) hipFree(q.dev);
  if (c->stage) hipHostFree(c->stage);
  for (Lane& l : c->lanes) lane_destroy(l);
  delete c;
}

/* 1: pictures run one after the other on the context's stream (default).  2: consecutive decodes alternate between two
 * lanes (own streams, working planes and scratch) and overlap wherever the frames they touch allow it: a decode waits
 * for the last writer of every reference frame it reads, and — only right before its first write — for the last writer
 * and the readers of its destination frame. */
int m355_set_pipeline_depth(m355_ctx* c, int depth)
{
  if (depth < 1 || depth > M355_MAX_LANES) return fail(M355_ERR_INVALID, "pipeline depth must be 1..%d", M355_MAX_LANES);
  hipSetDevice(c->device);
  HIPCHK(sync_all(c));
  select_lane(c, 0);
  for (int k = 1; k < depth; k++)
    if (!c->lanes[k].stream) {
      int rc = lane_create(c, c->lanes[k], k);
      if (rc) return rc;
    }
  c->depth = depth;
  return M355_OK;
}

/* the stream the active lane's last decode / phase ran on (an intra picture on lane 3.. runs on the lane's class stream, decode()) */
void* m355_stream(m355_ctx* c) { const Lane& l = lane(c); return (void*)(l.last_stream ? l.last_stream : l.stream); }

/* ------------------------------------------------------------------------------ frames -------- */

int m355_frame_create(m355_ctx* c, int width, int height, int cf, int bdl, int bdc)
{
  if (width <= 0 || height <= 0 || cf < 0 || cf > 3 || bdl < 8 || bdl > 16 || bdc < 8 || bdc > 16) return -fail(M355_ERR_INVALID, "bad frame geometry");
  if ((width & 7) || (height & 7)) return -fail(M355_ERR_INVALID, "frame size %dx%d: HEVC pictures are multiples of the minimum coding block size (>= 8)", width, height);
  if ((bdl <= 8) != (bdc <= 8) && cf != 0) return -fail(M355_ERR_INVALID, "luma/chroma must both be 8-bit or both be 9..16-bit");
  hipSetDevice(c->device);
  int idx = -1;
  for (size_t i = 0; i < c->frames.size(); i++) if (!c->frames[i].used) { idx = (int)i; break; }
  if (idx < 0) { c->frames.push_back(Frame()); idx = (int)c->frames.size() - 1; }
  Frame& f = c->frames[idx];
  f = Frame();
  frame_geometry(f, width, height, cf, bdl, bdc);
  int rc = frame_alloc(f, lane(c).stream);
  if (rc) { frame_free(f); return -rc; }
  /* the zero fill is this frame's first write: whichever lane touches the frame next orders itself after it */
  ev_mark(c, lane(c).stream, &f.wr);
  return idx;
}
Frame* get_frame(m355_ctx* c, int h) {
  if (h < 0 || h >= (int)c->frames.size() || !c->frames[h].used) return nullptr;
  return &c->frames[h];
}
int m355_frame_destroy(m355_ctx* c, int h)
{
  Frame* f = get_frame(c, h);
  if (!f) return fail(M355_ERR_INVALID, "bad frame handle %d", h);
  hipSetDevice(c->device);
  sync_all(c);
  frame_free(*f);
  return M355_OK;
}
/* The blocking transfers of a plane go through a pinned staging buffer of the context and a copy QUEUED ON A STREAM OF THE LIBRARY (the frame's last writer's for a
 * download) — not a blocking hipMemcpy2D between the device and pageable memory on the null stream.  Round 6's soak with 32 processes sharing the GPU and pictures of
 * 1-14 Mi samples (tools/soak_recheck.py, profiles/r06_v35_*): the blocking copies now and then delivered planes with stale / missing rows IN BOTH DIRECTIONS — 46 of
 * 1600 pictures: a reference uploaded wrong (every decode from it then repeats the same wrong samples), or a correct frame downloaded wrong with a different set of
 * samples on every call — while the copies of m355_frame_download_async (pinned planes, the writer's stream) were right every time; alone on the GPU neither fails. */
static int stage_reserve(m355_ctx* c, size_t bytes)
{
  if (bytes <= c->stage_bytes) return M355_OK;
  if (c->stage) { hipHostFree(c->stage); c->stage = nullptr; c->stage_bytes = 0; }
  const size_t want = (bytes + ((size_t)4 << 20) - 1) & ~(((size_t)4 << 20) - 1);
  if (hipHostMalloc(&c->stage, want, hipHostMallocDefault) != hipSuccess) { c->stage = nullptr; return fail(M355_ERR_NOMEM, "staging buffer of %zu bytes", want); }
  c->stage_bytes = want;
  return M355_OK;
}
/* rows of row_bytes bytes: device plane -> host (pitch dst_pitch bytes) */
static int frame_stage_down(m355_ctx* c, Frame* f, int cidx, void* dst, size_t dst_pitch)
{
  const size_t rb = (size_t)f->pw[cidx] * f->bpp[cidx];
  int rc = stage_reserve(c, rb * f->ph[cidx]);
  if (rc) return rc;
  hipStream_t st = f->wr_stream ? f->wr_stream : lane(c).stream;
  HIPCHK(hipMemcpy2DAsync(c->stage, rb, f->plane[cidx], (size_t)f->stride[cidx] * f->bpp[cidx], rb, f->ph[cidx], hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (dst_pitch == rb) memcpy(dst, c->stage, rb * f->ph[cidx]);
  else for (int y = 0; y < f->ph[cidx]; y++) memcpy((uint8_t*)dst + (size_t)y * dst_pitch, (const uint8_t*)c->stage + (size_t)y * rb, rb);
  return M355_OK;
}
static int frame_stage_up(m355_ctx* c, Frame* f, int cidx, const void* src, size_t src_pitch)
{
  const size_t rb = (size_t)f->pw[cidx] * f->bpp[cidx];
  int rc = stage_reserve(c, rb * f->ph[cidx]);
  if (rc) return rc;
  if (src_pitch == rb) memcpy(c->stage, src, rb * f->ph[cidx]);
  else for (int y = 0; y < f->ph[cidx]; y++) memcpy((uint8_t*)c->stage + (size_t)y * rb, (const uint8_t*)src + (size_t)y * src_pitch, rb);
  const hipStream_t st = lane(c).stream;
  HIPCHK(hipMemcpy2DAsync(f->plane[cidx], (size_t)f->stride[cidx] * f->bpp[cidx], c->stage, rb, rb, f->ph[cidx], hipMemcpyHostToDevice, st));
  HIPCHK(hipStreamSynchronize(st));
  return M355_OK;
}
int m355_frame_upload(m355_ctx* c, int h, int cidx, const void* src, ptrdiff_t stride)
{
  Frame* f = get_frame(c, h);
  if (!f || cidx < 0 || cidx > 2 || !f->pw[cidx]) return fail(M355_ERR_INVALID, "bad frame/plane");
  hipSetDevice(c->device);
  HIPCHK(sync_all(c));
  return frame_stage_up(c, f, cidx, src, (size_t)stride * f->bpp[cidx]);
}
int m355_frame_download(m355_ctx* c, int h, int cidx, void* dst, ptrdiff_t stride)
{
  Frame* f = get_frame(c, h);
  if (!f || cidx < 0 || cidx > 2 || !f->pw[cidx]) return fail(M355_ERR_INVALID, "bad frame/plane");
  hipSetDevice(c->device);
  HIPCHK(sync_all(c));
  return frame_stage_down(c, f, cidx, dst, (size_t)stride * f->bpp[cidx]);
}
/* The download of a whole frame, asynchronous: a READER of the frame (reader_begin) — the copies run behind the frame's last writer and beside the
 * decodes of later pictures; the next picture written into the frame waits for them.  dst planes should be pinned (m355_host_alloc), else the
 * copies are staged by the runtime and block. */
int m355_frame_download_async(m355_ctx* c, int h, void* const dst[3], const ptrdiff_t stride[3])
{
  Frame* f = get_frame(c, h);
  if (!f || !dst || !stride) return fail(M355_ERR_INVALID, "bad frame / destination");
  for (int cc = 0; cc < 3; cc++) if (f->pw[cc] && !dst[cc]) return fail(M355_ERR_INVALID, "no destination for plane %d", cc);
  hipSetDevice(c->device);
  const hipStream_t cs = reader_begin(c, f, RD_DOWNLOAD);
  for (int cc = 0; cc < 3; cc++) {
    if (!f->pw[cc]) continue;
    HIPCHK(hipMemcpy2DAsync(dst[cc], (size_t)stride[cc] * f->bpp[cc], f->plane[cc], (size_t)f->stride[cc] * f->bpp[cc],
                            (size_t)f->pw[cc] * f->bpp[cc], f->ph[cc], hipMemcpyDeviceToHost, cs));
  }
  return reader_end(c, f, RD_DOWNLOAD, cs);
}
/* wait (this frame's download only) until the planes handed to m355_frame_download_async hold the picture */
int m355_frame_download_wait(m355_ctx* c, int h)
{
  Frame* f = get_frame(c, h);
  if (!f) return fail(M355_ERR_INVALID, "bad frame handle %d", h);
  hipSetDevice(c->device);
  HIPCHK(ev_sync(c, f->reader[RD_DOWNLOAD]));
  f->reader[RD_DOWNLOAD] = EvRef();
  return M355_OK;
}
/* What m355_frame_export and m355_frame_export_scaled share: the argument checks and, per plane of the launch (semi-planar: plane 1 = Cb and Cr
 * interleaved), where the rectangle starts in the frame, its size and where it goes.  log2_scale = k: the rectangle must divide into blocks of 1 << k
 * samples on every plane's grid, and row_bytes / the pitch check are those of the SCALED row. */
struct ExportPlane {
  const uint8_t* src[2];            /* the rectangle's first sample (src[1]: the Cr plane of an interleaved row) */
  uint8_t* dst;
  long long src_pitch, dst_pitch;   /* bytes */
  int pw, ph, bd, sb, db;           /* the rectangle on this plane (source samples), bit depth, bytes per source / destination sample */
  int64_t row_bytes;                /* of a destination row */
};
struct ExportPlan { Frame* f; int np; bool semi; ExportPlane p[3]; };
static int export_plan(m355_ctx* c, int h, const m355_export_desc* e, int k, const char* who, ExportPlan& P)
{
  Frame* f = get_frame(c, h);
  if (!f || !e) return fail(M355_ERR_INVALID, "bad frame handle %d / null descriptor", h);
  if (e->layout != M355_EXPORT_PLANAR && e->layout != M355_EXPORT_SEMIPLANAR) return fail(M355_ERR_INVALID, "%s: unknown layout %d", who, e->layout);
  if (e->samples != M355_EXPORT_NATIVE && e->samples != M355_EXPORT_MSB16 && e->samples != M355_EXPORT_U8) return fail(M355_ERR_INVALID, "%s: unknown sample format %d", who, e->samples);
  const int sw = (f->cf == 1 || f->cf == 2) ? 2 : 1, sh = f->cf == 1 ? 2 : 1, fs = 1 << k;
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
    q.row_bytes = (int64_t)(q.pw >> k) * q.db * (P.semi && p ? 2 : 1);
    if (!e->dst[p]) return fail(M355_ERR_INVALID, "%s: no destination for plane %d", who, p);
    if (e->pitch[p] < q.row_bytes) return fail(M355_ERR_INVALID, "%s: pitch %lld of plane %d is below its row of %lld bytes", who, (long long)e->pitch[p], p, (long long)q.row_bytes);
    q.dst = (uint8_t*)e->dst[p]; q.dst_pitch = e->pitch[p];
    q.src_pitch = (long long)f->stride[p] * q.sb;
    for (int j = 0; j < (P.semi && p ? 2 : 1); j++) q.src[j] = (const uint8_t*)f->plane[p + j] + (size_t)py * q.src_pitch + (size_t)px * q.sb;
  }
  return M355_OK;
}

extern "C++" {             /* (templates over the descriptors and the kernel arguments) */
/* export_plan for the calls that check their destinations themselves: r = what holds the rectangle (a descriptor or a region; null: no descriptor),
 * planned as an export of `layout` / `samples` whose destinations — `dst` for every plane, with a pitch no row exceeds — cannot fail unless dst is null */
template <class R>
static int export_plan_rect(m355_ctx* c, int h, const R* r, const void* dst, const char* who, ExportPlan& P, int layout = M355_EXPORT_PLANAR, int samples = M355_EXPORT_NATIVE)
{
  m355_export_desc yuv = {};
  if (r) {
    yuv.layout = layout; yuv.samples = samples;
    yuv.x0 = r->x0; yuv.y0 = r->y0; yuv.width = r->width; yuv.height = r->height;
    for (int p = 0; p < 3; p++) { yuv.dst[p] = (void*)dst; yuv.pitch[p] = INT64_MAX; }
  }
  return export_plan(c, h, r ? &yuv : nullptr, 0, who, P);
}
/* The checks of the R'G'B' descriptors (m355_rgb_desc, m355_resize_rgb_desc) behind the plan: the layout, the conversion (into a.k) and the destinations
 * of rows of `width` pixels (into a.dst / a.dst_pitch) */
template <class D, class A>
static int rgb_desc_check(const char* who, const D* e, const Frame* f, int64_t width, A& a, bool* planar_out, int* db_out)
{
  if (e->layout != M355_RGB_PACKED && e->layout != M355_RGB_PLANAR) return fail(M355_ERR_INVALID, "%s: unknown layout %d", who, e->layout);
  int rc = m355_rgb_coefficients(e->matrix, e->full_range, f->bdl, f->bdc, e->samples, &a.k);
  if (rc) return rc;
  const bool planar = e->layout == M355_RGB_PLANAR;
  const int db = e->samples == M355_RGB_U16 ? 2 : 1;
  const int64_t row_bytes = width * db * (planar ? 1 : 3);
  for (int p = 0; p < (planar ? 3 : 1); p++) {
    if (!e->dst[p]) return fail(M355_ERR_INVALID, "%s: no destination for plane %d", who, p);
    if (e->pitch[p] < row_bytes) return fail(M355_ERR_INVALID, "%s: pitch %lld of plane %d is below its row of %lld bytes", who, (long long)e->pitch[p], p, (long long)row_bytes);
    if (db == 2 && (((uintptr_t)e->dst[p] | (uint64_t)e->pitch[p]) & 1)) return fail(M355_ERR_INVALID, "%s: 16-bit plane %d at an odd address or pitch", who, p);
    a.dst[p] = (uint8_t*)e->dst[p]; a.dst_pitch[p] = e->pitch[p];
  }
  *planar_out = planar; *db_out = db;
  return M355_OK;
}
}
/* The frame, or a rectangle of it, converted into memory of the caller (k_export.hip): one launch for all planes.  The export is a READER of the
 * frame (reader_begin): the mark behind it is what the next decode into the frame waits for (dst_hazards), what m355_frame_export_wait blocks on
 * and what m355_frame_export_order makes a consumer's stream wait for. */
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
      a.dst[p] = q.dst; a.dst_pitch[p] = q.dst_pitch;
      a.src_pitch[p] = q.src_pitch;
      a.row_bytes[p] = (uint32_t)q.row_bytes; a.chunks[p] = (uint32_t)((q.row_bytes + 1023) / 1024);
      a.shift[p] = e->samples == M355_EXPORT_MSB16 ? 16 - q.bd : (e->samples == M355_EXPORT_U8 ? q.bd - 8 : 0);
      units += a.chunks[p] * (uint32_t)q.ph;
      a.src[p] = q.src[0];
      if (P.semi && p) a.src[2] = q.src[1];
    }
    a.unit_end[p] = units;
  }
  hipSetDevice(c->device);
  const hipStream_t cs = reader_begin(c, P.f, RD_EXPORT, &a.timeout, &a.epoch);
  m355_launch_export(a, P.f->bpp[0], P.p[0].db, P.semi, cs);
  HIPCHK(hipGetLastError());
  return reader_end(c, P.f, RD_EXPORT, cs);
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
      a.dst[p] = q.dst; a.dst_pitch[p] = q.dst_pitch;
      a.src_pitch[p] = q.src_pitch;
      a.out_w[p] = (uint32_t)(q.pw >> log2_scale); a.chunks[p] = (uint32_t)(((int64_t)q.pw * q.sb + 1023) / 1024);
      a.rshift[p] = 2 * log2_scale + (e->samples == M355_EXPORT_U8 ? q.bd - 8 : 0);
      a.lshift[p] = e->samples == M355_EXPORT_MSB16 ? 16 - q.bd : 0;
      units += a.chunks[p] * (uint32_t)(q.ph >> log2_scale);
      a.src[p] = q.src[0];
      if (P.semi && p) a.src[2] = q.src[1];
    }
    a.unit_end[p] = units;
  }
  hipSetDevice(c->device);
  const hipStream_t cs = reader_begin(c, P.f, RD_EXPORT, &a.timeout, &a.epoch);
  m355_launch_export_scaled(a, P.f->bpp[0], P.p[0].db, P.semi, log2_scale, cs);
  HIPCHK(hipGetLastError());
  return reader_end(c, P.f, RD_EXPORT, cs);
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
/* m355_export_opts behind the plan of a frame like f (a batch: frames[0], whose chroma format every frame shares): null = the defaults; the reserved
 * entries, the colour transform and the chroma sample location type, which is 4:2:0's alone.  The filter is checked where it is used (resize_check); resizes = false: the
 * call has no filter to choose. */
static int opts_check(const char* who, m355_ctx* c, const m355_export_opts* o, const Frame* f, bool resizes, m355_export_opts& out, ColourArgs* colour = nullptr)
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
  }
  if (!resizes && o->filter != M355_FILTER_TRIANGLE) return fail(M355_ERR_INVALID, "%s: filter %d where nothing is resized", who, o->filter);
  if (o->chroma_loc < 0 || o->chroma_loc > 3) return fail(M355_ERR_INVALID, "%s: chroma sample location type %d is not 0..3", who, o->chroma_loc);
  if (o->chroma_loc && f->cf != 1) return fail(M355_ERR_INVALID, "%s: chroma sample location type %d for a frame that is not 4:2:0", who, o->chroma_loc);
  out = *o;
  return M355_OK;
}
/* The frame, or a rectangle of it, as R'G'B' (k_export_rgb.hip): the frame handle and the rectangle are checked by export_plan — as a planar NATIVE
 * export whose destinations cannot fail —, the destinations here.  A reader of the kind RD_EXPORT, like the two above. */
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
  hipSetDevice(c->device);
  const hipStream_t cs = reader_begin(c, f, RD_EXPORT, &a.timeout, &a.epoch);
  m355_launch_export_rgb(a, sb, db, planar, f->cf, o.chroma_loc, cs);
  HIPCHK(hipGetLastError());
  return reader_end(c, f, RD_EXPORT, cs);
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
/* The width of k_export_resized's tiles on one plane: 256 output columns, or a few less where that saves a wavefront — the lanes of the vertical pass
 * own the 16-byte vectors of the tile's source span, and a span of 64 k + a few vectors (256 columns at ratio 4: 129) would run a wavefront for them. */
static uint32_t resize_tile_w(int filter, int64_t sn, int64_t dn, int sb)
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
static int resize_check(const char* who, const ExportPlan* P, int entries, int ow, int oh, int filter)
{
  if (filter != M355_FILTER_TRIANGLE && filter != M355_FILTER_CUBIC) return fail(M355_ERR_INVALID, "%s: unknown filter %d", who, filter);
  const Frame* f = P[0].f;
  const int sw = (f->cf == 1 || f->cf == 2) ? 2 : 1, sh = f->cf == 1 ? 2 : 1;
  if (ow <= 0 || oh <= 0 || ow % sw || oh % sh)
    return fail(M355_ERR_INVALID, "%s: output size %dx%d is not positive or no multiple of %dx%d luma samples", who, ow, oh, sw, sh);
  for (int i = 0; i < (entries ? entries : 1); i++) {
    const int pw = P[i].p[0].pw, ph = P[i].p[0].ph;
    if (m355_resize_ratio_ok_filtered(filter, pw, ow) && m355_resize_ratio_ok_filtered(filter, ph, oh)) continue;
    if (filter == M355_FILTER_CUBIC && entries)
      return fail(M355_ERR_INVALID, "%s: entry %d, %dx%d to %dx%d is more than 4x down or 8x up, or a size above %d (cubic filter)", who, i, pw, ph, ow, oh, M355_RESIZE_CUBIC_MAX_N);
    if (filter == M355_FILTER_CUBIC)
      return fail(M355_ERR_INVALID, "%s: %dx%d to %dx%d is more than 4x down or 8x up, or a size above %d (cubic filter)", who, pw, ph, ow, oh, M355_RESIZE_CUBIC_MAX_N);
    if (entries) return fail(M355_ERR_INVALID, "%s: entry %d, %dx%d to %dx%d is more than 8x down or up", who, i, pw, ph, ow, oh);
    return fail(M355_ERR_INVALID, "%s: %dx%d to %dx%d is more than 8x down or up", who, pw, ph, ow, oh);
  }
  return M355_OK;
}
/* The frame, or a rectangle of it, resized to out_width x out_height luma samples (k_export_resized.hip): the frame handle, the rectangle, the layout and
 * the samples are checked by export_plan — with destinations that cannot fail, as for the R'G'B' export —, the output size, the ratio and the destinations
 * here.  A reader of the kind RD_EXPORT, like the three above. */
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
  const int sw = (f->cf == 1 || f->cf == 2) ? 2 : 1, sh = f->cf == 1 ? 2 : 1;
  rc = resize_check(who, &P, 0, e->out_width, e->out_height, filter);
  if (rc) return rc;
  const bool cubic = filter == M355_FILTER_CUBIC;               /* (its intermediate keeps 16 bits of fraction and its sums their sign: shifts 2 and 1 less) */
  ExportResizedArgs a = {};
  uint32_t units = 0;
  for (int p = 0; p < 3; p++) {
    if (p < P.np) {
      const ExportPlane& q = P.p[p];
      const int ow = p ? e->out_width / sw : e->out_width, oh = p ? e->out_height / sh : e->out_height;
      const int64_t row_bytes = (int64_t)ow * q.db * (P.semi && p ? 2 : 1);
      if (!e->dst[p]) return fail(M355_ERR_INVALID, "%s: no destination for plane %d", who, p);
      if (e->pitch[p] < row_bytes) return fail(M355_ERR_INVALID, "%s: pitch %lld of plane %d is below its row of %lld bytes", who, (long long)e->pitch[p], p, (long long)row_bytes);
      a.src[p] = q.src[0];
      if (P.semi && p) a.src[2] = q.src[1];
      a.dst[p] = (uint8_t*)e->dst[p]; a.dst_pitch[p] = e->pitch[p];
      a.src_pitch[p] = q.src_pitch;
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
  hipSetDevice(c->device);
  const hipStream_t cs = reader_begin(c, f, RD_EXPORT, &a.timeout, &a.epoch);
  m355_launch_export_resized(a, f->bpp[0], P.p[0].db, P.semi, filter, cs);
  HIPCHK(hipGetLastError());
  return reader_end(c, f, RD_EXPORT, cs);
}
extern "C++" {
/* the options of a _filtered call: that filter, chroma sample location type 0 */
static m355_export_opts filter_opts(int filter) { m355_export_opts o = {}; o.filter = filter; return o; }
}
int m355_frame_export_resized_filtered(m355_ctx* c, int h, const m355_resize_desc* e, int filter)
{
  const m355_export_opts o = filter_opts(filter);
  return m355_frame_export_resized_opts(c, h, e, &o);
}
int m355_frame_export_resized(m355_ctx* c, int h, const m355_resize_desc* e) { return m355_frame_export_resized_opts(c, h, e, nullptr); }
/* The width of k_export_resized_rgb's tiles: a pass of that kernel takes two luma rows, or two rows of Cb and of Cr, where their source vectors fit
 * the workgroup's 256 lanes, and a workgroup's time follows its number of passes — so the widest width (even for 4:2:0 / 4:2:2: a tile's first column
 * is a chroma column) not above resize_tile_w's at which they fit, but at least 64 columns, then the narrowest one with the same number of tiles. */
static uint32_t resize_rgb_tile_w(int filter, int64_t sn, int64_t dn, int64_t csn, int64_t cdn, int sb, int sw, int centre)
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
extern "C++" {
/* The colour transform stage of a composed export into its kernel arguments: the object's tables and matrix, and the coefficients of M355_RGB_U16
 * in place of the descriptor's samples', which then only pick the delivery (the kernel's element bytes, or the tensors' u16) */
template <class D, class A> static int colour_apply(const ColourArgs& colour, const D* e, const Frame* f, A& a)
{
  if (!colour.t) return M355_OK;
  a.colour = colour;
  return m355_rgb_coefficients(e->matrix, e->full_range, f->bdl, f->bdc, M355_RGB_U16, &a.k);
}
}
/* The colour transform objects (include/de265_mi355x.h, COLOUR TRANSFORM): the tables go to device memory of the context through its pinned staging
 * buffer and the active lane's stream, like m355_device_write's bytes; the exports find an object by its handle (opts_check). */
static std::atomic<int> g_colour_handle{0x100};
int m355_colour_create(m355_ctx* c, const m355_colour_tables* t, int* handle)
{
  if (!c || !t || !handle) return fail(M355_ERR_INVALID, "m355_colour_create: no context / tables / handle");
  const int bad = m355_ct_tables_check(t);
  if (bad) return fail(M355_ERR_INVALID, "m355_colour_create: %s", bad == 1 ? "an entry of lut_in is above M355_COLOUR_ONE" : (bad == 2 ? "a matrix entry is outside -65535..65535" : "pad is not 0"));
  m355_ctx::ColourObj* obj = nullptr;
  for (auto& q : c->colour) if (!q.handle && !obj) obj = &q;
  if (!obj) return fail(M355_ERR_BUSY, "m355_colour_create: %d colour transforms live (destroy one: m355_colour_destroy)", M355_COLOUR_OBJECTS);
  hipSetDevice(c->device);
  int rc = stage_reserve(c, sizeof(*t));
  if (rc) return rc;
  uint8_t* dev = nullptr;
  if (hipMalloc(&dev, sizeof(*t)) != hipSuccess) return fail(M355_ERR_NOMEM, "m355_colour_create: hipMalloc(%zu) failed", sizeof(*t));
  memcpy(c->stage, t, sizeof(*t));
  const hipStream_t st = lane(c).stream;
  if (hipMemcpyAsync(dev, c->stage, sizeof(*t), hipMemcpyHostToDevice, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
    hipFree(dev);
    return fail(M355_ERR_HIP, "m355_colour_create: the copy of the tables failed");
  }
  obj->dev = dev;
  for (int k = 0; k < 9; k++) obj->matrix[k] = t->matrix[k];
  *handle = obj->handle = g_colour_handle.fetch_add(1);
  return M355_OK;
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
extern "C++" {             /* (templates over the descriptors and the kernel arguments) */
/* What the kernel arguments of k_export_resized_rgb.hip take from a plan.  plan_sources: the rectangle's first samples and the two pitches, into the
 * launch's or the slice's record.  plan_geometry: the source size on both grids, the tile width, the tiles per row of tiles and the units into g (the
 * launch's or the slice's record), the output size on both grids into d (the launch's). */
template <class R> static void plan_sources(const ExportPlan& Q, R& r)
{
  for (int p = 0; p < Q.np; p++) r.src[p] = Q.p[p].src[0];
  r.src_pitch[0] = Q.p[0].src_pitch; r.src_pitch[1] = Q.np > 1 ? Q.p[1].src_pitch : 0;
}
template <class G, class D> static void plan_geometry(const ExportPlan& Q, int ow, int oh, int filter, int chroma_loc, G& g, D& d)
{
  const Frame* f = Q.f;
  const int sw = (f->cf == 1 || f->cf == 2) ? 2 : 1, sh = f->cf == 1 ? 2 : 1;
  g.sn_x[0] = (uint32_t)Q.p[0].pw; g.sn_y[0] = (uint32_t)Q.p[0].ph; d.dn_x[0] = (uint32_t)ow; d.dn_y[0] = (uint32_t)oh;
  if (Q.np > 1) { g.sn_x[1] = (uint32_t)Q.p[1].pw; g.sn_y[1] = (uint32_t)Q.p[1].ph; d.dn_x[1] = (uint32_t)(ow / sw); d.dn_y[1] = (uint32_t)(oh / sh); }
  g.tile_w = resize_rgb_tile_w(filter, Q.p[0].pw, ow, Q.np > 1 ? Q.p[1].pw : 0, ow / sw, f->bpp[0], sw, chroma_loc & 1);
  g.tiles_x = ((uint32_t)ow + g.tile_w - 1) / g.tile_w;
  g.units = g.tiles_x * (((uint32_t)oh + M355_RESIZE_TILE_H - 1) / M355_RESIZE_TILE_H);
}
}
/* The same resize with the R'G'B' conversion of the resized picture behind it, in one launch (k_export_resized_rgb.hip, RR_FRAME): the frame handle and
 * the rectangle are checked by export_plan — with destinations that cannot fail —, the output size and the ratio as for the resized export, the
 * conversion and the destinations as for the R'G'B' export, with the OUTPUT width.  A reader of the kind RD_EXPORT, like the four above. */
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
  hipSetDevice(c->device);
  const hipStream_t cs = reader_begin(c, f, RD_EXPORT, &a.timeout, &a.epoch);
  m355_launch_export_resized_rgb(a, f->bpp[0], db, filter, cs);
  HIPCHK(hipGetLastError());
  return reader_end(c, f, RD_EXPORT, cs);
}
int m355_frame_export_resized_rgb_filtered(m355_ctx* c, int h, const m355_resize_rgb_desc* e, int filter)
{
  const m355_export_opts o = filter_opts(filter);
  return m355_frame_export_resized_rgb_opts(c, h, e, &o);
}
int m355_frame_export_resized_rgb(m355_ctx* c, int h, const m355_resize_rgb_desc* e) { return m355_frame_export_resized_rgb_opts(c, h, e, nullptr); }
/* the float stage of m355_frames_export_tensor for one value (tensor_element.h: the function the kernel calls) */
int m355_tensor_element(uint32_t v, float scale, float bias, int dtype, uint32_t* bits)
{
  const auto finite = [](float x) { return (m355_te_bits(x) & 0x7F800000u) != 0x7F800000u; };
  if (!bits || (dtype != M355_TENSOR_F32 && dtype != M355_TENSOR_F16 && dtype != M355_TENSOR_BF16) || !finite(scale) || !finite(bias))
    return fail(M355_ERR_INVALID, "m355_tensor_element: null result / unknown dtype %d / scale or bias not finite", dtype);
  *bits = m355_te_element(v, scale, bias, dtype);
  return M355_OK;
}
extern "C++" {             /* (templates over the descriptors and the kernel arguments) */
/* What the two tensor exports share (k_export_resized_rgb.hip, RR_BATCH and RR_ROIS).  batch_frame_check: frame i of the batch against frame 0 —
 * chroma format and bit depths, and the size where whole frames must agree. */
static int batch_frame_check(const char* who, const int* frames, int i, const ExportPlan* P, bool same_size)
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
static int tensor_desc_check(const char* who, const m355_tensor_desc* e, int n, const Frame* f, A& a, int* eb_out)
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
static hipStream_t batch_reader_begin(m355_ctx* c, const ExportPlan* P, int n, R* fr)
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
static int batch_reader_end(m355_ctx* c, const ExportPlan* P, int n, hipStream_t cs)
{
  Frame* f = P[0].f;
  int rc = reader_end(c, f, RD_EXPORT, cs);
  if (rc) return rc;
  for (int i = 1; i < n; i++) P[i].f->reader[RD_EXPORT] = f->reader[RD_EXPORT];
  return M355_OK;
}
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
  hipSetDevice(c->device);
  const hipStream_t cs = batch_reader_begin(c, P, n, a.fr);
  m355_launch_export_tensor(a, P[0].f->bpp[0], eb, filter, cs);
  HIPCHK(hipGetLastError());
  return batch_reader_end(c, P, n, cs);
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
  hipSetDevice(c->device);
  const hipStream_t cs = batch_reader_begin(c, P, n, a.fr);
  m355_launch_export_tensor_rois(a, P[0].f->bpp[0], eb, filter, cs);
  HIPCHK(hipGetLastError());
  return batch_reader_end(c, P, n, cs);
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
/* Device memory for the destinations of m355_frame_export, for applications (and tests) that have no HIP runtime of their own in the process */
void* m355_device_alloc(m355_ctx* c, size_t bytes)
{
  if (!c) { fail(M355_ERR_INVALID, "m355_device_alloc: no context"); return nullptr; }
  hipSetDevice(c->device);
  void* p = nullptr;
  if (hipMalloc(&p, bytes ? bytes : 1) != hipSuccess) { fail(M355_ERR_NOMEM, "hipMalloc(%zu) failed", bytes); return nullptr; }
  return p;
}
void m355_device_free(m355_ctx* c, void* p)
{
  if (!c || !p) return;
  hipSetDevice(c->device);
  sync_all(c);                                              /* (an export into it may still be running) */
  hipFree(p);
}
int m355_device_read(m355_ctx* c, const void* src, void* dst, size_t bytes)
{
  if (!c || (bytes && (!src || !dst))) return fail(M355_ERR_INVALID, "m355_device_read: bad arguments");
  if (!bytes) return M355_OK;
  hipSetDevice(c->device);
  HIPCHK(sync_all(c));                                      /* whichever lane's export wrote the memory */
  int rc = stage_reserve(c, bytes);
  if (rc) return rc;
  const hipStream_t st = lane(c).stream;
  HIPCHK(hipMemcpyAsync(c->stage, src, bytes, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  memcpy(dst, c->stage, bytes);
  return M355_OK;
}
int m355_device_write(m355_ctx* c, void* dst, const void* src, size_t bytes)
{
  if (!c || (bytes && (!src || !dst))) return fail(M355_ERR_INVALID, "m355_device_write: bad arguments");
  if (!bytes) return M355_OK;
  hipSetDevice(c->device);
  HIPCHK(sync_all(c));                                      /* (an export into the memory, on whichever lane) */
  int rc = stage_reserve(c, bytes);
  if (rc) return rc;
  memcpy(c->stage, src, bytes);
  const hipStream_t st = lane(c).stream;
  HIPCHK(hipMemcpyAsync(dst, c->stage, bytes, hipMemcpyHostToDevice, st));
  HIPCHK(hipStreamSynchronize(st));
  return M355_OK;
}
int m355_frame_fill(m355_ctx* c, int h, int vl, int vc)
{
  Frame* f = get_frame(c, h);
  if (!f) return fail(M355_ERR_INVALID, "bad frame handle %d", h);
  hipSetDevice(c->device);
  HIPCHK(sync_all(c));
  const hipStream_t st = lane(c).stream;
  for (int cc = 0; cc < 3; cc++) {
    if (!f->pw[cc]) continue;
    const size_t n = (size_t)f->stride[cc] * f->ph[cc];
    const int v = cc ? vc : vl;
    if (f->bpp[cc] == 1) { HIPCHK(hipMemsetAsync(f->plane[cc], v, n, st)); HIPCHK(sync_all(c)); }
    else {
      int rc = stage_reserve(c, n * 2);
      if (rc) return rc;
      std::fill((uint16_t*)c->stage, (uint16_t*)c->stage + n, (uint16_t)v);
      HIPCHK(hipMemcpyAsync(f->plane[cc], c->stage, n * 2, hipMemcpyHostToDevice, st));
      HIPCHK(hipStreamSynchronize(st));
    }
  }
  return M355_OK;
}

/* float4 copy, grid-stride, streaming stores: the shape of the guide's "6.29 TB/s measured (float4 copy)" figure */
__global__ void __launch_bounds__(256) k_copy_rate(const uint4* __restrict__ src, uint4* __restrict__ dst, size_t n16)
{
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (size_t)gridDim.x * 256) {
    const uint4 v = src[i];
    d_st_nt8(&dst[i].x, v.x, v.y); d_st_nt8(&dst[i].z, v.z, v.w);
  }
}
int m355_measure_copy_rate(m355_ctx* c, size_t bytes, int iters, double* gbps)
{
  if (!c || !gbps || bytes < (1u << 20) || iters < 1) return fail(M355_ERR_INVALID, "bad arguments");
  hipSetDevice(c->device);
  HIPCHK(sync_all(c));
  void *a = nullptr, *b = nullptr;
  if (hipMalloc(&a, bytes) != hipSuccess || hipMalloc(&b, bytes) != hipSuccess) { if (a) hipFree(a); return fail(M355_ERR_NOMEM, "hipMalloc(%zu) failed", bytes); }
  const hipStream_t st = lane(c).stream;
  hipMemsetAsync(a, 0x5A, bytes, st);
  hipEvent_t e0, e1;
  hipEventCreate(&e0); hipEventCreate(&e1);
  const size_t n16 = bytes / 16;
  const unsigned grid = (unsigned)std::min<size_t>((n16 + 255) / 256, 256 * 32);
  std::vector<float> ms((size_t)iters, 0.f);
  for (int i = -2; i < iters; i++) {
    hipEventRecord(e0, st);
    hipLaunchKernelGGL(k_copy_rate, dim3(grid), dim3(256), 0, st, (const uint4*)a, (uint4*)b, n16);
    hipEventRecord(e1, st);
    hipEventSynchronize(e1);
    if (i >= 0) hipEventElapsedTime(&ms[(size_t)i], e0, e1);
  }
  hipEventDestroy(e0); hipEventDestroy(e1);
  hipFree(a); hipFree(b);
  std::sort(ms.begin(), ms.end());
  const float med = ms[ms.size() / 2];
  *gbps = med > 0.f ? 2.0 * (double)(n16 * 16) / (med * 1e-3) / 1e9 : 0.0;
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? M355_OK : fail(M355_ERR_HIP, "copy kernel failed: %s", hipGetErrorString(e));
}

void* m355_host_alloc(size_t bytes)
{
  void* p = nullptr;
  if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) { fail(M355_ERR_NOMEM, "hipHostMalloc(%zu) failed", bytes); return nullptr; }
  return p;
}
void m355_host_free(void* p) { if (p) hipHostFree(p); }

/* the launch arguments of the hash kernels for the frame's planes (a.out / the request stay with the caller) */
static void hash_args_fill(const Frame* f, HashArgs& a)
{
  const int np = f->pw[1] ? 3 : 1;
  /* enough waves to fill 1024 SIMDs a few times over, each still covering >= 1 row */
  int rows = 0, nw = 0;
  for (int cc = 0; cc < np; cc++) rows += f->ph[cc];
  a.rows_per_wave = std::max(1, rows / 4096);
  for (int cc = 0; cc < 3; cc++) {
    a.first[cc] = nw;
    if (cc >= np) continue;
    a.pl[cc].base = (const uint8_t*)f->plane[cc];
    a.pl[cc].pitch = (size_t)f->stride[cc] * f->bpp[cc];
    a.pl[cc].row_bytes = f->pw[cc] * f->bpp[cc];
    a.pl[cc].h = f->ph[cc];
    a.pl[cc].bpp = f->bpp[cc];
    nw += (f->ph[cc] + a.rows_per_wave - 1) / a.rows_per_wave;
  }
  a.first[3] = nw;
}
/* MD5 of `np` planes in host memory (rows packed: pitch = row_bytes), one thread per plane: each is one serial chain (k_hash.hip) */
static void md5_planes(int np, const uint8_t* const base[3], const int row_bytes[3], const int rows[3], m355_picture_hash* out)
{
  std::vector<std::thread> th;
  for (int cc = 0; cc < np; cc++) th.emplace_back([=] { m355_md5_rows(base[cc], (size_t)row_bytes[cc], row_bytes[cc], rows[cc], out->md5[cc]); });
  for (auto& t : th) t.join();
}

int m355_frame_hash(m355_ctx* c, int h, int type, m355_picture_hash* out)
{
  Frame* f = get_frame(c, h);
  if (!f || !out) return fail(M355_ERR_INVALID, "bad frame handle %d / null result", h);
  if (type != M355_HASH_MD5 && type != M355_HASH_CRC && type != M355_HASH_CHECKSUM) return fail(M355_ERR_INVALID, "bad hash type %d", type);
  hipSetDevice(c->device);
  HIPCHK(sync_all(c));
  const int np = f->pw[1] ? 3 : 1;
  if (type == M355_HASH_MD5) {
    std::vector<uint8_t> host[3];
    const uint8_t* base[3] = {nullptr, nullptr, nullptr};
    int row_bytes[3] = {0, 0, 0};
    for (int cc = 0; cc < np; cc++) {
      row_bytes[cc] = f->pw[cc] * f->bpp[cc];
      host[cc].resize((size_t)row_bytes[cc] * f->ph[cc]);
      const int rc = frame_stage_down(c, f, cc, host[cc].data(), (size_t)row_bytes[cc]);
      if (rc) return rc;
      base[cc] = host[cc].data();
    }
    md5_planes(np, base, row_bytes, f->ph, out);
    return M355_OK;
  }
  if (!c->hash_acc) HIPCHK(hipMalloc(&c->hash_acc, 4 * sizeof(uint32_t)));
  HashArgs a = {};
  a.out = c->hash_acc;
  hash_args_fill(f, a);
  uint32_t acc[4] = {0, 0, 0, 0};
  const hipStream_t st = lane(c).stream;
  HIPCHK(hipMemsetAsync(c->hash_acc, 0, 4 * sizeof(uint32_t), st));
  m355_launch_frame_hash(a, type, st);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(acc, c->hash_acc, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  for (int cc = 0; cc < np; cc++) {
    if (type == M355_HASH_CRC) out->crc[cc] = (uint16_t)(acc[cc] ^ m355_crc_init_term((uint64_t)a.pl[cc].row_bytes * a.pl[cc].h));
    else out->checksum[cc] = acc[cc];
  }
  return M355_OK;
}

/* ---- hash requests (m355_frame_hash_async / m355_frame_hash_result) ---- */

static m355_ctx::HashSlot* hash_slot_of(m355_ctx* c, unsigned long long ticket)
{
  if (ticket) for (auto& s : c->hash_slot) if (s.ticket == ticket) return &s;
  return nullptr;
}
/* an MD5 request's pinned planes: the smallest idle buffer that fits, else a new one (nothing is freed here: hipHostFree may wait for the device —
   a buffer smaller than the largest one made is freed when its request is collected, hash_slot_free) */
static int hash_planes_take(m355_ctx* c, m355_ctx::HashSlot& s, size_t bytes)
{
  int best = -1;
  for (int k = 0; k < (int)c->hash_pool.size(); k++)
    if (c->hash_pool[k].second >= bytes && (best < 0 || c->hash_pool[k].second < c->hash_pool[best].second)) best = k;
  if (best < 0) {
    void* p = nullptr;
    const size_t want = (bytes + ((size_t)1 << 20) - 1) & ~(((size_t)1 << 20) - 1);
    if (hipHostMalloc(&p, want, hipHostMallocDefault) != hipSuccess) return fail(M355_ERR_NOMEM, "pinned planes of %zu bytes for an MD5 request", want);
    s.planes = (uint8_t*)p; s.planes_cap = want;
    return M355_OK;
  }
  s.planes = c->hash_pool[best].first; s.planes_cap = c->hash_pool[best].second;
  c->hash_pool.erase(c->hash_pool.begin() + best);
  return M355_OK;
}
static void hash_slot_free(m355_ctx* c, m355_ctx::HashSlot& s)
{
  if (s.planes) {
    /* the pool grows to the largest frame seen: smaller buffers of earlier, smaller frames are idle pinned memory, and they go here — where the caller
       has just waited for its request anyway — first the pool's, then this one if a larger one exists */
    size_t largest = s.planes_cap;
    for (const auto& x : c->hash_slot) largest = std::max(largest, x.planes_cap);
    for (const auto& b : c->hash_pool) largest = std::max(largest, b.second);
    for (size_t k = c->hash_pool.size(); k-- > 0;) if (c->hash_pool[k].second < largest) { hipHostFree(c->hash_pool[k].first); c->hash_pool.erase(c->hash_pool.begin() + k); }
    if (s.planes_cap < largest) hipHostFree(s.planes);
    else c->hash_pool.push_back(std::make_pair(s.planes, s.planes_cap));
  }
  s.planes = nullptr; s.planes_cap = 0;
  /* a request is collected behind its mark: the next decode into its frame has nothing to wait for (a wait packet saved where the request is collected before
     the frame is recycled: about 2 us, profiles/r04_aj_stage_events_ab.txt) — if the frame's mark is still this request's: handles are reused, tickets are not */
  Frame* f = get_frame(c, s.frame);
  if (f && s.mark.ticket && f->reader[RD_HASH].ticket == s.mark.ticket) f->reader[RD_HASH] = EvRef();
  s.mark = EvRef(); s.frame = -1;
  s.ticket = 0;
}

/* Enqueue only: the host waits for nothing here.  A READER of the frame (reader_begin), like m355_frame_export: the next decode into the frame waits for the
   request's mark (dst_hazards), which the slot remembers for m355_frame_hash_result. */
int m355_frame_hash_async(m355_ctx* c, int h, int type, unsigned long long* ticket)
{
  Frame* f = get_frame(c, h);
  if (!f || !ticket) return fail(M355_ERR_INVALID, "m355_frame_hash_async: bad frame handle %d / null ticket", h);
  if (type != M355_HASH_MD5 && type != M355_HASH_CRC && type != M355_HASH_CHECKSUM) return fail(M355_ERR_INVALID, "m355_frame_hash_async: bad hash type %d", type);
  if (c->shard_n > 0) return fail(M355_ERR_INVALID, "m355_frame_hash_async: not on a tile-sharded context (its frames are complete only behind the gather)");
  m355_ctx::HashSlot* s = nullptr;
  for (auto& x : c->hash_slot) if (!x.ticket) { s = &x; break; }
  if (!s) return fail(M355_ERR_BUSY, "m355_frame_hash_async: %d requests outstanding (collect one: m355_frame_hash_result)", M355_HASH_REQUESTS);
  const int slot = (int)(s - c->hash_slot);
  hipSetDevice(c->device);
  s->type = type; s->np = f->pw[1] ? 3 : 1;
  size_t plane_ofs[3] = {0, 0, 0}, bytes = 0;
  for (int cc = 0; cc < 3; cc++) {
    s->row_bytes[cc] = cc < s->np ? f->pw[cc] * f->bpp[cc] : 0;
    s->rows[cc] = cc < s->np ? f->ph[cc] : 0;
    plane_ofs[cc] = bytes;
    bytes += ((size_t)s->row_bytes[cc] * s->rows[cc] + 255) & ~(size_t)255;
  }
  if (type == M355_HASH_MD5) { int rc = hash_planes_take(c, *s, bytes); if (rc) return rc; }
  HashReq q = {};
  q.rec = c->hash_rec + slot * HASH_REC_WORDS;
  q.res = c->hash_res + slot * HASH_RES_WORDS;
  q.seq = (uint32_t)(c->hash_ticket + 1);
  q.res[3] = HASH_RES_NONE;                                                     /* (the slot is idle: nothing in flight writes its record) */
  HashArgs a = {};
  a.out = q.rec;
  if (type != M355_HASH_MD5) hash_args_fill(f, a);
  const hipStream_t cs = reader_begin(c, f, RD_HASH, &q.timeout, &q.epoch);
  /* (MD5: behind a rejected decode the copies bring an older picture's planes: the verdict says so, the result is never made of them) */
  for (int cc = 0; type == M355_HASH_MD5 && cc < s->np; cc++)
    if (hipMemcpy2DAsync(s->planes + plane_ofs[cc], (size_t)s->row_bytes[cc], f->plane[cc], (size_t)f->stride[cc] * f->bpp[cc], (size_t)s->row_bytes[cc], s->rows[cc],
                         hipMemcpyDeviceToHost, cs) != hipSuccess) { hash_slot_free(c, *s); return fail(M355_ERR_HIP, "m355_frame_hash_async: copy of plane %d failed", cc); }
  m355_launch_frame_hash_req(a, q, type, cs);
  if (hipGetLastError() != hipSuccess || reader_end(c, f, RD_HASH, cs) != M355_OK) { hash_slot_free(c, *s); return fail(M355_ERR_HIP, "m355_frame_hash_async: launch failed"); }
  s->mark = f->reader[RD_HASH]; s->frame = h;
  s->ticket = ++c->hash_ticket;
  *ticket = s->ticket;
  return M355_OK;
}

int m355_frame_hash_result(m355_ctx* c, unsigned long long ticket, int block, m355_picture_hash* out)
{
  m355_ctx::HashSlot* s = hash_slot_of(c, ticket);
  if (!s) return fail(M355_ERR_INVALID, "m355_frame_hash_result: ticket %llu is unknown or was collected", ticket);
  if (!out) return fail(M355_ERR_INVALID, "m355_frame_hash_result: null result");
  hipSetDevice(c->device);
  if (block) HIPCHK(ev_sync(c, s->mark));                                       /* this request's mark only */
  else {
    const hipError_t e = ev_query(c, s->mark);
    if (e == hipErrorNotReady) return M355_ERR_BUSY;
    if (e != hipSuccess) return fail(M355_ERR_HIP, "hipEventQuery failed: %s", hipGetErrorString(e));
  }
  const uint32_t* res = c->hash_res + (s - c->hash_slot) * HASH_RES_WORDS;
  const uint32_t state = res[3], seq = res[4];
  if (state == HASH_RES_GATED && seq == (uint32_t)ticket) {
    hash_slot_free(c, *s);
    return fail(M355_ERR_INVALID, "hash request %llu was queued behind a decode whose lists were rejected: no value", ticket);
  }
  if (state != HASH_RES_VALID || seq != (uint32_t)ticket) {
    hash_slot_free(c, *s);
    return fail(M355_ERR_HIP, "hash request %llu finished without a result (state %u, sequence %u)", ticket, state, seq);
  }
  if (s->type == M355_HASH_MD5) {
    const uint8_t* base[3] = {s->planes, nullptr, nullptr};
    for (int cc = 1; cc < s->np; cc++) base[cc] = base[cc - 1] + (((size_t)s->row_bytes[cc - 1] * s->rows[cc - 1] + 255) & ~(size_t)255);
    md5_planes(s->np, base, s->row_bytes, s->rows, out);
  } else
    for (int cc = 0; cc < s->np; cc++) {
      if (s->type == M355_HASH_CRC) out->crc[cc] = (uint16_t)(res[cc] ^ m355_crc_init_term((uint64_t)s->row_bytes[cc] * s->rows[cc]));
      else out->checksum[cc] = res[cc];
    }
  hash_slot_free(c, *s);
  return M355_OK;
}

/* ---- comparison requests (m355_frame_measure_async / m355_frame_measure_result): the hash requests' machinery with another kernel (k_measure.hip),
   a second frame to read, and a pinned row array per request ---- */

static m355_ctx::MeasSlot* meas_slot_of(m355_ctx* c, unsigned long long ticket)
{
  if (ticket) for (auto& s : c->meas_slot) if (s.ticket == ticket) return &s;
  return nullptr;
}
/* a request's pinned row array (one 64-bit sum per row of every plane: 69 KB for an 8K 4:2:0 frame): the smallest idle one that fits, else a new one.  Nothing
   is freed here: hipHostFree may wait for the device, and the enqueue waits for nothing (hash_planes_take) — arrays smaller than the largest one made go when a
   request is collected, meas_slot_free */
static int meas_rows_take(m355_ctx* c, m355_ctx::MeasSlot& s, size_t entries)
{
  int best = -1;
  for (int k = 0; k < (int)c->meas_pool.size(); k++)
    if (c->meas_pool[k].second >= entries && (best < 0 || c->meas_pool[k].second < c->meas_pool[best].second)) best = k;
  if (best < 0) {
    void* p = nullptr;
    const size_t want = (entries + 8191) & ~(size_t)8191;
    if (hipHostMalloc(&p, want * sizeof(unsigned long long), hipHostMallocDefault) != hipSuccess) return fail(M355_ERR_NOMEM, "pinned row array of %zu entries for a comparison request", want);
    s.rows = (unsigned long long*)p; s.rows_cap = want;
    return M355_OK;
  }
  s.rows = c->meas_pool[best].first; s.rows_cap = c->meas_pool[best].second;
  c->meas_pool.erase(c->meas_pool.begin() + best);
  return M355_OK;
}
static void meas_slot_free(m355_ctx* c, m355_ctx::MeasSlot& s)
{
  if (s.rows) {
    /* the arrays grow to the tallest frame seen; smaller ones of earlier, shorter frames go here, where the caller has just waited for its request anyway
       (hash_slot_free): first the pool's, then this one if a larger one exists */
    size_t largest = s.rows_cap;
    for (const auto& x : c->meas_slot) largest = std::max(largest, x.rows_cap);
    for (const auto& b : c->meas_pool) largest = std::max(largest, b.second);
    for (size_t k = c->meas_pool.size(); k-- > 0;) if (c->meas_pool[k].second < largest) { hipHostFree(c->meas_pool[k].first); c->meas_pool.erase(c->meas_pool.begin() + k); }
    if (s.rows_cap < largest) hipHostFree(s.rows);
    else c->meas_pool.push_back(std::make_pair(s.rows, s.rows_cap));
  }
  s.rows = nullptr; s.rows_cap = 0;
  /* collected behind its mark: the next decode into either frame has nothing to wait for, if the frame's mark is still this request's (hash_slot_free) */
  for (int k = 0; k < 2; k++) {
    Frame* f = get_frame(c, s.frame[k]);
    if (f && s.mark.ticket && f->reader[RD_MEASURE].ticket == s.mark.ticket) f->reader[RD_MEASURE] = EvRef();
    s.frame[k] = -1;
  }
  s.mark = EvRef();
  s.ticket = 0;
}

/* Enqueue only: the host waits for nothing here.  A READER of the frame (reader_begin) and of the reference frame: the kernel runs on the stream of the frame's
   last writer, which first continues behind the reference frame's last writer (as a decode waits for the writers of its reference frames) and behind that frame's
   earlier comparison mark; ONE mark behind the launch is kept by both frames and by the slot. */
int m355_frame_measure_async(m355_ctx* c, int h, const m355_measure_desc* e, unsigned long long* ticket)
{
  Frame* f = c ? get_frame(c, h) : nullptr;
  if (!f || !e || !ticket) return fail(M355_ERR_INVALID, "m355_frame_measure_async: bad frame handle %d / null descriptor / null ticket", h);
  if (c->shard_n > 0) return fail(M355_ERR_INVALID, "m355_frame_measure_async: not on a tile-sharded context (its frames are complete only behind the gather)");
  const int sw = (f->cf == 1 || f->cf == 2) ? 2 : 1, sh = f->cf == 1 ? 2 : 1;
  int x0 = 0, y0 = 0, w = f->w, hgt = f->h;
  if (e->width != 0) {
    x0 = e->x0; y0 = e->y0; w = e->width; hgt = e->height;
    if (x0 < 0 || y0 < 0 || w <= 0 || hgt <= 0 || x0 > f->w - w || y0 > f->h - hgt) return fail(M355_ERR_INVALID, "m355_frame_measure_async: rectangle %d,%d %dx%d leaves the %dx%d frame", x0, y0, w, hgt, f->w, f->h);
    if (f->cf && ((x0 | w) % sw || (y0 | hgt) % sh)) return fail(M355_ERR_INVALID, "m355_frame_measure_async: rectangle %d,%d %dx%d is not aligned to the chroma grid (%dx%d luma samples)", x0, y0, w, hgt, sw, sh);
  }
  Frame* r = nullptr;
  if (e->ref_frame != -1) {
    r = get_frame(c, e->ref_frame);
    if (!r) return fail(M355_ERR_INVALID, "m355_frame_measure_async: bad reference frame handle %d", e->ref_frame);
    if (r->cf != f->cf || r->bdl != f->bdl || r->bdc != f->bdc || r->bpp[0] != f->bpp[0]) return fail(M355_ERR_INVALID, "m355_frame_measure_async: the reference frame's chroma format / bit depths differ from the frame's");
    if (x0 > r->w - w || y0 > r->h - hgt) return fail(M355_ERR_INVALID, "m355_frame_measure_async: the %dx%d reference frame does not contain the rectangle %d,%d %dx%d", r->w, r->h, x0, y0, w, hgt);
  }
  const int np = f->cf == 0 ? 1 : 3;
  MeasArgs a = {};
  int rows = 0, nw = 0;
  for (int p = 0; p < np; p++) rows += p ? hgt / sh : hgt;
  a.rows_per_wave = std::max(1, rows / 4096);                                   /* (hash_args_fill: enough waves to fill 1024 SIMDs a few times over) */
  m355_ctx::MeasSlot geom;
  for (int p = 0, row0 = 0; p < 3; p++) {
    a.first[p] = nw;
    if (p >= np) continue;
    const int sb = f->bpp[p];
    const int pw = p ? w / sw : w, ph = p ? hgt / sh : hgt, px = p ? x0 / sw : x0, py = p ? y0 / sh : y0;
    MeasPlane& m = a.pl[p];
    m.pitch_a = (long long)f->stride[p] * sb;
    m.a = (const uint8_t*)f->plane[p] + (size_t)py * m.pitch_a + (size_t)px * sb;
    if (r) {
      m.pitch_b = (long long)r->stride[p] * sb;
      m.b = (const uint8_t*)r->plane[p] + (size_t)py * m.pitch_b + (size_t)px * sb;
    } else {
      if (!e->ref[p]) return fail(M355_ERR_INVALID, "m355_frame_measure_async: no reference for plane %d", p);
      if (e->pitch[p] < (int64_t)pw * sb) return fail(M355_ERR_INVALID, "m355_frame_measure_async: pitch %lld of plane %d is below its row of %lld bytes", (long long)e->pitch[p], p, (long long)pw * sb);
      if (((uintptr_t)e->ref[p] | (uintptr_t)e->pitch[p]) & (uintptr_t)(sb - 1)) return fail(M355_ERR_INVALID, "m355_frame_measure_async: pointer / pitch of plane %d is no multiple of the %d-byte element", p, sb);
      m.pitch_b = e->pitch[p];
      m.b = (const uint8_t*)e->ref[p];
    }
    m.row_bytes = pw * sb; m.h = ph; m.px = px; m.py = py; m.row0 = row0;
    geom.pw[p] = pw; geom.ph[p] = ph; geom.row0[p] = row0;
    row0 += ph;
    nw += (ph + a.rows_per_wave - 1) / a.rows_per_wave;
  }
  a.first[3] = nw;
  m355_ctx::MeasSlot* s = nullptr;
  for (auto& x : c->meas_slot) if (!x.ticket) { s = &x; break; }
  if (!s) return fail(M355_ERR_BUSY, "m355_frame_measure_async: %d requests outstanding (collect one: m355_frame_measure_result)", M355_MEASURE_REQUESTS);
  const int slot = (int)(s - c->meas_slot);
  hipSetDevice(c->device);
  int rc = meas_rows_take(c, *s, (size_t)rows);
  if (rc) return rc;
  s->np = np;
  for (int p = 0; p < 3; p++) { s->pw[p] = geom.pw[p]; s->ph[p] = geom.ph[p]; s->row0[p] = geom.row0[p]; }
  MeasReq q = {};
  q.rec = c->meas_rec + slot * MEAS_REC_WORDS;
  q.res = c->meas_res + slot * MEAS_RES_WORDS;
  q.rows = s->rows;
  q.seq = (uint32_t)(c->meas_ticket + 1);
  q.res[15] = MEAS_RES_NONE;                                                    /* (the slot is idle: nothing in flight writes its record) */
  const hipStream_t cs = reader_begin(c, f, RD_MEASURE, &q.timeout[0], &q.epoch[0]);
  q.timeout[1] = q.timeout[0]; q.epoch[1] = q.epoch[0];
  if (r && r != f) {
    ev_wait(c, cs, r->wr);                                                      /* the reference frame's last writer (nothing to enqueue when that ran on `cs`) */
    ev_wait(c, cs, r->reader[RD_MEASURE]);                                      /* ... and its earlier comparison on another stream: the one mark kept stands for both */
    if (r->wr_stream && r->wr_gate) { q.timeout[1] = r->wr_gate; q.epoch[1] = r->wr_epoch; }
  }
  m355_launch_measure(a, q, f->bpp[0], cs);
  if (hipGetLastError() != hipSuccess || reader_end(c, f, RD_MEASURE, cs) != M355_OK) { meas_slot_free(c, *s); return fail(M355_ERR_HIP, "m355_frame_measure_async: launch failed"); }
  s->mark = f->reader[RD_MEASURE]; s->frame[0] = h; s->frame[1] = -1;
  if (r && r != f) { r->reader[RD_MEASURE] = s->mark; s->frame[1] = e->ref_frame; }
  s->ticket = ++c->meas_ticket;
  *ticket = s->ticket;
  return M355_OK;
}

int m355_frame_measure_result(m355_ctx* c, unsigned long long ticket, int block, m355_measure* out)
{
  m355_ctx::MeasSlot* s = c ? meas_slot_of(c, ticket) : nullptr;
  if (!s) return fail(M355_ERR_INVALID, "m355_frame_measure_result: ticket %llu is unknown or was collected", ticket);
  if (!out) return fail(M355_ERR_INVALID, "m355_frame_measure_result: null result");
  hipSetDevice(c->device);
  if (block) HIPCHK(ev_sync(c, s->mark));                                       /* this request's mark only */
  else {
    const hipError_t e = ev_query(c, s->mark);
    if (e == hipErrorNotReady) return M355_ERR_BUSY;
    if (e != hipSuccess) return fail(M355_ERR_HIP, "hipEventQuery failed: %s", hipGetErrorString(e));
  }
  const unsigned long long* res = c->meas_res + (s - c->meas_slot) * MEAS_RES_WORDS;
  const unsigned long long state = res[15], seq = res[16];
  if (state == MEAS_RES_GATED && seq == (uint32_t)ticket) {
    meas_slot_free(c, *s);
    return fail(M355_ERR_INVALID, "comparison request %llu was queued behind a decode whose lists were rejected: no value", ticket);
  }
  if (state != MEAS_RES_VALID || seq != (uint32_t)ticket) {
    meas_slot_free(c, *s);
    return fail(M355_ERR_HIP, "comparison request %llu finished without a result (state %llu, sequence %llu)", ticket, state, seq);
  }
  memset(out, 0, sizeof(*out));
  for (int p = 0; p < 3; p++) {
    out->first_x[p] = out->first_y[p] = -1;
    if (p >= s->np) continue;
    const unsigned long long* v = res + p * MEAS_PER_PLANE;
    out->ssd[p] = v[MEAS_SSD]; out->sad[p] = v[MEAS_SAD]; out->n_diff[p] = v[MEAS_NDIFF]; out->max_abs[p] = (uint32_t)v[MEAS_MAX];
    if (v[MEAS_FIRST]) { const unsigned long long pos = ~v[MEAS_FIRST]; out->first_x[p] = (int32_t)(pos & 0xFFFFFFFFu); out->first_y[p] = (int32_t)(pos >> 32); }
    /* MSE() of quality.cc:71-95, in its order of operations */
    double sum = 0.0;
    for (int y = 0; y < s->ph[p]; y++) sum += ((double)s->rows[s->row0[p] + y]) / s->pw[p];
    out->mse[p] = sum / s->ph[p];
  }
  meas_slot_free(c, *s);
  return M355_OK;
}

/* room for `k` entries per list in the arenas of `r` (grown when it does not fit), list pointers into its pinned half */
static int arena_into(m355_ctx* c, Resident& r, m355_arena_caps* k, int halo_units, bool sharded, m355_picture* pic)
{
  Lay L;
  make_layout(*k, k->n_ctbs, halo_units, sharded, true, L);
  if (L.total > r.cap) {
    if (r.dev || r.host) HIPCHK(sync_all(c));
    if (r.dev) hipFree(r.dev);
    if (r.host) hipHostFree(r.host);
    r.dev = r.host = nullptr;
    r.cap = L.total + L.total / 4;
    HIPCHK(hipMalloc(&r.dev, r.cap));
    HIPCHK(hipHostMalloc(&r.host, r.cap, hipHostMallocDefault));
  } else if (r.done.ticket) {
    HIPCHK(ev_sync(c, r.done));                            /* the last decode of the lists that lived here */
    r.done = EvRef();
  }
  memset(pic, 0, sizeof(*pic));
  pic->slices = (const m355_slice*)(r.host + L.seg[L.i_sl].ofs);
  pic->ctbs = (const m355_ctb*)(r.host + L.seg[L.i_ct].ofs);
  pic->cus = (const m355_cu*)(r.host + L.seg[L.i_cu].ofs);
  pic->tus = (const m355_tu*)(r.host + L.seg[L.i_tu].ofs);
  pic->pbs = (const m355_pb*)(r.host + L.seg[L.i_pb].ofs);
  pic->wts = (const m355_wt*)(r.host + L.seg[L.i_wt].ofs);
  pic->rbs = (const m355_rb*)(r.host + L.seg[L.i_rb[0]].ofs);
  for (int b = 0; b < 4; b++) k->rb_bin[b] = (m355_rb*)(r.host + L.seg[L.i_rb[b]].ofs);
  r.arena = true; r.caps = *k; r.arena_halo_units = halo_units;
  pic->ibs = (const m355_ib*)(r.host + L.seg[L.i_ibin].ofs);
  pic->coeffs = (const uint32_t*)(r.host + L.seg[L.i_co].ofs);
  pic->pcm = (const uint16_t*)(r.host + L.seg[L.i_pc].ofs);
  pic->scaling_factors = k->scaling ? (const uint8_t*)(r.host + L.seg[L.i_sc].ofs) : nullptr;
  pic->dst_frame = -1;
  for (int i = 0; i < M355_MAX_REF_FRAMES; i++) pic->ref_frames[i] = -1;
  return M355_OK;
}
static bool caps_ok(const m355_arena_caps* k, const m355_picture* pic)
{
  return k && pic && k->n_ctbs > 0 && k->n_slices > 0 && k->n_cus >= 0 && k->n_tus >= 0 && k->n_pbs >= 0 && k->n_wts >= 0 && k->n_ibs >= 0 &&
         k->n_rbs[0] >= 0 && k->n_rbs[1] >= 0 && k->n_rbs[2] >= 0 && k->n_rbs[3] >= 0;
}

int m355_arena_begin(m355_ctx* c, m355_arena_caps* k, m355_picture* pic)
{
  if (!caps_ok(k, pic)) return fail(M355_ERR_INVALID, "bad arena capacities");
  if (c->shard_n >= 1) return fail(M355_ERR_INVALID, "m355_arena_begin is not available on a tile-sharded context (its pictures are decoded from handles: m355_picture_arena_begin)");
  hipSetDevice(c->device);
  return arena_into(c, c->transient[c->next_transient], k, 0, false, pic);   /* the arena the next m355_submit_picture uses */
}

/* residual records + coefficient list with every block that fits in the 16-bit entry form (M355_RBF_NARROW); host only.  rbs_out may be rbs_in. */
int m355_pack_narrow(const m355_rb* rbs_in, int n_rbs, const uint32_t* co_in, uint32_t n_in, m355_rb* rbs_out, uint32_t* co_out, uint32_t* n_out)
{
  if (n_rbs < 0 || (n_rbs && (!rbs_in || !rbs_out)) || (n_in && (!co_in || !co_out)) || !n_out) return fail(M355_ERR_INVALID, "m355_pack_narrow: bad arguments");
  /* the blocks keep the order they have in the list (records are binned by size, the list is in decode order): unpacking gives the input back word for word */
  std::vector<int> order((size_t)n_rbs);
  for (int i = 0; i < n_rbs; i++) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return rbs_in[a].coeff_ofs < rbs_in[b].coeff_ofs; });
  uint64_t o = 0;
  for (int i : order) {
    m355_rb rb = rbs_in[i];
    const uint32_t n = rb.ncoeff, words_in = (rb.flags & M355_RBF_NARROW) ? (n + 1) / 2 : n;
    if ((uint64_t)rb.coeff_ofs + words_in > n_in) return fail(M355_ERR_INVALID, "m355_pack_narrow: rb %d: coefficient range", i);
    const uint32_t* src = co_in + rb.coeff_ofs;
    bool fits = n > 0 && !(rb.flags & M355_RBF_NARROW);
    for (uint32_t k = 0; k < n && fits; k++) {
      const int lvl = (int16_t)(src[k] >> 16);
      fits = (src[k] & 0xFFFFu) < 256 && lvl >= -128 && lvl <= 127;
    }
    const uint32_t words_out = fits ? (n + 1) / 2 : words_in;
    /* (only lists whose blocks overlap can grow past their own length) */
    if (o + words_out > n_in) return fail(M355_ERR_INVALID, "m355_pack_narrow: rb %d: blocks share coefficients, the packed list would outgrow the input", i);
    uint32_t* dst = co_out + o;
    if (fits) {
      for (uint32_t k = 0; k < n; k += 2) {
        const uint32_t lo = (src[k] & 0xFFu) | ((src[k] >> 8) & 0xFF00u);
        const uint32_t hi = k + 1 < n ? (src[k + 1] & 0xFFu) | ((src[k + 1] >> 8) & 0xFF00u) : 0;     /* (the spare half of an odd block: never read) */
        dst[k >> 1] = lo | (hi << 16);
      }
      rb.flags |= M355_RBF_NARROW;
    } else if (words_out) memcpy(dst, src, 4 * (size_t)words_out);
    rb.coeff_ofs = (uint32_t)o;
    rbs_out[i] = rb;
    o += words_out;
  }
  *n_out = (uint32_t)o;
  return M355_OK;
}

/* the same for the arenas of a RESIDENT picture (tile-sharded contexts decode from handles): handle -1 makes one */
int m355_picture_arena_begin(m355_ctx* c, int h, m355_arena_caps* k, const m355_pic_params* pp, m355_picture* pic)
{
  if (!caps_ok(k, pic)) return -fail(M355_ERR_INVALID, "bad arena capacities");
  const bool sharded = c->shard_n >= 1;
  if (sharded && !pp) return -fail(M355_ERR_INVALID, "m355_picture_arena_begin: a tile-sharded context needs the picture parameters (room for the border units of other ranks)");
  int halo_units = 0;
  if (sharded) {
    if (pp->num_tile_cols < 1 || pp->num_tile_rows < 1 || pp->num_tile_cols > M355_MAX_TILE_COLS || pp->num_tile_rows > M355_MAX_TILE_ROWS || pp->width < 8 || pp->height < 8)
      return -fail(M355_ERR_INVALID, "m355_picture_arena_begin: bad picture parameters");
    HaloLayout halo;
    halo_layout(*pp, halo);
    halo_units = halo.n_units;
  }
  hipSetDevice(c->device);
  if (h < 0) {
    for (size_t i = 0; i < c->resident.size(); i++) if (!c->resident[i].used && !c->resident[i].reserved) { h = (int)i; break; }
    if (h < 0) { c->resident.push_back(Resident()); h = (int)c->resident.size() - 1; }
    c->resident[h].reserved = true;
  } else if (h >= (int)c->resident.size() || !(c->resident[h].used || c->resident[h].reserved)) return -fail(M355_ERR_INVALID, "bad picture handle");
  const int rc = arena_into(c, c->resident[h], k, halo_units, sharded, pic);
  return rc ? -rc : h;
}

int m355_submit_picture(m355_ctx* c, const m355_picture* pic)
{
  Resident& t = c->transient[c->next_transient];
  c->next_transient = (c->next_transient + 1) % c->transient_ring();
  /* the lists travel on the stream of the lane that decodes them: the copy of picture k runs beside the kernels of
     picture k-1 on the previous lane (uploading on the lane that is still active would queue it BEHIND those kernels) */
  if (c->depth >= 2) select_lane(c, (c->active + 1) % c->depth);
  static const bool prof = getenv("M355_PROFILE_UPLOAD") != nullptr;
  const auto t0 = std::chrono::steady_clock::now();
  int rc = upload(c, t, pic);
  t.arena = false;                                          /* pointers handed out by m355_arena_begin are spent */
  if (rc) return rc;
  const auto t1 = std::chrono::steady_clock::now();
  rc = decode(c, t, false);
  if (prof) fprintf(stderr, "m355 submit: upload (host phases + copy enqueue) %.3f ms, decode enqueue %.3f ms\n",
                    std::chrono::duration<double, std::milli>(t1 - t0).count(), std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count());
  return rc;
}

int m355_wait(m355_ctx* c)
{
  hipSetDevice(c->device);
  HIPCHK(sync_all(c));
  for (auto& f : c->frames) { f.wr = EvRef(); for (EvRef& m : f.reader) m = EvRef(); for (int k = 0; k < M355_MAX_LANES; k++) f.rd[k] = EvRef(); }   /* everything is complete */
  uint32_t t = 0;
  for (const Lane& l : c->lanes)
    if (l.timeout) { uint32_t t2 = 0; HIPCHK(hipMemcpy(&t2, l.timeout, 4, hipMemcpyDeviceToHost)); t |= t2; }
  /* lists checked on the device (recorded in place): the first rejected decode not reported yet (everything has finished) */
  {
    m355_ctx::Status* first = nullptr;
    for (m355_ctx::Status& st_ : c->status)
      if (st_.serial && st_.validated && !st_.reported && c->status_words[4 * (st_.serial % M355_STATUS_RING) + 1] == st_.epoch && (!first || st_.serial < first->serial)) first = &st_;
    if (c->lost_count) {
      const unsigned long long f = c->lost_first; const int n = c->lost_count;
      c->lost_first = 0; c->lost_count = 0;
      return fail(M355_ERR_INVALID, "picture %llu%s rejected by the device-side list validation (not decoded; its status had left the %d-entry ring: %d such picture%s)",
                  f, n > 1 ? " and later ones" : "", M355_STATUS_RING, n, n > 1 ? "s" : "");
    }
    if (first) return status_of(c, *first);
  }
  if (t) {
    for (const Lane& l : c->lanes) if (l.timeout) hipMemsetAsync(l.timeout, 0, 4, l.stream);
    sync_all(c);
    return fail(M355_ERR_TIMEOUT, "intra wavefront spin bound exceeded");
  }
  return M355_OK;
}

int m355_picture_upload(m355_ctx* c, const m355_picture* pic)
{
  int idx = -1;
  for (size_t i = 0; i < c->resident.size(); i++) if (!c->resident[i].used && !c->resident[i].reserved) { idx = (int)i; break; }
  if (idx < 0) { c->resident.push_back(Resident()); idx = (int)c->resident.size() - 1; }
  int rc = upload(c, c->resident[idx], pic);
  if (rc) { resident_free(c->resident[idx]); return -rc; }
  return idx;
}
/* new lists into the arenas of an uploaded picture (waits for the last decode of the old ones only — no allocation when they
   fit, no synchronisation of the context): how a caller cycles a few handles through a stream of pictures */
int m355_picture_replace(m355_ctx* c, int h, const m355_picture* pic)
{
  if (h < 0 || h >= (int)c->resident.size() || !(c->resident[h].used || c->resident[h].reserved) || !pic) return fail(M355_ERR_INVALID, "bad picture handle");
  Resident& r = c->resident[h];
  hipSetDevice(c->device);
  if (r.done.ticket) { HIPCHK(ev_sync(c, r.done)); r.done = EvRef(); }
  if (r.xb[0] && (memcmp(&r.hdr.pp, &pic->pp, sizeof(pic->pp)) != 0 || r.shard_n != c->shard_n || r.shard_rank != c->shard_rank)) {
    /* the exchange buffers of a sharded picture are sized by its geometry and tile structure */
    if (c->ipc) ipc_before_free(c, h);
    drain_all_devices(c->device);
    for (void*& b : r.xb) { if (b) hipFree(b); b = nullptr; }
    if (r.xscratch) { hipFree(r.xscratch); r.xscratch = nullptr; }
    for (hipEvent_t e : r.x3_read) if (e) hipEventDestroy(e);
    r.x3_read.clear();
    r.peers.clear();
  }
  const int rc = upload(c, r, pic);
  r.arena = false;                                          /* pointers handed out by m355_picture_arena_begin are spent */
  if (!rc) r.reserved = false;
  return rc;
}

int m355_picture_release(m355_ctx* c, int h)
{
  if (h < 0 || h >= (int)c->resident.size() || !(c->resident[h].used || c->resident[h].reserved)) return fail(M355_ERR_INVALID, "bad picture handle");
  hipSetDevice(c->device);
  sync_all(c);
  if (c->ipc && c->resident[h].xb[0]) ipc_before_free(c, h);     /* (the other rank processes' last reads of this handle's gather buffer) */
  resident_free(c->resident[h]);
  return M355_OK;
}
int m355_decode_resident(m355_ctx* c, int h)
{
  if (h < 0 || h >= (int)c->resident.size() || !c->resident[h].used) return fail(M355_ERR_INVALID, "bad picture handle");
  return decode(c, c->resident[h]);
}
int m355_set_stages(m355_ctx* c, int mask) { c->stages = mask & M355_STAGE_ALL; return M355_OK; }

int m355_timing_reset(m355_ctx* c) { c->ev_used = 0; c->timing_on = true; return M355_OK; }

/* averages over every decode enqueued since m355_timing_reset(); waits for them to finish */
int m355_timing_collect(m355_ctx* c, int* n_decodes, float* total_ms, float stage_ms[6])
{
  c->timing_on = false;
  if (c->ev_used == 0) return fail(M355_ERR_INVALID, "m355_timing_collect: no decode was timed — m355_timing_reset opens the timing window, this call (or an earlier one) closes it, and the pictures of m355_decode_batch are never stage-timed");
  hipSetDevice(c->device);
  HIPCHK(sync_all(c));
  double tot = 0, st[6] = {0, 0, 0, 0, 0, 0};
  for (int k = 0; k < c->ev_used; k++) {
    hipEvent_t* ev = &c->evs[k * 7];
    float ms;
    HIPCHK(hipEventElapsedTime(&ms, ev[0], ev[6])); tot += ms;
    /* stage order of the events: [meta, inter, residual, intra, deblock, sao] */
    for (int i = 0; i < 6; i++) { HIPCHK(hipEventElapsedTime(&ms, ev[i], ev[i + 1])); st[i] += ms; }
  }
  if (n_decodes) *n_decodes = c->ev_used;
  if (total_ms) *total_ms = (float)(tot / c->ev_used);
  if (stage_ms) for (int i = 0; i < 6; i++) stage_ms[i] = (float)(st[i] / c->ev_used);
  return M355_OK;
}

} /* extern "C" */
