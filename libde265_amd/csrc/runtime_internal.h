/*
 * runtime_internal.h — what the parts of the host runtime share: the context and its lanes, frames, resident pictures, the event
 * ring, the layout of an uploaded picture, and the prototypes of the functions one part calls in another.
 *   runtime.hip        context / lanes / frames / hashes / arenas / submit / wait / timing (the C ABI's entry points of those)
 *   runtime_export.hip the exports of a frame into memory of the caller (m355_frame_export* / m355_frames_export_tensor*), colour transform objects
 *   runtime_upload.hip host pool, validation, intra schedule, upload (lists -> one pinned arena -> device)
 *   runtime_decode.hip prepare, the per-picture launch sequence, decode status, m355_decode_batch
 *   runtime_stats.hip  statistics requests (m355_frame_stats_async)
 *   runtime_ssim.hip   SSIM requests (m355_frame_ssim_async)
 *   runtime_msssim.hip MS-SSIM requests (m355_frame_msssim_async)
 *   runtime_maps.hip   side maps of a picture's lists (m355_picture_maps_async)
 *   runtime_shard.hip  tile sharding: phases, exchanges, the in-process group, the built-in RCCL transport
 */
#ifndef M355_RUNTIME_INTERNAL_H
#define M355_RUNTIME_INTERNAL_H
#include <dlfcn.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <string>
#include <utility>
#include <vector>

#include <pthread.h>
#include "k_common.h"
#include "k_hash.h"
#include "k_measure.h"
#include "k_stats.h"
#include "k_ssim.h"
#include "k_msssim.h"
#include "k_maps.h"


extern thread_local std::string g_err;
int fail(int code, const char* fmt, ...);     /* sets the thread's last error text, returns `code` */
#define HIPCHK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return fail(M355_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); } while (0)

#define M355_STATUS_RING 64
#define M355_BATCH_RING 16 /* m355_decode_batch: picture-record arrays in flight (the host runs this many batches ahead) */
#define M355_MAX_LANES 32  /* pictures in flight per context (m355_set_pipeline_depth) */
#define M355_TRANSIENT_MAX 12 /* staging arenas of m355_submit_picture (m355_ctx::transient_ring) */

/* ---- THE SCHEDULE TABLE: every size / depth at which the runtime picks another launch order, in one place, with the measurement that set it
 * (all A/Bs of two settings in ONE gpurun call on one box; boxes of the pool differ by +-5 %).  Each row is a separate correctness surface: the
 * forced-schedule tests (tests/test_gpu_chain_forced.py, tests/test_emu_chain.py, tests/test_chain_residuals_emu.py, tests/test_meta_merged_emu.py)
 * walk every one of them deterministically. ---- */
namespace sched {
/* pictures of up to this many luma samples run ALL their launches on the lane's main stream (no fork / join packets: six packets at ~2 us each are
   worth more than what the side stream buys once the kernels are short): C3 / C4 0.110 -> 0.098 / 0.100 ms three in flight, C5 0.347 -> 0.351
   (profiles/r04_al_*).  Above it the metadata planes + border plans and the small-block residual launch run on the lane's side stream. */
constexpr long long one_stream_max_samples = 16ll << 20;
/* from this many prediction blocks on, the zero fill of the metadata planes rides in k_job_count's workgroups (one per 256 PBs) and the planes + job list
   are roles of one launch; below it a fill of its own is faster (a handful of workgroups cannot spread it): profiles/r04_ak_*, r05_v29_* */
constexpr int clear_in_count_min_pbs = 64 * 256;
/* transform edges + border plans inside the residual launch: only when the context decodes ONE picture at a time (C3 0.1494 -> 0.1427 ms, C4 0.1627 ->
   0.1564; with lanes the separate launch runs beside other pictures' kernels: C3 0.0688 -> 0.0697, a chain's picture 0.132 -> 0.136, profiles/r05_v30_*) */
constexpr int tu_plan_in_residuals_max_depth = 1;
/* k_intra's halo keeper (13th wave): with one picture in flight, or for an intra picture when no other lane is busy (C2 1.22 -> 0.90 ms one at a time;
   with three in flight the 13-wave workgroup crowds the other pictures' kernels out: 0.468 -> 0.536 ms, profiles/r05_v14_*) */
constexpr int intra_keeper_max_depth = 1;
/* a dependent chain's picture: front part on a spare lane from three lanes on (two lanes: the whole picture follows its reference onto that lane: C3 0.162 ->
   0.178 ms when split there, profiles/r05_v27_*); its residual transforms move into the front part (int16 tiles + k_residual_add) on one-stream lanes only
   (C3 0.131 -> 0.124 ms, C4 0.148 -> 0.140; C5 0.42-0.44 -> 0.44-0.45: profiles/r05_v31_*) */
constexpr int chain_split_min_depth = 3;
constexpr int chain_residual_tiles_min_depth = 3;
/* lanes 3.. decode INTRA pictures on a stream of the next priority class (own hardware queues): C2 0.340 ms per picture at depth 9 (profiles/r03_v_*) */
constexpr int intra_class_first_lane = 3;
/* inter pictures: the CTBs without a cross-CTB intra dependency run as LIGHT items of k_intra's launch — one wave per CTB and colour component, no CTB body
   in LDS (k_intra_light.h) — instead of one workgroup each: C5 0.3210 / 0.3215 / 0.3224 -> 0.3148 / 0.3139 / 0.3119 ms three in flight (three alternating rounds
   against the build before, medians of 5 regions; k_intra 39.3 -> 34.6 us one picture at a time, 90 -> 73 us three in flight, its wave-cycles 9.7e7 -> 5.4e7),
   C3 0.0677 -> 0.0665, C4 0.0761 -> 0.0757 (profiles/r07_a_light_ab.txt, r07_a_*_kernel_stats.txt, r07_a_*_pmc_summary.txt).  This row: do the CTBs that hold a
   32x32 intra block go there too?  One wave then predicts the block alone, where the CTB workgroup shares it among its component's waves: NO — on one box C5
   0.3390 / 0.3378 / 0.3375 before, 0.3298 / 0.3305 / 0.3286 with them on the light path, 0.3280 / 0.3284 / 0.3277 with them kept as workgroups
   (profiles/r07_a_light_32x32_ab.txt; M355_INTRA_LIGHT_32=0 / 1 overrides, tests/test_emu_intra_light.py and test_gpu_intra_light.py force the other setting) */
constexpr bool intra_light_32x32 = false;
}

/* A MARK = "everything enqueued on `stream` up to here", one event of the context's ring (ev_mark / ev_wait / ev_sync below).  The
 * objects a decode touches — destination and reference frames, its lists, its lane, its status slot — all remember the SAME mark
 * behind its last kernel: one event packet per decode instead of one per object (each costs about 2 us of pipeline time on this
 * runtime, profiles/r04_aj_stage_events_ab.txt). */
struct EvRef { unsigned long long ticket = 0; hipStream_t stream = nullptr; };
#define M355_EV_RING 256

enum ReaderKind { RD_DOWNLOAD, RD_EXPORT, RD_HASH, RD_MEASURE, RD_STATS, RD_SSIM, RD_MSSSIM, RD_KINDS };
struct Frame {
  bool used = false;
  int w = 0, h = 0, cf = 0, bdl = 0, bdc = 0;
  int pw[3] = {0, 0, 0}, ph[3] = {0, 0, 0}, stride[3] = {0, 0, 0}, bpp[3] = {1, 1, 1};
  void* plane[3] = {nullptr, nullptr, nullptr};
  /* pictures in flight on different lanes (m355_set_pipeline_depth): last writer / last readers per lane */
  EvRef wr, rd[M355_MAX_LANES];
  hipStream_t wr_stream = nullptr;         /* the stream that last wrote the frame */
  /* the gate of the decode that last wrote the frame (its lane's gate words, its epoch): a reader's kernel queued behind a decode whose lists were
     rejected does nothing, like that decode's own kernels (M355_GATE) */
  const uint32_t* wr_gate = nullptr; uint32_t wr_epoch = 0;
  /* READERS queued behind the decode that wrote the frame — a download (m355_frame_download_async), an export (m355_frame_export), a hash request
     (m355_frame_hash_async), a comparison (m355_frame_measure_async, which reads two frames and marks both), a statistics request (m355_frame_stats_async), an SSIM request (m355_frame_ssim_async, two frames like the comparison), an MS-SSIM request (m355_frame_msssim_async, likewise): per kind the mark behind the LAST one.  reader_begin picks the stream (the writer's, so stream order stands for the wait for the
     picture) and lets it continue behind the kind's earlier mark, so that the one mark kept stands for both; reader_end marks; the next decode into the frame
     waits for every kind in front of its first write (readers_wait, from dst_hazards).  The kinds are separate because the HOST waits per kind
     (m355_frame_download_wait, m355_frame_export_wait, m355_frame_hash_result, m355_frame_measure_result, m355_frame_stats_result, m355_frame_ssim_result, m355_frame_msssim_result), and a finished wait clears its mark: readers of different kinds need no order. */
  EvRef reader[RD_KINDS];
};

static void frame_geometry(Frame& f, int w, int h, int cf, int bdl, int bdc)
{
  f.w = w; f.h = h; f.cf = cf; f.bdl = bdl; f.bdc = bdc;
  const int sw = (cf == 1 || cf == 2) ? 2 : 1, sh = (cf == 1) ? 2 : 1;
  for (int c = 0; c < 3; c++) {
    f.bpp[c] = ((c ? bdc : bdl) <= 8) ? 1 : 2;
    if (c && cf == 0) { f.pw[c] = f.ph[c] = f.stride[c] = 0; continue; }
    f.pw[c] = c ? w / sw : w;
    f.ph[c] = c ? h / sh : h;
    const int pitch_bytes = (f.pw[c] * f.bpp[c] + 127) & ~127;
    f.stride[c] = pitch_bytes / f.bpp[c];
  }
}
/* NOTE on memsets: hipMemset() on the null stream may return before the fill has run, and the context's
 * stream is non-blocking (it does not order against the null stream) — a fill issued that way can land AFTER
 * kernels launched later on the context's stream (seen with 8 contexts sharing one GPU).  Every fill is
 * therefore enqueued on the context's own stream. */
static int frame_alloc(Frame& f, hipStream_t st)
{
  for (int c = 0; c < 3; c++) {
    if (!f.pw[c]) continue;
    const size_t bytes = (size_t)f.stride[c] * f.ph[c] * f.bpp[c] + 256;
    HIPCHK(hipMalloc(&f.plane[c], bytes));
    HIPCHK(hipMemsetAsync(f.plane[c], 0, bytes, st)); /* planes are zero at allocation (image.cc:164) */
  }
  f.used = true;
  return M355_OK;
}
static void frame_free(Frame& f)
{
  for (int c = 0; c < 3; c++) { if (f.plane[c]) hipFree(f.plane[c]); f.plane[c] = nullptr; }
  f.wr = EvRef();
  for (int k = 0; k < M355_MAX_LANES; k++) f.rd[k] = EvRef();
  for (EvRef& m : f.reader) m = EvRef();
  f.wr_stream = nullptr; f.wr_gate = nullptr; f.wr_epoch = 0;
  f.used = false;
}

/* one picture's lists resident in HBM */
struct Resident {
  bool used = false;
  m355_picture hdr;            /* counts + params (pointers are NOT valid) */
  char* dev = nullptr;         /* device arena */
  char* host = nullptr;        /* pinned staging arena */
  size_t cap = 0, bytes = 0;
  DevPic dp;                   /* device pointers filled at upload; frame planes at decode */
  DevRef* refs_dev = nullptr;  /* reference-frame table (device) */
  DevRef* refs_host = nullptr; /* pinned staging + last uploaded contents */
  bool refs_valid = false;
  int n_intra_work = 0;
  int n_intra_ticket = 0, n_intra_heavy = 0, n_intra_light = 0;   /* (what m355_debug_intra_counts reports) */
  uint32_t n_iplan = 0;        /* border-plan entries of the picture's intra blocks (k_intra_plan -> k_intra) */
  /* tile sharding (m355_decode_phase) */
  bool sharded = false;
  int shard_rank = 0, shard_n = 1;
  HaloLayout halo;
  DevPic live;                 /* the descriptor prepared by phase 0, reused by phases 1..4 */
  bool live_sao = false, live_valid = false;
  void* xprev = nullptr;       /* exchange buffer handed to the previous phase */
  int lane = 0;                /* the lane phase 0 ran on: the picture's working planes and scratch live there */
  void* xb[4] = {nullptr, nullptr, nullptr, nullptr};   /* m355_decode_sharded: the picture's exchange buffers X0..X3 + peer scratch (library-owned) */
  size_t xb_bytes[4] = {0, 0, 0, 0};
  void* xscratch = nullptr;
  /* m355_group_decode: x3_read[q] = rank q has copied this handle's gather buffer xb[3] (recorded by q on its own stream, created on q's
     device); the NEXT decode of this handle waits for them before it repacks the buffer — per buffer, not per rank: handles need not
     rotate in step with the lane streams */
  std::vector<hipEvent_t> x3_read;
  unsigned long long xb_epoch = 0;   /* which allocation xb[] is (counted per process: the interprocess transport exports a new one again) */
  std::vector<int> peers;      /* ranks this rank exchanges halos with */
  EvRef up;                    /* lists copied to the device (decodes on another lane continue behind it) */
  EvRef done;                  /* last decode of these lists: behind it the arenas may be overwritten ... */
  EvRef maps;                  /* ... and behind the last side-map request that reads them (m355_picture_maps_async, on a stream of its own): maps_lists_idle */
  bool fresh = false;          /* uploaded and not decoded since: nothing in flight reads its reference table */
  bool arena = false;          /* m355_arena_begin handed out list pointers into `host`: the next upload of lists that sit there copies nothing */
  m355_arena_caps caps;        /* ... with room for this many entries */
  int arena_halo_units = 0;    /* ... and, on a tile-sharded context, for this many foreign border units behind cus[] / pbs[] */
  bool reserved = false;       /* m355_picture_arena_begin made this handle; no lists yet (m355_picture_replace brings them) */
  bool device_validate = false;    /* the record checks of these lists run on the device (k_validate) */
  size_t xscratch_pitch = 0;       /* m355_decode_sharded / m355_group_decode: bytes between the peers' slots of xscratch */
  std::vector<uint8_t> sched_u8;   /* upload(): per-CTB scratch of the intra schedule */
  std::vector<uint32_t> sched_u32;
  std::vector<uint32_t> sched_order, sched_cand, sched_bucket, sched_u32b;   /* ... and of the work list (order, counting-sort buckets, plan bases) */
};

/* Everything ONE picture in flight writes: streams, working planes, metadata / job / residual scratch.  The context holds
 * M355_MAX_LANES of them and addresses the active one as lane(c) (m355_set_pipeline_depth(ctx, n) decodes consecutive pictures
 * round-robin on n lanes: the dependency-bound tail of one picture's intra stage and its filters overlap the next picture's
 * prediction; frame hazards are ordered with per-frame events). */
struct Lane {
  hipStream_t stream = nullptr, stream2 = nullptr;   /* stream2: metadata planes are rasterised on it while k_inter / k_residual run */
  hipEvent_t ev_fork = nullptr, ev_fork2 = nullptr, ev_join = nullptr;
  /* intra pictures on lanes 3.. run on a stream of the lane's priority class (own hardware queues, lane_class below); the lane's
     scratch is shared by both streams: a decode waits for the lane's previous one when that ran on the other stream */
  hipStream_t stream_hi = nullptr, last_stream = nullptr;
  EvRef last;                  /* behind the lane's last decode */
  Frame work;                  /* pre-SAO working planes */
  uint32_t *pb_of = nullptr, *ticket = nullptr, *timeout = nullptr;
  unsigned long long* edge = nullptr;   /* k_intra halo granules */
  uint8_t *edge_tu = nullptr, *cuf = nullptr;   /* edge_tu also holds edge_pb and cb_cu (one allocation) */
  int16_t* resbuf = nullptr;
  uint32_t* jobs = nullptr;
  uint16_t* sao_nb = nullptr;
  uint16_t* iplan = nullptr;   /* border plans of the picture's intra blocks */
  uint32_t* job_base = nullptr; /* per 256-PB chunk its jobs per range (MAIN, EDGE), behind them the two range ends = DevPic::job_tot (k_job_count / k_meta_pb) */
  size_t cap_cb = 0, cap_u4 = 0, cap_edge = 0, cap_cuf = 0, cap_res = 0, cap_jobs = 0, cap_sao = 0, cap_iplan = 0, cap_jobbase = 0;
};

struct m355_ctx {
  int device = 0;
  Lane lanes[M355_MAX_LANES];
  int depth = 1, active = 0;   /* pipeline depth, index of the active lane */
  std::vector<std::pair<uint32_t, uint32_t*>> inter_tabs;   /* k_inter_jobs' tap tables per (plane type, bit depths): m355_inter_tables */
  /* the ring of marks (EvRef): a slot is taken over M355_EV_RING marks later, behind a host wait for its old mark — so "the slot
     carries another ticket" means "that mark has passed" */
  struct EvSlot { hipEvent_t ev = nullptr; unsigned long long ticket = 0; };
  EvSlot evring[M355_EV_RING];
  unsigned long long ev_ticket = 0;
  std::vector<Frame> frames;
  std::vector<Resident> resident;
  /* m355_submit_picture: rotating staging arenas, so the host prepares picture k+1 while k decodes; a slot is free again when the
     decode of the lists it held has finished.  THREE slots: a longer ring was measured and buys nothing — the submitting thread's own work per picture (list checks, schedules,
     ~20 launches: 0.45 ms at 8K) is what bounds a submit-every-picture decoder, and with more slots it runs further ahead of the
     three lanes, which costs more than it hides (C5 submit_only 0.74-0.79 ms with 3 slots, 0.80-0.94 with 4, 0.81-0.92 with 6:
     profiles/r04_ai_submit_ring.txt). */
  Resident transient[M355_TRANSIENT_MAX];
  int next_transient = 0;
  int last_transient = -1;     /* the arena that holds the lists of the most recent m355_submit_picture (M355_PICTURE_LAST); -1: none, or that submit's upload failed */
  int transient_ring() const { return 3; }
  uint32_t epoch = 0;
  /* per-decode status (m355_decode_status): the last M355_STATUS_RING decodes; a device-validated decode copies its lane's gate
     words into `words` (pinned) behind its last kernel */
  struct Status { unsigned long long serial = 0; uint32_t epoch = 0; bool validated = false, reported = false; EvRef done; };
  Status status[M355_STATUS_RING];
  uint32_t* status_words = nullptr;   /* pinned: 4 words per ring slot = the lane's timeout[0..3] at the end of the decode */
  unsigned long long serial = 0;
  /* rejected decodes that left the status ring unreported (more than M355_STATUS_RING submits between two waits): latched when
     their slot is reused, reported by the next m355_wait */
  unsigned long long lost_first = 0; int lost_count = 0;
  int stages = M355_STAGE_ALL;
  int dbg_intra[4] = {0, 0, 0, 0};   /* the last prepared decode's intra work items, those of dependency chains (ticket), those run by a workgroup, light items: m355_debug_intra_counts */
  int shard_rank = 0, shard_n = 0;   /* shard_n == 0: sharding off */
  m355_comm comm = {nullptr, nullptr, nullptr};   /* exchanges of m355_decode_sharded */
  void* rccl = nullptr;              /* built-in RCCL communicator (m355_shard_rccl_init) */
  void* ipc = nullptr;               /* interprocess transport (m355_shard_ipc_init, runtime_ipc.hip) */
  int xchg_h = -1, xchg_k = -1;      /* m355_decode_sharded: the picture handle / exchange the callbacks are being called for */
  std::vector<hipEvent_t> evs;  /* 7 events per timed decode (ring grows on demand) */
  int ev_used = 0;             /* decodes recorded since the last m355_timing_reset */
  bool timing_on = false;      /* between m355_timing_reset and m355_timing_collect: decodes record their seven stage events */
  uint32_t* hash_acc = nullptr; /* m355_frame_hash accumulators */
  /* m355_frame_hash_async: M355_HASH_REQUESTS slots, each with a device record (zero between requests: the kernel leaves it so) and a pinned
     result record, allocated when the context is created, and the mark behind its request.  ticket == 0: the slot is free. */
  struct HashSlot {
    unsigned long long ticket = 0; int type = 0, np = 0;
    int row_bytes[3] = {0, 0, 0}, rows[3] = {0, 0, 0};
    EvRef mark; int frame = -1;                         /* the request's mark and the frame it reads (collecting it clears that frame's mark, if still this one) */
    uint8_t* planes = nullptr; size_t planes_cap = 0;   /* MD5: pinned copy of the planes, taken from hash_pool */
  };
  HashSlot hash_slot[M355_HASH_REQUESTS];
  unsigned long long hash_ticket = 0;
  uint32_t *hash_rec = nullptr, *hash_res = nullptr;    /* HASH_REC_WORDS (device) / HASH_RES_WORDS (pinned) per slot */
  std::vector<std::pair<uint8_t*, size_t>> hash_pool;   /* idle pinned plane buffers of MD5 requests: they grow to the largest frame seen */
  /* m355_frame_measure_async: M355_MEASURE_REQUESTS slots like the hash slots — a device record the kernel leaves zero, a pinned result record — and a
     pinned row array (the rows' sums of squared differences, which the host adds in row order at collection) taken from meas_pool, sized at the request.
     frame[1] / the second mark's frame: the reference frame of a frame-against-frame request, -1 otherwise. */
  struct MeasSlot {
    unsigned long long ticket = 0;
    int np = 0, pw[3] = {0, 0, 0}, ph[3] = {0, 0, 0}, row0[3] = {0, 0, 0};
    EvRef mark; int frame[2] = {-1, -1};
    unsigned long long* rows = nullptr; size_t rows_cap = 0;
  };
  MeasSlot meas_slot[M355_MEASURE_REQUESTS];
  unsigned long long meas_ticket = 0;
  unsigned long long *meas_rec = nullptr, *meas_res = nullptr;   /* MEAS_REC_WORDS (device) / MEAS_RES_WORDS (pinned) per slot */
  std::vector<std::pair<unsigned long long*, size_t>> meas_pool; /* idle pinned row arrays (entries) */
  /* m355_frame_stats_async (runtime_stats.hip): M355_STATS_REQUESTS slots of their own like the comparison slots — a device record the kernel leaves zero and a
     pinned result record of STATS_REC_WORDS 32-bit words each (k_stats.h), the request's mark and the frame it reads */
  struct StatsSlot {
    unsigned long long ticket = 0;
    int np = 0, light = 0;
    EvRef mark; int frame = -1;
  };
  StatsSlot stats_slot[M355_STATS_REQUESTS];
  unsigned long long stats_ticket = 0;
  uint32_t *stats_rec = nullptr, *stats_res = nullptr;
  /* m355_frame_ssim_async (runtime_ssim.hip): M355_SSIM_REQUESTS slots of their own — a device record the kernel leaves zero and a pinned result record of
     SSIM_REC_WORDS 64-bit words each (k_ssim.h), the request's mark, the frames it reads (frame[1]: the reference frame, -1 with memory), and per plane the
     number of windows (0: not measured) */
  struct SsimSlot {
    unsigned long long ticket = 0;
    uint64_t n[3] = {0, 0, 0};
    EvRef mark; int frame[2] = {-1, -1};
  };
  SsimSlot ssim_slot[M355_SSIM_REQUESTS];
  unsigned long long ssim_ticket = 0;
  unsigned long long *ssim_rec = nullptr, *ssim_res = nullptr;
  /* m355_frame_msssim_async (runtime_msssim.hip): M355_MSSSIM_REQUESTS slots of their own, as the SSIM slots — records of MSSSIM_REC_WORDS 64-bit words
     (k_msssim.h), the mark, the frames, the level count and per plane and level the number of windows (0: not measured) — and per slot the SCRATCH that
     holds levels 1 .. L - 1 of both sides between the request's two launches: allocated when a request needs more than the slot has, kept, freed with the context */
  struct MsssimSlot {
    unsigned long long ticket = 0;
    uint64_t n[3][M355_MSSSIM_LEVELS] = {};
    int levels = 0;
    EvRef mark; int frame[2] = {-1, -1};
  };
  MsssimSlot msssim_slot[M355_MSSSIM_REQUESTS];
  uint8_t* msssim_scratch[M355_MSSSIM_REQUESTS] = {};
  size_t msssim_scratch_cap[M355_MSSSIM_REQUESTS] = {};
  unsigned long long msssim_ticket = 0;
  unsigned long long *msssim_rec = nullptr, *msssim_res = nullptr;
  /* m355_picture_maps_async (runtime_maps.hip): M355_MAPS_REQUESTS slots of their own — a device record the kernels leave zero and a pinned result record of
     MAPS_REC_WORDS 32-bit words each (k_maps.h), the request's mark, the unit grid and the maps it wrote (bit m: map m).  The requests run in order on
     maps_stream (made with the first request) and share maps_scratch, the planes on the picture's 4x4 grid, grown on demand. */
  struct MapsSlot {
    unsigned long long ticket = 0;
    EvRef mark; int units_w = 0, units_h = 0; uint32_t want = 0;
  };
  MapsSlot maps_slot[M355_MAPS_REQUESTS];
  unsigned long long maps_ticket = 0;
  uint32_t *maps_rec = nullptr, *maps_res = nullptr;
  hipStream_t maps_stream = nullptr;
  uint8_t* maps_scratch = nullptr; size_t maps_scratch_cap = 0;
  /* pinned staging buffer of the blocking frame transfers (m355_frame_upload / _download / _fill, MD5 of m355_frame_hash): the copy itself is queued on the
     stream that last wrote the frame, between pinned memory and the frame (frame_stage_* in runtime.hip) */
  void* stage = nullptr; size_t stage_bytes = 0;
  /* m355_colour_create: the colour transform objects of the composed exports — the tables in device memory, the matrix for the kernel arguments.
     handle == 0: the slot is free; handles count up over all contexts of the process and are never given twice.  A tone object
     (m355_colour_create_tone) has its gain table behind the tables in the same allocation (gain != null), and norm and weights for the arguments */
  struct ColourObj { int handle = 0; uint8_t* dev = nullptr; int32_t matrix[9] = {}; uint32_t* gain = nullptr; int32_t norm = 0, weights[3] = {}; };
  ColourObj colour[M355_COLOUR_OBJECTS];
  /* m355_decode_batch: ring of picture-record arrays (pinned staging + device copy + the batch's ticket word); a slot's event is
     recorded behind the batch's k_intra — what the pictures' filter stages wait for, and what guards the slot's reuse */
  struct BatchSlot { DevPic* host = nullptr; DevPic* dev = nullptr; uint32_t* ticket = nullptr; hipEvent_t ev = nullptr; bool pending = false; };
  BatchSlot batch[M355_BATCH_RING];
  int batch_next = 0;
  hipStream_t batch_stream[4] = {nullptr, nullptr, nullptr, nullptr};   /* consecutive batches' k_intra launches alternate between two streams of priority
                                                         classes of their own (own hardware queues): the tail of one batch's wavefronts
                                                         overlaps the head of the next batch's when they run on different lanes */
  unsigned batch_count = 0;
  hipEvent_t batch_ev_pre[M355_MAX_LANES] = {};   /* the front part of picture k of the current batch is enqueued */
  /* CtbAddrRStoTS / TStoRS / TileIdRS of the last tile structure seen (pps.cc:589-606), upload() */
  struct ScanCache { int ctbW = 0, ctbH = 0, ntc = 0, ntr = 0; decltype(m355_pic_params::col_bd) col_bd; decltype(m355_pic_params::row_bd) row_bd;
                     std::vector<uint32_t> ctb_ts, ts2rs; std::vector<uint16_t> tile_id; } scan;
};
static inline Lane& lane(m355_ctx* c) { return c->lanes[c->active]; }   /* the lane the next decode / phase / transfer addresses */
static inline void select_lane(m355_ctx* c, int index) { c->active = index; }

/* ---- shared between the parts ---- */
struct TileRect { int x0, y0, x1, y1; };   /* luma samples */
struct Seg { const void* src; size_t bytes; size_t ofs; };
struct Lay {
  Seg seg[32];
  int ns;
  size_t total;
  int i_sl, i_ct, i_cu, i_tu, i_pb, i_wt, i_rb[4], i_ibin, i_ib, i_il, i_co, i_pc, i_sc, i_ts, i_rs, i_ti, i_iw, i_dp, i_ow, i_lt;
};
struct Id128 { char b[128]; };
struct Rccl {
  void* so = nullptr;
  void* comm = nullptr;
  int (*GetUniqueId)(void*) = nullptr;
  int (*CommInitRank)(void**, int, /* ncclUniqueId by value: 128 bytes */ Id128, int) = nullptr;
  int (*CommDestroy)(void*) = nullptr;
  int (*GroupStart)() = nullptr;
  int (*GroupEnd)() = nullptr;
  int (*Send)(const void*, size_t, int, int, void*, void*) = nullptr;
  int (*Recv)(void*, size_t, int, int, void*, void*) = nullptr;
  int (*AllGather)(const void*, void*, size_t, int, void*, void*) = nullptr;
};
extern Rccl g_rccl;            /* runtime_shard.hip */
int ipc_before_repack(m355_ctx* c, int h, hipStream_t st);      /* runtime_ipc.hip: hooks of m355_decode_sharded */
int ipc_end_picture(m355_ctx* c, int rc_own);
int ipc_before_free(m355_ctx* c, int h);
extern "C" int m355_shard_ipc_close(m355_ctx* c);
template <class T> static int grow(T** p, size_t* cap, size_t need, hipStream_t st, bool zero)
{
  if (need <= *cap) return M355_OK;
  HIPCHK(hipStreamSynchronize(st));
  if (*p) hipFree(*p);
  *p = nullptr;
  const size_t n = need + need / 4 + 64;
  HIPCHK(hipMalloc(p, n * sizeof(T)));
  if (zero) HIPCHK(hipMemsetAsync(*p, 0, n * sizeof(T), st));
  *cap = n;
  return M355_OK;
}

extern "C" {
void clear_target(m355_ctx* c, const DevPic& d, Frame* tgt, bool gated, hipStream_t st);
int copy_tiles(m355_ctx* c, const m355_pic_params& pp, Frame* f, int k0, int k1, int skip, int nranks, char* xbuf, size_t slot, bool to_slot);
int decode(m355_ctx* c, Resident& r, bool rotate = true);
void dst_hazards(m355_ctx* c, Frame* dstf, bool piped, hipStream_t st);
int ev_mark(m355_ctx* c, hipStream_t st, EvRef* out);
hipError_t ev_query(m355_ctx* c, const EvRef& r);
hipError_t ev_sync(m355_ctx* c, const EvRef& r);
void ev_wait(m355_ctx* c, hipStream_t st, const EvRef& r);
Frame* get_frame(m355_ctx* c, int h);
hipStream_t reader_begin(m355_ctx* c, Frame* f, int kind, const uint32_t** gate = nullptr, uint32_t* epoch = nullptr);
int reader_end(m355_ctx* c, Frame* f, int kind, hipStream_t st);
void readers_wait(m355_ctx* c, hipStream_t st, const Frame* f);
int stats_requests_create(m355_ctx* c);            /* runtime_stats.hip: the slots of m355_frame_stats_async, made and dropped with the context */
void stats_requests_destroy(m355_ctx* c);
void halo_layout(const m355_pic_params& pp, HaloLayout& h);
int lane_class_priority(int index);
int lane_priorities_mode();
hipStream_t launch_prediction(m355_ctx* c, const Resident& r, const DevPic& d, bool hbd, hipStream_t st, hipEvent_t* ev, bool with_intra = true, hipStream_t chain = nullptr, Frame* hazard_dst = nullptr);
void make_layout(const m355_arena_caps& k, int nCtb, int halo_units, bool sharded, bool with_ib_input, Lay& L);
int mark_done(m355_ctx* c, Resident& r, Frame* dstf, hipStream_t st, const DevPic* d = nullptr);
int prepare(m355_ctx* c, Resident& r, DevPic& d_out, bool& want_sao_out, hipStream_t st);
size_t slot_bytes(const m355_pic_params& pp, int nranks);
int stage_reserve(m355_ctx* c, size_t bytes);   /* runtime.hip: the context's pinned staging buffer holds at least `bytes` */
int status_of(m355_ctx* c, m355_ctx::Status& s);
hipError_t sync_all(m355_ctx* c);
int upload(m355_ctx* c, Resident& r, const m355_picture* pic);
int ssim_requests_create(m355_ctx* c);             /* runtime_ssim.hip: the slots of m355_frame_ssim_async, made and dropped with the context */
void ssim_requests_destroy(m355_ctx* c);
int msssim_requests_create(m355_ctx* c);           /* runtime_msssim.hip: the slots of m355_frame_msssim_async and their scratch, made and dropped with the context */
void msssim_requests_destroy(m355_ctx* c);
int maps_requests_create(m355_ctx* c);             /* runtime_maps.hip: the slots of m355_picture_maps_async, made and dropped with the context */
void maps_requests_destroy(m355_ctx* c);
int maps_lists_idle(m355_ctx* c, Resident& r);     /* the host waits for the side-map requests that read the lists of `r` (Resident::maps) */
}

/* What the requests that compare a frame with another picture share (m355_frame_measure_async, m355_frame_ssim_async, m355_frame_msssim_async): the frame, the rectangle
   (width == 0: the whole frame) and the other picture — ref_frame >= 0, or ref[] / pitch[] — checked, and per plane of the frame both sides'
   first sample of the rectangle.  `who` opens the error texts.  -> M355_OK, or M355_ERR_INVALID with nothing touched. */
struct PairPlane {
  const uint8_t *a, *b;         /* the frame's / the reference's samples at the rectangle's first sample */
  long long pitch_a, pitch_b;   /* bytes between rows */
  int pw, ph, px, py;           /* the rectangle on this plane: size, first sample in plane coordinates of the frame */
};
struct PairGeom {
  Frame *f, *r;                 /* r: the reference frame, null with ref[] */
  int np;                       /* planes of the frame */
  PairPlane pl[3];
};
static int pair_geometry(m355_ctx* c, const char* who, int h, bool have_args, int ref_frame, int x0, int y0, int w, int hgt, const void* const* ref, const int64_t* pitch, PairGeom* g)
{
  Frame* f = c ? get_frame(c, h) : nullptr;
  if (!f || !have_args) return fail(M355_ERR_INVALID, "%s: bad frame handle %d / null descriptor / null ticket", who, h);
  if (c->shard_n > 0) return fail(M355_ERR_INVALID, "%s: not on a tile-sharded context (its frames are complete only behind the gather)", who);
  const int sw = (f->cf == 1 || f->cf == 2) ? 2 : 1, sh = f->cf == 1 ? 2 : 1;
  if (w != 0) {
    if (x0 < 0 || y0 < 0 || w <= 0 || hgt <= 0 || x0 > f->w - w || y0 > f->h - hgt) return fail(M355_ERR_INVALID, "%s: rectangle %d,%d %dx%d leaves the %dx%d frame", who, x0, y0, w, hgt, f->w, f->h);
    if (f->cf && ((x0 | w) % sw || (y0 | hgt) % sh)) return fail(M355_ERR_INVALID, "%s: rectangle %d,%d %dx%d is not aligned to the chroma grid (%dx%d luma samples)", who, x0, y0, w, hgt, sw, sh);
  } else { x0 = y0 = 0; w = f->w; hgt = f->h; }
  Frame* r = nullptr;
  if (ref_frame != -1) {
    r = get_frame(c, ref_frame);
    if (!r) return fail(M355_ERR_INVALID, "%s: bad reference frame handle %d", who, ref_frame);
    if (r->cf != f->cf || r->bdl != f->bdl || r->bdc != f->bdc || r->bpp[0] != f->bpp[0]) return fail(M355_ERR_INVALID, "%s: the reference frame's chroma format / bit depths differ from the frame's", who);
    if (x0 > r->w - w || y0 > r->h - hgt) return fail(M355_ERR_INVALID, "%s: the %dx%d reference frame does not contain the rectangle %d,%d %dx%d", who, r->w, r->h, x0, y0, w, hgt);
  }
  g->f = f; g->r = r; g->np = f->cf == 0 ? 1 : 3;
  for (int p = 0; p < g->np; p++) {
    const int sb = f->bpp[p];
    PairPlane& m = g->pl[p];
    m.pw = p ? w / sw : w; m.ph = p ? hgt / sh : hgt; m.px = p ? x0 / sw : x0; m.py = p ? y0 / sh : y0;
    m.pitch_a = (long long)f->stride[p] * sb;
    m.a = (const uint8_t*)f->plane[p] + (size_t)m.py * m.pitch_a + (size_t)m.px * sb;
    if (r) {
      m.pitch_b = (long long)r->stride[p] * sb;
      m.b = (const uint8_t*)r->plane[p] + (size_t)m.py * m.pitch_b + (size_t)m.px * sb;
    } else {
      if (!ref[p]) return fail(M355_ERR_INVALID, "%s: no reference for plane %d", who, p);
      if (pitch[p] < (int64_t)m.pw * sb) return fail(M355_ERR_INVALID, "%s: pitch %lld of plane %d is below its row of %lld bytes", who, (long long)pitch[p], p, (long long)m.pw * sb);
      if (((uintptr_t)ref[p] | (uintptr_t)pitch[p]) & (uintptr_t)(sb - 1)) return fail(M355_ERR_INVALID, "%s: pointer / pitch of plane %d is no multiple of the %d-byte element", who, p, sb);
      m.pitch_b = pitch[p];
      m.b = (const uint8_t*)ref[p];
    }
  }
  return M355_OK;
}

#endif
