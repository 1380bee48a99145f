// pipeline.hip -- the host-buffer IVFADC calls (what the PostgreSQL hosts make: freddy_gpu_ivfadc_search, and by row id
// freddy_gpu_ivfadc_search_ids) as a pipeline of sub-batches over the chunk driver of ivfadc.hip.
#include "internal.h"

#include <functional>

#include "io_kernels.h"
#include "ivf_run.h"
#include "query_ids.h"
#include "stage_plan.h"

// ---------------------------------------------------------------------------------------
// The host-buffer call (what the PostgreSQL hosts make: one synchronous call per batch, freddy.c:679-999) as a
// pipeline.  The batch is cut into sub-batches of <= pipeline_batch queries; sub-batch j goes to lane j mod L
// (L <= 4 library-owned streams, each with its own workspace, pinned staging and device buffers):
//   host memcpy of its queries into the lane's pinned buffer (skipped when the caller's buffer is pinned itself:
//   freddy_gpu_host_alloc) -> asynchronous H2D -> round one of the search with an explicit scan share of L -> asynchronous
//   D2H of the lists and of the round's straggler count into pinned memory -> event.
// The host only waits when it needs a lane again (or at the end), and that is where a sub-batch's rare extra probing
// rounds run and its lists are copied out: the transfers and the latency-bound ends of one sub-batch hide under the
// scans of its neighbours, and ONE stream synchronisation per lane ends the call.
// ---------------------------------------------------------------------------------------
// stage_bytes: what the sub-batch stages in pinned memory (its queries, or their row numbers: query_ids.h); in_bytes: its query block
static int lane_open(freddy_gpu_index* ix, Lane& l, LaneSlot& c, size_t stage_bytes, size_t in_bytes, size_t n, size_t n_out) {
  // lane 0 is the handle's own stream: a call of one sub-batch (<= pipeline_batch queries: what a PostgreSQL backend makes) uses
  // ONE stream per process, and only larger calls create further streams -- every stream a process creates takes a hardware
  // queue, and the queues of several backends on one GPU are what decides their aggregate rate (profiles/r06_backends.txt)
  if (!l.stream && &l == &ix->lanes[0] && !ix->tune.lane0_own) l.stream = ix->stream;
  if (!l.stream) HIP_TRY(hipStreamCreateWithFlags(&l.stream, hipStreamNonBlocking));
  if (!c.done) HIP_TRY(hipEventCreateWithFlags(&c.done, hipEventDisableTiming));
  const size_t out_bytes = (n_out * 2 + 1 + n + 1) * 4;   // (+ the completion word)
  if (c.h_in.ensure(stage_bytes) || c.h_out.ensure(out_bytes)) return fail(FREDDY_E_NOMEM, "pinned staging allocation failed");
  if (c.d_q.ensure(in_bytes + 16) || c.d_ids.ensure(n_out * 4) || c.d_dist.ensure(n_out * 4))
    return fail(FREDDY_E_NOMEM, "workspace allocation failed");
  return 0;
}

// The old shape of the call, kept for what the pipeline hands back: a (small) batch searched to the end on the library's
// own stream -- round one, then the extra rounds of the reference's "while (foundInstances < k)" loop with a host sync each.
// A device-resident source (query_ids.h) brings its row numbers in MAPPED host memory (qs.rows): the block is gathered, not copied.
static int ivfadc_sync_search(freddy_gpu_index* ix, const QuerySrc& qs, int Q, int k, int W, float sentinel, int found_rule,
                              int32_t* out_ids, float* out_dist) {
  Workspace* ws = workspace_for(ix, ix->stream);
  hipStream_t s = ix->stream;
  if (ws->w_q.ensure(sizeof(float) * (size_t)Q * ix->d) || ws->w_out_ids.ensure(sizeof(int32_t) * (size_t)Q * k) ||
      ws->w_out_dist.ensure(sizeof(float) * (size_t)Q * k))
    return fail(FREDDY_E_NOMEM, "workspace allocation failed");
  if (qs.host) HIP_TRY(hipMemcpyAsync(ws->w_q.p, qs.host, sizeof(float) * (size_t)Q * ix->d, hipMemcpyHostToDevice, s));
  else if (int rc = launch_query_gather(ix, s, qs, qs.rows, ws->w_q.as<float>(), Q, ix->d)) return rc;
  if (int rc = for_chunks(Q, max_queries_per_chunk(ix, W, k), [&](int q0, int n) {
        IvfRun r;
        if (int rc = ivfadc_begin(ix, s, scan_share_now(ix->tune.scan_share, true, ix->device), ws->w_q.as<float>() + (size_t)q0 * ix->d, n, k, W, sentinel, found_rule,
                                  ws->w_out_ids.as<int32_t>() + (size_t)q0 * k, ws->w_out_dist.as<float>() + (size_t)q0 * k, nullptr, r))
          return rc;
        return ivfadc_finish(r, -1);
      }))
    return rc;
  HIP_TRY(hipMemcpyAsync(out_ids, ws->w_out_ids.p, sizeof(int32_t) * (size_t)Q * k, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(out_dist, ws->w_out_dist.p, sizeof(float) * (size_t)Q * k, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return 0;
}

struct PipeCall {   // the arguments of one host-buffer call, for the lanes' retire step
  freddy_gpu_index* ix;
  QuerySrc src;
  int k, W, found_rule;
  float sentinel;
  int32_t* out_ids;
  float* out_dist;
};

// Wait for a slot's sub-batch and hand its lists to the caller.  Queries that round one left unfinished (their first W
// cells hold fewer than k rows -- rare) are searched again from the start, synchronously, with all their rounds: the
// search is deterministic, so that is the list the round-by-round continuation would have produced, and no lane has to
// keep per-round state while its stream already runs the next sub-batch.
// (a device-resident source: the stragglers' row numbers go into the slot's staging block, free by now, and the re-search gathers them)
static int lane_retire(LaneSlot& c, const PipeCall& pc) {
  if (!c.busy) return 0;
  c.busy = false;
  const int k = pc.k;
  const size_t n_out = (size_t)c.n * k;
  const int32_t* ho = c.h_out.as<const int32_t>();
  // the copy-out kernel's last store is a completion word behind the lists: polled for up to a millisecond, then the event is
  // waited for the usual way -- which is also where a fault in one of the lane's kernels surfaces, before its output is trusted
  if (wait_word(ho + 2 * n_out + 1 + (size_t)c.n, 1000) == 0) {
    HIP_TRY(hipEventSynchronize(c.done));
    HIP_TRY(hipGetLastError());
  }
  memcpy(pc.out_ids + (size_t)c.q0 * k, ho, n_out * 4);
  memcpy(pc.out_dist + (size_t)c.q0 * k, ho + n_out, n_out * 4);
  const int n_next = std::min(ho[2 * n_out], c.n);
  if (n_next <= 0) return 0;
  const int d = pc.ix->d;
  std::vector<int32_t> who(ho + 2 * n_out + 1, ho + 2 * n_out + 1 + n_next);
  // (device-written numbers index the caller's buffers: a value outside the sub-batch -- e.g. after a kernel fault whose
  // error has not surfaced yet -- must never become a host read or write out of bounds)
  for (int i = 0; i < n_next; ++i)
    if (who[(size_t)i] < 0 || who[(size_t)i] >= c.n) return fail(FREDDY_E_HIP, "sub-batch returned a straggler index %d outside [0, %d)", who[(size_t)i], c.n);
  std::vector<float> q(pc.src.host ? (size_t)n_next * d : 0);
  std::vector<int32_t> ri((size_t)n_next * k);
  std::vector<float> rd((size_t)n_next * k);
  QuerySrc again = pc.src;
  if (pc.src.host) {
    for (int i = 0; i < n_next; ++i) memcpy(&q[(size_t)i * d], pc.src.host + ((size_t)c.q0 + who[(size_t)i]) * d, sizeof(float) * d);
    again.host = q.data();
  } else {
    if (c.h_in.ensure(sizeof(int32_t) * (size_t)n_next)) return fail(FREDDY_E_NOMEM, "pinned staging allocation failed");
    for (int i = 0; i < n_next; ++i) c.h_in.as<int32_t>()[i] = pc.src.rows[(size_t)c.q0 + who[(size_t)i]];
    again.rows = c.h_in.as<const int32_t>();
  }
  if (int rc = ivfadc_sync_search(pc.ix, again, n_next, k, pc.W, pc.sentinel, pc.found_rule, ri.data(), rd.data())) return rc;
  for (int i = 0; i < n_next; ++i) {
    memcpy(pc.out_ids + ((size_t)c.q0 + who[(size_t)i]) * k, &ri[(size_t)i * k], sizeof(int32_t) * k);
    memcpy(pc.out_dist + ((size_t)c.q0 + who[(size_t)i]) * k, &rd[(size_t)i * k], sizeof(float) * k);
  }
  return 0;
}

// ---- a host-buffer call, stage by stage: ivf_one_try, or pipe_plan and per sub-batch lane_retire (the slot's previous one) ->
// ---- sub_batch_source -> sub_batch_submit (stage_piece inside ivfadc_begin), then pipe_drain; pipe_abort after a failure ----------

// ONE query as one launch (one.hip; the caller has asked ivf_one_shape).  A device source's row is read back first: the kernel takes the
// query by value.  *answered: the lists are in the caller's buffers; else the call goes on as a pipeline of one sub-batch.
static int ivf_one_try(const PipeCall& pc, bool* answered) {
  freddy_gpu_index* ix = pc.ix;
  const float* const queries = pc.src.host;   // (NULL: the queries are rows of a device table, query_ids.h)
  int verdict = 0;
  float* const row_q = queries ? nullptr : (ix->hio_in.ensure(sizeof(float) * (size_t)ix->d) ? nullptr : ix->hio_in.as<float>());
  if (!queries && !row_q) return fail(FREDDY_E_NOMEM, "pinned staging allocation failed");
  if (!queries) if (int rc = fetch_query_row(ix->stream, pc.src, ix->d, row_q)) return rc;
  if (int rc = ivf_one(ix, queries ? queries : row_q, pc.k, pc.W, pc.sentinel, pc.found_rule, pc.out_ids, pc.out_dist, &verdict)) return rc;
  *answered = verdict == 2;
  return 0;
}

// What holds for the whole call: its cuts (stage_plan.h), the device view of the caller's buffer if that is pinned itself
// (freddy_gpu_host_alloc; NULL: pageable memory or a device source), the bytes of a query and the call's scan share.
struct PipePlan : PipeCuts {
  const float* pinned_in;
  size_t row;
  int share_call;
};
static PipePlan pipe_plan(const PipeCall& pc, int Q) {
  freddy_gpu_index* ix = pc.ix;
  PipePlan p;
  static_cast<PipeCuts&>(p) = pipe_cuts(Q, max_queries_per_chunk(ix, pc.W, pc.k), ix->tune.pipeline_batch, ix->tune.pipeline_lanes, FREDDY_LANES);
  p.pinned_in = pc.src.host ? static_cast<const float*>(pinned_device_pointer(pc.src.host)) : nullptr;
  p.row = sizeof(float) * (size_t)ix->d;
  p.share_call = scan_share_now(ix->tune.scan_share, true, ix->device);
  return p;
}

struct SubBatch {   // one sub-batch on its way in
  Lane* lane;
  LaneSlot* slot;
  int q0, n;
  bool in_place, stage;     // how its queries reach the device (stage_plan.h query_source)
  const float* src;         // host queries read without the lane's staging block: their device address in the caller's pinned buffer
  const float* d_queries;   // where the search reads the sub-batch
};

// The one place that decides how a sub-batch's queries reach the device; the lane's buffers are opened for it, and what is staged as
// a whole is staged here: the floats of a handful of host queries, the row numbers of a device source (4 bytes per query where the
// floats are staged).  Everything else crosses piece by piece (stage_piece).
static int sub_batch_source(const PipeCall& pc, const PipePlan& plan, SubBatch& b) {
  freddy_gpu_index* ix = pc.ix;
  const float* const queries = pc.src.host;
  LaneSlot& c = *b.slot;
  const int q0 = b.q0, n = b.n;
  if (int rc = lane_open(ix, *b.lane, c, queries ? plan.row * n : sizeof(int32_t) * (size_t)n, plan.row * n, (size_t)n, (size_t)n * pc.k)) return rc;
  c.q0 = q0; c.n = n;
  b.src = plan.pinned_in ? plan.pinned_in + (size_t)q0 * ix->d : nullptr;
  const QuerySource how = query_source(queries != nullptr, reinterpret_cast<uintptr_t>(b.src), plan.row, n);
  b.in_place = how.in_place; b.stage = how.stage;
  b.d_queries = c.d_q.as<float>();
  if (b.in_place && queries) {
    // a handful of queries: the kernels read them where they are staged (pinned, mapped) -- one launch less
    if (b.stage) { memcpy(c.h_in.p, queries + (size_t)q0 * ix->d, plan.row * n); b.src = c.h_in.as<const float>(); }
    b.d_queries = b.src;
  } else if (b.in_place) {
    b.d_queries = pc.src.row_ptr((size_t)q0, ix->d);
  } else if (!queries) {
    memcpy(c.h_in.p, pc.src.rows + q0, sizeof(int32_t) * (size_t)n);
  }
  return 0;
}

// The queries [q_lo, q_hi) of the sub-batch into its device block, on the lane's stream.
// Pageable queries cross in pieces: the copy kernel of a piece reads it over PCIe while the host stages the next one (1.2 MB per
// 1024 queries: 28 us of memcpy + 25 us of PCIe, back to back until round 4) -- and, since round 6, the piece's cell-selection /
// table launch runs behind its copy while the next piece is staged (ivfadc_begin calls this once per piece).
static int stage_piece(const PipeCall& pc, const SubBatch& b, int q_lo, int q_hi) {
  if (b.in_place) return 0;
  freddy_gpu_index* ix = pc.ix;
  LaneSlot& c = *b.slot;
  if (!pc.src.host)   // the piece's rows of the table -> the query block, by the row numbers staged above (one launch, as the copy)
    return launch_query_gather(ix, b.lane->stream, pc.src, c.h_in.as<const int32_t>() + q_lo, c.d_q.as<float>() + (size_t)q_lo * ix->d, q_hi - q_lo, ix->d);
  const PieceWords w = piece_words(sizeof(float) * (size_t)ix->d, q_lo, q_hi, b.n, b.stage);
  if (!w.aligned()) return fail(FREDDY_E_ARG, "internal: a staged piece must start at a 16-byte word");
  if (b.stage) memcpy(c.h_in.as<char>() + w.b_lo, reinterpret_cast<const char*>(pc.src.host + (size_t)b.q0 * ix->d) + w.b_lo, w.b_hi - w.b_lo);
  const void* from = b.stage ? c.h_in.p : static_cast<const void*>(b.src);
  for (int ci = 0; ci < w.cuts && w.cut_lo(ci) < w.cut_hi(ci); ++ci) launch_copy_in(b.lane->stream, from, c.d_q.p, w.cut_lo(ci), w.cut_hi(ci));
  if (hipGetLastError() != hipSuccess) return fail(FREDDY_E_HIP, "launch of the query copy failed");
  return 0;
}

// Round one of the sub-batch on its lane, its lists and straggler numbers out behind it, and the event the retire step waits for.
// (a call of ONE sub-batch launches its cell selection piece by piece behind the staged pieces: 0.398 -> 0.374 ms at 2048 queries;
// with several lanes the extra launches only get in the way of the other lanes' chains: 0.613 -> 0.666 ms at 4096)
// t_begun (lab builds' trace): the host time between the search's launches and the copy-out
static int sub_batch_submit(const PipeCall& pc, const PipePlan& plan, const SubBatch& b, double (*now_us)(), double* t_begun) {
  LaneSlot& c = *b.slot;
  const std::function<int(int, int)> stage = [&](int q_lo, int q_hi) { return stage_piece(pc, b, q_lo, q_hi); };
  IvfRun r;
  const int n_out = b.n * pc.k;
  int32_t* h_flag = c.h_out.as<int32_t>() + 2 * (size_t)n_out + 1 + (size_t)b.n;
  *h_flag = 0;
  if (int rc = ivfadc_begin(pc.ix, b.lane->stream, plan.n_lanes * plan.share_call, b.d_queries, b.n, pc.k, pc.W, pc.sentinel, pc.found_rule,
                            c.d_ids.as<int32_t>(), c.d_dist.as<float>(), nullptr, r, &stage, plan.n_sub == 1))
    return rc;
  if (now_us) *t_begun = now_us();
  hipLaunchKernelGGL(lane_copy_out_flag_kernel, dim3(1), dim3(1024), 0, b.lane->stream, c.d_ids.as<int32_t>(),
                     c.d_dist.as<float>(), r.ws->w_cnt.as<int32_t>(), r.next, c.h_out.as<int32_t>(), n_out, b.n, h_flag);
  if (hipGetLastError() != hipSuccess || hipEventRecord(c.done, b.lane->stream) != hipSuccess) return fail(FREDDY_E_HIP, "launch of the result copy failed");
  c.busy = true;
  return 0;
}

static double pipe_now_us() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// what is still in flight, in submission order (oldest first)
static int pipe_drain(const PipeCall& pc, const PipePlan& plan, double (*now_us)(), double t_start) {
  for (int j = std::max(0, plan.n_sub - 2 * plan.n_lanes); j < plan.n_sub; ++j) {
    const double t0 = now_us ? now_us() : 0.0;
    if (int rc = lane_retire(pc.ix->lanes[plan.lane(j)].slot[plan.slot(j)], pc)) return rc;
    if (now_us) fprintf(stderr, "[pipe] drain sub %d  t=%.0f us: %.0f\n", j, t0 - t_start, now_us() - t0);
  }
  return 0;
}

// a failed call: nothing of it may still be in flight when the caller gets its buffers back
static void pipe_abort(freddy_gpu_index* ix) {
  for (Lane& l : ix->lanes) {
    if (l.stream) (void)hipStreamSynchronize(l.stream);
    for (LaneSlot& c : l.slot) c.busy = false;
  }
}

// the batch [0, Q) of one device's handle
static int ivfadc_host_search(freddy_gpu_index* ix, const QuerySrc& qs, int Q, int k, int W, float sentinel, int found_rule,
                              int32_t* out_ids, float* out_dist) {
  HIP_TRY(hipSetDevice(ix->device));
  const PipeCall pc{ix, qs, k, W, found_rule, sentinel, out_ids, out_dist};
  if (ivf_one_shape(ix, Q, k, W, found_rule)) {
    bool answered = false;
    if (int rc = ivf_one_try(pc, &answered)) return rc;
    if (answered) return FREDDY_OK;
  }
  const BackendBusy busy;   // (the registry of backends on this GPU: core.hip)
  const PipePlan plan = pipe_plan(pc, Q);
#ifdef FREDDY_LAB
  static const bool trace = getenv("FREDDY_GPU_PIPE_TRACE") != nullptr;   // host timestamps of the pipeline's steps on stderr (lab builds)
  double (*const now_us)() = trace ? &pipe_now_us : nullptr;
#else
  double (*const now_us)() = nullptr;
#endif
  const double t_start = now_us ? now_us() : 0.0;
  int rc = 0;
  for (int j = 0; j < plan.n_sub && !rc; ++j) {
    SubBatch b{&ix->lanes[plan.lane(j)], &ix->lanes[plan.lane(j)].slot[plan.slot(j)], plan.q0(j), plan.n(j, Q)};
    double t0 = now_us ? now_us() : 0.0, t1 = 0, t2 = 0, t3 = 0;
    if ((rc = lane_retire(*b.slot, pc))) break;
    if (now_us) t1 = now_us();
    if ((rc = sub_batch_source(pc, plan, b))) break;
    if (now_us) t2 = now_us();
    if ((rc = sub_batch_submit(pc, plan, b, now_us, &t3))) break;
    if (now_us)
      fprintf(stderr, "[pipe] sub %d lane %d n=%d  t=%.0f us: retire %.0f, stage %.0f, launches %.0f, copy-out + event %.0f\n", j, plan.lane(j), b.n,
              t0 - t_start, t1 - t0, t2 - t1, t3 - t2, now_us() - t3);
  }
  if (!rc) rc = pipe_drain(pc, plan, now_us, t_start);
  if (rc) pipe_abort(ix);
  return rc;
}

// the host-buffer search of a handle without replicas, for either query source (query_ids.h); the arguments are checked
int ivfadc_search_src(freddy_gpu_index* ix, const QuerySrc& qs, int Q, int k, int W, float sentinel, int found_rule, int32_t* out_ids, float* out_dist) {
  if (Q == 0) return FREDDY_OK;
  return ivfadc_host_search(ix, qs, Q, k, W, sentinel, found_rule, out_ids, out_dist);
}

extern "C" int freddy_gpu_ivfadc_search_ids(freddy_gpu_index_t* ivf, freddy_gpu_index_t* vecs, const int32_t* query_ids, int32_t n_ids, int32_t id_rule,
                                            int32_t k, int32_t W, float sentinel, int32_t found_rule, int32_t* out_query_ids, int32_t* n_queries,
                                            int32_t* out_ids, float* out_dist) {
  if (int rc = check_query_ids_front(ivf, vecs, query_ids, n_ids, id_rule, out_query_ids, n_queries, out_ids, out_dist)) return rc;
  if (int rc = check_list_count(n_ids, k)) return rc;
  if (int rc = check_list_limit(k)) return rc;
  if (int rc = check_probe_args(W, found_rule)) return rc;
  if (int rc = check_ann_vecs(ivf, KIND_IVF, vecs, "a search by row id")) return rc;
  if (W > ivf->C) W = ivf->C;
  return search_selected_ids(vecs, query_ids, n_ids, id_rule, k, sentinel, out_query_ids, n_queries, out_ids, out_dist,
                             [&](const QuerySrc& qs, int n, int32_t* oi, float* od) { return ivfadc_search_src(ivf, qs, n, k, W, sentinel, found_rule, oi, od); });
}

// Q queries split contiguously over a handle and its replicas (freddy_gpu_pin_ivf_multi): part g of G gets
// [lo, hi) with sizes differing by at most one.  fn(part, index of that part, lo, hi) runs on its own host thread
// for every part but the first; the first failure's code and message are returned on the caller's thread.
extern "C" int freddy_gpu_ivfadc_search(freddy_gpu_index_t* ix, const float* queries, int32_t Q, int32_t k, int32_t W,
                                        float sentinel, int32_t found_rule, int32_t* out_ids, float* out_dist) {
  if (int rc = check_ivfadc_args(ix, queries, Q, k, &W, found_rule, out_ids, out_dist)) return rc;
  if (Q == 0) return FREDDY_OK;
  return over_replicas(ix, Q, [&](freddy_gpu_index* part, int lo, int hi) {
    return ivfadc_host_search(part, QuerySrc::of_host(queries + (size_t)lo * ix->d), hi - lo, k, W, sentinel, found_rule, out_ids + (size_t)lo * k,
                              out_dist + (size_t)lo * k);
  });
}
