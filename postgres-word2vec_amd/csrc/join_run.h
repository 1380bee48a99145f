// join_run.h -- the host side of a kNN-join call (ivpq_search_in.c:61-699): the run record (JoinRun) and the stages that
// fill it in; join_run() at the end of the file is the whole call, top to bottom.  The stages enqueue on ONE stream and the
// order of what they enqueue is part of the design: buffers are reused in stream order (JW_SCAN, JoinIndex::h_q) and the
// target buckets are on the host only after the call's first synchronisation -- the comments at those places say so.
#pragma once

#include "internal.h"
#include "bigk.h"
#include "join.h"
#include "query_ids.h"

namespace freddy {

// Where the queries of a call come from.  After front() the host never reads them again: everything later comes from
// JW_QUERIES / JW_SUB.
//   host      [Q][d] floats in the caller's memory (freddy_gpu_knn_join): staged, or read where they lie when they are pinned
//   rows      rows of a device table, row numbers in host memory (freddy_gpu_knn_join_ids): 4 bytes per query go into the pinned block
//             and sub_dist_rows_kernel gathers while it computes the sub-distances
//   in_block  the caller has filled JW_QUERIES on the join's stream (freddy_gpu_ivpq_analogy: aa_query_kernel writes the unit rows
//             there), sized through join_query_block() -- workspaces() finds the block large enough and leaves it where it is
struct JoinQueries {
  QuerySrc src;
  bool in_block = false;
  freddy_gpu_index* ix = nullptr;   // the handle whose profile records the front's launches (rows)
  static JoinQueries of_host(const float* q) { JoinQueries s; s.src = QuerySrc::of_host(q); return s; }
  static JoinQueries of_rows(freddy_gpu_index* ix, const float* table, int64_t n_table, const int32_t* rows) {
    JoinQueries s; s.src.table = table; s.src.n_table = n_table; s.src.rows = rows; s.ix = ix; return s;
  }
  static JoinQueries of_block() { JoinQueries s; s.in_block = true; return s; }
};
// The block an in_block caller fills: JW_QUERIES with room for Q queries.
static inline int join_query_block(JoinIndex* j, int Q, float** out) { return join_buf(j, JW_QUERIES, (size_t)Q * j->d, out); }

// The pinned landing zone of a call (JoinIndex::h_sum), described once as byte offsets and applied to the host's and to the
// device's address of the block.  The kernels read the lists and write summaries / results in it DIRECTLY (it is mapped into
// the device's address space): every hipMemcpyAsync between two kernels of a stream is an SDMA copy ordered against them by
// signals, ~12 us per hop, and a round had five of them.
struct JoinZone {
  int32_t* summary;   // [Q][TRAV_SUM_DW] traversal summaries, row x of the active list
  int32_t* out_ids;   // [Q][k]           result lists, row x of the scan list
  float* out_dist;    // [Q][k]
  int32_t* active;    // [Q]              the active list on its way to JW_ACTIVE
  int32_t* scan;      // [Q]              the scan list on its way to JW_SCAN
  float* fb_sub;      // [Q][2 * Kc]      sub-distances of the queries the device traversal hands back
};
struct JoinZoneLayout {
  size_t summary, out_ids, out_dist, active, scan, fb_sub, bytes;
  JoinZoneLayout(int Q, int k, int Kc) {
    size_t off = 0;
    auto words = [&off](size_t n) { const size_t o = off; off += 4 * n; return o; };
    summary = words((size_t)Q * TRAV_SUM_DW);
    out_ids = words((size_t)Q * k);
    out_dist = words((size_t)Q * k);
    active = words((size_t)Q);
    scan = words((size_t)Q);
    fb_sub = words((size_t)Q * 2 * Kc);
    bytes = off + 64;
  }
  JoinZone at(void* base) const {
    char* b = static_cast<char*>(base);
    return {reinterpret_cast<int32_t*>(b + summary), reinterpret_cast<int32_t*>(b + out_ids), reinterpret_cast<float*>(b + out_dist),
            reinterpret_cast<int32_t*>(b + active), reinterpret_cast<int32_t*>(b + scan), reinterpret_cast<float*>(b + fb_sub)};
  }
};

struct JoinRun {
  using Clock = std::chrono::steady_clock;
  // ---- the call
  JoinIndex* j;
  hipStream_t s;
  const float* queries;   // host floats, or NULL with
  JoinQueries qsrc;       // the source of the call
  int Q, k;
  const int32_t* target_ids;
  int64_t n_targets;
  int alpha, alpha_original, pvf, method, use_tl;
  float confidence;
  int32_t* out_ids;
  float* out_dist;
  int32_t* iterations_out;
  // ---- its shape
  int L, V;                // candidates the replay / post verification walks, selection width of join_query_kernel
  bool big, double_codes;  // join_query_kernel<16, true>; pair codes
  bool replay;             // methods 0 / 1 of a big call: bigk_replay_kernel writes the lists behind the join kernel
  size_t lds;
  int SV, TV;              // widths of side_sort_kernel (Kc codes) and join_traverse_kernel (cells)
  bool dev_trav;           // the multi-index traversal runs on the device
  // ---- device workspaces (JoinSlot)
  float *d_q, *d_sub;
  int32_t *d_tcell, *d_trow, *d_scan, *d_qoff, *d_win, *d_cnt;
  u64* d_sorted;
  int32_t *d_active = nullptr, *d_qcells = nullptr, *d_qcnt = nullptr;   // device traversal only
  // ---- pinned host memory
  const int32_t* tcell_off;   // [cells + 1] target buckets by cell; complete on the host after the first synchronisation
  int32_t* h_tids;            // the target array as the mark kernel reads it
  bool tl_hit;                // the previous call's buckets serve this target array
  JoinZone h, p;              // the landing zone as the host and as the device see it
  // ---- per query, over the rounds
  std::vector<int32_t> active, target_count;
  std::vector<int32_t> q_n, q_rows;             // this round: cells taken, target rows in them
  std::vector<uint8_t> q_host, q_exh;           // this round: traversed on the host / exhausted every cell
  std::vector<std::vector<int32_t>> qcells;     // host-traversed queries only
  // Round r + 1's traversal (alpha doubled) is launched right behind round r's join kernel, for every query still active: its
  // summaries arrive with round r's lists in one synchronisation, and the queries that go on find theirs at spec_index[q].
  std::vector<int32_t> spec_index;
  bool spec_valid = false;
  // ---- the host heap's inputs: sub-distances and their stable per-side order (they do not depend on alpha)
  std::vector<float> sub;
  std::vector<JoinSide> sides;
  std::vector<int32_t> side_slot;   // query -> its rows in sub / sides (-1: not fetched)
  bool host_sides_all = false;
  // ---- this round
  int iterations = 0, n_active = 0, min_target = 0;
  double replay_ms = 0.0;                       // HIP-event time of the replay launches (inside join_kernel_time)
  bool last = false;
  std::vector<int32_t> fb;                      // queries the host heap has to traverse
  std::vector<int32_t> scan, scan_fb, qoff, flat;
  int n_dev = 0, n_fb = 0, n_scan = 0;          // scan = n_dev device-traversed queries, then n_fb host-traversed ones
  // ---- stage timers under the names of the reference's elog(INFO, "TRACK <stage> %f") lines (freddy_gpu_last_track)
  Clock::time_point t_start, t_last;
  void track(double freddy_track::*stage) {
    const auto t = Clock::now();
    j->track.*stage += std::chrono::duration<double>(t - t_last).count();
    t_last = t;
  }
#ifdef FREDDY_LAB
  void mark(const char* what) const {   // host timeline of a call on stderr (lab builds; tools/lab/join_trace_host.py)
    static const bool jtrace = getenv("FREDDY_GPU_JOIN_TRACE") != nullptr;
    if (jtrace) fprintf(stderr, "[join] %7.1f us  %s\n", std::chrono::duration<double, std::micro>(Clock::now() - t_start).count(), what);
  }
#else
  void mark(const char*) const {}
#endif

  size_t side_row() const { return (size_t)2 * j->Kc; }
  size_t grow_sides(size_t n);
  int sort_sides(unsigned rows, const int32_t* only);
  int fetch_sides(const std::vector<int32_t>& need);
  int launch_traverse(int n_act, int min_target);
  int launch_query(const JoinArgs& a, int n);
  int launch_replay(const u64* keys);
  bool stop_confirmed(const int32_t* sm);
  int enqueue_fb_rows();
  int enqueue_join();

  int begin(JoinIndex* j, hipStream_t s, const JoinQueries& queries, int Q, int k, const int32_t* target_ids, int64_t n_targets, int alpha,
            int pvf, int method, int use_tl, float confidence, int double_threshold, int32_t* out_ids, float* out_dist,
            int32_t* iterations_out);
  int workspaces();
  int targets();
  int front();
  int front_rows();
  int prepare_rounds();
  int traverse_round();
  void check_stops();
  int host_heap();
  void scan_list();
  int scan_round();
  void requeue();
  void end();
};

// What a call is refused for besides its pointers and counts, in begin()'s order; nothing here touches a device or the handle (the
// entry points that check their arguments before they resolve ids ask it first, begin() asks it again).
static inline int join_refusals(const JoinIndex* j, int k, int64_t n_targets, int alpha, int pvf, int method, int double_threshold) {
  if (method < 0 || method > 2) return join_fail(FREDDY_E_ARG, "Unknown computation method!");   // ivpq_search_in.c:374-376
  if (method != FREDDY_METHOD_PQ && !j->has_vectors) return join_fail(FREDDY_E_ARG, "methods 1 and 2 need the vectors to be pinned");
  if (n_targets > INT32_MAX) return join_fail(FREDDY_E_LIMIT, "too many targets");
  if (pvf < 1) pvf = 1;                                                                       // :207-209
  const bool double_codes = method != FREDDY_METHOD_EXACT && (int64_t)alpha * k > double_threshold;      // :262-266
  if (double_codes && (int64_t)j->K * j->K > 32768) return join_fail(FREDDY_E_LIMIT, "pair codes of K=%d overflow the reference's int16", j->K);
  const bool pv = method == FREDDY_METHOD_PQ_PV;
  const int64_t Lw = pv ? (int64_t)k * pvf : 2 * (int64_t)k;
  // (more than 1024 candidates, up to 8192, are selected 1024 per pass -- join_query_kernel<16, true>: post verification walks
  // them in (ADC distance, row) order whatever their number; the replay of methods 0 / 1 holds up to 1024 keys in one wave's
  // registers, and beyond that bigk_replay_kernel computes the list the replay would leave -- bigk.h)
  if (!pv && k > BIGK_KMAX) return join_fail(FREDDY_E_LIMIT, "k=%d exceeds this build's limit of %d", k, BIGK_KMAX);
  if (pv && Lw > 8192) return join_fail(FREDDY_E_LIMIT, "k*pvf=%lld exceeds this build's limit of 8192", (long long)Lw);
  return 0;
}

// ---- argument checks, the shape of the call, initTopKs
inline int JoinRun::begin(JoinIndex* j_, hipStream_t s_, const JoinQueries& queries_, int Q_, int k_, const int32_t* target_ids_,
                          int64_t n_targets_, int alpha_, int pvf_, int method_, int use_tl_, float confidence_,
                          int double_threshold, int32_t* out_ids_, float* out_dist_, int32_t* iterations_out_) {
  j = j_; s = s_; qsrc = queries_; queries = qsrc.src.host; Q = Q_; k = k_; target_ids = target_ids_; n_targets = n_targets_;
  alpha = alpha_original = alpha_; pvf = pvf_; method = method_; use_tl = use_tl_; confidence = confidence_;
  out_ids = out_ids_; out_dist = out_dist_; iterations_out = iterations_out_;
  if (int rc = join_refusals(j, k, n_targets, alpha, pvf, method, double_threshold)) return rc;
  j->track = freddy_track();
  t_start = t_last = Clock::now();
  if (pvf < 1) pvf = 1;                                                                       // :207-209
  double_codes = method != FREDDY_METHOD_EXACT && (int64_t)alpha * k > double_threshold;      // :262-266
  const bool pv = method == FREDDY_METHOD_PQ_PV;
  const int64_t Lw = pv ? (int64_t)k * pvf : 2 * (int64_t)k;
  big = Lw > 1024;
  replay = big && !pv;
  L = (int)Lw;
  V = big ? 16 : pick_V(L);
  for (int i = 0; i < Q * k; ++i) { out_ids[i] = -1; out_dist[i] = JOIN_MAX_DIST; }            // initTopKs :238
  if (iterations_out) *iterations_out = 0;
  return 0;
}

// ---- the rest of the shape, the device workspaces and the pinned block of the target array
inline int JoinRun::workspaces() {
  const int d = j->d, Kc = j->Kc, cells = j->cells;
  lds = join_lds_bytes(d, j->m, j->K, k, V);
  if (lds > 160 * 1024) return join_fail(FREDDY_E_LIMIT, "LDS need of %zu bytes exceeds 160 KiB (m=%d K=%d k*pvf=%d)", lds, j->m, j->K, L);
  SV = pick_V(Kc);
  if (SV == 0) return join_fail(FREDDY_E_LIMIT, "coarse_codes=%d exceeds this build's limit of 1024", Kc);
  // The multi-index traversal runs on the device for <= 1024 cells (join_traverse_kernel; the host's libm checks every
  // stop); larger multi-indexes, option join_host_traversal and the queries the device hands back use the host heap.
  dev_trav = cells <= 1024 && !j->host_traversal;
  TV = pick_V(cells);
  const size_t nt = std::max<size_t>((size_t)n_targets, 1);
  if (join_buf(j, JW_QUERIES, (size_t)Q * d, &d_q) || join_buf(j, JW_SUB, (size_t)Q * 2 * Kc, &d_sub) ||
      join_buf(j, JW_TCELL_OFF, (size_t)(cells + 1), &d_tcell) || join_buf(j, JW_TROW, nt, &d_trow) ||
      join_buf(j, JW_SCAN, (size_t)Q, &d_scan) || join_buf(j, JW_QCELL_OFF, (size_t)(Q + 1), &d_qoff) ||
      join_buf(j, JW_WIN, nt, &d_win) || join_buf(j, JW_CELL_CNT, (size_t)cells * 2, &d_cnt) ||
      join_buf(j, JW_SORTED, (size_t)Q * 2 * Kc, &d_sorted))
    return FREDDY_E_NOMEM;
  const size_t tl_bytes = sizeof(int32_t) * ((size_t)cells + 1 + nt);
  if (tl_bytes > j->h_tl.cap) j->tl_valid = false;   // (a new block: the previous target array is gone)
  if (j->h_tl.ensure(tl_bytes)) return join_fail(FREDDY_E_NOMEM, "pinned staging allocation failed");
  tcell_off = j->h_tl.as<const int32_t>();
  h_tids = j->h_tl.as<int32_t>() + (size_t)cells + 1;
  return 0;
}

// ---- "fq.id IN (targets)": resolved, de-duplicated and bucketed by cell on the device (see join_mark_kernel)
inline int JoinRun::targets() {
  const int cells = j->cells;
  tl_hit = j->tl_valid && j->tl_n == n_targets && j->tl_cells == cells &&
           (n_targets == 0 || memcmp(h_tids, target_ids, sizeof(int32_t) * (size_t)n_targets) == 0);
  if (!tl_hit) {   // (a hit: JW_TCELL_OFF / JW_TROW and the pinned offsets still hold this target array's buckets)
    j->tl_valid = false;
    int32_t* cnt = d_cnt;
    int32_t* fill = cnt + cells;
    JOIN_HIP(hipMemsetAsync(j->markbits, 0, sizeof(uint32_t) * (size_t)((j->N + 31) / 32 + 1), s));
    JOIN_HIP(hipMemsetAsync(d_cnt, 0, sizeof(int32_t) * (size_t)cells * 2, s));
    void* p_tl = nullptr;
    JOIN_HIP(hipHostGetDevicePointer(&p_tl, j->h_tl.p, 0));
    const dim3 grid((unsigned)((n_targets + 255) / 256));
    if (n_targets > 0) {
      memcpy(h_tids, target_ids, sizeof(int32_t) * (size_t)n_targets);
      hipLaunchKernelGGL(join_mark_kernel, grid, dim3(256), 0, s, static_cast<const int32_t*>(p_tl) + (size_t)cells + 1, (int)n_targets,
                         (const int32_t*)j->ids, j->N, j->ids_affine ? 1 : 0, (const int32_t*)j->cell, j->markbits, d_win, cnt);
    }
    hipLaunchKernelGGL(join_offsets_kernel, dim3(1), dim3(256), 0, s, (const int32_t*)cnt, cells, d_tcell, fill, static_cast<int32_t*>(p_tl));
    if (n_targets > 0)
      hipLaunchKernelGGL(join_place_kernel, grid, dim3(256), 0, s, (const int32_t*)d_win, (int)n_targets, (const int32_t*)j->cell, fill, d_trow);
    JOIN_HIP(hipGetLastError());
    j->tl_n = n_targets; j->tl_cells = cells;   // (valid once the offsets have arrived: the first synchronisation, see end())
  }
  mark("target array enqueued");
  track(&freddy_track::data_retrieval_time);   // "fq.id IN (targets)" (enqueue only: the device work overlaps what follows)
  return 0;
}

// ---- the queries to the device, and their sub-distances to the multi-index centroids
inline int JoinRun::front() {
  const int d = j->d, Kc = j->Kc;
  if (qsrc.in_block) {   // the caller's kernel wrote JW_QUERIES on this stream: nothing to copy
    hipLaunchKernelGGL(sub_dist_kernel, dim3((unsigned)Q, 2), dim3(64), 0, s, (const float*)d_q, j->coarseT, d_sub, d, Kc, (float*)nullptr, 0);
    JOIN_HIP(hipGetLastError());
    mark("queries in place, sub-distances enqueued");
    return 0;
  }
  if (qsrc.src.table) return front_rows();
  // a query buffer that is pinned already (freddy_gpu_host_alloc: what pg/freddy_gpu_glue.c's query_buffer() hands over) is read
  // where it is -- the 6 MB staging copy of 5 000 queries is the longest host step of a call
  const float* p_queries = static_cast<const float*>(pinned_device_pointer(queries));
  // sub_dist_kernel reads with 16-byte loads: a VIEW into a pinned buffer at an odd offset goes through the staging copy (whose
  // base is aligned), and so does a buffer another device's context pinned (no device address here)
  if (p_queries && (reinterpret_cast<uintptr_t>(p_queries) & 15u)) p_queries = nullptr;
  const bool fused_front = (d & 1) == 0 && d / 2 <= 512;   // (the kernel's staging buffer; odd d: the halves do not cover the vector)
  if (p_queries && fused_front) {
    hipLaunchKernelGGL(sub_dist_kernel, dim3((unsigned)Q, 2), dim3(64), 0, s, p_queries, j->coarseT, d_sub, d, Kc, d_q, 0);
    JOIN_HIP(hipGetLastError());
  } else {   // queries: host copy into pinned staging, read by a copy kernel (1.2 KB per query over PCIe)
    if (j->h_q.ensure(sizeof(float) * (size_t)Q * d)) return join_fail(FREDDY_E_NOMEM, "pinned staging allocation failed");
    // (in pieces of whole queries: the host copies piece i + 1 while sub_dist_kernel pulls piece i over PCIe, writes the device
    // copy and computes the piece's sub-distances)
    const int piece_q = std::max((Q + 3) / 4, 64);
    for (int qa = 0; qa < Q; qa += piece_q) {
      const int nq = std::min(piece_q, Q - qa);
      memcpy(j->h_q.as<float>() + (size_t)qa * d, queries + (size_t)qa * d, sizeof(float) * (size_t)nq * d);
      if (fused_front)
        hipLaunchKernelGGL(sub_dist_kernel, dim3((unsigned)nq, 2), dim3(64), 0, s, j->h_q.as<const float>(), j->coarseT, d_sub, d, Kc, d_q, qa);
      else
        hipLaunchKernelGGL(join_copy_kernel, dim3((unsigned)std::min<size_t>(((size_t)nq * d + 255) / 256, 1024)), dim3(256), 0, s,
                           j->h_q.as<const uint32_t>() + (size_t)qa * d, (uint32_t*)d_q + (size_t)qa * d, (size_t)nq * d);
    }
    if (!fused_front)
      hipLaunchKernelGGL(sub_dist_kernel, dim3((unsigned)Q, 2), dim3(64), 0, s, (const float*)d_q, j->coarseT, d_sub, d, Kc, (float*)nullptr, 0);
    JOIN_HIP(hipGetLastError());
  }
  mark("queries staged, sub-distances enqueued");
  return 0;
}

// Queries that are rows of a device table: their numbers (4 bytes per query) into the pinned block, and ONE launch that gathers the
// rows into JW_QUERIES and computes their sub-distances (sub_dist_rows_kernel).  Half vectors beyond the kernel's staging buffer, and
// option join_front_gather = 0, take two launches: query_gather_kernel into JW_QUERIES, then sub_dist_kernel over it.
inline int JoinRun::front_rows() {
  const int d = j->d, Kc = j->Kc;
  if (j->h_q.ensure(sizeof(int32_t) * (size_t)Q)) return join_fail(FREDDY_E_NOMEM, "pinned staging allocation failed");
  memcpy(j->h_q.p, qsrc.src.rows, sizeof(int32_t) * (size_t)Q);
  void* p_rows = nullptr;
  JOIN_HIP(hipHostGetDevicePointer(&p_rows, j->h_q.p, 0));
  const int32_t* rows = static_cast<const int32_t*>(p_rows);
  if (d / 2 <= 512 && j->front_gather) {
    timed_launch(qsrc.ix, s, "join_front_rows", [&] {
      hipLaunchKernelGGL(sub_dist_rows_kernel, dim3((unsigned)Q, 2), dim3(64), 0, s, qsrc.src.table, rows, qsrc.src.n_table, (const float*)j->coarseT,
                         d_sub, d, Kc, d_q);
    });
    JOIN_HIP(hipGetLastError());
  } else {
    if (launch_query_gather(qsrc.ix, s, qsrc.src, rows, d_q, Q, d)) return join_fail(FREDDY_E_HIP, "launch of the query gather failed");
    hipLaunchKernelGGL(sub_dist_kernel, dim3((unsigned)Q, 2), dim3(64), 0, s, (const float*)d_q, j->coarseT, d_sub, d, Kc, (float*)nullptr, 0);
    JOIN_HIP(hipGetLastError());
  }
  mark("row numbers staged, gather + sub-distances enqueued");
  return 0;
}

// ---- the host heap's inputs
// Room for n more queries in sub / sides; the first new slot.  (The caller fills the rows -- copies from the device land in
// them directly -- and records side_slot.)
inline size_t JoinRun::grow_sides(size_t n) {
  if (side_slot.empty()) side_slot.assign((size_t)Q, -1);
  const size_t base = sub.size() / side_row();
  sub.resize((base + n) * side_row());
  sides.resize((base + n) * side_row());
  return base;
}

inline int JoinRun::sort_sides(unsigned rows, const int32_t* only) {
  const bool known = with_V(SV, [&](auto v) {
    hipLaunchKernelGGL((side_sort_kernel<decltype(v)::value>), dim3(rows), dim3(64), 0, s, (const float*)d_sub, d_sorted, j->Kc, only);
  });
  if (!known) return join_fail(FREDDY_E_LIMIT, "unsupported side-sort width");
  JOIN_HIP(hipGetLastError());
  return 0;
}

// sub-distances and sorted sides of the queries of `need`: all queries at once when many are asked for, else just those (the
// device traversal hands back a query or two per call: sorting and copying 5 000 queries' sides for them cost 0.2 ms)
inline int JoinRun::fetch_sides(const std::vector<int32_t>& need) {
  if (host_sides_all) return 0;
  std::vector<int32_t> miss;
  for (int32_t q : need) if (side_slot.empty() || side_slot[(size_t)q] < 0) miss.push_back(q);
  if (miss.empty()) return 0;
  const size_t row = side_row();
  const bool all = miss.size() * 8 > (size_t)Q;
  if (all) { sub.clear(); sides.clear(); }
  const size_t base = grow_sides(all ? (size_t)Q : miss.size());
  if (all) {
    if (int rc = sort_sides((unsigned)Q * 2, nullptr)) return rc;
    JOIN_HIP(hipMemcpyAsync(sub.data(), d_sub, sizeof(float) * sub.size(), hipMemcpyDeviceToHost, s));
    JOIN_HIP(hipMemcpyAsync(sides.data(), d_sorted, sizeof(JoinSide) * sides.size(), hipMemcpyDeviceToHost, s));
  } else {
    JOIN_HIP(hipMemcpyAsync(d_scan, miss.data(), sizeof(int32_t) * miss.size(), hipMemcpyHostToDevice, s));   // (the scan list goes into this buffer later, in stream order)
    if (int rc = sort_sides((unsigned)miss.size() * 2, d_scan)) return rc;
    for (size_t i = 0; i < miss.size(); ++i) {
      JOIN_HIP(hipMemcpyAsync(sub.data() + (base + i) * row, d_sub + (size_t)miss[i] * row, sizeof(float) * row, hipMemcpyDeviceToHost, s));
      JOIN_HIP(hipMemcpyAsync(sides.data() + (base + i) * row, d_sorted + (size_t)miss[i] * row, sizeof(JoinSide) * row, hipMemcpyDeviceToHost, s));
    }
  }
  JOIN_HIP(hipStreamSynchronize(s));
  if (all) for (int q = 0; q < Q; ++q) side_slot[(size_t)q] = q;
  else for (size_t i = 0; i < miss.size(); ++i) side_slot[(size_t)miss[i]] = (int32_t)(base + i);
  host_sides_all = all;
  return 0;
}

// ---- what the rounds need: the host heap's sides (host traversal), the landing zone, the traversal's buffers, per-query state
inline int JoinRun::prepare_rounds() {
  const int cells = j->cells;
  if (!dev_trav) {
    std::vector<int32_t> all_queries((size_t)Q);
    for (int i = 0; i < Q; ++i) all_queries[(size_t)i] = i;
    if (int rc = fetch_sides(all_queries)) return rc;
  }
  const JoinZoneLayout zone(Q, k, j->Kc);
  if (j->h_sum.ensure(zone.bytes)) return join_fail(FREDDY_E_NOMEM, "pinned staging allocation failed");
  void* dp = nullptr;
  JOIN_HIP(hipHostGetDevicePointer(&dp, j->h_sum.p, 0));
  h = zone.at(j->h_sum.p);
  p = zone.at(dp);
  if (dev_trav) {
    if (join_buf(j, JW_ACTIVE, (size_t)Q, &d_active) || join_buf(j, JW_QCELLS, (size_t)Q * cells, &d_qcells) ||
        join_buf(j, JW_QCELL_CNT, (size_t)Q, &d_qcnt))
      return FREDDY_E_NOMEM;
  }
  if (!dev_trav) JOIN_HIP(hipStreamSynchronize(s));   // (tcell_off is on the host now; the device path waits with its first summaries)
  track(&freddy_track::precomputation_time);   // queries in, sub-distances (+ side sorts and their way back for the host heap)
  active.resize((size_t)Q);
  for (int i = 0; i < Q; ++i) active[(size_t)i] = i;
  target_count.assign((size_t)Q, 0);
  qcells.resize((size_t)Q);
  q_n.assign((size_t)Q, 0); q_rows.assign((size_t)Q, 0);
  q_host.assign((size_t)Q, 0); q_exh.assign((size_t)Q, 0);
  spec_index.assign((size_t)Q, 0);
  return 0;
}

// ---- device traversal
// Traversal of the n_act queries listed in JW_ACTIVE for `min_target` expected targets; the summaries are on their way to
// h.summary (row x of the list) when this returns.
inline int JoinRun::launch_traverse(int n_act, int min_target_) {
  TravArgs ta;
  ta.sub = d_sub; ta.active = d_active; ta.stats = j->d_stats; ta.tcell_off = d_tcell;
  ta.qcells = d_qcells; ta.qcell_cnt = d_qcnt; ta.summary = p.summary; ta.fb_sub = p.fb_sub;
  ta.Kc = j->Kc; ta.cells = j->cells; ta.n_targets = (int)n_targets; ta.min_target = min_target_; ta.confidence = confidence;
  // (the 64 smallest keys suffice when the stop is expected far below 63 cells: four times the cells min_target needs at
  // the targets' average density; a query that needs more goes to the host heap)
  const double per_cell = (double)n_targets / (double)std::max(j->cells, 1);
  const bool small = TV > 1 && per_cell > 0.0 && 3.0 * (double)min_target_ / per_cell < 31.0;
  const bool known = with_V(TV, [&](auto v) {
    constexpr int W = decltype(v)::value;
    if constexpr (W > 1) {   // (one wave's 64 keys are all the cells there are: no SMALL kernel of width 1)
      if (small) { hipLaunchKernelGGL((join_traverse_kernel<W, true>), dim3((unsigned)n_act), dim3(64), 0, s, ta); return; }
    }
    hipLaunchKernelGGL((join_traverse_kernel<W>), dim3((unsigned)n_act), dim3(64), 0, s, ta);
  });
  if (!known) return join_fail(FREDDY_E_LIMIT, "unsupported traversal width");
  JOIN_HIP(hipGetLastError());
  return 0;
}

// The round's active list to the device, and its traversal -- unless the previous round launched it already (spec_index).
inline int JoinRun::traverse_round() {
  // (the list on the device is this round's in any case: the traversal launched behind this round's join reads it)
  // (lists go host -> pinned -> a copy kernel: a workgroup that reads its query number over PCIe starts 2 us late, 20 workgroups
  // deep per CU that was +70 us on the join kernel; nothing of the previous round is in flight: it ended with a synchronisation)
  memcpy(h.active, active.data(), sizeof(int32_t) * (size_t)n_active);
  hipLaunchKernelGGL(join_copy_kernel, dim3((unsigned)((n_active + 255) / 256)), dim3(256), 0, s, (const uint32_t*)p.active, (uint32_t*)d_active, (size_t)n_active);
  if (!spec_valid) {
    if (int rc = launch_traverse(n_active, min_target)) return rc;
    mark("traversal enqueued");
    JOIN_HIP(hipStreamSynchronize(s));
    mark("traversal synchronised");
    for (int x = 0; x < n_active; ++x) spec_index[(size_t)active[x]] = x;
  }
  spec_valid = false;
  return 0;
}

// The host's libm decides: the reference's expression at the stop a summary proposes and one step before it.  The device's own
// values of it stand where they are further than libm_margin from the confidence.
inline bool JoinRun::stop_confirmed(const int32_t* sm) {
  const int cells = j->cells, n = sm[0];
  const int stat_size = (int)j->h_stats[(size_t)cells];
  float Pn, Pm, Cn, Cm;
  memcpy(&Pn, &sm[4], 4); memcpy(&Pm, &sm[5], 4); memcpy(&Cn, &sm[6], 4); memcpy(&Cm, &sm[7], 4);
  bool ok = !(sm[3] & 1) && n >= 0 && n <= cells;
  const float margin = j->libm_margin;
  if (ok && n < cells) {
    ok = !(Cn < confidence);
    if (!(fabsf(Cn - confidence) > margin)) { ok = !(join_confidence_expr(min_target, (int)n_targets, Pn, stat_size) < confidence); ++j->track.libm_checks; }
  }
  if (ok && n > 0) {
    ok = Cm < confidence;
    if (!(fabsf(Cm - confidence) > margin)) { ok = join_confidence_expr(min_target, (int)n_targets, Pm, stat_size) < confidence; ++j->track.libm_checks; }
  }
  return ok;
}

// Every active query's summary: a confirmed stop is the query's traversal of this round, the others go to the host heap (fb).
inline void JoinRun::check_stops() {
  const size_t row = side_row();
  for (int x = 0; x < n_active; ++x) {
    const int q = active[x];
    const size_t at = (size_t)spec_index[(size_t)q];
    const int32_t* sm = h.summary + at * TRAV_SUM_DW;
    const bool ok = stop_confirmed(sm);
    q_host[q] = ok ? 0 : 1;
    if (ok) { q_n[q] = sm[0]; q_rows[q] = sm[2]; q_exh[q] = sm[0] >= j->cells; }
    if (!ok && (sm[3] & 1) && !host_sides_all && (side_slot.empty() || side_slot[(size_t)q] < 0)) {
      // handed back by the device with its sub-distances: the two sides are sorted here
      const size_t slot = grow_sides(1);
      memcpy(sub.data() + slot * row, h.fb_sub + at * row, sizeof(float) * row);
      join_sort_sides_host(h.fb_sub + at * row, j->Kc, sides.data() + slot * row);
      side_slot[(size_t)q] = (int32_t)slot;
    }
  }
  for (int q : active) if (q_host[q]) fb.push_back(q);
  mark("summaries checked");
}

// ---- the reference's heap for the queries of fb; `last`: every active query has exhausted the cells
inline int JoinRun::host_heap() {
  if (!fb.empty()) {
    if (int rc = fetch_sides(fb)) return rc;
    for (int q : fb) q_host[q] = 1;
    const int Kc = j->Kc;
    join_parallel_for((int)fb.size(), [&](int lo, int hi, int) {                            // :327-331
      JoinTraversal w;
      for (int x = lo; x < hi; ++x) {
        const int q = fb[x];
        qcells[q].clear();
        const size_t sl = (size_t)side_slot[(size_t)q];
        const bool exhausted = join_select_cells(sides.data() + (sl * 2) * Kc, sides.data() + (sl * 2 + 1) * Kc,
                                                 sub.data() + (sl * 2) * Kc, sub.data() + (sl * 2 + 1) * Kc, Kc,
                                                 j->h_stats.data(), (int)n_targets, min_target, confidence, w, qcells[q]);
        q_exh[q] = exhausted ? 1 : 0;
        int64_t cnt = 0;
        for (int32_t c : qcells[q]) cnt += tcell_off[c + 1] - tcell_off[c];
        q_rows[q] = (int)cnt;
        q_n[q] = (int)qcells[q].size();
      }
    });
  }
  j->track.host_traversals += (int64_t)fb.size();
  last = true;
  for (int q : active) if (!q_exh[q]) { last = false; break; }
  track(&freddy_track::determine_coarse_quantization_time);
  return 0;
}

// ---- targetCounts (:459), the target-list skip rule (:553-557), and the order of the round's launch
inline void JoinRun::scan_list() {
  scan.clear(); scan_fb.clear(); qoff.assign(1, 0); flat.clear();
  for (int x = 0; x < n_active; ++x) {
    const int q = active[x];
    target_count[q] += q_rows[q];
    if (use_tl && target_count[q] < k * alpha_original && !last) { target_count[q] = 0; continue; }
    j->track.candidate_rows += q_rows[q];
    if (!q_host[q]) { scan.push_back(q); continue; }
    scan_fb.push_back(q);
    for (int32_t c : qcells[q]) if (tcell_off[c + 1] > tcell_off[c]) flat.push_back(c);
    qoff.push_back((int32_t)flat.size());
  }
  // longest first: a query's workgroup is a chain whose length grows with its target rows (a few queries have ten times
  // the average), and the launch ends with whatever was started last -- counting sort on rows / 128, descending
  if (scan.size() > 256) {
    constexpr int NBK = 64;
    int cnt[NBK + 1] = {0};
    auto bucket = [&](int q) { const int b = q_rows[q] >> 7; return NBK - 1 - (b < NBK ? b : NBK - 1); };
    for (int q : scan) ++cnt[bucket(q) + 1];
    for (int b = 0; b < NBK; ++b) cnt[b + 1] += cnt[b];
    std::vector<int32_t> sorted(scan.size());
    for (int q : scan) sorted[(size_t)cnt[bucket(q)]++] = q;
    scan.swap(sorted);
  }
  n_dev = (int)scan.size(); n_fb = (int)scan_fb.size(); n_scan = n_dev + n_fb;
  scan.insert(scan.end(), scan_fb.begin(), scan_fb.end());
  mark("scan list built");
  track(&freddy_track::query_construction_time);
}

// ---- the round's join launch(es)
inline int JoinRun::launch_query(const JoinArgs& a, int n) {
  const dim3 grid((unsigned)n), block(JOIN_WG);
  if (big) hipLaunchKernelGGL((join_query_kernel<16, true>), grid, block, lds, s, a);
  else if (!with_V(V, [&](auto v) { hipLaunchKernelGGL((join_query_kernel<decltype(v)::value>), grid, block, lds, s, a); }))
    return join_fail(FREDDY_E_LIMIT, "unsupported selection width");
  JOIN_HIP(hipGetLastError());
  return 0;
}

// Methods 0 / 1 of a big call: the round's lists in closed form from the 2k keys join_query_kernel<16, true> left per scanned
// query.  A round starts from empty lists (first_round), a row's arrival is its row number (the key's low word), and the lists go
// to the landing zone, row x of the scan list.
inline int JoinRun::launch_replay(const u64* keys) {
  BigkArgs b;
  b.sel = keys; b.active = nullptr; b.pos_to_id = j->ids; b.round_rows = nullptr; b.cand_count = nullptr;
  b.out_ids = p.out_ids; b.out_dist = p.out_dist; b.found = nullptr; b.next_active = nullptr; b.n_next = nullptr; b.status = nullptr;
  b.n_active = n_scan; b.nsel = L; b.k = k; b.found_rule = 0; b.first_round = 1; b.sentinel = JOIN_MAX_DIST;
  b.npad = 2048;
  while (b.npad < k + L) b.npad *= 2;   // (<= 16384: k <= BIGK_KMAX, L = 2k)
  hipLaunchKernelGGL(bigk_replay_kernel, dim3((unsigned)n_scan), dim3(BIGK_T), bigk_lds_bytes(b.npad, k), s, b);
  JOIN_HIP(hipGetLastError());
  return 0;
}

// Cell lists of the host-traversed queries into their rows of JW_QCELLS (join_fb_rows_kernel), through the query staging block.
inline int JoinRun::enqueue_fb_rows() {
  const int cells = j->cells;
  int32_t* hf = j->h_q.as<int32_t>();   // (the query staging block: its copy kernels finished before the first synchronisation)
  for (int x = 0; x < n_fb; ++x) {
    int32_t* row = hf + (size_t)x * (cells + 1);
    const int cnt = qoff[(size_t)x + 1] - qoff[(size_t)x];
    row[0] = cnt;
    memcpy(row + 1, flat.data() + qoff[(size_t)x], sizeof(int32_t) * (size_t)cnt);
  }
  hipLaunchKernelGGL(join_fb_rows_kernel, dim3((unsigned)n_fb), dim3(256), 0, s, j->h_q.as<const int32_t>(), (const int32_t*)d_scan + n_dev, d_qcells, d_qcnt, cells);
  JOIN_HIP(hipGetLastError());
  return 0;
}

// Scan list up, join kernel over it between the two events, and the NEXT round's traversal behind it.
inline int JoinRun::enqueue_join() {
  const int cells = j->cells;
  memcpy(h.scan, scan.data(), sizeof(int32_t) * (size_t)n_scan);
  hipLaunchKernelGGL(join_copy_kernel, dim3((unsigned)((n_scan + 255) / 256)), dim3(256), 0, s, (const uint32_t*)p.scan, (uint32_t*)d_scan, (size_t)n_scan);
  JoinArgs a;
  a.queries = d_q; a.tcell_off = d_tcell; a.trow = d_trow;
  a.ids = j->ids; a.codes = j->codes; a.MP = j->MP; a.vectors = j->vectors; a.cbT = j->cbT;
  a.d = j->d; a.m = j->m; a.K = j->K; a.S = j->S; a.k = k; a.L = L; a.method = method; a.double_codes = double_codes ? 1 : 0;
  if (big && (join_buf(j, JW_BIG_KEYS, (size_t)n_scan * L, &a.big_keys) ||
              (!replay && join_buf(j, JW_BIG_EXACT, (size_t)n_scan * L, &a.big_exact))))
    return FREDDY_E_NOMEM;
  u64* const big_keys = a.big_keys;
  if (!j->ev0) { JOIN_HIP(hipEventCreate(&j->ev0)); JOIN_HIP(hipEventCreate(&j->ev1)); JOIN_HIP(hipEventCreate(&j->ev_replay)); }
  JOIN_HIP(hipEventRecord(j->ev0, s));
  // (a separate launch for the host-traversed queries ran behind the main one -- a lone workgroup's 45 us -- and its two
  // list uploads were SDMA hops: a query with a tie cost the call 0.1 ms)
  const bool fb_rows = dev_trav && n_fb > 0 && j->h_q.p && (size_t)n_fb * (size_t)(cells + 1) * sizeof(int32_t) <= j->h_q.cap;
  if (fb_rows) if (int rc = enqueue_fb_rows()) return rc;
  if (n_dev > 0 || fb_rows) {     // cell lists written by the traversal kernel (and join_fb_rows_kernel): row q of [Q][cells]
    a.scan_query = d_scan; a.qcell_off = nullptr; a.qcell_cnt = d_qcnt; a.qstride = cells;
    a.qcells = d_qcells; a.out_ids = p.out_ids; a.out_dist = p.out_dist;
    if (int rc = launch_query(a, fb_rows ? n_scan : n_dev)) return rc;
  }
  if (n_fb > 0 && !fb_rows) {      // host-traversed queries: flat lists with offsets
    int32_t* d_flat = nullptr;
    if (join_buf(j, JW_QCELLS_FLAT, std::max<size_t>(flat.size(), 1), &d_flat)) return FREDDY_E_NOMEM;
    JOIN_HIP(hipMemcpyAsync(d_qoff, qoff.data(), sizeof(int32_t) * (n_fb + 1), hipMemcpyHostToDevice, s));
    if (!flat.empty()) JOIN_HIP(hipMemcpyAsync(d_flat, flat.data(), sizeof(int32_t) * flat.size(), hipMemcpyHostToDevice, s));
    a.scan_query = d_scan + n_dev; a.qcell_off = d_qoff; a.qcell_cnt = nullptr; a.qstride = 0;
    a.qcells = d_flat; a.out_ids = p.out_ids + (size_t)n_dev * k; a.out_dist = p.out_dist + (size_t)n_dev * k;
    if (big) { a.big_keys += (size_t)n_dev * L; if (a.big_exact) a.big_exact += (size_t)n_dev * L; }   // (rows x of the scan list, as the lists)
    if (int rc = launch_query(a, n_fb)) return rc;
  }
  if (replay) {
    JOIN_HIP(hipEventRecord(j->ev_replay, s));
    if (int rc = launch_replay(big_keys)) return rc;
  }
  JOIN_HIP(hipEventRecord(j->ev1, s));
  if (dev_trav && !last && (int64_t)k * alpha * 2 < INT32_MAX) {   // the next round's cells for everyone still active (see spec_index)
    if (int rc = launch_traverse(n_active, k * (alpha + alpha))) return rc;
    for (int x = 0; x < n_active; ++x) spec_index[(size_t)active[x]] = x;
    spec_valid = true;
  }
  mark("join (+ next traversal) enqueued");
  return 0;
}

// ---- the round on the device: LUTs, ADC / exact distances, post verification -- one kernel -- and its lists back to the caller
inline int JoinRun::scan_round() {
  if (n_scan > 0) {
    if (int rc = enqueue_join()) return rc;
    JOIN_HIP(hipStreamSynchronize(s));
    mark("join synchronised");
    { float ms = 0.0f; if (hipEventElapsedTime(&ms, j->ev0, j->ev1) == hipSuccess) j->track.join_kernel_time += 1e-3 * ms; }
    if (replay) { float ms = 0.0f; if (hipEventElapsedTime(&ms, j->ev_replay, j->ev1) == hipSuccess) replay_ms += ms; }
    for (int x = 0; x < n_scan; ++x) {
      memcpy(out_ids + (size_t)scan[x] * k, h.out_ids + (size_t)x * k, sizeof(int32_t) * k);
      memcpy(out_dist + (size_t)scan[x] * k, h.out_dist + (size_t)x * k, sizeof(float) * k);
    }
  }
  mark("lists copied out");
  track(&freddy_track::computation_time);
  return 0;
}

// ---- queries whose list is still at MAX_DIST go on with alpha doubled (:639-669, :680)
inline void JoinRun::requeue() {
  if (!last) {
    std::vector<int32_t> next;
    for (int q : active) {
      if (out_dist[(size_t)q * k + k - 1] == JOIN_MAX_DIST) {
        for (int i = 0; i < k; ++i) { out_ids[(size_t)q * k + i] = -1; out_dist[(size_t)q * k + i] = JOIN_MAX_DIST; }
        next.push_back(q);
      }
    }
    active.swap(next);
  } else {
    active.clear();
  }
  alpha += alpha;
  track(&freddy_track::recalculate_query_indices_time);
}

inline void JoinRun::end() {
  if (!tl_hit) j->tl_valid = true;   // (the offsets arrived with the first synchronisation)
  j->track.iterations = iterations;
  j->track.replay_us = (int32_t)std::min(replay_ms * 1e3 + 0.5, (double)INT32_MAX);
  j->track.total_time = std::chrono::duration<double>(Clock::now() - t_start).count();
  if (iterations_out) *iterations_out = iterations;
}

static inline int join_run(JoinIndex* j, hipStream_t s, const JoinQueries& queries, int Q, int k, const int32_t* target_ids,
                           int64_t n_targets, int alpha, int pvf, int method, int use_tl, float confidence,
                           int double_threshold, int32_t* out_ids, float* out_dist, int32_t* iterations_out) {
  JoinRun r;
  if (int rc = r.begin(j, s, queries, Q, k, target_ids, n_targets, alpha, pvf, method, use_tl, confidence, double_threshold,
                       out_ids, out_dist, iterations_out)) return rc;
  if (Q == 0) return 0;
  if (int rc = r.workspaces()) return rc;
  if (int rc = r.targets()) return rc;
  if (int rc = r.front()) return rc;
  if (int rc = r.prepare_rounds()) return rc;
  while (!r.active.empty()) {                                                               // :299
    ++r.iterations;
    r.n_active = (int)r.active.size();
    r.min_target = r.k * r.alpha;
    r.fb.clear();
    if (r.dev_trav) {
      if (int rc = r.traverse_round()) return rc;
      r.check_stops();
    } else {
      r.fb = r.active;
    }
    if (int rc = r.host_heap()) return rc;
    r.scan_list();
    if (int rc = r.scan_round()) return rc;
    r.requeue();
  }
  r.end();
  return 0;
}

}  // namespace freddy
