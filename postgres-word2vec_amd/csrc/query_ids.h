// query_ids.h -- searches whose queries are rows of a pinned vector table, named by id (freddy_gpu_*_search_ids, include/freddy_gpu.h):
// what pipeline.hip, pq.hip, exact.hip and rerank.hip share for them (similarity.hip: the gather).
//   QuerySrc             where the queries of a host-buffer search come from: the caller's floats, or (device table, row numbers).  Every place
//                        that read the caller's host pointer takes one; with `host` set it does exactly what it did before.
//   query_gather_kernel  rows[0..n) of the row-major table [N][d] -> a contiguous query block [n][d].  The row numbers arrive in the
//                        pinned staging block where the floats of a host-buffer call are staged (4 bytes per query instead of 4 d) and
//                        are read from mapped host memory; the launch takes lane_copy_in_kernel's place in the stream.
//   select_query_ids     the id rule, on the host: query_ids -> the selected ids, the rows of those that have one, and their slots.
//   check_ann_vecs       the handles of a call that takes a pq / ivf handle and the raw-vector handle (post verification, approximate
//                        analogies, searches by id).
// A single query is never gathered: the chain's kernels read it where its row lies (table + row * d); the one-launch kernels take
// the query by value in their dispatch packet (one.h), so for them the row is read back first (4 d bytes, no launch).
#pragma once
#include "internal.h"

struct QuerySrc {
  const float* host = nullptr;    // [Q][d] in the caller's memory, or
  const float* table = nullptr;   // the device table [n_table][d], row-major (a vector handle's `coarse`), and
  const int32_t* rows = nullptr;  // [Q] row numbers in HOST memory, every one in [0, n_table)
  int64_t n_table = 0;
  static QuerySrc of_host(const float* q) { QuerySrc s; s.host = q; return s; }
  static QuerySrc of_rows(const freddy_gpu_index* vecs, const int32_t* rows) {
    QuerySrc s; s.table = vecs->coarse; s.rows = rows; s.n_table = vecs->N; return s;
  }
  QuerySrc from(size_t q0, int d) const {   // the source of the queries [q0, ...)
    QuerySrc s = *this;
    if (host) s.host += q0 * (size_t)d; else s.rows += q0;
    return s;
  }
  const float* row_ptr(size_t q, int d) const { return table + (size_t)rows[q] * d; }   // (device pointer)
};

// T = uint4 (d % 4 == 0: rows of the hipMalloc'd table and of the block are 16-byte aligned; U = d / 4 units per row -- 75 at
// d = 300, so a row does not fill a whole number of waves and the units of all rows are walked as one flat range) or float (U = d).
// Consecutive lanes read consecutive units of a row and write consecutive units of the block; the lanes of a row read the same
// word of mapped host memory for its number.  (A version that brought sixteen row numbers per workgroup into LDS first, one 64-byte
// read over PCIe, was no faster at 64 queries and slower from 4096 on -- 27.7 against 18.5 - 22.5 us per call at 4096 -- with a
// sixteenth of the workgroups in flight: DESIGN.md 5.1c.)  A row number outside the table (never produced by select_query_ids)
// reads nothing and leaves zeros.
// (32-bit indices: the launcher cuts a block of more than 2^32 - 1 units into launches)
template <class T>
static __global__ __launch_bounds__(256) void query_gather_kernel(const T* __restrict__ table, const int32_t* __restrict__ rows, T* __restrict__ dst,
                                                                  uint32_t total, uint32_t U, int64_t n_table) {
  const uint32_t stride = gridDim.x * 256u;
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < total; i += stride) {
    const uint32_t q = i / U, u = i - q * U;
    const int64_t r = rows[q];
    T v{};
    if (r >= 0 && r < n_table) v = table[(size_t)r * U + u];
    dst[i] = v;
    if (total - i <= stride) break;   // (i + stride would pass total, and may wrap)
  }
}

// mapped_rows: n row numbers in pinned (mapped) host memory; dst: [n][d] in device memory.  Recorded as "query_gather" on `ann`.
static inline int launch_query_gather(freddy_gpu_index* ann, hipStream_t s, const QuerySrc& qs, const int32_t* mapped_rows, float* dst, int n, int d) {
  if (n <= 0) return 0;
  const bool wide = d % 4 == 0 && reinterpret_cast<uintptr_t>(dst) % 16 == 0 && reinterpret_cast<uintptr_t>(qs.table) % 16 == 0;
  const uint32_t U = wide ? (uint32_t)d / 4 : (uint32_t)d;
  const int per = (int)std::min<uint64_t>((uint64_t)n, 0xffffffffull / U);   // rows per launch: their units fit 32 bits
  for (int q0 = 0; q0 < n; q0 += per) {
    const int nq = std::min(per, n - q0);
    const uint32_t total = (uint32_t)nq * U;   // (i / U < nq for every i the kernel walks: no row number beyond mapped_rows[q0 + nq - 1] is read)
    const dim3 grid((unsigned)std::min<uint32_t>(total / 256 + 1, 2048));
    float* const out = dst + (size_t)q0 * d;
    timed_launch(ann, s, "query_gather", [&] {
      if (wide) hipLaunchKernelGGL(query_gather_kernel<uint4>, grid, dim3(256), 0, s, reinterpret_cast<const uint4*>(qs.table), mapped_rows + q0, reinterpret_cast<uint4*>(out), total, U, qs.n_table);
      else hipLaunchKernelGGL(query_gather_kernel<float>, grid, dim3(256), 0, s, qs.table, mapped_rows + q0, out, total, U, qs.n_table);
    });
    if (hipGetLastError() != hipSuccess) return fail(FREDDY_E_HIP, "launch of the query gather failed");
  }
  return 0;
}

// One query of a device-resident source in host memory (the one-launch kernels' by-value argument): 4 d bytes read back into pinned
// memory (h_q; a pageable destination goes through the runtime's staging and costs twice the time), no launch.
static inline int fetch_query_row(hipStream_t s, const QuerySrc& qs, int d, float* h_q) {
  HIP_TRY(hipMemcpyAsync(h_q, qs.row_ptr(0, d), sizeof(float) * (size_t)d, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return 0;
}

// ---- the id rule (host only) ---------------------------------------------------------------------------------------------------
struct QidSelection {
  std::vector<int32_t> sel;    // the selected ids: out_query_ids[0..Q)
  std::vector<int32_t> rows;   // the rows of those that have one, compacted
  std::vector<int32_t> slot;   // slot[i]: the output slot of rows[i]
  bool dense() const { return rows.size() == sel.size(); }
};
// TABLE_ORDER is rows_of_ids, POSITIONAL one lookup per slot; the lookup is row_of_near (internal.h): the tables these calls name are
// google_vecs_norm and its like, ids 1 .. N less what was deleted, and thousands of plain binary searches over millions of ids cost
// more than a batch's device work (0.37 ms at 8192 ids over 3 M; DESIGN.md 5.1c has both kinds of table).
static inline QidSelection select_query_ids(const std::vector<int32_t>& h_ids, const int32_t* query_ids, int32_t n_ids, int id_rule) {
  QidSelection s;
  if (id_rule == FREDDY_QIDS_TABLE_ORDER) {
    s.rows = rows_of_ids_by(row_of_near, h_ids, query_ids, n_ids);
    s.sel.reserve(s.rows.size()); s.slot.reserve(s.rows.size());
    for (size_t j = 0; j < s.rows.size(); ++j) { s.sel.push_back(h_ids[(size_t)s.rows[j]]); s.slot.push_back((int32_t)j); }
    return s;
  }
  s.sel.assign(query_ids, query_ids + n_ids);
  for (int32_t j = 0; j < n_ids; ++j)
    if (const int32_t r = row_of_near(h_ids, query_ids[j]); r >= 0) { s.rows.push_back(r); s.slot.push_back(j); }
  return s;
}

// The handles of a call that takes a pq / ivf handle and the raw-vector handle; nothing here touches a device.
static inline int check_ann_vecs(const freddy_gpu_index* ann, int kind, const freddy_gpu_index* vecs, const char* what) {
  if (!ann || !vecs) return fail(FREDDY_E_ARG, "NULL index");
  if (ann->kind != kind || vecs->kind != KIND_VEC) return fail(FREDDY_E_KIND, "index handle has the wrong kind for this call");
  if (int rc = refuse_poisoned(ann)) return rc;
  if (int rc = refuse_poisoned(vecs)) return rc;
  if (!ann->replicas.empty())
    return fail(FREDDY_E_ARG, "%s does not take a handle with replicas (%d devices): the vectors are pinned on one device", what, 1 + (int)ann->replicas.size());
  if (vecs->device != ann->device) return fail(FREDDY_E_ARG, "the vectors are pinned on device %d, the index on device %d", vecs->device, ann->device);
  if (vecs->d != ann->d) return fail(FREDDY_E_ARG, "the vectors have %d dimensions, the index has %d", vecs->d, ann->d);
  return 0;
}

// What the four *_ids entry points refuse first, before the checks of the entry point underneath and before the handles' kinds.
static inline int check_query_ids_front(const void* ann, const void* vecs, const int32_t* query_ids, int32_t n_ids, int32_t id_rule, const void* out_query_ids,
                                        const int32_t* n_queries, const void* out_ids, const void* out_val) {
  if (!ann || !vecs) return fail(FREDDY_E_ARG, "NULL index");
  if (n_ids < 0) return fail(FREDDY_E_ARG, "bad sizes (n_ids=%d)", n_ids);
  if (id_rule != FREDDY_QIDS_TABLE_ORDER && id_rule != FREDDY_QIDS_POSITIONAL) return fail(FREDDY_E_ARG, "bad id_rule %d", id_rule);
  if (!n_queries) return fail(FREDDY_E_ARG, "NULL n_queries");
  if (n_ids > 0 && (!query_ids || !out_query_ids || !out_ids || !out_val)) return fail(FREDDY_E_ARG, "NULL buffer");
  return 0;
}

// The frame of the four entry points once nothing is refused: select, search the compacted rows with `search(QuerySrc, n, ids, val)`,
// put every list in its slot and fillers (-1, filler) in the slots without a row.  No device work before all ids are resolved; none at
// all when no id has a row.
// (search_selected_rows: the same over any ascending id column -- the kNN-join by row id reads the ivpq handle's own when it is given
// no vector handle -- with `search(rows, n, ids, val)`)
template <class F>
static int search_selected_rows(const std::vector<int32_t>& h_ids, const int32_t* query_ids, int32_t n_ids, int32_t id_rule, int32_t k, float filler,
                                int32_t* out_query_ids, int32_t* n_queries, int32_t* out_ids, float* out_val, F&& search) {
  *n_queries = 0;
  if (n_ids == 0) return FREDDY_OK;
  const QidSelection s = select_query_ids(h_ids, query_ids, n_ids, id_rule);
  const int Q = (int)s.sel.size(), n = (int)s.rows.size();
  int rc = 0;
  if (s.dense()) {
    if (n) rc = search(s.rows.data(), n, out_ids, out_val);
  } else {
    for (size_t i = 0; i < (size_t)Q * k; ++i) { out_ids[i] = -1; out_val[i] = filler; }
    std::vector<int32_t> ti((size_t)n * k);
    std::vector<float> tv((size_t)n * k);
    if (n) rc = search(s.rows.data(), n, ti.data(), tv.data());
    for (int i = 0; i < n && !rc; ++i) {
      memcpy(out_ids + (size_t)s.slot[(size_t)i] * k, &ti[(size_t)i * k], sizeof(int32_t) * (size_t)k);
      memcpy(out_val + (size_t)s.slot[(size_t)i] * k, &tv[(size_t)i * k], sizeof(float) * (size_t)k);
    }
  }
  if (rc) return rc;
  if (Q) memcpy(out_query_ids, s.sel.data(), sizeof(int32_t) * (size_t)Q);
  *n_queries = Q;
  return FREDDY_OK;
}
template <class F>
static int search_selected_ids(const freddy_gpu_index* vecs, const int32_t* query_ids, int32_t n_ids, int32_t id_rule, int32_t k, float filler,
                               int32_t* out_query_ids, int32_t* n_queries, int32_t* out_ids, float* out_val, F&& search) {
  return search_selected_rows(vecs->h_ids, query_ids, n_ids, id_rule, k, filler, out_query_ids, n_queries, out_ids, out_val,
                              [&](const int32_t* rows, int n, int32_t* oi, float* ov) { return search(QuerySrc::of_rows(vecs, rows), n, oi, ov); });
}

// ---- join.hip: the kNN-join for the approximate analogy over an ivpq handle (rerank.hip freddy_gpu_ivpq_analogy) ---------------------
// knn_join_check: what freddy_gpu_knn_join refuses about its scalars and its shape (nothing touches a device).  join_query_block_for: the
// join's query block with room for Q queries, for a kernel of the caller's to fill on the handle's stream; knn_join_block: the join over
// the first Q queries of that block (arguments already checked), enqueued behind whatever filled it -- no host synchronisation before.
int knn_join_check(const freddy_gpu_index* ivpq, int32_t k, const int32_t* target_ids, int64_t n_targets, int32_t alpha, int32_t pvf, int32_t method,
                   int32_t double_threshold);
int join_query_block_for(freddy_gpu_index* ivpq, int Q, float** block);
int knn_join_block(freddy_gpu_index* ivpq, int Q, int k, const int32_t* target_ids, int64_t n_targets, int alpha, int pvf, int method, int use_target_lists,
                   float confidence, int double_threshold, int32_t* out_ids, float* out_dist, int32_t* iterations_out);

// ---- pipeline.hip / pq.hip: the host-buffer searches behind the public entry points, for either source (arguments already checked) ----
int ivfadc_search_src(freddy_gpu_index* ix, const QuerySrc& qs, int Q, int k, int W, float sentinel, int found_rule, int32_t* out_ids, float* out_dist);
int pq_search_src(freddy_gpu_index* ix, const QuerySrc& qs, int Q, int k, float sentinel, const int32_t* subset_ids, int64_t n_subset, int32_t* out_ids,
                  float* out_dist);
