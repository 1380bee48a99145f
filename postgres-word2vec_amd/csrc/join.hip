// join.hip -- pin_ivpq and knn_join (ivpq_search_in.c:61-699): the entry points.  join.h says which header holds what; the
// call itself is join_run() in join_run.h.  Behind them the statistics row of a pinned handle: set_statistics / get_statistics /
// create_statistics (kernels in stat_kernels.h).
#include "internal.h"

#include "join.h"
#include "join_run.h"
#include "stat_kernels.h"

// the ivpq tables in the layouts the kernels read (checked first: ascending ids, cells and codes in range)
static int join_pin(JoinIndex* j, const freddy_ivpq_desc* t, int64_t* bytes) {
  j->d = t->d; j->m = t->m; j->K = t->K; j->S = t->d / t->m; j->Kc = t->coarse_codes;
  j->cells = t->coarse_codes * t->coarse_codes;
  j->MP = (t->m + 7) & ~7;
  j->N = t->N;
  j->has_vectors = t->vectors != nullptr;
  if (t->K > 32767) return join_fail(FREDDY_E_LIMIT, "K=%d does not fit an int16 code", t->K);
  for (int64_t r = 0; r < t->N; ++r) {
    if (r && t->ids[r] <= t->ids[r - 1]) return join_fail(FREDDY_E_ARG, "ids must be strictly ascending (row %lld)", (long long)r);
    if (t->coarse_id[r] < 0 || t->coarse_id[r] >= j->cells) return join_fail(FREDDY_E_ARG, "coarse_id %d out of range at row %lld", t->coarse_id[r], (long long)r);
    for (int l = 0; l < t->m; ++l) {
      const int c = t->codes[(size_t)r * t->m + l];
      if (c < 0 || c >= t->K) return join_fail(FREDDY_E_ARG, "code %d out of range at row %lld", c, (long long)r);
    }
  }
  const int m = j->m, K = j->K, S = j->S, half = j->d / 2, Kc = j->Kc;
  std::vector<float> cbT((size_t)m * S * K);
  for (int p = 0; p < m; ++p)
    for (int c = 0; c < K; ++c)
      for (int i = 0; i < S; ++i) cbT[((size_t)p * S + i) * K + c] = t->codebook[((size_t)p * K + c) * S + i];
  std::vector<float> cqT((size_t)2 * half * Kc);
  for (int p = 0; p < 2; ++p)
    for (int c = 0; c < Kc; ++c)
      for (int i = 0; i < half; ++i) cqT[((size_t)p * half + i) * Kc + c] = t->coarse[((size_t)p * Kc + c) * half + i];
  if (upload(&j->cbT, cbT.data(), cbT.size(), bytes) || upload(&j->coarseT, cqT.data(), cqT.size(), bytes) ||
      upload(&j->ids, t->ids, (size_t)t->N, bytes) || upload(&j->codes, join_pad_codes(t->codes, t->N, m, j->MP).data(), (size_t)t->N * j->MP, bytes) ||
      upload(&j->cell, t->coarse_id, (size_t)t->N, bytes) || upload(&j->d_stats, t->stats, (size_t)j->cells + 1, bytes) ||
      (t->vectors && upload(&j->vectors, t->vectors, (size_t)t->N * t->d, bytes)))
    return join_fail(FREDDY_E_NOMEM, "device allocation failed while pinning the ivpq tables");
  j->h_ids.assign(t->ids, t->ids + t->N);
  j->h_cell.assign(t->coarse_id, t->coarse_id + t->N);
  j->h_stats.assign(t->stats, t->stats + j->cells + 1);
  if (dev_malloc((void**)&j->markbits, sizeof(uint32_t) * (size_t)((t->N + 31) / 32 + 1)) != hipSuccess)
    return join_fail(FREDDY_E_NOMEM, "device allocation failed while pinning the ivpq tables");
  j->ids_affine = t->N > 0 && (int64_t)t->ids[t->N - 1] - t->ids[0] == t->N - 1;   // strictly ascending => consecutive
  return 0;
}

extern "C" int freddy_gpu_pin_ivpq(const freddy_ivpq_desc* t, int device, freddy_gpu_index_t** out) {
  if (!t || !out || !t->codebook || !t->coarse || !t->stats || (t->N && (!t->ids || !t->codes || !t->coarse_id)))
    return fail(FREDDY_E_ARG, "NULL argument");
  if (t->d <= 0 || t->m <= 0 || t->K <= 0 || t->d % t->m) return fail(FREDDY_E_ARG, "bad d/m/K");
  if (t->coarse_positions != 2) return fail(FREDDY_E_LIMIT, "only 2 coarse positions are supported (as in the reference, index_utils.c:322)");
  if (t->coarse_codes <= 0 || t->d % 2) return fail(FREDDY_E_ARG, "bad coarse multi-index shape");
  freddy_gpu_index* ix = new freddy_gpu_index();
  ix->kind = KIND_IVPQ;
  ix->d = t->d; ix->m = t->m; ix->K = t->K; ix->S = t->d / t->m; ix->N = t->N;
  int rc = open_device(ix, device);
  if (!rc) {
    rc = join_pin(&ix->join, t, &ix->bytes);
    ix->join.host_traversal = env_int("FREDDY_GPU_JOIN_HOST_TRAVERSAL", 0) != 0;
    if (rc) rc = fail(rc, "%s", join_error());
  }
  if (rc) { free_index(ix); return rc; }
  *out = ix;
  return FREDDY_OK;
}

// ---------------------------------------------------------------------------------------
// kNN-join (ivpq_search_in): host loop in join_run.h
// ---------------------------------------------------------------------------------------
extern "C" int freddy_gpu_knn_join(freddy_gpu_index_t* ix, const float* queries, int32_t Q, int32_t k,
                                   const int32_t* target_ids, int64_t n_targets, int32_t alpha, int32_t pvf,
                                   int32_t method, int32_t use_target_lists, float confidence, int32_t double_threshold,
                                   int32_t* out_ids, float* out_dist, int32_t* iterations_out) {
  if (!ix) return fail(FREDDY_E_ARG, "NULL index");
  if (ix->kind != KIND_IVPQ) return fail(FREDDY_E_KIND, "index handle has the wrong kind for this call");
  if (int rc = refuse_poisoned(ix)) return rc;
  if (Q < 0 || k <= 0 || n_targets < 0) return fail(FREDDY_E_ARG, "bad sizes");
  if (Q > 0 && (!queries || !out_ids || !out_dist)) return fail(FREDDY_E_ARG, "NULL buffer");
  if (n_targets > 0 && !target_ids) return fail(FREDDY_E_ARG, "NULL target ids");
  HIP_TRY(hipSetDevice(ix->device));
  int rc = join_run(&ix->join, ix->stream, JoinQueries::of_host(queries), Q, k, target_ids, n_targets, alpha, pvf, method,
                    use_target_lists, confidence, double_threshold, out_ids, out_dist, iterations_out);
  if (rc) return fail(rc, "%s", join_error());
  return FREDDY_OK;
}

// ---- the kNN-join whose queries are on the device already (join_run.h JoinQueries) ---------------------------------------------------
// What freddy_gpu_knn_join refuses about its scalars, then what JoinRun::begin refuses about the shape of the call, with their messages.
int knn_join_check(const freddy_gpu_index* ivpq, int32_t k, const int32_t* target_ids, int64_t n_targets, int32_t alpha, int32_t pvf, int32_t method,
                   int32_t double_threshold) {
  if (k <= 0 || n_targets < 0) return fail(FREDDY_E_ARG, "bad sizes");
  if (n_targets > 0 && !target_ids) return fail(FREDDY_E_ARG, "NULL target ids");
  if (int rc = join_refusals(&ivpq->join, k, n_targets, alpha, pvf, method, double_threshold)) return fail(rc, "%s", join_error());
  return 0;
}

int join_query_block_for(freddy_gpu_index* ivpq, int Q, float** block) {
  if (join_query_block(&ivpq->join, Q, block)) return fail(FREDDY_E_NOMEM, "%s", join_error());
  return 0;
}

int knn_join_block(freddy_gpu_index* ivpq, int Q, int k, const int32_t* target_ids, int64_t n_targets, int alpha, int pvf, int method, int use_target_lists,
                   float confidence, int double_threshold, int32_t* out_ids, float* out_dist, int32_t* iterations_out) {
  HIP_TRY(hipSetDevice(ivpq->device));
  if (int rc = join_run(&ivpq->join, ivpq->stream, JoinQueries::of_block(), Q, k, target_ids, n_targets, alpha, pvf, method, use_target_lists, confidence,
                        double_threshold, out_ids, out_dist, iterations_out))
    return fail(rc, "%s", join_error());
  return FREDDY_OK;
}

// The queries are the rows of `vecs` (NULL: of the ivpq handle's own vectors) with these ids: the id rule on the host, the rows that
// have one compacted, their numbers to the device (4 bytes per query) and ONE join over them -- sub_dist_rows_kernel gathers the rows
// where freddy_gpu_knn_join's front pulls the caller's floats over PCIe.
extern "C" int freddy_gpu_knn_join_ids(freddy_gpu_index_t* ivpq, freddy_gpu_index_t* vecs, const int32_t* query_ids, int32_t n_ids, int32_t id_rule, int32_t k,
                                       const int32_t* target_ids, int64_t n_targets, int32_t alpha, int32_t pvf, int32_t method,
                                       int32_t use_target_lists, float confidence, int32_t double_threshold, int32_t* out_query_ids,
                                       int32_t* n_queries, int32_t* out_ids, float* out_dist, int32_t* iterations_out) {
  if (int rc = check_query_ids_front(ivpq, ivpq, query_ids, n_ids, id_rule, out_query_ids, n_queries, out_ids, out_dist)) return rc;
  if (int rc = knn_join_check(ivpq, k, target_ids, n_targets, alpha, pvf, method, double_threshold)) return rc;
  if (vecs) {
    if (int rc = check_ann_vecs(ivpq, KIND_IVPQ, vecs, "a kNN-join by row id")) return rc;
  } else {
    if (ivpq->kind != KIND_IVPQ) return fail(FREDDY_E_KIND, "index handle has the wrong kind for this call");
    if (int rc = refuse_poisoned(ivpq)) return rc;
    if (!ivpq->join.has_vectors)
      return fail(FREDDY_E_ARG, "this ivpq handle was pinned without vectors: a kNN-join by row id needs a vector handle to take its queries from");
  }
  JoinIndex& j = ivpq->join;
  const float* table = vecs ? vecs->coarse : j.vectors;
  const int64_t n_table = vecs ? vecs->N : j.N;
  if (iterations_out) *iterations_out = 0;
  return search_selected_rows(vecs ? vecs->h_ids : j.h_ids, query_ids, n_ids, id_rule, k, JOIN_MAX_DIST, out_query_ids, n_queries, out_ids, out_dist,
                              [&](const int32_t* rows, int n, int32_t* oi, float* od) {
    HIP_TRY(hipSetDevice(ivpq->device));
    if (int rc = join_run(&j, ivpq->stream, JoinQueries::of_rows(ivpq, table, n_table, rows), n, k, target_ids, n_targets, alpha, pvf, method,
                          use_target_lists, confidence, double_threshold, oi, od, iterations_out))
      return fail(rc, "%s", join_error());
    return (int)FREDDY_OK;
  });
}

// ---------------------------------------------------------------------------------------
// the statistics row of a pinned handle: set_statistics_table and create_statistics of the reference
// ---------------------------------------------------------------------------------------
// ids per pass of create_statistics: 16 MiB of pinned staging per half.  (freddy_amd/gpu.py keeps a copy, STAT_PASS, from which the
// tests build a list of one pass + 1 ids: change both together.)
static constexpr int64_t STAT_PASS = 1 << 22;
static constexpr int64_t STAT_ROWS_PASS = 1 << 30;   // rows per launch when every pinned row counts once (nothing is staged)

static int stat_handle(const freddy_gpu_index* ix) {
  if (!ix) return fail(FREDDY_E_ARG, "NULL index");
  if (ix->kind != KIND_IVPQ) return fail(FREDDY_E_KIND, "index handle has the wrong kind for this call");
  if (int rc = refuse_poisoned(ix)) return rc;
  return 0;
}

// d_stats first, h_stats only once the device holds the row: the two copies never disagree after a failure
static int stat_install(freddy_gpu_index* ix, const float* src, hipMemcpyKind kind, const float* host_row) {
  JoinIndex& j = ix->join;
  const size_t n = (size_t)j.cells + 1;
  HIP_TRY(hipMemcpyAsync(j.d_stats, src, sizeof(float) * n, kind, ix->stream));
  HIP_TRY(hipStreamSynchronize(ix->stream));
  j.h_stats.assign(host_row, host_row + n);
  return 0;
}

extern "C" int freddy_gpu_set_statistics(freddy_gpu_index_t* ix, const float* stats, int32_t n_stats) {
  if (int rc = stat_handle(ix)) return rc;
  if (n_stats != ix->join.cells + 1)
    return fail(FREDDY_E_ARG, "n_stats = %d: the statistics row of this index has cells + 1 = %d entries", n_stats, ix->join.cells + 1);
  if (!stats) return fail(FREDDY_E_ARG, "NULL statistics");
  HIP_TRY(hipSetDevice(ix->device));
  HIP_TRY(hipStreamSynchronize(ix->stream));
  return stat_install(ix, stats, hipMemcpyHostToDevice, stats);
}

extern "C" int freddy_gpu_get_statistics(const freddy_gpu_index_t* ix, float* out, int32_t n_stats) {
  if (int rc = stat_handle(ix)) return rc;
  if (n_stats != ix->join.cells + 1)
    return fail(FREDDY_E_ARG, "n_stats = %d: the statistics row of this index has cells + 1 = %d entries", n_stats, ix->join.cells + 1);
  if (!out) return fail(FREDDY_E_ARG, "NULL buffer");
  HIP_TRY(hipSetDevice(ix->device));
  HIP_TRY(hipMemcpyAsync(out, ix->join.d_stats, sizeof(float) * (size_t)n_stats, hipMemcpyDeviceToHost, ix->stream));
  HIP_TRY(hipStreamSynchronize(ix->stream));
  return FREDDY_OK;
}

// one launch of the count kernel over n entries: ids staged in mapped host memory (d_tids), or the rows [row0, row0 + n)
static int stat_count(freddy_gpu_index* ix, const int32_t* d_tids, int64_t n, int64_t row0, unsigned long long* d_count) {
  const JoinIndex& j = ix->join;
  const unsigned grid = (unsigned)std::min<int64_t>(std::max<int64_t>((n + STAT_WG * STAT_PER_LANE - 1) / (STAT_WG * STAT_PER_LANE), 1), STAT_MAX_GRID);
  if (j.cells <= STAT_LDS_CELLS)
    hipLaunchKernelGGL(stat_count_kernel<true>, dim3(grid), dim3(STAT_WG), sizeof(uint32_t) * (size_t)j.cells, ix->stream, d_tids, n, row0,
                       (const int32_t*)j.ids, j.N, j.ids_affine ? 1 : 0, (const int32_t*)j.cell, j.cells, d_count);
  else
    hipLaunchKernelGGL(stat_count_kernel<false>, dim3(grid), dim3(STAT_WG), 0, ix->stream, d_tids, n, row0, (const int32_t*)j.ids, j.N,
                       j.ids_affine ? 1 : 0, (const int32_t*)j.cell, j.cells, d_count);
  HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int freddy_gpu_create_statistics(freddy_gpu_index_t* ix, const int32_t* ids, int64_t n, int32_t install, float* out_stats,
                                            int64_t* matched) {
  if (int rc = stat_handle(ix)) return rc;
  if (n < 0 || (n > 0 && !ids)) return fail(FREDDY_E_ARG, "bad argument: n = %lld ids%s", (long long)n, ids ? "" : ", no ids");
  if (ids && n == 0) return fail(FREDDY_E_ARG, "an empty list of ids has no row: the total is 0 (the reference divides by it)");
  JoinIndex& j = ix->join;
  if (j.N == 0) return fail(FREDDY_E_ARG, "no row is pinned: the total is 0 (the reference divides by it)");
  const int cells = j.cells;
  const size_t row_n = (size_t)cells + 1;
  HIP_TRY(hipSetDevice(ix->device));
  HIP_TRY(hipStreamSynchronize(ix->stream));
  // device: the counts, then the row; pinned: the total, the row, then (ids given) one or two halves of a pass
  unsigned long long* d_count = nullptr;
  // (one block of u64: cells counts, then the row's cells + 1 floats, which fill ceil((cells + 1) / 2) <= row_n / 2 + 1 of them)
  if (join_buf(&j, JW_STAT, (size_t)cells + row_n / 2 + 1, &d_count)) return fail(FREDDY_E_NOMEM, "%s", join_error());
  float* d_row = reinterpret_cast<float*>(d_count + cells);
  const size_t head = (sizeof(unsigned long long) + sizeof(float) * row_n + 255) & ~(size_t)255;
  const int64_t pass = ids ? std::min(n, STAT_PASS) : 0;
  const int halves = n > pass ? 2 : 1;
  if (j.h_stat.ensure(head + sizeof(int32_t) * (size_t)pass * halves)) return fail(FREDDY_E_NOMEM, "pinned staging allocation failed");
  for (int h = 0; h < halves; ++h)
    if (ids && !j.ev_stat[h]) HIP_TRY(hipEventCreateWithFlags(&j.ev_stat[h], hipEventDisableTiming));
  void* p_dev = nullptr;
  HIP_TRY(hipHostGetDevicePointer(&p_dev, j.h_stat.p, 0));
  char* const h_base = j.h_stat.as<char>();
  char* const d_base = static_cast<char*>(p_dev);
  HIP_TRY(hipMemsetAsync(d_count, 0, sizeof(unsigned long long) * (size_t)cells, ix->stream));
  if (!ids) {
    for (int64_t r0 = 0; r0 < j.N; r0 += STAT_ROWS_PASS)
      if (int rc = stat_count(ix, nullptr, std::min(STAT_ROWS_PASS, j.N - r0), r0, d_count)) return rc;
  } else {
    int64_t p = 0;
    for (int64_t a = 0; a < n; a += pass, ++p) {   // the host fills one half while the kernel of the pass before reads the other
      const int h = (int)(p & 1);
      const int64_t len = std::min(pass, n - a);
      if (p >= 2) HIP_TRY(hipEventSynchronize(j.ev_stat[h]));
      const size_t off = head + sizeof(int32_t) * (size_t)pass * h;
      memcpy(h_base + off, ids + a, sizeof(int32_t) * (size_t)len);
      if (int rc = stat_count(ix, reinterpret_cast<const int32_t*>(d_base + off), len, 0, d_count)) return rc;
      HIP_TRY(hipEventRecord(j.ev_stat[h], ix->stream));
    }
  }
  hipLaunchKernelGGL(stat_finish_kernel, dim3(1), dim3(STAT_WG), 0, ix->stream, (const unsigned long long*)d_count, cells, d_row,
                     reinterpret_cast<float*>(d_base + sizeof(unsigned long long)), reinterpret_cast<unsigned long long*>(d_base));
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(ix->stream));
  const unsigned long long total = *reinterpret_cast<const unsigned long long*>(h_base);
  const float* h_row = reinterpret_cast<const float*>(h_base + sizeof(unsigned long long));
  if (total == 0) return fail(FREDDY_E_ARG, "none of the %lld ids has a pinned row: the total is 0 (the reference divides by it)", (long long)n);
  if (install)
    if (int rc = stat_install(ix, d_row, hipMemcpyDeviceToDevice, h_row)) return rc;
  if (out_stats) memcpy(out_stats, h_row, sizeof(float) * row_n);
  if (matched) *matched = (int64_t)total;
  return FREDDY_OK;
}

extern "C" int freddy_gpu_last_track(const freddy_gpu_index_t* ix, freddy_track* out) {
  if (!ix || !out) return fail(FREDDY_E_ARG, "NULL argument");
  if (ix->kind != KIND_IVPQ) return fail(FREDDY_E_KIND, "index handle has the wrong kind for this call");
  *out = ix->join.track;
  return FREDDY_OK;
}

extern "C" int freddy_gpu_last_track_sized(const freddy_gpu_index_t* ix, void* out, size_t out_size) {
  if (!ix || !out) return fail(FREDDY_E_ARG, "NULL argument");
  if (ix->kind != KIND_IVPQ) return fail(FREDDY_E_KIND, "index handle has the wrong kind for this call");
  const size_t n = std::min(out_size, sizeof(freddy_track));
  memcpy(out, &ix->join.track, n);
  return (int)n;
}

// The kernels of this unit that want more than the default 64 KiB of dynamic LDS.
std::vector<LdsLimit> lds_limits_join() {
  return {&join_query_kernel<1>, &join_query_kernel<2>, &join_query_kernel<4>, &join_query_kernel<8>, &join_query_kernel<16>,
          &join_query_kernel<16, true>,
          // (this unit's copy of the replay kernel: k = 4096 with its 8192 keys sorts 16384 slots)
          {&bigk_replay_kernel, (int)bigk_lds_bytes(16384, BIGK_KMAX)}};
}
