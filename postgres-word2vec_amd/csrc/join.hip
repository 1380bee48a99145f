// join.hip -- pin_ivpq and knn_join (ivpq_search_in.c:61-699): the entry points.  join.h says which header holds what; the
// call itself is join_run() in join_run.h.
#include "internal.h"

#include "join.h"
#include "join_run.h"

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
  if (hipMalloc((void**)&j->markbits, sizeof(uint32_t) * (size_t)((t->N + 31) / 32 + 1)) != hipSuccess)
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
  if (Q < 0 || k <= 0 || n_targets < 0) return fail(FREDDY_E_ARG, "bad sizes");
  if (Q > 0 && (!queries || !out_ids || !out_dist)) return fail(FREDDY_E_ARG, "NULL buffer");
  if (n_targets > 0 && !target_ids) return fail(FREDDY_E_ARG, "NULL target ids");
  HIP_TRY(hipSetDevice(ix->device));
  int rc = join_run(&ix->join, ix->stream, queries, Q, k, target_ids, n_targets, alpha, pvf, method,
                    use_target_lists, confidence, double_threshold, out_ids, out_dist, iterations_out);
  if (rc) return fail(rc, "%s", join_error());
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
