// cluster.hip -- the assignment step of cluster_exact on a raw-vector handle (freddy_gpu_exact_assign; assign.h) and the whole k-means
// of cluster_exact / cluster_pq in one call (freddy_gpu_cluster; cluster.h), which assigns through that step or through pq.hip's.
#include "internal.h"

#include "assign.h"
#include "cluster.h"

// ---- the assignment step of cluster_exact (assign.h) ----------------------------------------------------------------------
// Targets per pass: the ids go up and the two result arrays come back through workspace buffers of this many entries.
static constexpr int64_t AS_PASS = (int64_t)1 << 22;

// One pass of n targets with everything on the device, enqueued on s (freddy_gpu_exact_assign and freddy_gpu_cluster share it).
static int exact_assign_pass(freddy_gpu_index* ix, hipStream_t s, const float* d_queries, int Q, const int32_t* d_targets, int n, int32_t* d_best,
                             float* d_sim) {
  AssignExactArgs aa;
  aa.targets = d_targets; aa.vec_ids = ix->ids; aa.rows = ix->coarse; aa.queries = d_queries;
  aa.out_query = d_best; aa.out_sim = d_sim; aa.N = ix->N; aa.n_targets = n; aa.Q = Q; aa.d = ix->d;
  timed_launch(ix, s, "assign_exact_kernel", [&] { hipLaunchKernelGGL(assign_exact_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, aa); });
  HIP_TRY(hipGetLastError());
  return FREDDY_OK;
}

extern "C" int freddy_gpu_exact_assign(freddy_gpu_index_t* ix, const float* queries, int32_t Q, const int32_t* target_ids, int64_t n_targets,
                                       int32_t* out_query, float* out_sim) {
  // (the scalar arguments first: they are checked before the handle is looked at, so no device is needed to see these errors)
  if (Q < 0 || n_targets < 0) return fail(FREDDY_E_ARG, "bad sizes (Q=%d, n_targets=%lld)", Q, (long long)n_targets);
  if (Q > 0 && n_targets > 0 && (!queries || !target_ids || !out_query || !out_sim)) return fail(FREDDY_E_ARG, "NULL buffer");
  if (Q > AS_MAX_Q) return fail(FREDDY_E_LIMIT, "Q=%d exceeds this build's limit of %d queries per assign call", Q, AS_MAX_Q);
  if (int rc = check_vec_handle(ix)) return rc;
  if (Q == 0 || n_targets == 0) return FREDDY_OK;
  HIP_TRY(hipSetDevice(ix->device));
  Workspace* ws = workspace_for(ix, ix->stream);
  hipStream_t s = ix->stream;
  const int d = ix->d;
  const int64_t pass = std::min(AS_PASS, n_targets);
  if (ws->w_q.ensure(sizeof(float) * (size_t)Q * d) || ws->w_sub_rows.ensure(sizeof(int32_t) * (size_t)pass) ||
      ws->w_out_ids.ensure(sizeof(int32_t) * (size_t)pass) || ws->w_out_dist.ensure(sizeof(float) * (size_t)pass))
    return fail(FREDDY_E_NOMEM, "workspace allocation failed");
  HIP_TRY(hipMemcpyAsync(ws->w_q.p, queries, sizeof(float) * (size_t)Q * d, hipMemcpyHostToDevice, s));
  for (int64_t t0 = 0; t0 < n_targets; t0 += pass) {
    const int n = (int)std::min(pass, n_targets - t0);
    HIP_TRY(hipMemcpyAsync(ws->w_sub_rows.p, target_ids + t0, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, s));
    if (int rc = exact_assign_pass(ix, s, ws->w_q.as<float>(), Q, ws->w_sub_rows.as<int32_t>(), n, ws->w_out_ids.as<int32_t>(), ws->w_out_dist.as<float>())) return rc;
    HIP_TRY(hipMemcpyAsync(out_query + t0, ws->w_out_ids.p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(out_sim + t0, ws->w_out_dist.p, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));   // (the next pass overwrites the three buffers)
  }
  return FREDDY_OK;
}

// ---- the whole k-means of cluster_exact / cluster_pq (cluster.h) ---------------------------------------------------------------
// Everything is enqueued on the vector handle's stream and nothing waits for the device between the rounds: ids and draws go up,
// the kernels of all rounds follow, the unknown-id word comes down behind them, and only a call that word clears copies its outputs.
static constexpr int64_t CL_PASS = (int64_t)1 << 22;   // targets per assignment pass (option cluster_pass)

extern "C" int freddy_gpu_cluster(freddy_gpu_index_t* vecs, freddy_gpu_index_t* pq, float sentinel, const int32_t* token_ids, int64_t n, int32_t kc,
                                  int32_t rounds, const double* draws, int64_t n_draws, int32_t* out_cluster, float* out_sim, float* out_centroids) {
  // (the scalar arguments first: they are checked before a handle is looked at, so no device is needed to see these errors)
  if (n <= 0 || kc <= 0 || rounds <= 0) return fail(FREDDY_E_ARG, "bad sizes (n=%lld, kc=%d, rounds=%d)", (long long)n, kc, rounds);
  if (!token_ids || !draws || !out_cluster) return fail(FREDDY_E_ARG, "NULL buffer");
  if (kc > AS_MAX_Q) return fail(FREDDY_E_LIMIT, "kc=%d exceeds this build's limit of %d clusters", kc, AS_MAX_Q);
  if (n > (int64_t)INT32_MAX) return fail(FREDDY_E_LIMIT, "n=%lld exceeds this build's limit of %d tokens per cluster call", (long long)n, INT32_MAX);
  const int64_t need = (int64_t)kc + (int64_t)CL_SAMPLES * kc * ((int64_t)rounds - 1);
  if (n_draws < need) return fail(FREDDY_E_ARG, "n_draws=%lld, but kc=%d clusters over %d rounds take %lld draws", (long long)n_draws, kc, rounds, (long long)need);
  for (int64_t i = 0; i < need; ++i)
    if (draws[i] != draws[i]) return fail(FREDDY_E_ARG, "draw %lld is not a number", (long long)i);
  if (pq && !(sentinel <= 16777216.0f)) return fail(FREDDY_E_ARG, "sentinel=%g is not a number or above 2^24, the range the similarity of a distance is defined for", (double)sentinel);
  if (!vecs) return fail(FREDDY_E_ARG, "NULL index");
  if (vecs->kind != KIND_VEC || (pq && pq->kind != KIND_PQ)) return fail(FREDDY_E_KIND, "index handle has the wrong kind for this call");
  if (int rc = refuse_poisoned(vecs)) return rc;
  if (pq) {
    if (int rc = refuse_poisoned(pq)) return rc;
    if (pq->device != vecs->device) return fail(FREDDY_E_ARG, "the two handles are pinned on different devices (%d and %d)", vecs->device, pq->device);
    if (pq->d != vecs->d) return fail(FREDDY_E_ARG, "the two tables have different dimensions (%d and %d)", vecs->d, pq->d);
  }
  HIP_TRY(hipSetDevice(vecs->device));
  hipStream_t s = vecs->stream;
  Workspace* ws = workspace_for(vecs, s);
  Workspace* wpq = pq ? workspace_for(pq, s) : nullptr;
  const int d = vecs->d, nn = (int)n;
  const int64_t pass = std::min<int64_t>(vecs->tune.cluster_pass > 0 ? vecs->tune.cluster_pass : CL_PASS, n);
  const int Qc = pq ? pq_assign_lut_queries(pq, kc) : 0;
  const size_t head = 64;   // bytes in front of lens[]: the unknown-id word
  const int n_blk = (int)((n + CL_STEP - 1) / CL_STEP);
  // the sample kernel walks only the steps its ranks fall into: from 16 steps on (below, the sum over the block counts costs what it saves)
  const bool two_level = kc <= CL_HIST && rounds > 1 && (vecs->tune.cluster_walk == 2 || (vecs->tune.cluster_walk == 0 && n_blk > 16));
  if (ws->w_sub_rows.ensure(sizeof(int32_t) * (size_t)n) || ws->w_rows.ensure(sizeof(int32_t) * (size_t)n) || ws->w_cand.ensure(sizeof(int32_t) * (size_t)n) ||
      ws->w_out_ids.ensure(sizeof(int32_t) * (size_t)n) || ws->w_out_dist.ensure(sizeof(float) * (size_t)n) ||
      ws->w_q.ensure(sizeof(float) * (size_t)kc * d) || ws->w_cnt.ensure(head + sizeof(int32_t) * (size_t)kc) || ws->w_qc.ensure(sizeof(double) * (size_t)need) ||
      (two_level && ws->w_cellcnt.ensure(sizeof(int32_t) * (size_t)kc * n_blk)) ||
      (pq && (ws->w_found.ensure(sizeof(float) * (size_t)n) || wpq->w_lut.ensure((size_t)pq->m * pq->K * sizeof(float) * (size_t)Qc))))
    return fail(FREDDY_E_NOMEM, "workspace allocation failed");
  int32_t* d_ids = ws->w_sub_rows.as<int32_t>();
  int32_t* d_row = ws->w_rows.as<int32_t>();
  int32_t* d_clusters = ws->w_cand.as<int32_t>();
  int32_t* d_best = ws->w_out_ids.as<int32_t>();
  float* d_sim = ws->w_out_dist.as<float>();
  float* d_cent = ws->w_q.as<float>();
  uint32_t* d_flag = ws->w_cnt.as<uint32_t>();
  int32_t* d_lens = reinterpret_cast<int32_t*>(ws->w_cnt.as<char>() + head);
  double* d_draws = ws->w_qc.as<double>();
  HIP_TRY(hipMemcpyAsync(d_ids, token_ids, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(d_draws, draws, sizeof(double) * (size_t)need, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemsetAsync(d_flag, 0xff, sizeof(uint32_t), s));   // CL_NO_FLAG
  {
    ClusterInitArgs ia;
    ia.token_ids = d_ids; ia.vec_ids = vecs->ids; ia.rows = vecs->coarse; ia.draws = d_draws; ia.row_of = d_row; ia.clusters = d_clusters; ia.lens = d_lens;
    ia.centroids = d_cent; ia.flag = d_flag; ia.N = vecs->N; ia.n = nn; ia.kc = kc; ia.d = d; ia.pos_blocks = (unsigned)((n + CL_WG - 1) / CL_WG);
    timed_launch(vecs, s, "cluster_init_kernel", [&] { hipLaunchKernelGGL(cluster_init_kernel, dim3(ia.pos_blocks + (unsigned)kc), dim3(CL_WG), 0, s, ia); });
    HIP_TRY(hipGetLastError());
  }
  for (int J = 1; J <= rounds; ++J) {
    int lut_q0 = -1;   // (new centroids: no LUT of the round before is theirs)
    for (int64_t t0 = 0; t0 < n; t0 += pass) {
      const int np = (int)std::min(pass, n - t0);
      if (pq) {
        if (int rc = pq_assign_pass(pq, s, wpq->w_lut.as<float>(), Qc, &lut_q0, d_cent, kc, sentinel, d_ids + t0, np, d_best + t0, d_sim + t0, ws->w_found.as<float>() + t0)) return rc;
      } else {
        if (int rc = exact_assign_pass(vecs, s, d_cent, kc, d_ids + t0, np, d_best + t0, d_sim + t0)) return rc;
      }
    }
    ClusterApplyArgs pa;
    pa.best = d_best; pa.clusters = d_clusters; pa.lens = d_lens; pa.n = nn; pa.kc = kc; pa.n_blk = n_blk;
    pa.blk_members = two_level && J < rounds ? ws->w_cellcnt.as<int32_t>() : nullptr;
    timed_launch(vecs, s, "cluster_apply_kernel", [&] { hipLaunchKernelGGL(cluster_apply_kernel, dim3((unsigned)n_blk), dim3(CL_WG), 0, s, pa); });
    HIP_TRY(hipGetLastError());
    if (J == rounds) break;
    ClusterSampleArgs sa;
    sa.clusters = d_clusters; sa.row_of = d_row; sa.rows = vecs->coarse; sa.draws = d_draws + kc + (size_t)(J - 1) * kc * CL_SAMPLES; sa.lens = d_lens;
    sa.centroids = d_cent; sa.n = nn; sa.d = d; sa.n_blk = n_blk; sa.blk_members = pa.blk_members;
    timed_launch(vecs, s, "cluster_sample_kernel", [&] { hipLaunchKernelGGL(cluster_sample_kernel, dim3((unsigned)kc), dim3(CL_WG), 0, s, sa); });
    HIP_TRY(hipGetLastError());
  }
  uint32_t unknown = CL_NO_FLAG;
  HIP_TRY(hipMemcpyAsync(&unknown, d_flag, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (unknown != CL_NO_FLAG) return fail(FREDDY_E_ARG, "token id %d has no vector", token_ids[unknown]);   // (the first such position; nothing was written)
  HIP_TRY(hipMemcpyAsync(out_cluster, d_clusters, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, s));
  if (out_sim) HIP_TRY(hipMemcpyAsync(out_sim, d_sim, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, s));
  if (out_centroids) HIP_TRY(hipMemcpyAsync(out_centroids, d_cent, sizeof(float) * (size_t)kc * d, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return FREDDY_OK;
}
