// rerank.hip -- lists of a pq / ivf / ivpq handle re-ranked by exact similarity against a raw-vector handle: the post verification of
// pq / ivf lists (pv.h; also for queries named by row id, query_ids.h) and the approximate analogies over such lists
// (approx_analogy.h).  Stage one of each is a search of another unit, through its public entry point or its *_src form.
#include "internal.h"

#include "pv.h"
#include "approx_analogy.h"
#include "query_ids.h"

// ---- the re-rank stage of post verification and the approximate analogies (pv.h, approx_analogy.h) ----------------------------
// Queries (triples) per pass: stage one's lists of `n_cand` entries hold at most 8 M entries
static int rerank_pass(int64_t n, int n_cand) { return (int)std::min<int64_t>(n, std::max<int64_t>(1, ((int64_t)8 << 20) / n_cand)); }

// The pinned block of one pass of Qc queries: [stage one's lists][the result lists][per-query counts]; the approximate analogies put
// their unit rows (padded to 16 bytes) in front and the input rows and ids behind.
struct RerankBlock {
  float *unit, *l_dist, *o_sim;
  int32_t *l_ids, *o_ids, *o_cnt, *p_rows, *p_excl;
};
static int rerank_block(freddy_gpu_index* ann, int Qc, int n_cand, int k, bool analogy, const char* call, RerankBlock* b) {
  const int d = ann->d;
  const size_t n_unit = analogy ? ((size_t)Qc * d + 3) / 4 * 4 : 0, n_list = (size_t)Qc * n_cand, n_out = (size_t)Qc * k;
  if (ann->pv_io.ensure(4 * (n_unit + 2 * n_list + 2 * n_out + 2 * (size_t)Qc + (analogy ? 6 * (size_t)Qc : 0))) || ann->pv_q.ensure(sizeof(float) * (size_t)Qc * d))
    return fail(FREDDY_E_NOMEM, "%s: staging allocation failed", call);
  b->unit = ann->pv_io.as<float>();
  b->l_ids = reinterpret_cast<int32_t*>(b->unit + n_unit); b->l_dist = reinterpret_cast<float*>(b->l_ids + n_list);
  b->o_ids = b->l_ids + 2 * n_list; b->o_sim = reinterpret_cast<float*>(b->o_ids + n_out);
  b->o_cnt = b->o_ids + 2 * n_out;
  b->p_rows = b->o_cnt + 2 * (size_t)Qc; b->p_excl = b->p_rows + 3 * (size_t)Qc;
  return 0;
}
// The re-rank of `nq` lists of the block against the raw queries in pv_q, by pv_rerank_kernel<NW> or aa_rerank_kernel<NW> (which
// leaves out the ids at `exclude`): k1 = <1>, one wave per query, for lists of up to 64 entries, k4 = <4> beyond.
using RerankKernel = void (*)(PvArgs);
static int launch_rerank(freddy_gpu_index* ann, const freddy_gpu_index* vecs, hipStream_t s, const char* label, RerankKernel k1, RerankKernel k4,
                         const RerankBlock& b, const int32_t* exclude, int nq, int n_cand, int k) {
  const int d = ann->d, P = pv_pad(n_cand);
  PvArgs pa;
  pa.cand = b.l_ids; pa.vec_ids = vecs->ids; pa.rows = vecs->coarse; pa.queries = ann->pv_q.as<float>(); pa.exclude = exclude; pa.out_ids = b.o_ids;
  pa.out_sim = b.o_sim; pa.counts = b.o_cnt; pa.N = vecs->N; pa.n_cand = n_cand; pa.k = k; pa.d = d; pa.P = P;
  timed_launch(ann, s, label, [&] {
    if (P == 64) hipLaunchKernelGGL(k1, dim3((unsigned)nq), dim3(64), pv_lds_bytes(1, P, d), s, pa);
    else hipLaunchKernelGGL(k4, dim3((unsigned)nq), dim3(256), pv_lds_bytes(4, P, d), s, pa);
  });
  HIP_TRY(hipGetLastError());
  return 0;
}

// ---- post verification of pq / ivf result lists (pv.h) -------------------------------------------------------------------
// The handles of a call that takes a pq / ivf handle and the raw-vector handle it re-ranks against (post verification, approximate
// analogies): check_ann_vecs (query_ids.h, which the searches by id share); nothing there touches a device.
static int pv_check_handles(const freddy_gpu_index* ann, int kind, const freddy_gpu_index* vecs, const char* what) { return check_ann_vecs(ann, kind, vecs, what); }

// The scalar refusals of post verification, each with its one message (the host-vector entry points and the ones by row id;
// pv_check_subset: internal.h)
static int pv_check_count(int32_t Q, int32_t k, int32_t pvf) { return (Q < 0 || k < 1 || pvf < 1) ? fail(FREDDY_E_ARG, "bad sizes (Q=%d, k=%d, pvf=%d)", Q, k, pvf) : 0; }
static int pv_check_limit(int32_t k, int32_t pvf) {
  return (int64_t)k * pvf > PV_MAX_CAND ? fail(FREDDY_E_LIMIT, "k * pvf = %lld exceeds this build's limit of %d candidates", (long long)k * pvf, PV_MAX_CAND) : 0;
}
// Everything both entry points refuse, in the order of the header's table; nothing here touches a device.
static int pv_check(const freddy_gpu_index* ann, int kind, const freddy_gpu_index* vecs, const float* queries, int32_t Q, int32_t k, int32_t pvf,
                    const int32_t* out_ids, const float* out_sim) {
  if (int rc = pv_check_count(Q, k, pvf)) return rc;
  if (Q > 0 && (!queries || !out_ids || !out_sim)) return fail(FREDDY_E_ARG, "NULL buffer");
  if (int rc = pv_check_limit(k, pvf)) return rc;
  return pv_check_handles(ann, kind, vecs, "post verification");
}

// Stage one (`search`: the public entry point at k * pvf, writing its lists into the pinned block) and stage two (pv_rerank) for
// passes of queries that bound the pinned block; the kernel reads the lists where stage one left them and writes the result lists
// and the counts beside them, one synchronisation per pass.
template <class F>
static int pv_search(freddy_gpu_index* ann, freddy_gpu_index* vecs, const QuerySrc& queries, int32_t Q, int32_t k, int32_t pvf, int32_t* out_ids,
                     float* out_sim, F&& search) {
  ann->pv_stats[0] = ann->pv_stats[1] = 0;
  if (Q == 0) return FREDDY_OK;
  const int kc = k * pvf, d = ann->d;
  const int Qc = rerank_pass(Q, kc);
  HIP_TRY(hipSetDevice(ann->device));
  RerankBlock b;
  if (int rc = rerank_block(ann, Qc, kc, k, false, "post verification", &b)) return rc;
  hipStream_t s = ann->stream;
  for (int q0 = 0; q0 < Q; q0 += Qc) {
    const int nq = std::min(Qc, Q - q0);
    const QuerySrc qp = queries.from((size_t)q0, d);
    if (int rc = search(qp, nq, kc, b.l_ids, b.l_dist)) return rc;
    HIP_TRY(hipSetDevice(ann->device));
    if (qp.host) {
      HIP_TRY(hipMemcpyAsync(ann->pv_q.p, qp.host, sizeof(float) * (size_t)nq * d, hipMemcpyHostToDevice, s));
    } else {
      // queries by row id (query_ids.h): the raw queries are rows of `vecs` -- gathered, by row numbers staged in the handle's pinned
      // block (stage one has returned: the block is free)
      if (ann->hio_in.ensure(sizeof(int32_t) * (size_t)nq)) return fail(FREDDY_E_NOMEM, "pinned staging allocation failed");
      memcpy(ann->hio_in.p, qp.rows, sizeof(int32_t) * (size_t)nq);
      if (int rc = launch_query_gather(ann, s, qp, ann->hio_in.as<const int32_t>(), ann->pv_q.as<float>(), nq, d)) return rc;
    }
    if (int rc = launch_rerank(ann, vecs, s, "pv_rerank", pv_rerank_kernel<1>, pv_rerank_kernel<4>, b, nullptr, nq, kc, k)) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    memcpy(out_ids + (size_t)q0 * k, b.o_ids, sizeof(int32_t) * (size_t)nq * k);
    memcpy(out_sim + (size_t)q0 * k, b.o_sim, sizeof(float) * (size_t)nq * k);
    for (int q = 0; q < nq; ++q) { ann->pv_stats[0] += b.o_cnt[2 * q]; ann->pv_stats[1] += b.o_cnt[2 * q + 1]; }
  }
  return FREDDY_OK;
}

extern "C" int freddy_gpu_ivfadc_search_pv(freddy_gpu_index_t* ivf, freddy_gpu_index_t* vecs, const float* queries, int32_t Q, int32_t k, int32_t pvf,
                                           int32_t W, float sentinel, int32_t found_rule, int32_t* out_ids, float* out_sim) {
  if (int rc = pv_check(ivf, KIND_IVF, vecs, queries, Q, k, pvf, out_ids, out_sim)) return rc;
  if (int rc = check_probe_args(W, found_rule)) return rc;
  return pv_search(ivf, vecs, QuerySrc::of_host(queries), Q, k, pvf, out_ids, out_sim, [&](const QuerySrc& qp, int nq, int kc, int32_t* l_ids, float* l_dist) {
    return freddy_gpu_ivfadc_search(ivf, qp.host, nq, kc, W, sentinel, found_rule, l_ids, l_dist);
  });
}

extern "C" int freddy_gpu_pq_search_pv(freddy_gpu_index_t* pq, freddy_gpu_index_t* vecs, const float* queries, int32_t Q, int32_t k, int32_t pvf,
                                       float sentinel, const int32_t* subset_ids, int64_t n_subset, int32_t* out_ids, float* out_sim) {
  if (int rc = pv_check_subset(subset_ids, n_subset)) return rc;
  if (int rc = pv_check(pq, KIND_PQ, vecs, queries, Q, k, pvf, out_ids, out_sim)) return rc;
  return pv_search(pq, vecs, QuerySrc::of_host(queries), Q, k, pvf, out_ids, out_sim, [&](const QuerySrc& qp, int nq, int kc, int32_t* l_ids, float* l_dist) {
    return freddy_gpu_pq_search(pq, qp.host, nq, kc, sentinel, subset_ids, n_subset, l_ids, l_dist);
  });
}

// Post verification of queries named by row id (query_ids.h): stage one is the search by id's body (ivfadc_search_src / pq_search_src
// at k * pvf), the raw queries of stage two are gathered from `vecs`.  The counts of freddy_gpu_last_pv_stats cover the searched slots.
extern "C" int freddy_gpu_ivfadc_search_pv_ids(freddy_gpu_index_t* ivf, freddy_gpu_index_t* vecs, const int32_t* query_ids, int32_t n_ids, int32_t id_rule,
                                               int32_t k, int32_t pvf, int32_t W, float sentinel, int32_t found_rule, int32_t* out_query_ids,
                                               int32_t* n_queries, int32_t* out_ids, float* out_sim) {
  if (int rc = check_query_ids_front(ivf, vecs, query_ids, n_ids, id_rule, out_query_ids, n_queries, out_ids, out_sim)) return rc;
  if (int rc = pv_check_count(n_ids, k, pvf)) return rc;
  if (int rc = pv_check_limit(k, pvf)) return rc;
  if (int rc = check_probe_args(W, found_rule)) return rc;
  if (int rc = check_ann_vecs(ivf, KIND_IVF, vecs, "a search by row id")) return rc;
  if (W > ivf->C) W = ivf->C;
  ivf->pv_stats[0] = ivf->pv_stats[1] = 0;
  return search_selected_ids(vecs, query_ids, n_ids, id_rule, k, -HUGE_VALF, out_query_ids, n_queries, out_ids, out_sim,
                             [&](const QuerySrc& qs, int n, int32_t* oi, float* os) {
    return pv_search(ivf, vecs, qs, n, k, pvf, oi, os, [&](const QuerySrc& qp, int nq, int kc, int32_t* l_ids, float* l_dist) {
      return ivfadc_search_src(ivf, qp, nq, kc, W, sentinel, found_rule, l_ids, l_dist);
    });
  });
}

extern "C" int freddy_gpu_pq_search_pv_ids(freddy_gpu_index_t* pq, freddy_gpu_index_t* vecs, const int32_t* query_ids, int32_t n_ids, int32_t id_rule,
                                           int32_t k, int32_t pvf, float sentinel, const int32_t* subset_ids, int64_t n_subset, int32_t* out_query_ids,
                                           int32_t* n_queries, int32_t* out_ids, float* out_sim) {
  if (int rc = check_query_ids_front(pq, vecs, query_ids, n_ids, id_rule, out_query_ids, n_queries, out_ids, out_sim)) return rc;
  if (int rc = pv_check_subset(subset_ids, n_subset)) return rc;
  if (int rc = pv_check_count(n_ids, k, pvf)) return rc;
  if (int rc = pv_check_limit(k, pvf)) return rc;
  if (int rc = check_ann_vecs(pq, KIND_PQ, vecs, "a search by row id")) return rc;
  pq->pv_stats[0] = pq->pv_stats[1] = 0;
  return search_selected_ids(vecs, query_ids, n_ids, id_rule, k, -HUGE_VALF, out_query_ids, n_queries, out_ids, out_sim,
                             [&](const QuerySrc& qs, int n, int32_t* oi, float* os) {
    return pv_search(pq, vecs, qs, n, k, pvf, oi, os, [&](const QuerySrc& qp, int nq, int kc, int32_t* l_ids, float* l_dist) {
      return pq_search_src(pq, qp, nq, kc, sentinel, subset_ids, n_subset, l_ids, l_dist);
    });
  });
}

extern "C" int freddy_gpu_last_pv_stats(const freddy_gpu_index_t* ann, int64_t* candidates, int64_t* scored) {
  if (!ann) return fail(FREDDY_E_ARG, "NULL index");
  if (ann->kind != KIND_PQ && ann->kind != KIND_IVF) return fail(FREDDY_E_KIND, "index handle has the wrong kind for this call");
  if (candidates) *candidates = ann->pv_stats[0];
  if (scored) *scored = ann->pv_stats[1];
  return FREDDY_OK;
}

// ---- approximate analogies: 3CosAdd over the candidates of pq / ivf lists (approx_analogy.h) ---------------------------------------
// Everything both entry points refuse, scalars before handles; nothing here touches a device.
static int aa_check_scalars(const int32_t* triples, int32_t Q, int32_t k, int32_t n_cand, const int32_t* out_ids, const float* out_sim) {
  if (Q < 0 || k < 1 || n_cand < k) return fail(FREDDY_E_ARG, "bad sizes (Q=%d, k=%d, n_cand=%d)", Q, k, n_cand);
  if (Q > 0 && (!triples || !out_ids || !out_sim)) return fail(FREDDY_E_ARG, "NULL buffer");
  if (n_cand > PV_MAX_CAND) return fail(FREDDY_E_LIMIT, "n_cand = %d exceeds this build's limit of %d candidates", n_cand, PV_MAX_CAND);
  return 0;
}
static int aa_check(const freddy_gpu_index* ann, int kind, const freddy_gpu_index* vecs, const int32_t* triples, int32_t Q, int32_t k, int32_t n_cand,
                    const int32_t* out_ids, const float* out_sim) {
  if (int rc = aa_check_scalars(triples, Q, k, n_cand, out_ids, out_sim)) return rc;
  return pv_check_handles(ann, kind, vecs, "the approximate analogy");
}

// The triples whose three ids have a row, compacted, in passes that bound the pinned block as pv_search's do: aa_query writes a
// pass's raw rows to device memory and its unit rows into the pinned block, stage one (`search`: the public entry point at n_cand,
// reading its queries from that block and writing its lists into it) runs once the kernel has finished, and the re-rank scores the
// lists against the raw rows without the inputs; the result rows are scattered back to their triples.
// unit_block (the ivpq form): `block(Qc, &p)` names device memory for a pass's unit rows instead of the pinned block -- the kNN-join's
// query block, which stage one reads in stream order: aa_query is not waited for, and the unit rows never reach the host.
static int aa_pinned_units(int, float** block) { *block = nullptr; return 0; }   // (the pq / ivf forms: the pinned block's unit rows)
template <class F, class B>
static int aa_search(freddy_gpu_index* ann, freddy_gpu_index* vecs, const int32_t* triples, int32_t Q, int32_t k, int32_t n_cand, int32_t* out_ids,
                     float* out_sim, F&& search, B&& unit_block) {
  ann->aa_stats[0] = ann->aa_stats[1] = ann->aa_stats[2] = 0;
  for (size_t i = 0; i < (size_t)Q * k; ++i) { out_ids[i] = -1; out_sim[i] = -HUGE_VALF; }
  std::vector<int32_t> live, rows3, ids3;
  resolve_triples(vecs->h_ids, triples, Q, live, rows3, &ids3);
  const int na = (int)live.size();
  if (na == 0) return FREDDY_OK;   // (before any launch)
  const int d = ann->d;
  int Qc = rerank_pass(na, n_cand);   // triples per pass
  if (ann->tune.analogy_pass > 0) Qc = std::min(Qc, ann->tune.analogy_pass);
  HIP_TRY(hipSetDevice(ann->device));
  RerankBlock b;
  if (int rc = rerank_block(ann, Qc, n_cand, k, true, "approximate analogy", &b)) return rc;
  float* d_unit = nullptr;
  if (int rc = unit_block(Qc, &d_unit)) return rc;
  hipStream_t s = ann->stream;
  for (int q0 = 0; q0 < na; q0 += Qc) {
    const int nq = std::min(Qc, na - q0);
    memcpy(b.p_rows, rows3.data() + (size_t)q0 * 3, sizeof(int32_t) * 3 * (size_t)nq);
    memcpy(b.p_excl, ids3.data() + (size_t)q0 * 3, sizeof(int32_t) * 3 * (size_t)nq);
    AaQueryArgs qa;
    qa.rows = vecs->coarse; qa.in_rows = b.p_rows; qa.raw = ann->pv_q.as<float>(); qa.unit = d_unit ? d_unit : b.unit; qa.d = d;
    timed_launch(ann, s, "aa_query", [&] { hipLaunchKernelGGL(aa_query_kernel, dim3((unsigned)nq), dim3(64), aa_query_lds(d), s, qa); });
    HIP_TRY(hipGetLastError());
    if (!d_unit) HIP_TRY(hipStreamSynchronize(s));   // (stage one reads the unit rows on streams of its own)
    if (int rc = search(qa.unit, nq, b.l_ids, b.l_dist)) return rc;
    HIP_TRY(hipSetDevice(ann->device));
    if (int rc = launch_rerank(ann, vecs, s, "aa_rerank", aa_rerank_kernel<1>, aa_rerank_kernel<4>, b, b.p_excl, nq, n_cand, k)) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    for (int q = 0; q < nq; ++q) {
      memcpy(out_ids + (size_t)live[(size_t)q0 + q] * k, b.o_ids + (size_t)q * k, sizeof(int32_t) * k);
      memcpy(out_sim + (size_t)live[(size_t)q0 + q] * k, b.o_sim + (size_t)q * k, sizeof(float) * k);
      ann->aa_stats[1] += b.o_cnt[2 * q]; ann->aa_stats[2] += b.o_cnt[2 * q + 1];
    }
    ann->aa_stats[0] += nq;
  }
  return FREDDY_OK;
}

extern "C" int freddy_gpu_ivfadc_analogy(freddy_gpu_index_t* ivf, freddy_gpu_index_t* vecs, const int32_t* triples, int32_t Q, int32_t k, int32_t n_cand,
                                         int32_t W, float sentinel, int32_t found_rule, int32_t* out_ids, float* out_sim) {
  if (int rc = check_probe_args(W, found_rule)) return rc;
  if (int rc = aa_check(ivf, KIND_IVF, vecs, triples, Q, k, n_cand, out_ids, out_sim)) return rc;
  return aa_search(ivf, vecs, triples, Q, k, n_cand, out_ids, out_sim, [&](const float* qp, int nq, int32_t* l_ids, float* l_dist) {
    return freddy_gpu_ivfadc_search(ivf, qp, nq, n_cand, W, sentinel, found_rule, l_ids, l_dist);
  }, aa_pinned_units);
}

extern "C" int freddy_gpu_pq_analogy(freddy_gpu_index_t* pq, freddy_gpu_index_t* vecs, const int32_t* triples, int32_t Q, int32_t k, int32_t n_cand,
                                     float sentinel, const int32_t* subset_ids, int64_t n_subset, int32_t* out_ids, float* out_sim) {
  if (int rc = pv_check_subset(subset_ids, n_subset)) return rc;
  if (int rc = aa_check(pq, KIND_PQ, vecs, triples, Q, k, n_cand, out_ids, out_sim)) return rc;
  return aa_search(pq, vecs, triples, Q, k, n_cand, out_ids, out_sim, [&](const float* qp, int nq, int32_t* l_ids, float* l_dist) {
    return freddy_gpu_pq_search(pq, qp, nq, n_cand, sentinel, subset_ids, n_subset, l_ids, l_dist);
  }, aa_pinned_units);
}

// analogy_3cosadd_in_ivpq (freddy--0.0.1.sql:1383-1425) for a batch of triples: stage one is ONE kNN-join per pass at k = n_cand (the
// reference's literal 4) over the unit rows of the pass's live triples, which aa_query writes straight into the join's query block; the
// join's fillers (-1, 1000.0) are no candidates.
extern "C" int freddy_gpu_ivpq_analogy(freddy_gpu_index_t* ivpq, freddy_gpu_index_t* vecs, const int32_t* triples, int32_t Q, int32_t k, int32_t n_cand,
                                       const int32_t* target_ids, int64_t n_targets, int32_t alpha, int32_t pvf, int32_t method, int32_t use_target_lists,
                                       float confidence, int32_t double_threshold, int32_t* out_ids, float* out_sim) {
  if (int rc = aa_check_scalars(triples, Q, k, n_cand, out_ids, out_sim)) return rc;
  if (!ivpq || !vecs) return fail(FREDDY_E_ARG, "NULL index");
  if (int rc = knn_join_check(ivpq, n_cand, target_ids, n_targets, alpha, pvf, method, double_threshold)) return rc;
  if (int rc = check_ann_vecs(ivpq, KIND_IVPQ, vecs, "the approximate analogy")) return rc;
  return aa_search(ivpq, vecs, triples, Q, k, n_cand, out_ids, out_sim, [&](const float*, int nq, int32_t* l_ids, float* l_dist) {
    return knn_join_block(ivpq, nq, n_cand, target_ids, n_targets, alpha, pvf, method, use_target_lists, confidence, double_threshold, l_ids, l_dist, nullptr);
  }, [&](int Qc, float** block) { return join_query_block_for(ivpq, Qc, block); });
}

extern "C" int freddy_gpu_last_approx_analogy_stats(const freddy_gpu_index_t* ann, int64_t* searched, int64_t* candidates, int64_t* scored) {
  if (!ann) return fail(FREDDY_E_ARG, "NULL index");
  if (ann->kind != KIND_PQ && ann->kind != KIND_IVF && ann->kind != KIND_IVPQ) return fail(FREDDY_E_KIND, "index handle has the wrong kind for this call");
  if (searched) *searched = ann->aa_stats[0];
  if (candidates) *candidates = ann->aa_stats[1];
  if (scored) *scored = ann->aa_stats[2];
  return FREDDY_OK;
}

// The kernels of this unit that want more than the default 64 KiB of dynamic LDS.
std::vector<LdsLimit> lds_limits_rerank() {
  // (4096 keys + four tiles + the query: 66 KiB at d = 300, 83 KiB at EX_MAX_D; the kernel has static LDS beside the dynamic)
  return {{&pv_rerank_kernel<4>, (int)pv_lds_bytes(4, PV_MAX_CAND, EX_MAX_D)}, {&aa_rerank_kernel<4>, (int)pv_lds_bytes(4, PV_MAX_CAND, EX_MAX_D)}};
}
