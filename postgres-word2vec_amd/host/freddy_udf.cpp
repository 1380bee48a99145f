// freddy_udf.cpp -- host-side mirror of the FREDDY search UDFs (include/freddy_udf.h).
//
// Stands where freddy_extension/freddy.c and ivpq_search_in.c stand in a PostgreSQL backend:
// keeps the tables and the config functions, resolves ids, pins the tables into HBM once
// (the reference re-reads them through SPI on every call: freddy.c:69,239-241,746-749;
// ivpq_search_in.c:218-232) and forwards every search through the device C ABI.  No distance
// is computed here.
//
// One translation unit: session.h (the tables, their handles and loaders), index_file.h (FRDYIDX1 files) and cluster.h
// (generic_cluster) are included below; this file keeps the entry points, which read check, resolve, call, emit.
// tests/test_host_trace_cpu.py pins everything they check, say, send to the device and emit against a recorded trace.
#include "session.h"
#include "index_file.h"

namespace {

// ---- the checks entry points start with; each keeps its own order of them (the recorded trace pins it) ----------------------
#define REQUIRE(check) if (int rc_ = (check)) return rc_
int need_table(const freddy_session* s, int t) { return !s || !s->code[t].h ? fail(-1, "%s", kNotLoaded[t]) : 0; }
// google_vecs_norm loaded AND of `d` dimensions (a code table's, or the query's)
int need_norm(const freddy_session* s, int d) { return s->norm.empty() || s->norm.d != d ? fail(-1, "google_vecs_norm is not loaded") : 0; }
int need_index_dim(const CodeTable& t, int dim) { return dim != t.d ? fail(-1, "query has %d dimensions, index has %d", dim, t.d) : 0; }
int need_table_of_dim(const freddy_session* s, int t, int dim) { return need_table(s, t) ? -1 : need_index_dim(s->code[t], dim); }
int need_table_and_norm(const freddy_session* s, int t) { return need_table(s, t) ? -1 : need_norm(s, s->code[t].d); }
// the exact functions: google_vecs_norm loaded at all; ... and the query of its dimensions
int need_vecs(const freddy_session* s) { return !s || s->norm.empty() ? fail(-1, "google_vecs_norm is not loaded") : 0; }
int need_vecs_of_dim(const freddy_session* s, int dim) {
  return need_vecs(s) ? -1 : dim != s->norm.d ? fail(-1, "query has %d dimensions, table has %d", dim, s->norm.d) : 0;
}
// every entry point's last two lines
int rows_out(int32_t* n_rows, int32_t n) { if (n_rows) *n_rows = n; return 0; }

// ---- the device calls more than one entry point makes -------------------------------------------------------------------------
// what the reference fills its result lists with: pq_search with 100, every other SRF with 1000
constexpr float kPqSearchFiller = 100.0f, kFiller = 1000.0f;

// pq_search(q, k) resp. ivfadc_search(q, k) with W = get_w(), as the plpgsql callers call them
int plain_search(freddy_session* s, int t, const float* query, int k, std::vector<int32_t>& ids, std::vector<float>& dist) {
  ids.resize((size_t)k); dist.resize((size_t)k);
  const int rc = t == IVF ? freddy_gpu_ivfadc_search(s->code[IVF].h, query, 1, k, s->w, kFiller, FREDDY_FOUND_ROWS, ids.data(), dist.data())
                          : freddy_gpu_pq_search(s->code[PQ].h, query, 1, k, kPqSearchFiller, nullptr, 0, ids.data(), dist.data());
  return rc ? gpu_fail(rc) : 0;
}

// "id = ANY(input_ids)" as the device takes it: an empty list is a list nothing is in (NULL would mean the whole table)
struct InList { const int32_t* ids; int64_t n; };
InList in_list(const int32_t* input_ids, int32_t n_ids) {
  static const int32_t none = -1;
  return n_ids ? InList{input_ids, n_ids} : InList{&none, 1};
}
// pq_search_in(q, k, input_ids) for Q queries
int pq_in_search(freddy_session* s, const float* queries, int Q, int k, const int32_t* input_ids, int32_t n_ids, std::vector<int32_t>& ids,
                 std::vector<float>& dist) {
  ids.resize((size_t)Q * k); dist.resize((size_t)Q * k);
  const InList in = in_list(input_ids, n_ids);
  if (int rc = freddy_gpu_pq_search(s->code[PQ].h, queries, Q, k, kFiller, in.ids, in.n, ids.data(), dist.data())) return gpu_fail(rc);
  return 0;
}

// ivpq_search_in with alpha / pvf / method / use_targetlist / confidence / long_codes_threshold from the getters
int session_knn_join(freddy_session* s, const float* queries, int Q, int k, const int32_t* targets, int64_t n_targets, int32_t* ids, float* dist) {
  if (int rc = freddy_gpu_knn_join(s->code[IVPQ].h, queries, Q, k, targets, n_targets, s->alpha, s->pvf, s->method_flag, s->use_targetlist,
                                   s->confidence, s->long_codes_threshold, ids, dist, nullptr))
    return gpu_fail(rc);
  return 0;
}

// ---- row emission ---------------------------------------------------------------------------------------------------------------
int emit2(const std::vector<int32_t>& ids, const std::vector<float>& dist, int k, freddy_row2* out, int32_t* n_rows) {
  for (int i = 0; i < k; ++i) { out[i].id = ids[i]; out[i].distance = dist[i]; }
  return rows_out(n_rows, k);   // the SRF returns k rows, unfilled ones are (-1, sentinel)  freddy.c:154-169
}
int emit3(const int32_t* qids, int Q, int k, const std::vector<int32_t>& ids, const std::vector<float>& dist, freddy_row3* out, int32_t* n_rows) {
  // iter / k -> query, iter % k -> rank   (freddy.c:654-674, 1001-1023; ivpq_search_in.c:700-720)
  for (int i = 0; i < Q * k; ++i) { out[i].query_id = qids[i / k]; out[i].id = ids[i]; out[i].distance = dist[i]; }
  return rows_out(n_rows, Q * k);
}
// FETCH FIRST k ROWS ONLY of Q lists of k slots: the leading rows (id >= 0) of each, fewer than k where fewer exist; list q under qids[q]
int32_t emit_lists(const int32_t* qids, int Q, int k, const std::vector<int32_t>& ids, const std::vector<float>& sim, freddy_row3* out) {
  int32_t n = 0;
  for (int q = 0; q < Q; ++q)
    for (int r = 0; r < k && ids[(size_t)q * k + r] >= 0; ++r) out[n++] = {qids[q], ids[(size_t)q * k + r], sim[(size_t)q * k + r]};
  return n;
}

// SRF text round trip of a distance: snprintf("%f") into the tuple, float4in on the way out (freddy.c:164)
static float emitted(float distance) {
  char buf[16];
  snprintf(buf, sizeof buf, "%f", distance);
  return strtof(buf, nullptr);
}
// (1.0 - (distance / 2.0))::float4 -- float4 / numeric is evaluated in float8   freddy--0.0.1.sql:527,617
// (The text round trip stays the definition here; include/freddy_similarity.h restates it in exact arithmetic for the device --
// freddy_gpu_pq_assign's key -- and tests/assign_sim_check.c compares the two bit for bit.)
static float similarity_of(float distance) { return (float)(1.0 - (double)emitted(distance) / 2.0); }

// the plpgsql callers' "INNER JOIN ... ON idx = id" over SRF rows: the (-1, sentinel) rows drop out, the distance becomes the similarity
template <class Row>
int32_t found_rows(const Row* rows, int n, Row* out) {
  int32_t m = 0;
  for (int i = 0; i < n; ++i)
    if (rows[i].id >= 0) { out[m] = rows[i]; out[m].distance = similarity_of(rows[i].distance); ++m; }
  return m;
}

}  // namespace

#include "cluster.h"

extern "C" {

// ---- set_statistics_table / create_statistics (freddy--0.0.1.sql:70, :150-171): the statistics row of the pinned ivpq handle ----
int freddy_set_statistics_table(freddy_session_t* s, const int32_t* stat_coarse_id, const float* stat_freq, int32_t n_stat) {
  if (!s || !stat_coarse_id || !stat_freq) return fail(-1, "bad argument");
  REQUIRE(need_table(s, IVPQ));
  std::vector<float> stats;
  REQUIRE(stat_row(s->cq_multi.K * s->cq_multi.K, stat_coarse_id, stat_freq, n_stat, stats));
  if (int rc = freddy_gpu_set_statistics(s->code[IVPQ].h, stats.data(), (int32_t)stats.size())) return gpu_fail(rc);
  return 0;
}

int32_t freddy_statistics_rows(const freddy_session_t* s) { return s && s->code[IVPQ].h ? s->cq_multi.K * s->cq_multi.K + 1 : 0; }

// computed over the pinned rows and installed, as the bootstrap block does (:183-184: create_statistics, then set_statistics_table)
int create_statistics(freddy_session_t* s, const int32_t* token_ids, int64_t n, float* out_stats) {
  if (!s || n < 0 || (n > 0 && !token_ids)) return fail(-1, "bad argument");
  REQUIRE(need_table(s, IVPQ));
  if (int rc = freddy_gpu_create_statistics(s->code[IVPQ].h, token_ids, n, 1, out_stats, nullptr)) return gpu_fail(rc);
  return 0;
}

// ---- config functions ------------------------------------------------------------------------
#define CONFIG(name, field, type) \
  int freddy_set_##name(freddy_session_t* s, type v) { if (!s) return fail(-1, "NULL session"); s->field = v; return 0; } \
  type freddy_get_##name(const freddy_session_t* s) { return s->field; }
CONFIG(w, w, int32_t)
CONFIG(pvf, pvf, int32_t)
CONFIG(alpha, alpha, int32_t)
CONFIG(confidence_value, confidence, float)
CONFIG(long_codes_threshold, long_codes_threshold, int32_t)
CONFIG(method_flag, method_flag, int32_t)
CONFIG(use_targetlist, use_targetlist, int32_t)
#undef CONFIG
// the names the dispatchers call (freddy--0.0.1.sql:197-200): any name is accepted, as by the SQL setters; a name without a function fails at call time
#define NAME_SETTER(name, field) \
  int freddy_set_##name(freddy_session_t* s, const char* v) { if (!s || !v) return fail(-1, "bad argument"); s->field = v; return 0; } \
  const char* freddy_get_##name(const freddy_session_t* s) { return s ? s->field.c_str() : ""; }
NAME_SETTER(knn_batch_function, knn_batch_fn)
NAME_SETTER(analogy_function, analogy_fn)
NAME_SETTER(analogy_in_function, analogy_in_fn)
NAME_SETTER(groups_function, groups_fn)
#undef NAME_SETTER

// ---- UDFs ------------------------------------------------------------------------------------
// pq_search / ivfadc_search: the SRF's k rows; `joined`: their plpgsql callers k_nearest_neighbour_pq / _ivfadc
static int srf_search(freddy_session_t* s, int t, bool joined, const float* query, int32_t dim, int32_t k, freddy_row2* out, int32_t* n_rows) {
  REQUIRE(need_table_of_dim(s, t, dim));
  if (k <= 0 || !query || !out) return fail(-1, "bad argument");
  std::vector<int32_t> ids; std::vector<float> dist;
  REQUIRE(plain_search(s, t, query, k, ids, dist));
  if (!joined) return emit2(ids, dist, k, out, n_rows);
  std::vector<freddy_row2> rows((size_t)k);
  emit2(ids, dist, k, rows.data(), nullptr);
  return rows_out(n_rows, found_rows(rows.data(), k, out));
}
int pq_search(freddy_session_t* s, const float* query, int32_t dim, int32_t k, freddy_row2* out, int32_t* n_rows) {
  return srf_search(s, PQ, false, query, dim, k, out, n_rows);
}
int ivfadc_search(freddy_session_t* s, const float* query, int32_t dim, int32_t k, freddy_row2* out, int32_t* n_rows) {
  return srf_search(s, IVF, false, query, dim, k, out, n_rows);
}
int k_nearest_neighbour_pq(freddy_session_t* s, const float* query, int32_t dim, int32_t k, freddy_row2* out, int32_t* n_rows) {
  return srf_search(s, PQ, true, query, dim, k, out, n_rows);
}
int k_nearest_neighbour_ivfadc(freddy_session_t* s, const float* query, int32_t dim, int32_t k, freddy_row2* out, int32_t* n_rows) {
  return srf_search(s, IVF, true, query, dim, k, out, n_rows);
}

int pq_search_in(freddy_session_t* s, const float* query, int32_t dim, int32_t k, const int32_t* input_ids,
                 int32_t n_ids, freddy_row2* out, int32_t* n_rows) {
  REQUIRE(need_table_of_dim(s, PQ, dim));
  if (k <= 0 || !query || !out || n_ids < 0) return fail(-1, "bad argument");
  std::vector<int32_t> ids; std::vector<float> dist;
  REQUIRE(pq_in_search(s, query, 1, k, input_ids, n_ids, ids, dist));
  return emit2(ids, dist, k, out, n_rows);
}

int pq_search_in_batch(freddy_session_t* s, const float* queries, int32_t n_queries, int32_t dim,
                       const int32_t* query_ids, int32_t n_query_ids, int32_t k, const int32_t* input_ids,
                       int32_t n_ids, int32_t use_target_lists, freddy_row3* out, int32_t* n_rows) {
  (void)use_target_lists;   // both branches of the reference give identical lists (freddy.c:596-628)
  REQUIRE(need_table(s, PQ));
  if (n_query_ids != n_queries) return fail(-1, "Number of query vectors and query vector ids differs!");   // freddy.c:495
  REQUIRE(need_index_dim(s->code[PQ], dim));
  if (k <= 0 || n_queries < 0 || n_ids < 0) return fail(-1, "bad argument");
  std::vector<int32_t> ids; std::vector<float> dist;
  REQUIRE(pq_in_search(s, queries, n_queries, k, input_ids, n_ids, ids, dist));
  return emit3(query_ids, n_queries, k, ids, dist, out, n_rows);
}

int ivfadc_batch_search(freddy_session_t* s, const int32_t* query_ids, int32_t n_query_ids, int32_t k, freddy_row3* out,
                        int32_t* n_rows) {
  REQUIRE(need_table_and_norm(s, IVF));
  if (k <= 0 || n_query_ids < 0 || !out) return fail(-1, "bad argument");
  std::vector<int32_t> qid;
  std::vector<float> qv;
  s->norm.select_in(query_ids, n_query_ids, qid, qv);
  const int Q = (int)qid.size();
  std::vector<int32_t> ids((size_t)Q * k); std::vector<float> dist((size_t)Q * k);
  if (Q > 0)
    if (int rc = freddy_gpu_ivfadc_search(s->code[IVF].h, qv.data(), Q, k, 1, 100.0f, FREDDY_FOUND_BATCH_UDF, ids.data(), dist.data()))   // (this SRF's own W and filler)
      return gpu_fail(rc);
  return emit3(qid.data(), Q, k, ids, dist, out, n_rows);
}

int ivpq_search_in(freddy_session_t* s, const float* queries, int32_t n_queries, int32_t dim, const int32_t* query_ids,
                   int32_t n_query_ids, int32_t k, const int32_t* input_ids, int32_t n_ids, int32_t alpha, int32_t pvf,
                   int32_t method, int32_t use_target_lists, float confidence, int32_t double_threshold,
                   freddy_row3* out, int32_t* n_rows) {
  REQUIRE(need_table(s, IVPQ));
  if (n_query_ids != n_queries)   // ivpq_search_in.c:180
    return fail(-1, "Number of query vectors and query vector ids differs! ( %d, %d)", n_query_ids, n_queries);
  REQUIRE(need_index_dim(s->code[IVPQ], dim));
  if (k <= 0 || n_queries < 0 || n_ids < 0) return fail(-1, "bad argument");
  std::vector<int32_t> ids((size_t)n_queries * k); std::vector<float> dist((size_t)n_queries * k);
  if (int rc = freddy_gpu_knn_join(s->code[IVPQ].h, queries, n_queries, k, input_ids, n_ids, alpha, pvf, method, use_target_lists,
                                   confidence, double_threshold, ids.data(), dist.data(), nullptr))
    return gpu_fail(rc);
  return emit3(query_ids, n_queries, k, ids, dist, out, n_rows);
}

int knn_join(freddy_session_t* s, const float* queries, int32_t n_queries, int32_t dim, const int32_t* query_ids,
             int32_t k, const int32_t* input_ids, int32_t n_ids, freddy_row3* out, int32_t* n_rows) {
  if (!s) return fail(-1, "NULL session");
  return ivpq_search_in(s, queries, n_queries, dim, query_ids, n_queries, k, input_ids, n_ids, s->alpha, s->pvf,
                        s->method_flag, s->use_targetlist, s->confidence, s->long_codes_threshold, out, n_rows);
}

// ---- exact brute force -------------------------------------------------------------
static int exact_common(freddy_session_t* s, const float* query, int32_t dim, int32_t k, const int32_t* input_ids,
                        int32_t n_ids, bool subset, freddy_row2* out, int32_t* n_rows) {
  REQUIRE(need_vecs_of_dim(s, dim));
  if (k <= 0 || !query || !out || n_ids < 0) return fail(-1, "bad argument");
  REQUIRE(s->norm.pinned(s->device));
  std::vector<int32_t> ids((size_t)k); std::vector<float> sim((size_t)k);
  const InList sub = subset ? in_list(input_ids, n_ids) : InList{nullptr, 0};
  if (int rc = freddy_gpu_exact_search(s->norm.h, query, 1, k, sub.ids, sub.n, ids.data(), sim.data())) return gpu_fail(rc);
  int n = 0;   // FETCH FIRST k ROWS ONLY returns fewer rows when fewer exist
  while (n < k && ids[n] >= 0) { out[n].id = ids[n]; out[n].distance = sim[n]; ++n; }
  return rows_out(n_rows, n);
}

int k_nearest_neighbour(freddy_session_t* s, const float* query, int32_t dim, int32_t k, freddy_row2* out, int32_t* n_rows) {
  return exact_common(s, query, dim, k, nullptr, 0, false, out, n_rows);
}

int knn_in_exact(freddy_session_t* s, const float* query, int32_t dim, int32_t k, const int32_t* input_ids, int32_t n_ids,
                 freddy_row2* out, int32_t* n_rows) {
  return exact_common(s, query, dim, k, input_ids, n_ids, true, out, n_rows);
}

// ---- grouping and analogy on the PQ / IVFADC indexes ---------------------------------------
int grouping_pq(freddy_session_t* s, const int32_t* input_ids, int32_t n_ids, const int32_t* group_ids, int32_t n_groups,
                freddy_group_row* out, int32_t* n_rows) {
  REQUIRE(need_table_and_norm(s, PQ));
  if (n_ids < 0 || n_groups <= 0 || !group_ids || !out || (n_ids > 0 && !input_ids)) return fail(-1, "bad argument");
  const int d = s->norm.d;
  std::vector<int32_t> groups(group_ids, group_ids + n_groups);
  std::sort(groups.begin(), groups.end());                                       // freddy.c:1241
  std::vector<float> gvec((size_t)n_groups * d);
  for (int g = 0; g < n_groups; ++g) {
    // "SELECT id, vector ... WHERE id IN (groups) ORDER BY id ASC" must return one row per group id (:1262-1265)
    const float* v = (g > 0 && groups[g] == groups[g - 1]) ? nullptr : s->norm.find(groups[g]);
    if (!v) return fail(-1, "Group ids do not exist");
    memcpy(&gvec[(size_t)g * d], v, sizeof(float) * d);
  }
  if (n_rows) *n_rows = 0;
  if (n_ids == 0) return 0;
  std::vector<int32_t> ids((size_t)n_ids), grp((size_t)n_ids);
  int64_t n = 0;
  if (int rc = freddy_gpu_grouping_pq(s->code[PQ].h, gvec.data(), n_groups, input_ids, n_ids, ids.data(), grp.data(), &n)) return gpu_fail(rc);
  for (int64_t i = 0; i < n; ++i) { out[i].id = ids[i]; out[i].group_id = grp[i] >= 0 ? groups[grp[i]] : -1; }
  return rows_out(n_rows, (int32_t)n);
}

// vec_minus_bytea / vec_plus_bytea / vec_normalize_bytea / cosine_similarity_bytea   core_functions.c:118-136,177-195,241-266,67-81
static void vec3cosadd(const float* v1, const float* v2, const float* v3, int d, std::vector<float>& raw, std::vector<float>& unit) {
  raw.resize(d); unit.resize(d);
  for (int i = 0; i < d; ++i) { const float t = v3[i] - v1[i]; raw[i] = t + v2[i]; }
  float sq = 0;
  for (int i = 0; i < d; ++i) { const float p = raw[i] * raw[i]; sq = sq + p; }
  const float length = (float)sqrt((double)sq);
  for (int i = 0; i < d; ++i) unit[i] = raw[i] / length;
}
static float cos_sim_bytea(const float* a, const float* b, int d) {
  float scalar = 0;
  for (int i = 0; i < d; ++i) { const float p = a[i] * b[i]; scalar = scalar + p; }
  return scalar;
}

// analogy_3cosadd_pq / analogy_3cosadd_ivfadc (freddy--0.0.1.sql:1317-1346, 1428-1460) and, over an input set (`in`),
// analogy_3cosadd_in_pq / analogy_3cosadd_in_ivpq (:1348-1426), by row id: q = vec_normalize(v3 - v1 + v2), candidates from
//   pq_search / ivfadc_search(q, get_pvf() + 3), pq_search_in(q, get_pvf() + 3, ids of the input set), or
//   ivpq_search_in(ARRAY[q], '{0}', 4, ids, alpha, pvf, method_flag, use_targetlist, confidence, long_codes_threshold) -- k is the literal 4 there (:1414)
// and of those that have a vector and are none of the three inputs the best by the RAW vector's cosine (-1: none, the SQL's NULL)
static int analogy_common(freddy_session_t* s, int t, bool in, int32_t id1, int32_t id2, int32_t id3, const int32_t* input_ids, int32_t n_ids,
                          int32_t* result) {
  if (!s || !result || n_ids < 0 || (n_ids > 0 && !input_ids)) return fail(-1, "bad argument");
  REQUIRE(need_table_and_norm(s, t));
  *result = -1;
  const float *v1 = s->norm.find(id1), *v2 = s->norm.find(id2), *v3 = s->norm.find(id3);
  if (!v1 || !v2 || !v3) return 0;            // the cross join over the three words is empty: NULL
  std::vector<float> raw, unit;
  vec3cosadd(v1, v2, v3, s->norm.d, raw, unit);
  const int k = t == IVPQ ? 4 : s->pvf + 3;
  std::vector<int32_t> ids((size_t)k); std::vector<float> dist((size_t)k);
  REQUIRE(t == IVPQ ? session_knn_join(s, unit.data(), 1, k, input_ids, n_ids, ids.data(), dist.data())
          : in      ? pq_in_search(s, unit.data(), 1, k, input_ids, n_ids, ids, dist)
                    : plain_search(s, t, unit.data(), k, ids, dist));
  // ... ORDER BY cosine_similarity_bytea(v3 - v1 + v2, v4.vector) DESC FETCH FIRST 1 ROWS ONLY (ties: lowest id)
  bool have = false;
  float best = 0;
  for (int i = 0; i < k; ++i) {
    const int32_t id = ids[i];
    if (id < 0 || id == id1 || id == id2 || id == id3) continue;
    const float* v4 = s->norm.find(id);
    if (!v4) continue;
    const float sim = cos_sim_bytea(raw.data(), v4, s->norm.d);
    if (!have || sim > best || (sim == best && id < *result)) { have = true; best = sim; *result = id; }
  }
  return 0;
}
int analogy_3cosadd_pq(freddy_session_t* s, int32_t id1, int32_t id2, int32_t id3, int32_t* result) {
  return analogy_common(s, PQ, false, id1, id2, id3, nullptr, 0, result);
}
int analogy_3cosadd_ivfadc(freddy_session_t* s, int32_t id1, int32_t id2, int32_t id3, int32_t* result) {
  return analogy_common(s, IVF, false, id1, id2, id3, nullptr, 0, result);
}
int analogy_3cosadd_in_pq(freddy_session_t* s, int32_t id1, int32_t id2, int32_t id3, const int32_t* input_ids, int32_t n_ids, int32_t* result) {
  return analogy_common(s, PQ, true, id1, id2, id3, input_ids, n_ids, result);
}
int analogy_3cosadd_in_ivpq(freddy_session_t* s, int32_t id1, int32_t id2, int32_t id3, const int32_t* input_ids, int32_t n_ids, int32_t* result) {
  return analogy_common(s, IVPQ, true, id1, id2, id3, input_ids, n_ids, result);
}

// ... with post verification: get_pvf() * k candidates, ORDER BY cosine_similarity_bytea(q, v.vector) DESC
// FETCH FIRST k ROWS ONLY (equal similarities: ascending id)            freddy--0.0.1.sql:575-591, 625-641
static int knn_pv(freddy_session_t* s, int t, const float* query, int32_t dim, int32_t k, freddy_row2* out, int32_t* n_rows) {
  REQUIRE(need_table(s, t));
  REQUIRE(need_norm(s, dim));
  REQUIRE(need_index_dim(s->code[t], dim));
  if (k <= 0 || !query || !out) return fail(-1, "bad argument");
  const int64_t kc = (int64_t)k * std::max(s->pvf, 1);
  if (kc > 4096) return fail(-1, "pvf * k = %lld exceeds this build's limit of 4096 candidates", (long long)kc);
  std::vector<int32_t> ids; std::vector<float> dist;
  REQUIRE(plain_search(s, t, query, (int)kc, ids, dist));
  std::vector<freddy_row2> cand;
  for (int64_t i = 0; i < kc; ++i) {
    if (ids[i] < 0) continue;
    const float* v = s->norm.find(ids[i]);
    if (!v) continue;
    cand.push_back({ids[i], cos_sim_bytea(query, v, dim)});
  }
  std::sort(cand.begin(), cand.end(), [](const freddy_row2& a, const freddy_row2& b) {
    return a.distance != b.distance ? a.distance > b.distance : a.id < b.id;
  });
  const int n = (int)std::min<size_t>(cand.size(), (size_t)k);
  for (int i = 0; i < n; ++i) out[i] = cand[i];
  return rows_out(n_rows, n);
}
int k_nearest_neighbour_pq_pv(freddy_session_t* s, const float* query, int32_t dim, int32_t k, freddy_row2* out, int32_t* n_rows) {
  return knn_pv(s, PQ, query, dim, k, out, n_rows);
}
int k_nearest_neighbour_ivfadc_pv(freddy_session_t* s, const float* query, int32_t dim, int32_t k, freddy_row2* out, int32_t* n_rows) {
  return knn_pv(s, IVF, query, dim, k, out, n_rows);
}

// knn_in_pq(anyarray, int, int[])                                          freddy--0.0.1.sql:830-843
int knn_in_pq(freddy_session_t* s, const float* query, int32_t dim, int32_t k, const int32_t* input_ids, int32_t n_ids,
              freddy_row2* out, int32_t* n_rows) {
  if (k <= 0 || !out) return fail(-1, "bad argument");
  std::vector<freddy_row2> rows((size_t)k);
  int32_t n = 0;
  REQUIRE(pq_search_in(s, query, dim, k, input_ids, n_ids, rows.data(), &n));
  return rows_out(n_rows, found_rows(rows.data(), n, out));
}

// k_nearest_neighbour_ivfadc_batch(varchar[], int), by query ids            freddy--0.0.1.sql:535-553
int k_nearest_neighbour_ivfadc_batch(freddy_session_t* s, const int32_t* query_ids, int32_t n_query_ids, int32_t k,
                                     freddy_row3* out, int32_t* n_rows) {
  if (k <= 0 || !out || n_query_ids < 0) return fail(-1, "bad argument");
  std::vector<freddy_row3> rows((size_t)std::max(n_query_ids, 1) * k);
  int32_t n = 0;
  REQUIRE(ivfadc_batch_search(s, query_ids, n_query_ids, k, rows.data(), &n));
  return rows_out(n_rows, found_rows(rows.data(), n, out));
}

// ---- the batch form of the two post-verification functions, and knn_batch()      freddy--0.0.1.sql:556-662, 232-246 ----------
// Queries chosen as ivfadc_batch_search chooses them (rows of google_vecs_norm with id IN query_ids, table order); per query the rows
// of knn_pv for that vector with get_pvf() / get_w(): ONE device call (freddy_gpu_*_search_pv) instead of a call and a host loop each.
static int knn_pv_batch(freddy_session_t* s, int t, const int32_t* query_ids, int32_t n_query_ids, int32_t k, freddy_row3* out, int32_t* n_rows) {
  if (n_rows) *n_rows = 0;
  REQUIRE(need_table_and_norm(s, t));
  if (k <= 0 || n_query_ids < 0 || !out || (n_query_ids > 0 && !query_ids)) return fail(-1, "bad argument");
  const int pvf = std::max(s->pvf, 1);
  const int64_t kc = (int64_t)k * pvf;
  if (kc > 4096) return fail(-1, "pvf * k = %lld exceeds this build's limit of 4096 candidates", (long long)kc);
  std::vector<int32_t> qid;
  std::vector<float> qv;
  s->norm.select_in(query_ids, n_query_ids, qid, qv);
  const int Q = (int)qid.size();
  if (Q == 0) return 0;
  REQUIRE(s->norm.pinned(s->device));
  std::vector<int32_t> ids((size_t)Q * k); std::vector<float> sim((size_t)Q * k);
  const int rc = t == IVF ? freddy_gpu_ivfadc_search_pv(s->code[IVF].h, s->norm.h, qv.data(), Q, k, pvf, s->w, kFiller, FREDDY_FOUND_ROWS, ids.data(), sim.data())
                          : freddy_gpu_pq_search_pv(s->code[PQ].h, s->norm.h, qv.data(), Q, k, pvf, kPqSearchFiller, nullptr, 0, ids.data(), sim.data());
  if (rc) return gpu_fail(rc);
  return rows_out(n_rows, emit_lists(qid.data(), Q, k, ids, sim, out));   // fewer than k rows for a query when fewer of its candidates have vectors
}
int k_nearest_neighbour_ivfadc_pv_batch(freddy_session_t* s, const int32_t* query_ids, int32_t n_query_ids, int32_t k, freddy_row3* out, int32_t* n_rows) {
  return knn_pv_batch(s, IVF, query_ids, n_query_ids, k, out, n_rows);
}
int k_nearest_neighbour_pq_pv_batch(freddy_session_t* s, const int32_t* query_ids, int32_t n_query_ids, int32_t k, freddy_row3* out, int32_t* n_rows) {
  return knn_pv_batch(s, PQ, query_ids, n_query_ids, k, out, n_rows);
}

// EXECUTE format('SELECT * FROM %s(''%s'', %s)', get_knn_batch_function_name(), query_set, k)
int knn_batch(freddy_session_t* s, const int32_t* query_ids, int32_t n_query_ids, int32_t k, freddy_row3* out, int32_t* n_rows) {
  if (!s) return fail(-1, "bad argument");
  const std::string& f = s->knn_batch_fn;
  if (f == "k_nearest_neighbour_ivfadc_batch") return k_nearest_neighbour_ivfadc_batch(s, query_ids, n_query_ids, k, out, n_rows);
  if (f == "k_nearest_neighbour_ivfadc_pv_batch") return k_nearest_neighbour_ivfadc_pv_batch(s, query_ids, n_query_ids, k, out, n_rows);
  if (f == "k_nearest_neighbour_pq_pv_batch") return k_nearest_neighbour_pq_pv_batch(s, query_ids, n_query_ids, k, out, n_rows);
  return fail(-1, "function %s(character varying[], integer) does not exist", f.c_str());
}

// ---- insert_batch --------------------------------------------------------------------
int freddy_set_codebook_counts(freddy_session_t* s, int32_t table, const int32_t* pos, const int32_t* code, const int32_t* count, int32_t n) {
  if (!s || !pos || !code || !count) return fail(-1, "bad argument");
  CodeTable* t = table >= PQ && table <= IVPQ ? &s->code[table] : nullptr;
  if (!t || t->cb.m == 0) return fail(-1, "that codebook is not loaded");
  for (int i = 0; i < n; ++i) {
    if (pos[i] < 0 || pos[i] >= t->cb.m || code[i] < 0 || code[i] >= t->cb.K) return fail(-1, "(pos, code) out of range");
    t->counts[(size_t)pos[i] * t->cb.K + code[i]] = count[i];
  }
  return 0;
}

// sprintf("%f") -> '{...}'::float4[]: how every float reaches the tables (index_utils.c:976, :1053)
static float text_roundtrip(float v) {
  char buf[64];
  snprintf(buf, sizeof buf, "%f", v);
  return strtof(buf, nullptr);
}

// updateCodebook's bookkeeping + updateCodebookRelation (index_utils.c:940-991) for codes found on the device.
// Statement by statement, slips included: `nearestCentroidRaw` is ONE pointer for all positions -- after the
// scan in table order (position-major) it is the nearest entry of the LAST position --, that vector is what
// every position of the row adds to its bucket, the recalculation reads bucket [pos + code] and adds
// (1.0 / count) * bucket in double, only entries with an increment are written back, as "%f" text.
static void update_codebook_host(Codebook& cb, std::vector<int32_t>& counts, const int16_t* codes, int n) {
  const int m = cb.m, K = cb.K, sdim = cb.s, E = m * K;
  std::vector<float> differences((size_t)E * sdim, 0.0f), work(cb.dense);
  std::vector<int32_t> incs((size_t)E, 0), wcount(counts);
  for (int i = 0; i < n; ++i) {
    const float* nearest_raw = &work[((size_t)(m - 1) * K + codes[(size_t)i * m + (m - 1)]) * sdim];
    for (int j = 0; j < m; ++j) {
      const int code = codes[(size_t)i * m + j];
      incs[(size_t)j * K + code] += 1;
      for (int k = 0; k < sdim; ++k) differences[((size_t)j * K + code) * sdim + k] += nearest_raw[k];
    }
  }
  for (int i = 0; i < E; ++i) {
    const int pos = i / K, code = i % K;
    wcount[(size_t)i] += incs[(size_t)pos * K + code];
    for (int j = 0; j < sdim; ++j)
      work[(size_t)i * sdim + j] += (1.0 / wcount[(size_t)i]) * differences[(size_t)(pos + code) * sdim + j];
  }
  for (int i = 0; i < E; ++i)
    if (incs[(size_t)i] > 0) {
      for (int j = 0; j < sdim; ++j) cb.dense[(size_t)i * sdim + j] = text_roundtrip(work[(size_t)i * sdim + j]);
      counts[(size_t)i] = wcount[(size_t)i];
    }
}

// The codes and cells of new vectors against the codebooks as they are (freddy.c:1557-1623), on the device; a table that is not
// loaded is skipped (insert_batch has them all).  The multi-index cell from its two codes: factor *= POSITIONS (freddy.c:1599, sic) --
// a cell built with factor = positions can exceed codes^2 only if positions > codes; it is stored as the reference stores it.
namespace {
struct NewCodes {
  std::vector<int16_t> code[3], multi;   // [PQ], [IVF] (of the residual), [IVPQ]
  std::vector<int32_t> cq, cell;         // coarse cell (ivfadc), multi-index cell (ivpq)
};
}
static int quantize(freddy_session_t* s, const float* vectors, int64_t n, int32_t dim, NewCodes& z) {
  const CodeTable &pq = s->code[PQ], &ivf = s->code[IVF], &iv = s->code[IVPQ];
  const Codebook& cq = s->cq_multi;
  freddy_insert_desc desc = {dim, 0, 0, nullptr, 0, 0, nullptr, 0, nullptr, 0, 0, nullptr, 0, 0, nullptr};
  if (pq.h) { desc.pq_m = pq.cb.m; desc.pq_K = pq.cb.K; desc.pq_codebook = pq.cb.dense.data(); }
  if (ivf.h) { desc.res_m = ivf.cb.m; desc.res_K = ivf.cb.K; desc.residual_codebook = ivf.cb.dense.data(); desc.C = s->C; desc.coarse = s->coarse.data(); }
  if (iv.h) {
    desc.ivpq_m = iv.cb.m; desc.ivpq_K = iv.cb.K; desc.ivpq_codebook = iv.cb.dense.data();
    desc.multi_positions = cq.m; desc.multi_codes = cq.K; desc.coarse_multi = cq.dense.data();
  }
  for (int t = PQ; t <= IVPQ; ++t) if (s->code[t].h) z.code[t].resize((size_t)n * s->code[t].cb.m);
  if (ivf.h) z.cq.resize((size_t)n);
  if (iv.h) z.multi.resize((size_t)n * cq.m);
  if (int rc = freddy_gpu_insert_quantize(&desc, s->device, vectors, n, pq.h ? z.code[PQ].data() : nullptr, ivf.h ? z.cq.data() : nullptr,
                                          ivf.h ? z.code[IVF].data() : nullptr, iv.h ? z.code[IVPQ].data() : nullptr, iv.h ? z.multi.data() : nullptr))
    return gpu_fail(rc);
  if (iv.h) {
    z.cell.assign((size_t)n, 0);
    for (int64_t i = 0; i < n; ++i) {
      int factor = 1;
      for (int p = 0; p < cq.m; ++p) { z.cell[(size_t)i] += factor * z.multi[(size_t)i * cq.m + p]; factor *= cq.m; }
    }
  }
  return 0;
}

int insert_batch(freddy_session_t* s, const float* norm_vectors, int32_t n, int32_t dim, int32_t* new_ids) {
  if (!s || n < 0 || (n > 0 && !norm_vectors)) return fail(-1, "bad argument");
  CodeTable* const code = s->code;
  if (!code[PQ].h || !code[IVF].h || !code[IVPQ].h || s->norm.empty())
    return fail(-1, "insert_batch needs google_vecs_norm, the pq, ivfadc and ivpq tables (freddy.c:1467-1481)");
  if (dim != s->norm.d || dim != code[PQ].d || dim != code[IVF].d || dim != code[IVPQ].d)
    return fail(-1, "vectors have %d dimensions, the tables %d", dim, s->norm.d);
  if (n == 0) return 0;
  NewCodes z;
  REQUIRE(quantize(s, norm_vectors, n, dim, z));
  // the three codebooks (index_utils.c:940-991) -- on COPIES: the session's tables change only after every device
  // mutation below has succeeded; a failure midway leaves the host tables as they were and drops the pinned handles
  Codebook cb[3] = {code[PQ].cb, code[IVF].cb, code[IVPQ].cb};
  std::vector<int32_t> counts[3] = {code[PQ].counts, code[IVF].counts, code[IVPQ].counts};
  for (int t = PQ; t <= IVPQ; ++t) update_codebook_host(cb[t], counts[t], z.code[t].data(), n);
  // the rows: every INSERT takes (SELECT max(id) + 1 FROM <its table>)   index_utils.c:1003-1021, 1046-1058
  std::vector<int32_t> id[3], id_norm((size_t)n);
  std::vector<float> stored((size_t)n * dim);
  for (size_t i = 0; i < stored.size(); ++i) stored[i] = text_roundtrip(norm_vectors[i]);
  for (int t = PQ; t <= IVPQ; ++t) {
    id[t].resize((size_t)n);
    std::iota(id[t].begin(), id[t].end(), code[t].max_id() + 1);
  }
  std::iota(id_norm.begin(), id_norm.end(), s->norm.ids.back() + 1);
  auto device_side = [&]() -> int {
    if (int rc = freddy_gpu_append_rows(code[PQ].h, n, id[PQ].data(), nullptr, z.code[PQ].data(), nullptr)) return rc;
    if (int rc = freddy_gpu_append_rows(code[IVF].h, n, id[IVF].data(), z.cq.data(), z.code[IVF].data(), nullptr)) return rc;
    if (int rc = freddy_gpu_append_rows(code[IVPQ].h, n, id[IVPQ].data(), z.cell.data(), z.code[IVPQ].data(), stored.data())) return rc;
    for (int t = PQ; t <= IVPQ; ++t)
      if (int rc = freddy_gpu_update_codebook(code[t].h, cb[t].dense.data())) return rc;
    if (s->norm.h) if (int rc = freddy_gpu_append_rows(s->norm.h, n, id_norm.data(), nullptr, nullptr, stored.data())) return rc;
    return 0;
  };
  if (int rc = device_side()) return device_failed(s, rc, false);
  // commit
  for (int t = PQ; t <= IVPQ; ++t) {
    code[t].cb = std::move(cb[t]);
    code[t].counts = std::move(counts[t]);
    code[t].ids.insert(code[t].ids.end(), id[t].begin(), id[t].end());
  }
  s->norm.ids.insert(s->norm.ids.end(), id_norm.begin(), id_norm.end());
  s->norm.rows.insert(s->norm.rows.end(), stored.begin(), stored.end());
  if (new_ids) memcpy(new_ids, id_norm.data(), sizeof(int32_t) * (size_t)n);
  return 0;
}

// ---- delete_rows: DELETE FROM <every table of the session> WHERE id = ANY(ids) ----------------------------------
static int no_negative_id(const int32_t* ids, int64_t n) {   // (-1 is the filler of the result lists)
  for (int64_t i = 0; i < n; ++i)
    if (ids[i] < 0) return fail(-1, "id %d at position %lld is negative", ids[i], (long long)i);
  return 0;
}
// ascending, distinct `want` out of an ascending id list (and the rows of `e` floats that go with it); -> rows dropped
static int64_t drop_ids(std::vector<int32_t>& ids, std::vector<float>* rows, int e, const std::vector<int32_t>& want) {
  size_t w = 0;
  for (size_t r = 0; r < ids.size(); ++r) {
    if (std::binary_search(want.begin(), want.end(), ids[r])) continue;
    if (w != r) {
      ids[w] = ids[r];
      if (rows) std::copy(rows->begin() + r * e, rows->begin() + (r + 1) * e, rows->begin() + w * e);
    }
    ++w;
  }
  const int64_t gone = (int64_t)(ids.size() - w);
  ids.resize(w);
  if (rows) rows->resize(w * (size_t)e);
  return gone;
}

int delete_rows(freddy_session_t* s, const int32_t* ids, int64_t n, int64_t* removed) {
  if (!s || n < 0 || (n > 0 && !ids)) return fail(-1, "bad argument");
  if (removed) *removed = 0;
  REQUIRE(no_negative_id(ids, n));
  if (n == 0) return 0;
  // the pinned handles first: a failure there drops them (they may have lost part of the rows) and leaves the host tables as they were
  freddy_gpu_index_t* const handles[] = {s->code[PQ].h, s->code[IVF].h, s->code[IVPQ].h, s->norm.h, s->orig.h};
  for (freddy_gpu_index_t* h : handles)
    if (h)
      if (int rc = freddy_gpu_remove_rows(h, n, ids, nullptr)) return device_failed(s, rc, true);
  std::vector<int32_t> want(ids, ids + n);
  std::sort(want.begin(), want.end());
  want.erase(std::unique(want.begin(), want.end()), want.end());
  const int64_t gone = drop_ids(s->norm.ids, &s->norm.rows, s->norm.d, want);
  drop_ids(s->orig.ids, &s->orig.rows, s->orig.d, want);
  for (CodeTable& t : s->code) drop_ids(t.ids, nullptr, 0, want);
  if (removed) *removed = gone;
  return 0;
}

// ---- update_rows: UPDATE google_vecs_norm SET vector = ... WHERE id = ..., and the same ids re-quantised in the three code tables ----
int update_rows(freddy_session_t* s, const int32_t* ids, const float* norm_vectors, int64_t n, int32_t dim, int64_t* updated) {
  if (!s || n < 0 || (n > 0 && (!ids || !norm_vectors))) return fail(-1, "bad argument");
  if (updated) *updated = 0;
  REQUIRE(no_negative_id(ids, n));
  {
    const std::vector<int64_t> ord = order_by_id(ids, n);
    for (int64_t i = 1; i < n; ++i)
      if (ids[ord[(size_t)i]] == ids[ord[(size_t)i - 1]])
        return fail(-1, "id %d is listed twice, at positions %lld and %lld", ids[ord[(size_t)i]], (long long)ord[(size_t)i - 1], (long long)ord[(size_t)i]);
  }
  if (n == 0) return 0;
  if (n > INT32_MAX) return fail(-1, "too many rows in one call");
  const CodeTable* const code = s->code;
  for (int have : {s->norm.d, code[PQ].h ? code[PQ].d : 0, code[IVF].h ? code[IVF].d : 0, code[IVPQ].h ? code[IVPQ].d : 0})
    if (have && dim != have) return fail(-1, "vectors have %d dimensions, the tables %d", dim, have);
  NewCodes z;
  if (code[PQ].h || code[IVF].h || code[IVPQ].h) REQUIRE(quantize(s, norm_vectors, n, dim, z));
  auto device_side = [&]() -> int {
    if (code[PQ].h) if (int rc = freddy_gpu_update_rows(code[PQ].h, n, ids, nullptr, z.code[PQ].data(), nullptr, nullptr)) return rc;
    if (code[IVF].h) if (int rc = freddy_gpu_update_rows(code[IVF].h, n, ids, z.cq.data(), z.code[IVF].data(), nullptr, nullptr)) return rc;
    if (code[IVPQ].h) if (int rc = freddy_gpu_update_rows(code[IVPQ].h, n, ids, z.cell.data(), z.code[IVPQ].data(), norm_vectors, nullptr)) return rc;
    if (s->norm.h) if (int rc = freddy_gpu_update_rows(s->norm.h, n, ids, nullptr, nullptr, norm_vectors, nullptr)) return rc;
    return 0;
  };
  if (int rc = device_side()) return device_failed(s, rc, false);
  int64_t changed = 0;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t r = s->norm.row_of(ids[i]);
    if (r < 0) continue;
    memcpy(&s->norm.rows[(size_t)r * s->norm.d], norm_vectors + (size_t)i * dim, sizeof(float) * (size_t)dim);
    ++changed;
  }
  if (updated) *updated = changed;
  return 0;
}

// ---- the batch forms of analogy_3cosadd_pq / _ivfadc / _in_pq: ONE device call for n triples (approx_analogy.h) instead of a search
// and analogy_common's host loop per triple; the arguments are the ones analogy_common passes
static int analogy_batch_common(freddy_session_t* s, int t, bool in, const int32_t* triples, int32_t n, const int32_t* input_ids, int32_t n_ids,
                                int32_t* results) {
  if (!s || n < 0 || (n > 0 && (!triples || !results)) || n_ids < 0 || (n_ids > 0 && !input_ids)) return fail(-1, "bad argument");
  REQUIRE(need_table_and_norm(s, t));
  if (n == 0) return 0;
  REQUIRE(s->norm.pinned(s->device));
  const int n_cand = s->pvf + 3;
  std::vector<float> sim((size_t)n);
  const InList sub = in ? in_list(input_ids, n_ids) : InList{nullptr, 0};   // (an empty input set is an empty set, not "the whole table")
  const int rc = t == IVF ? freddy_gpu_ivfadc_analogy(s->code[IVF].h, s->norm.h, triples, n, 1, n_cand, s->w, kFiller, FREDDY_FOUND_ROWS, results, sim.data())
                          : freddy_gpu_pq_analogy(s->code[PQ].h, s->norm.h, triples, n, 1, n_cand, in ? kFiller : kPqSearchFiller, sub.ids, sub.n, results, sim.data());
  return rc ? gpu_fail(rc) : 0;
}
int analogy_3cosadd_pq_batch(freddy_session_t* s, const int32_t* triples, int32_t n, int32_t* results) {
  return analogy_batch_common(s, PQ, false, triples, n, nullptr, 0, results);
}
int analogy_3cosadd_ivfadc_batch(freddy_session_t* s, const int32_t* triples, int32_t n, int32_t* results) {
  return analogy_batch_common(s, IVF, false, triples, n, nullptr, 0, results);
}
int analogy_3cosadd_in_pq_batch(freddy_session_t* s, const int32_t* triples, int32_t n, const int32_t* input_ids, int32_t n_ids, int32_t* results) {
  return analogy_batch_common(s, PQ, true, triples, n, input_ids, n_ids, results);
}
// The two entry points by row id over the kNN-join came without a new ABI version (no struct grew, no entry point changed meaning), so --
// as freddy_gpu_cluster in cluster.h -- they are bound weakly: beside a library that does not have them yet the functions below run
// what their callers ran before, the single-triple loop and the join over vectors gathered from the host copy; the rows are the same.
extern "C" int freddy_gpu_ivpq_analogy(freddy_gpu_index_t*, freddy_gpu_index_t*, const int32_t*, int32_t, int32_t, int32_t, const int32_t*, int64_t, int32_t,
                                       int32_t, int32_t, int32_t, float, int32_t, int32_t*, float*) __attribute__((weak));
extern "C" int freddy_gpu_knn_join_ids(freddy_gpu_index_t*, freddy_gpu_index_t*, const int32_t*, int32_t, int32_t, int32_t, const int32_t*, int64_t, int32_t,
                                       int32_t, int32_t, int32_t, float, int32_t, int32_t*, int32_t*, int32_t*, float*, int32_t*) __attribute__((weak));

// ... and of analogy_3cosadd_in_ivpq: ONE kNN-join per pass of triples at the SQL's literal k = 4 (freddy_gpu_ivpq_analogy), the join's
// settings from the getters as session_knn_join passes them
int analogy_3cosadd_in_ivpq_batch(freddy_session_t* s, const int32_t* triples, int32_t n, const int32_t* input_ids, int32_t n_ids, int32_t* results) {
  if (!s || n < 0 || (n > 0 && (!triples || !results)) || n_ids < 0 || (n_ids > 0 && !input_ids)) return fail(-1, "bad argument");
  REQUIRE(need_table_and_norm(s, IVPQ));
  if (n == 0) return 0;
  if (!freddy_gpu_ivpq_analogy) {
    for (int32_t i = 0; i < n; ++i)
      REQUIRE(analogy_common(s, IVPQ, true, triples[3 * i], triples[3 * i + 1], triples[3 * i + 2], input_ids, n_ids, results + i));
    return 0;
  }
  REQUIRE(s->norm.pinned(s->device));
  std::vector<float> sim((size_t)n);
  const int rc = freddy_gpu_ivpq_analogy(s->code[IVPQ].h, s->norm.h, triples, n, 1, 4, input_ids, n_ids, s->alpha, s->pvf, s->method_flag, s->use_targetlist,
                                         s->confidence, s->long_codes_threshold, results, sim.data());
  return rc ? gpu_fail(rc) : 0;
}

// ---- exact analogies and the dispatchers      freddy--0.0.1.sql:1231-1315, 269-297 --------------------------------
// one triple on a vector table's handle
static int one_exact_analogy(freddy_session_t* s, VecTable& table, int32_t method, int32_t id1, int32_t id2, int32_t id3, const int32_t* sub,
                             int64_t n_sub, int32_t* result) {
  *result = -1;
  REQUIRE(table.pinned(s->device));
  const int32_t triple[3] = {id1, id2, id3};
  double score = 0;
  if (int rc = freddy_gpu_exact_analogy(table.h, method, triple, 1, 1, sub, n_sub, result, &score)) return gpu_fail(rc);
  return 0;
}
static int exact_analogy(freddy_session_t* s, int32_t method, int32_t id1, int32_t id2, int32_t id3, const int32_t* input_ids,
                         int32_t n_ids, bool subset, int32_t* result) {
  if (!s || !result || n_ids < 0 || (n_ids > 0 && !input_ids)) return fail(-1, "bad argument");
  REQUIRE(need_vecs(s));
  // an empty set is a non-NULL pointer with a count of 0 (NULL would mean the whole table)
  const int32_t unused = 0;
  const int32_t* sub = subset ? (n_ids ? input_ids : &unused) : nullptr;
  return one_exact_analogy(s, s->norm, method, id1, id2, id3, sub, subset ? n_ids : 0, result);
}
int analogy_3cosadd(freddy_session_t* s, int32_t id1, int32_t id2, int32_t id3, int32_t* result) {
  return exact_analogy(s, FREDDY_ANALOGY_3COSADD, id1, id2, id3, nullptr, 0, false, result);
}
int analogy_3cosmul(freddy_session_t* s, int32_t id1, int32_t id2, int32_t id3, int32_t* result) {
  return exact_analogy(s, FREDDY_ANALOGY_3COSMUL, id1, id2, id3, nullptr, 0, false, result);
}
int analogy_3cosadd_in(freddy_session_t* s, int32_t id1, int32_t id2, int32_t id3, const int32_t* input_ids, int32_t n_ids, int32_t* result) {
  return exact_analogy(s, FREDDY_ANALOGY_3COSADD, id1, id2, id3, input_ids, n_ids, true, result);
}
// freddy--0.0.1.sql:1212-1229: the one exact function that reads get_vecs_name_original(); google_vecs pinned on first use
int analogy_pair_direction(freddy_session_t* s, int32_t id1, int32_t id2, int32_t id3, int32_t* result) {
  if (!s || !result) return fail(-1, "bad argument");
  if (s->orig.empty()) return fail(-1, "google_vecs is not loaded");
  return one_exact_analogy(s, s->orig, FREDDY_ANALOGY_PAIR_DIRECTION, id1, id2, id3, nullptr, 0, result);
}

// ---- tokenize / tokenize_raw for a batch of texts             freddy--0.0.1.sql:1512-1536 ----------------------------------
// "SELECT vector FROM <table> WHERE word = ANY(tokens)": the distinct rows in table order (FREDDY_QIDS_TABLE_ORDER), their centroid,
// normalised for tokenize(); the table is pinned on first use and the rows are read on the device (freddy_gpu_tokenize).  The entry
// point came without a new ABI version and is bound weakly, as freddy_gpu_knn_join_ids above; it has no earlier path to fall back to,
// so beside a library without it the two functions fail and say so.
extern "C" int freddy_gpu_tokenize(freddy_gpu_index_t*, const int32_t*, const int64_t*, int32_t, int32_t, int32_t, float*, int32_t*) __attribute__((weak));
static int tokenize_table(freddy_session_t* s, VecTable freddy_session::*table, const char* missing, int normalize, const int32_t* token_ids,
                          const int64_t* offsets, int32_t n_texts, float* out_vectors, int32_t* out_count) {
  if (!s) return fail(-1, "bad argument");
  VecTable& t = s->*table;
  if (t.empty()) return fail(-1, "%s is not loaded", missing);
  if (!freddy_gpu_tokenize) return fail(-1, "the device library has no freddy_gpu_tokenize");
  REQUIRE(t.pinned(s->device));
  if (int rc = freddy_gpu_tokenize(t.h, token_ids, offsets, n_texts, FREDDY_QIDS_TABLE_ORDER, normalize, out_vectors, out_count)) return gpu_fail(rc);
  return 0;
}
int tokenize_batch(freddy_session_t* s, const int32_t* token_ids, const int64_t* offsets, int32_t n_texts, float* out_vectors, int32_t* out_count) {
  return tokenize_table(s, &freddy_session::norm, "google_vecs_norm", 1, token_ids, offsets, n_texts, out_vectors, out_count);
}
int tokenize_raw_batch(freddy_session_t* s, const int32_t* token_ids, const int64_t* offsets, int32_t n_texts, float* out_vectors, int32_t* out_count) {
  return tokenize_table(s, &freddy_session::orig, "google_vecs", 0, token_ids, offsets, n_texts, out_vectors, out_count);
}

// EXECUTE format('SELECT * FROM %s(''%s'', ''%s'',''%s'')', get_analogy_function_name(), ...)
int analogy(freddy_session_t* s, int32_t a, int32_t b, int32_t c, int32_t* result) {
  if (!s || !result) return fail(-1, "bad argument");
  const std::string& f = s->analogy_fn;
  if (f == "analogy_3cosadd") return analogy_3cosadd(s, a, b, c, result);
  if (f == "analogy_3cosmul") return analogy_3cosmul(s, a, b, c, result);
  if (f == "analogy_pair_direction") return analogy_pair_direction(s, a, b, c, result);
  if (f == "analogy_3cosadd_pq") return analogy_3cosadd_pq(s, a, b, c, result);
  if (f == "analogy_3cosadd_ivfadc") return analogy_3cosadd_ivfadc(s, a, b, c, result);
  return fail(-1, "function %s(unknown, unknown, unknown) does not exist", f.c_str());
}
// EXECUTE format('SELECT * FROM %s(''%s'', ''%s'',''%s'', ''%s''::varchar(100)[])', get_analogy_in_function_name(), ...)
int analogy_in(freddy_session_t* s, int32_t w1, int32_t w2, int32_t w3, const int32_t* input_ids, int32_t n_ids, int32_t* result) {
  if (!s || !result) return fail(-1, "bad argument");
  const std::string& f = s->analogy_in_fn;
  if (f == "analogy_3cosadd_in") return analogy_3cosadd_in(s, w1, w2, w3, input_ids, n_ids, result);
  if (f == "analogy_3cosadd_in_pq") return analogy_3cosadd_in_pq(s, w1, w2, w3, input_ids, n_ids, result);
  if (f == "analogy_3cosadd_in_ivpq") return analogy_3cosadd_in_ivpq(s, w1, w2, w3, input_ids, n_ids, result);
  return fail(-1, "function %s(unknown, unknown, unknown, character varying[]) does not exist", f.c_str());
}

// ---- the exact kNN-join and the grouping dispatcher          freddy--0.0.1.sql:456-501, 1462-1484, 299-311 --------------
// one freddy_gpu_exact_join over `queries`; rows of query i carry qids[i]
static int exact_join_rows(freddy_session_t* s, const float* queries, const int32_t* qids, int32_t nq, int32_t k, const int32_t* input_ids,
                           int32_t n_ids, freddy_row3* out, int32_t* n_rows) {
  if (n_rows) *n_rows = 0;
  if (k > 4096) return fail(-1, "k=%d exceeds this build's limit of 4096", k);   // (the device call's limit, before the table is pinned)
  if (nq == 0) return 0;
  REQUIRE(s->norm.pinned(s->device));
  std::vector<int32_t> ids((size_t)nq * k); std::vector<float> sim((size_t)nq * k);
  if (int rc = freddy_gpu_exact_join(s->norm.h, queries, nq, k, input_ids, n_ids, ids.data(), sim.data())) return gpu_fail(rc);
  return rows_out(n_rows, emit_lists(qids, nq, k, ids, sim, out));
}

int knn_search_in_batch(freddy_session_t* s, const float* queries, int32_t n_queries, int32_t dim, int32_t k, const int32_t* input_ids,
                        int32_t n_ids, freddy_row3* out, int32_t* n_rows) {
  REQUIRE(need_vecs_of_dim(s, dim));
  if (k <= 0 || n_queries < 0 || n_ids < 0 || !out || (n_queries > 0 && !queries) || (n_ids > 0 && !input_ids)) return fail(-1, "bad argument");
  std::vector<int32_t> qids((size_t)n_queries);
  std::iota(qids.begin(), qids.end(), 1);
  return exact_join_rows(s, queries, qids.data(), n_queries, k, input_ids, n_ids, out, n_rows);
}

// the rows of google_vecs_norm behind `ids`, in argument order (an unknown id yields nothing, a duplicate is answered again)
static void known_rows(const freddy_session_t* s, const int32_t* ids, size_t n, std::vector<int32_t>& qids, std::vector<float>& qv) {
  for (size_t i = 0; i < n; ++i)
    if (const float* v = s->norm.find(ids[i])) { qids.push_back(ids[i]); qv.insert(qv.end(), v, v + s->norm.d); }
}

int knn_search_in_batch_ids(freddy_session_t* s, const int32_t* query_ids, int32_t n_queries, int32_t k, const int32_t* input_ids,
                            int32_t n_ids, freddy_row3* out, int32_t* n_rows) {
  REQUIRE(need_vecs(s));
  if (k <= 0 || n_queries < 0 || n_ids < 0 || !out || (n_queries > 0 && !query_ids) || (n_ids > 0 && !input_ids)) return fail(-1, "bad argument");
  std::vector<int32_t> qids;
  std::vector<float> qv;
  known_rows(s, query_ids, (size_t)n_queries, qids, qv);
  return exact_join_rows(s, qv.data(), qids.data(), (int32_t)qids.size(), k, input_ids, n_ids, out, n_rows);
}

// knn_in_ivpq_batch(query_set varchar[], ...) (freddy--0.0.1.sql:720-761): the queries are rows of google_vecs_norm.  knn_search_in_batch_ids'
// rule -- argument order, an unknown id yields nothing, a duplicate is answered again, rows carry the query's id -- and knn_join's
// lists; the vectors stay on the device (freddy_gpu_knn_join_ids over the pinned vector table).
int knn_in_ivpq_batch_ids(freddy_session_t* s, const int32_t* query_ids, int32_t n_queries, int32_t k, const int32_t* input_ids, int32_t n_ids,
                          freddy_row3* out, int32_t* n_rows) {
  REQUIRE(need_table_and_norm(s, IVPQ));
  if (k <= 0 || n_queries < 0 || n_ids < 0 || !out || (n_queries > 0 && !query_ids) || (n_ids > 0 && !input_ids)) return fail(-1, "bad argument");
  if (n_rows) *n_rows = 0;
  std::vector<int32_t> qids;
  for (int32_t i = 0; i < n_queries; ++i) if (s->norm.find(query_ids[i])) qids.push_back(query_ids[i]);
  const int32_t Q = (int32_t)qids.size();
  if (Q == 0) return 0;
  std::vector<int32_t> ids((size_t)Q * k), sel((size_t)Q);
  std::vector<float> dist((size_t)Q * k);
  if (!freddy_gpu_knn_join_ids) {
    std::vector<float> qv;
    for (int32_t id : qids) { const float* v = s->norm.find(id); qv.insert(qv.end(), v, v + s->norm.d); }
    REQUIRE(session_knn_join(s, qv.data(), Q, k, input_ids, n_ids, ids.data(), dist.data()));
    return emit3(qids.data(), Q, k, ids, dist, out, n_rows);
  }
  REQUIRE(s->norm.pinned(s->device));
  int32_t nq = 0;
  if (int rc = freddy_gpu_knn_join_ids(s->code[IVPQ].h, s->norm.h, qids.data(), Q, FREDDY_QIDS_POSITIONAL, k, input_ids, n_ids, s->alpha, s->pvf,
                                       s->method_flag, s->use_targetlist, s->confidence, s->long_codes_threshold, sel.data(), &nq, ids.data(), dist.data(),
                                       nullptr))
    return gpu_fail(rc);
  return emit3(qids.data(), Q, k, ids, dist, out, n_rows);
}

int grouping_func(freddy_session_t* s, const int32_t* token_ids, int32_t n_tokens, const int32_t* group_ids, int32_t n_groups,
                  freddy_group_row* out, int32_t* n_rows) {
  REQUIRE(need_vecs(s));
  if (n_tokens < 0 || n_groups < 0 || !out || (n_tokens > 0 && !token_ids) || (n_groups > 0 && !group_ids)) return fail(-1, "bad argument");
  // "FROM google_vecs_norm AS v1 ... WHERE v1.word = ANY(tokens)": every token that is a row, once, in table order
  std::vector<int32_t> toks(token_ids, token_ids + n_tokens);
  std::sort(toks.begin(), toks.end());
  toks.erase(std::unique(toks.begin(), toks.end()), toks.end());
  std::vector<int32_t> qids;
  std::vector<float> qv;
  known_rows(s, toks.data(), toks.size(), qids, qv);
  std::vector<freddy_row3> rows(qids.size());
  int32_t n = 0;
  REQUIRE(exact_join_rows(s, qv.data(), qids.data(), (int32_t)qids.size(), 1, group_ids, n_groups, rows.data(), &n));
  for (int32_t i = 0; i < n; ++i) out[i] = {rows[(size_t)i].query_id, rows[(size_t)i].id};
  return rows_out(n_rows, n);
}

// EXECUTE format('SELECT * FROM %s(''%s''::varchar(100)[], ''%s''::varchar(100)[])', get_groups_function_name(), ...)
int groups(freddy_session_t* s, const int32_t* token_ids, int32_t n_tokens, const int32_t* group_ids, int32_t n_groups,
           freddy_group_row* out, int32_t* n_rows) {
  if (!s) return fail(-1, "bad argument");
  const std::string& f = s->groups_fn;
  if (f == "grouping_func") return grouping_func(s, token_ids, n_tokens, group_ids, n_groups, out, n_rows);
  if (f == "grouping_func_pq") return grouping_pq(s, token_ids, n_tokens, group_ids, n_groups, out, n_rows);
  return fail(-1, "function %s(character varying[], character varying[]) does not exist", f.c_str());
}

// The assignment step of generic_cluster (cluster.h) on its own, by row id (include/freddy_gpu.h: freddy_gpu_exact_assign / freddy_gpu_pq_assign).
int exact_assign(freddy_session_t* s, const float* queries, int32_t n_queries, int32_t dim, const int32_t* target_ids, int64_t n_targets,
                 int32_t* out_query, float* out_sim) {
  REQUIRE(need_vecs_of_dim(s, dim));
  REQUIRE(s->norm.pinned(s->device));
  if (int rc = freddy_gpu_exact_assign(s->norm.h, queries, n_queries, target_ids, n_targets, out_query, out_sim)) return gpu_fail(rc);
  return 0;
}
int pq_assign(freddy_session_t* s, const float* queries, int32_t n_queries, int32_t dim, const int32_t* target_ids, int64_t n_targets,
              int32_t* out_query, float* out_sim) {
  REQUIRE(need_table_of_dim(s, PQ, dim));
  if (int rc = freddy_gpu_pq_assign(s->code[PQ].h, queries, n_queries, kFiller, target_ids, n_targets, out_query, out_sim)) return gpu_fail(rc);
  return 0;
}

int cluster_exact(freddy_session_t* s, const int32_t* token_ids, int32_t n, int32_t k, const double* draws, int32_t n_draws, int32_t* cluster_out) {
  return generic_cluster(s, 0, token_ids, n, k, draws, n_draws, cluster_out);
}
int cluster_pq(freddy_session_t* s, const int32_t* token_ids, int32_t n, int32_t k, const double* draws, int32_t n_draws, int32_t* cluster_out) {
  return generic_cluster(s, 1, token_ids, n, k, draws, n_draws, cluster_out);
}
int cluster_ivpq(freddy_session_t* s, const int32_t* token_ids, int32_t n, int32_t k, const double* draws, int32_t n_draws, int32_t* cluster_out) {
  return generic_cluster(s, 2, token_ids, n, k, draws, n_draws, cluster_out);
}

void freddy_emit_row2(const freddy_row2* row, char values[2][16]) {
  snprintf(values[0], 16, "%d", row->id);
  snprintf(values[1], 16, "%f", row->distance);
}

void freddy_emit_row3(const freddy_row3* row, char values[3][16]) {
  snprintf(values[0], 16, "%d", row->query_id);
  snprintf(values[1], 16, "%d", row->id);
  snprintf(values[2], 16, "%f", row->distance);
}

}  // extern "C"
