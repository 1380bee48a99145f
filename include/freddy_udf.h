/*
 * freddy_udf.h -- host-side mirror of the FREDDY search UDFs (C ABI, libfreddy_host.so).
 *
 * PostgreSQL is not available in this image, so this library stands where the extension's
 * SRF hosts (freddy_extension/freddy.c, ivpq_search_in.c) stand: it owns what the SQL layer
 * owns -- the tables, the set_*()/get_*() "config functions" (freddy--0.0.1.sql:5-132,188-194),
 * id -> vector lookup, "WHERE id IN (...)" semantics, row emission -- and forwards the search
 * itself through the device C ABI (include/freddy_gpu.h).  Function names, argument order and
 * meaning, result row shapes and error messages follow the reference UDFs, so a test written
 * against this header reads like a SQL call of the extension.
 *
 * Every function returns 0 or a negative code; freddy_udf_last_error() gives the message the
 * reference would have raised with elog(ERROR, ...).
 */
#ifndef FREDDY_UDF_H
#define FREDDY_UDF_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct freddy_session freddy_session_t;

/* result rows: (Id, Distance)  freddy.c:142-146 ; (QueryId, TargetId|Id, Distance)  freddy.c:643-649,988-994 */
typedef struct freddy_row2 { int32_t id; float distance; } freddy_row2;
typedef struct freddy_row3 { int32_t query_id; int32_t id; float distance; } freddy_row3;
typedef struct freddy_group_row { int32_t id; int32_t group_id; } freddy_group_row;   /* grouping_pq: (Ids, GroupIds) */

int freddy_session_open(int device, freddy_session_t** out);
int freddy_session_close(freddy_session_t* s);
const char* freddy_udf_last_error(void);
/* The device handle behind a table group, for the diagnostics of include/freddy_gpu.h (freddy_gpu_profile_*, freddy_gpu_last_*):
 * "pq", "ivfadc", "ivpq" or "vecs" (google_vecs_norm, pinned by the first function that needs it); NULL while it is not pinned.
 * The session keeps the handle: the caller must not unpin it.  (void*: this header does not include freddy_gpu.h.) */
void* freddy_session_gpu_index(const freddy_session_t* s, const char* table);

/* ---- tables (what the index_creation scripts insert; rows may come in any order) -------- */
/* google_vecs_norm (id, vector)                                   vec2database.py:47-58 */
int freddy_load_vecs_norm(freddy_session_t* s, const int32_t* ids, const float* vectors, int64_t N, int32_t d);
/* pq_codebook (pos, code, vector) + pq_quantization (id, vector)   pq_index.py:25-26 */
int freddy_load_pq(freddy_session_t* s, const int32_t* cb_pos, const int32_t* cb_code, const float* cb_vectors,
                   int32_t n_entries, int32_t sub_dim, const int32_t* ids, const int16_t* codes, int64_t N);
/* coarse_quantization (id, vector) + residual_codebook + fine_quantization (id, coarse_id, vector)  ivfadc.py:28-30 */
int freddy_load_ivfadc(freddy_session_t* s, const int32_t* coarse_ids_tbl, const float* coarse_vectors, int32_t C,
                       const int32_t* cb_pos, const int32_t* cb_code, const float* cb_vectors, int32_t n_entries,
                       int32_t sub_dim, const int32_t* ids, const int32_t* coarse_id, const int16_t* codes, int64_t N);
/* codebook_ivpq + coarse_quantization_ivpq (pos, code, vector) + fine_quantization_ivpq (id, coarse_id, vector)
 * + stat table (coarse_id, coarse_freq); vectors for methods 1/2 come from google_vecs_norm.   ivpq.py:18-38 */
int freddy_load_ivpq(freddy_session_t* s, const int32_t* cb_pos, const int32_t* cb_code, const float* cb_vectors,
                     int32_t n_entries, int32_t sub_dim, const int32_t* cq_pos, const int32_t* cq_code,
                     const float* cq_vectors, int32_t n_cq_entries, const int32_t* ids, const int32_t* coarse_id,
                     const int16_t* codes, int64_t N, const int32_t* stat_coarse_id, const float* stat_freq,
                     int32_t n_stat);

/* ---- index files ("Postgres tables -> flat binary -> HBM loader") ------------------------
 * One little-endian container of named arrays, the tables exactly as the index_creation scripts insert
 * them (the reference exports a Python pickle, index_manager.py:10-18; this is the language-neutral
 * counterpart):
 *   "FRDYIDX1" | uint32 n_arrays | n_arrays x { uint16 name_len | name | uint8 dtype (0 float32, 1 int32,
 *   2 int16) | uint8 ndim | uint64 dims[ndim] | padding to 8 | data | padding to 8 }
 * Array names are "<table>.<column>":
 *   google_vecs_norm.id/.vector | pq_codebook.pos/.code/.vector, pq_quantization.id/.vector |
 *   coarse_quantization.id/.vector, residual_codebook.pos/.code/.vector, fine_quantization.id/.coarse_id/.vector |
 *   codebook_ivpq.pos/.code/.vector, coarse_quantization_ivpq.pos/.code/.vector,
 *   fine_quantization_ivpq.id/.coarse_id/.vector, stat.coarse_id/.coarse_freq
 * freddy_index_file_write writes the arrays it is given; freddy_import_index reads a file and loads every
 * table group that is complete in it (same effect as the freddy_load_* calls; google_vecs_norm first). */
typedef struct freddy_file_array {
  const char* name;
  int32_t dtype;        /* 0 float32, 1 int32, 2 int16 */
  int32_t ndim;         /* 1 or 2 */
  int64_t dims[2];
  const void* data;
} freddy_file_array;
int freddy_index_file_write(const char* path, const freddy_file_array* arrays, int32_t n_arrays);
int freddy_import_index(freddy_session_t* s, const char* path);

/* ---- config functions                                    freddy--0.0.1.sql:21-132, 188-194 */
int freddy_set_w(freddy_session_t* s, int32_t w);                       /* default 3 */
int freddy_set_pvf(freddy_session_t* s, int32_t pvf);                   /* default 20 */
int freddy_set_alpha(freddy_session_t* s, int32_t alpha);               /* default 3 */
int freddy_set_confidence_value(freddy_session_t* s, float c);          /* default 0.8 */
int freddy_set_long_codes_threshold(freddy_session_t* s, int32_t t);    /* default 10000000 */
int freddy_set_method_flag(freddy_session_t* s, int32_t m);             /* default 0 */
int freddy_set_use_targetlist(freddy_session_t* s, int32_t flag);       /* default true */
int32_t freddy_get_w(const freddy_session_t* s);
int32_t freddy_get_pvf(const freddy_session_t* s);
int32_t freddy_get_alpha(const freddy_session_t* s);
float freddy_get_confidence_value(const freddy_session_t* s);
int32_t freddy_get_long_codes_threshold(const freddy_session_t* s);
int32_t freddy_get_method_flag(const freddy_session_t* s);
int32_t freddy_get_use_targetlist(const freddy_session_t* s);

/* ---- the UDFs (out arrays are caller-allocated; *n_rows receives the number of rows) ----- */
/* pq_search(bytea, int) -> SETOF (Id, Distance)                              freddy.c:28-171 */
int pq_search(freddy_session_t* s, const float* query, int32_t dim, int32_t k, freddy_row2* out, int32_t* n_rows);
/* ivfadc_search(bytea, int) -> SETOF (Id, Distance); W = get_w()            freddy.c:174-410 */
int ivfadc_search(freddy_session_t* s, const float* query, int32_t dim, int32_t k, freddy_row2* out, int32_t* n_rows);
/* pq_search_in(bytea, int, int[]) -> SETOF (Id, Distance)                  freddy.c:1028-1174 */
int pq_search_in(freddy_session_t* s, const float* query, int32_t dim, int32_t k, const int32_t* input_ids,
                 int32_t n_ids, freddy_row2* out, int32_t* n_rows);
/* pq_search_in_batch(bytea[], int[], int, int[], bool) -> SETOF (QueryId, TargetId, Distance)  freddy.c:412-676
 * out holds n_queries*k rows, query-major, rank-minor. */
int pq_search_in_batch(freddy_session_t* s, const float* queries, int32_t n_queries, int32_t dim,
                       const int32_t* query_ids, int32_t n_query_ids, int32_t k, const int32_t* input_ids,
                       int32_t n_ids, int32_t use_target_lists, freddy_row3* out, int32_t* n_rows);
/* ivfadc_batch_search(int[], int) -> SETOF (QueryId, Id, Distance)          freddy.c:677-1025
 * queries = rows of google_vecs_norm whose id is in query_ids, in table order (ascending id),
 * duplicates and unknown ids dropped; out must hold n_query_ids*k rows. */
int ivfadc_batch_search(freddy_session_t* s, const int32_t* query_ids, int32_t n_query_ids, int32_t k,
                        freddy_row3* out, int32_t* n_rows);
/* ivpq_search_in(bytea[], int[], int, int[], int, int, int, bool, float4, int)   ivpq_search_in.c:59-721 */
int ivpq_search_in(freddy_session_t* s, const float* queries, int32_t n_queries, int32_t dim, const int32_t* query_ids,
                   int32_t n_query_ids, int32_t k, const int32_t* input_ids, int32_t n_ids, int32_t alpha, int32_t pvf,
                   int32_t method, int32_t use_target_lists, float confidence, int32_t double_threshold,
                   freddy_row3* out, int32_t* n_rows);
/* knn_in_ivpq_batch's parameter plumbing (freddy--0.0.1.sql:720-828): ivpq_search_in with
 * alpha/pvf/method/use_targetlist/confidence/long_codes_threshold taken from the getters. */
int knn_join(freddy_session_t* s, const float* queries, int32_t n_queries, int32_t dim, const int32_t* query_ids,
             int32_t k, const int32_t* input_ids, int32_t n_ids, freddy_row3* out, int32_t* n_rows);
/* (the same by query id, and analogy_3cosadd_in_ivpq for a batch of triples: include/freddy_udf_ivpq.h) */

/* Next row: the exact brute-force functions, by row id instead of word.
 * k_nearest_neighbour(bytea, int)             freddy--0.0.1.sql:426-439
 * knn_in_exact(bytea, int, integer[])         freddy--0.0.1.sql:1041-1054
 * ORDER BY cosine_similarity_bytea(q, vector) DESC FETCH FIRST k ROWS ONLY over google_vecs_norm;
 * row.distance carries the SIMILARITY; *n_rows <= k (fewer when fewer rows qualify). */
int k_nearest_neighbour(freddy_session_t* s, const float* query, int32_t dim, int32_t k, freddy_row2* out, int32_t* n_rows);
int knn_in_exact(freddy_session_t* s, const float* query, int32_t dim, int32_t k, const int32_t* input_ids, int32_t n_ids,
                 freddy_row2* out, int32_t* n_rows);

/* Next row: grouping and analogy on the same kernels, keyed by row id instead of word.
 * grouping_pq(integer[], integer[]) -> SETOF (Ids, GroupIds)                 freddy.c:1176-1401
 *   rows of pq_quantization with id IN input_ids (table order), each with the nearest of the groups
 *   (ADC distance to the group's normalised vector; groups tried in ascending id, first nearest wins;
 *   group_id -1 if none is nearer than 100).  Error "Group ids do not exist" as the reference.
 * analogy_3cosadd_pq / analogy_3cosadd_ivfadc                               freddy--0.0.1.sql:1317-1346, 1428-1460
 *   q = vec_normalize(v3 - v1 + v2); candidates = pq_search / ivfadc_search(q, get_pvf() + 3) minus the
 *   three inputs; result = the candidate with the largest cosine_similarity_bytea(v3 - v1 + v2, v4)
 *   (-1: none, the SQL returns NULL). */
int grouping_pq(freddy_session_t* s, const int32_t* input_ids, int32_t n_ids, const int32_t* group_ids, int32_t n_groups,
                freddy_group_row* out, int32_t* n_rows);
int analogy_3cosadd_pq(freddy_session_t* s, int32_t id1, int32_t id2, int32_t id3, int32_t* result);
int analogy_3cosadd_ivfadc(freddy_session_t* s, int32_t id1, int32_t id2, int32_t id3, int32_t* result);

/* The plpgsql callers of the two single-query SRFs, keyed by row id; row.distance
 * carries the SIMILARITY, *n_rows <= k (the joins drop the (-1, sentinel) filler rows).
 * k_nearest_neighbour_pq / k_nearest_neighbour_ivfadc (bytea, int)        freddy--0.0.1.sql:610-622, 520-531
 *   similarity = (1.0 - (distance / 2.0))::float4 of the distance as the SRF emits it ("%f")
 * k_nearest_neighbour_pq_pv / k_nearest_neighbour_ivfadc_pv (bytea, int)  freddy--0.0.1.sql:625-641, 575-591
 *   get_pvf() * k candidates, re-ranked by cosine_similarity_bytea(q, vector) DESC, first k */
int k_nearest_neighbour_pq(freddy_session_t* s, const float* query, int32_t dim, int32_t k, freddy_row2* out, int32_t* n_rows);
int k_nearest_neighbour_ivfadc(freddy_session_t* s, const float* query, int32_t dim, int32_t k, freddy_row2* out, int32_t* n_rows);
int k_nearest_neighbour_pq_pv(freddy_session_t* s, const float* query, int32_t dim, int32_t k, freddy_row2* out, int32_t* n_rows);
int k_nearest_neighbour_ivfadc_pv(freddy_session_t* s, const float* query, int32_t dim, int32_t k, freddy_row2* out, int32_t* n_rows);

/* knn_in_pq(anyarray, int, int[]) and k_nearest_neighbour_ivfadc_batch(varchar[], int) (by query ids):
 * pq_search_in / ivfadc_batch_search with the same similarity mapping     freddy--0.0.1.sql:830-843, 535-553 */
int knn_in_pq(freddy_session_t* s, const float* query, int32_t dim, int32_t k, const int32_t* input_ids, int32_t n_ids,
              freddy_row2* out, int32_t* n_rows);
int k_nearest_neighbour_ivfadc_batch(freddy_session_t* s, const int32_t* query_ids, int32_t n_query_ids, int32_t k,
                                     freddy_row3* out, int32_t* n_rows);

/* The batch form of the two post-verification functions, by query ids, and the reference's knn_batch() dispatcher.
 * k_nearest_neighbour_ivfadc_pv_batch / k_nearest_neighbour_pq_pv_batch (varchar[], int)
 *   queries = the rows of google_vecs_norm whose id is in query_ids, in table order, duplicates and unknown ids dropped (as
 *   ivfadc_batch_search chooses its queries); for each the rows of k_nearest_neighbour_ivfadc_pv (_pq_pv) for that vector with
 *   get_pvf() / get_w(), as (query_id, id, similarity), query-major; fewer than k rows for a query when fewer of its candidates
 *   have vectors.  ONE device call (freddy_gpu_ivfadc_search_pv / freddy_gpu_pq_search_pv): candidates are re-ranked on the device.
 *   get_pvf() * k > 4096 fails as the single-query functions do.  out must hold n_query_ids * k rows.
 * knn_batch(query_set, k)                                  freddy--0.0.1.sql:92-98, 197, 232-246
 *   calls the function set_knn_batch_function named (default k_nearest_neighbour_ivfadc_batch): that one or one of the two above.
 *   Any other name fails at call time: "function <name>(character varying[], integer) does not exist". */
int k_nearest_neighbour_ivfadc_pv_batch(freddy_session_t* s, const int32_t* query_ids, int32_t n_query_ids, int32_t k,
                                        freddy_row3* out, int32_t* n_rows);
int k_nearest_neighbour_pq_pv_batch(freddy_session_t* s, const int32_t* query_ids, int32_t n_query_ids, int32_t k,
                                    freddy_row3* out, int32_t* n_rows);
int freddy_set_knn_batch_function(freddy_session_t* s, const char* name);    /* default "k_nearest_neighbour_ivfadc_batch" */
const char* freddy_get_knn_batch_function(const freddy_session_t* s);
int knn_batch(freddy_session_t* s, const int32_t* query_ids, int32_t n_query_ids, int32_t k, freddy_row3* out, int32_t* n_rows);

/* Next row (remainder): analogy over an input set and the clustering functions, by row id.
 * analogy_3cosadd_in_pq / analogy_3cosadd_in_ivpq                        freddy--0.0.1.sql:1348-1426
 *   as analogy_3cosadd_pq, candidates from pq_search_in(q, get_pvf() + 3, input ids) resp.
 *   ivpq_search_in(ARRAY[q], '{0}', 4, input ids, get_alpha(), get_pvf(), get_method_flag(), ...) (k is the literal 4 there).
 * cluster_exact / cluster_pq / cluster_ivpq = generic_cluster             freddy--0.0.1.sql:1086-1209
 *   k-means in the reference's plpgsql: k random tokens as initial centroids, 10 rounds of "every token goes to the
 *   centroid that lists it with the highest similarity" (rows of knn_search_in_batch / knn_in_pq_batch /
 *   knn_in_ivpq_batch with k = all tokens, ORDER BY similarity DESC; ties: centroid, then token position), centroids
 *   re-estimated by centroid_bytea over 10 random members -- empty clusters draw their samples and keep their
 *   centroid, as the reference does.  `draws` are the values random() returns, in call order (k, then 10 per
 *   cluster and round): a caller-supplied sequence makes a run reproducible; once it is used up (or NULL) an
 *   internal generator continues.  cluster_out[i] = 1..k for token i (0: no centroid listed it).
 *   cluster_exact and cluster_pq take any number of tokens and are ONE device call (freddy_gpu_cluster): the draw sequence is filled
 *   first -- the caller's draws, then the internal generator, k + 90 k values -- and the ten rounds (the assignment of exact_assign /
 *   pq_assign below, the member ranks, the ten samples and their mean) stay on the device; a run with or without supplied draws
 *   returns what the loop around the assign calls returned.  (Loaded beside a libfreddy_gpu.so without that entry point, the mirror
 *   runs that loop.)  cluster_ivpq needs the kNN-join's lists themselves and keeps freddy_gpu_knn_join's limits on k = n. */
int analogy_3cosadd_in_pq(freddy_session_t* s, int32_t id1, int32_t id2, int32_t id3, const int32_t* input_ids, int32_t n_ids, int32_t* result);
/* The batch forms of the approximate analogies: results[i] = what the single-triple function returns for triples[i] (-1 where the SQL
 * returns NULL), all n triples in ONE device call (freddy_gpu_ivfadc_analogy / freddy_gpu_pq_analogy, approx_analogy.h) with
 * n_cand = get_pvf() + 3, k = 1 and the sentinels and W of the single-triple functions -- instead of a search and a host loop over
 * the candidates per triple.  analogy_3cosadd_in_ivpq goes through the kNN-join with the literal k = 4; its batch form is declared in
 * include/freddy_udf_ivpq.h. */
int analogy_3cosadd_pq_batch(freddy_session_t* s, const int32_t* triples /*[n][3]*/, int32_t n, int32_t* results /*[n]*/);
int analogy_3cosadd_ivfadc_batch(freddy_session_t* s, const int32_t* triples /*[n][3]*/, int32_t n, int32_t* results /*[n]*/);
int analogy_3cosadd_in_pq_batch(freddy_session_t* s, const int32_t* triples /*[n][3]*/, int32_t n, const int32_t* input_ids, int32_t n_ids,
                                int32_t* results /*[n]*/);
int analogy_3cosadd_in_ivpq(freddy_session_t* s, int32_t id1, int32_t id2, int32_t id3, const int32_t* input_ids, int32_t n_ids, int32_t* result);
int cluster_exact(freddy_session_t* s, const int32_t* token_ids, int32_t n, int32_t k, const double* draws, int32_t n_draws, int32_t* cluster_out);
int cluster_pq(freddy_session_t* s, const int32_t* token_ids, int32_t n, int32_t k, const double* draws, int32_t n_draws, int32_t* cluster_out);
int cluster_ivpq(freddy_session_t* s, const int32_t* token_ids, int32_t n, int32_t k, const double* draws, int32_t n_draws, int32_t* cluster_out);
/* The assignment step of cluster_exact / cluster_pq on its own (freddy--0.0.1.sql:1115-1127): out_query[i] = the 0-based index of the
 * query (centroid) that lists target_ids[i] first under "similarity DESC, query ASC", out_sim[i] its similarity -- the
 * cosine_similarity_bytea bits for exact_assign, (1.0 - (distance / 2.0))::float4 of the emitted ADC distance for pq_assign
 * (sentinel 1000, as knn_in_pq_batch's pq_search_in_batch); (-1, -inf) for a target no query lists.  Any n_targets. */
int exact_assign(freddy_session_t* s, const float* queries /*[n_queries][dim]*/, int32_t n_queries, int32_t dim, const int32_t* target_ids,
                 int64_t n_targets, int32_t* out_query /*[n_targets]*/, float* out_sim /*[n_targets]*/);
int pq_assign(freddy_session_t* s, const float* queries /*[n_queries][dim]*/, int32_t n_queries, int32_t dim, const int32_t* target_ids,
              int64_t n_targets, int32_t* out_query /*[n_targets]*/, float* out_sim /*[n_targets]*/);

/* Exact analogies and the analogy dispatchers, by row id (analogy.h; the device entry point freddy_gpu_exact_analogy).
 * analogy_3cosadd / analogy_3cosadd_in                      freddy--0.0.1.sql:1270-1315
 * analogy_3cosmul                                           freddy--0.0.1.sql:1231-1249
 *   the row v4 (v4 not w1, w2, w3; _in: id = ANY(input_ids)) with the largest score, ties by lowest id; *result = -1 where the
 *   SQL returns NULL (an unknown input id, no row left).
 * analogy(a, b, c) / analogy_in(w1, w2, w3, input_set)      freddy--0.0.1.sql:269-297
 *   call the function set_analogy_function / set_analogy_in_function named (defaults analogy_3cosadd / analogy_3cosadd_in,
 *   :198-199).  The setters accept any name, as the SQL ones do; a name this library does not implement fails at call time
 *   with PostgreSQL's wording: "function <name>(unknown, unknown, unknown) does not exist" (analogy_in: "..., character
 *   varying[])").  analogy(): analogy_3cosadd, analogy_3cosmul, analogy_pair_direction, analogy_3cosadd_pq,
 *   analogy_3cosadd_ivfadc; analogy_in(): analogy_3cosadd_in, analogy_3cosadd_in_pq, analogy_3cosadd_in_ivpq (the reference has
 *   no _in form of analogy_pair_direction: that name fails there with the four-argument wording).
 * analogy_pair_direction                                    freddy--0.0.1.sql:1212-1229
 *   the row v4 (v4 not w1, w2, w3) with the largest cosine_similarity_bytea(vec_normalize(v1 - v2), vec_normalize(v3 - v4)) over
 *   google_vecs, the ORIGINAL (un-normalised) table (get_vecs_name_original()): freddy_load_vecs_original, rows in any order,
 *   pinned as a second vector handle on first use.  Error "google_vecs is not loaded" before that.  A row that repeats v3's
 *   vector under another id scores NaN and wins (NaN sorts first); *result = -1 where the SQL returns NULL.  insert_batch
 *   receives only normalised vectors and does not extend google_vecs: an id it created is unknown here and gives -1. */
int freddy_load_vecs_original(freddy_session_t* s, const int32_t* ids, const float* vectors, int64_t N, int32_t d);
int analogy_pair_direction(freddy_session_t* s, int32_t id1, int32_t id2, int32_t id3, int32_t* result);
int analogy_3cosadd(freddy_session_t* s, int32_t id1, int32_t id2, int32_t id3, int32_t* result);
int analogy_3cosmul(freddy_session_t* s, int32_t id1, int32_t id2, int32_t id3, int32_t* result);
int analogy_3cosadd_in(freddy_session_t* s, int32_t id1, int32_t id2, int32_t id3, const int32_t* input_ids, int32_t n_ids, int32_t* result);
int freddy_set_analogy_function(freddy_session_t* s, const char* name);
const char* freddy_get_analogy_function(const freddy_session_t* s);
int freddy_set_analogy_in_function(freddy_session_t* s, const char* name);
const char* freddy_get_analogy_in_function(const freddy_session_t* s);
int analogy(freddy_session_t* s, int32_t a, int32_t b, int32_t c, int32_t* result);
int analogy_in(freddy_session_t* s, int32_t w1, int32_t w2, int32_t w3, const int32_t* input_ids, int32_t n_ids, int32_t* result);

/* The exact kNN-join and the grouping dispatcher, by row id (the device entry point freddy_gpu_exact_join).
 * knn_search_in_batch(bytea[], int, varchar[])             freddy--0.0.1.sql:480-501
 *   query_id = 1-based index of the query; rows query-major, rank-minor; fewer than k rows for a query when fewer targets
 *   exist; row.distance carries the SIMILARITY.  out must hold n_queries * k rows.
 * knn_search_in_batch(varchar[], int, varchar[])           freddy--0.0.1.sql:456-478
 *   queries are rows of google_vecs_norm; query_id = the query's id; an unknown query id yields no rows (the INNER JOIN is
 *   empty); duplicates are answered once each, in argument order.
 * grouping_func(tokens, groups)                            freddy--0.0.1.sql:1462-1484
 *   (token id, group id) for every token that is a row, table order: knn_in(token, 1, groups) with the default knn_in_exact --
 *   ONE exact join, queries = the tokens' vectors, k = 1, targets = the groups (no rows when no group is a row: knn_in is empty).
 * groups(tokens, groups)                                   freddy--0.0.1.sql:299-311
 *   calls the function set_groups_function named (default grouping_func, :200): grouping_func | grouping_func_pq (= grouping_pq).
 *   Any other name fails at call time: "function <name>(character varying[], character varying[]) does not exist". */
int knn_search_in_batch(freddy_session_t* s, const float* queries, int32_t n_queries, int32_t dim, int32_t k,
                        const int32_t* input_ids, int32_t n_ids, freddy_row3* out, int32_t* n_rows);
int knn_search_in_batch_ids(freddy_session_t* s, const int32_t* query_ids, int32_t n_queries, int32_t k,
                            const int32_t* input_ids, int32_t n_ids, freddy_row3* out, int32_t* n_rows);
int grouping_func(freddy_session_t* s, const int32_t* token_ids, int32_t n_tokens, const int32_t* group_ids,
                  int32_t n_groups, freddy_group_row* out, int32_t* n_rows);
int freddy_set_groups_function(freddy_session_t* s, const char* name);       /* default "grouping_func" */
const char* freddy_get_groups_function(const freddy_session_t* s);
int groups(freddy_session_t* s, const int32_t* token_ids, int32_t n_tokens, const int32_t* group_ids, int32_t n_groups,
           freddy_group_row* out, int32_t* n_rows);

/* tokenize(text) / tokenize_raw(text) for a batch of texts, by row id        freddy--0.0.1.sql:1512-1536
 *   A text is the list of the row ids of its tokens: token_ids[offsets[n_texts]], offsets[n_texts + 1] (non-decreasing, from 0; at
 *   most FREDDY_TOK_MAX_LEN ids per text).  out_vectors[t] = centroid_bytea of "SELECT vector FROM <table> WHERE word = ANY(tokens)"
 *   -- the DISTINCT rows, in table order; unknown ids vanish -- through vec_normalize_bytea for tokenize_batch (google_vecs_norm) and
 *   as it is for tokenize_raw_batch (google_vecs: freddy_load_vecs_original; "google_vecs is not loaded" before that).  The rows are
 *   read where they are pinned (freddy_gpu_tokenize), bit for bit the reference's arithmetic.  out_count[t] = the rows that went into
 *   text t; 0 (no token is a row: the reference returns a zero-length bytea) leaves a vector of zeros. */
int tokenize_batch(freddy_session_t* s, const int32_t* token_ids, const int64_t* offsets, int32_t n_texts,
                   float* out_vectors /*[n_texts][d]*/, int32_t* out_count /*[n_texts]*/);
int tokenize_raw_batch(freddy_session_t* s, const int32_t* token_ids, const int64_t* offsets, int32_t n_texts,
                       float* out_vectors /*[n_texts][d]*/, int32_t* out_count /*[n_texts]*/);

/* Next row: insert_batch(varchar[]) -> int4                  freddy.c:1403-1658
 * The tokenisation sub-query (:1503-1519: tokenize(term) for the terms NOT yet in the vocabulary) has a device form for terms
 * whose tokens are rows, tokenize_batch above; splitting a term into words and looking the words up stays with SQL, and
 * the caller passes the result, the normalised vectors of the new terms.  Per vector: PQ code, coarse cell +
 * residual code, ivpq code + multi-index cell (device); the three codebooks' running update exactly as
 * updateCodebook / updateCodebookRelation compute and store it (index_utils.c:908-991, "%f" text included);
 * one row per table with id = max(id) + 1 of THAT table (index_utils.c:993-1074); every pinned index is extended in
 * HBM.  new_ids (may be NULL) receives the ids given in google_vecs_norm.  The count column of a codebook is 1
 * unless freddy_set_codebook_counts (table: 0 pq_codebook, 1 residual_codebook, 2 codebook_ivpq) has set it. */
int freddy_set_codebook_counts(freddy_session_t* s, int32_t table, const int32_t* pos, const int32_t* code, const int32_t* count, int32_t n);
int insert_batch(freddy_session_t* s, const float* norm_vectors, int32_t n, int32_t dim, int32_t* new_ids);
/* The mirror of DELETE FROM <table> WHERE id = ANY(ids) on EVERY table of the session (google_vecs_norm, google_vecs,
 * pq_quantization, fine_quantization, fine_quantization_ivpq): the rows leave the session's host tables, and every handle the
 * session has pinned loses them in HBM (freddy_gpu_remove_rows) instead of being pinned again.  ids in any order; duplicates
 * and ids no table has are skipped; a negative id is refused before anything changes.  *removed (may be NULL) receives the
 * number of rows that left google_vecs_norm.  Afterwards every UDF, and a following insert_batch (whose "max(id) + 1" sees
 * the rows that are left), behaves as on a session loaded from the remaining rows.  The codebooks and their count columns stay. */
int delete_rows(freddy_session_t* s, const int32_t* ids, int64_t n, int64_t* removed);
/* The mirror of UPDATE google_vecs_norm SET vector = ... WHERE id = ... together with the re-quantisation of the same ids in
 * pq_quantization, fine_quantization and fine_quantization_ivpq: the rows keep their ids; their codes and cells come from
 * freddy_gpu_insert_quantize against the session's CURRENT codebooks (the multi-index cell by insert_batch's formula), and the
 * vectors are stored as given.  The codebooks and their count columns do not change: plain DML does not run updateCodebook.
 * Every handle the session has pinned is updated in HBM (freddy_gpu_update_rows) instead of being pinned again, and the host
 * copy of google_vecs_norm follows; google_vecs (the original table) is not touched.  ids are handled per table as delete_rows
 * handles them -- an id a table does not have is skipped there -- but an id listed twice, like a negative one, is refused
 * before anything changes.  *updated (may be NULL) receives the number of rows of google_vecs_norm that changed.  A device
 * failure drops the handles and leaves the host tables as they were, as in insert_batch. */
int update_rows(freddy_session_t* s, const int32_t* ids, const float* norm_vectors, int64_t n, int32_t dim, int64_t* updated);
/* set_statistics_table(regclass) (freddy--0.0.1.sql:70) for the loaded ivpq tables: the (coarse_id, coarse_freq) rows of a stat
 * table, in the row form and under the checks of freddy_load_ivpq (cells + 1 rows, every coarse_id in [0, cells]), become the
 * statistics row of the pinned handle (freddy_gpu_set_statistics) -- the handle is not pinned again.
 * create_statistics(table, column, coarse_table) (:150-171) over the pinned rows: token_ids[0..n) are the row ids of the
 * column's tokens with their multiplicity (ids no row has are skipped); token_ids == NULL with n == 0 is every row once, the
 * default stat_google_vecs_norm_word.  The row is computed on the device, installed as the bootstrap block installs it
 * (:183-184) and copied to out_stats ([cells + 1], may be NULL).  A column none of whose tokens has a row is the SQL's division
 * by zero: an error, and the row in force stays.  freddy_statistics_rows: cells + 1 of the loaded ivpq tables (what n_stat
 * must be and out_stats must hold), 0 while they are not loaded. */
int32_t freddy_statistics_rows(const freddy_session_t* s);
int freddy_set_statistics_table(freddy_session_t* s, const int32_t* stat_coarse_id, const float* stat_freq, int32_t n_stat);
int create_statistics(freddy_session_t* s, const int32_t* token_ids, int64_t n, float* out_stats /* may be NULL */);

/* per-call row emit: snprintf("%d") / snprintf("%f") into 16-byte buffers   freddy.c:154-169,1001-1023 */
void freddy_emit_row2(const freddy_row2* row, char values[2][16]);
void freddy_emit_row3(const freddy_row3* row, char values[3][16]);

#ifdef __cplusplus
}
#endif
#endif /* FREDDY_UDF_H */
