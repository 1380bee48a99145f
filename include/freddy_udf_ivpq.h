/* freddy_udf_ivpq.h -- the host mirror's forms of the kNN-join family whose queries are named by row id (libfreddy_host.so, beside
 * include/freddy_udf.h, whose session and row types they use).  Both keep their queries on the device: the ids go to
 * freddy_gpu_knn_join_ids / freddy_gpu_ivpq_analogy (include/freddy_gpu.h) with the pinned vector table of the session.
 *
 * knn_in_ivpq_batch(query_set varchar[], ...)              freddy--0.0.1.sql:720-761
 *   the queries are rows of google_vecs_norm, named by id.  The rule of knn_search_in_batch_ids -- argument order, an unknown id
 *   yields no rows, a duplicate is answered again, rows carry the query's id -- and knn_join's rows over those vectors (k per
 *   query, fillers included), with alpha / pvf / method / use_targetlist / confidence / long_codes_threshold from the getters.
 *   out must hold n_queries * k rows.
 * analogy_3cosadd_in_ivpq for n triples                    freddy--0.0.1.sql:1383-1425
 *   the rule of the other _batch analogies of freddy_udf.h: results[i] = what analogy_3cosadd_in_ivpq returns for triples[i] (-1
 *   where the SQL returns NULL), all n triples in ONE device call -- one kNN-join per pass of triples instead of one per triple --
 *   with the SQL's literal n_cand = 4, k = 1 and the join's settings from the getters.
 * Loaded beside a libfreddy_gpu.so that lacks the two device entry points (the ABI version did not move with them), both run what
 * their callers ran before: the join over vectors gathered from the session's host copy, the loop of single-triple calls. */
#ifndef FREDDY_UDF_IVPQ_H
#define FREDDY_UDF_IVPQ_H

#include "freddy_udf.h"

#ifdef __cplusplus
extern "C" {
#endif

int knn_in_ivpq_batch_ids(freddy_session_t* s, const int32_t* query_ids, int32_t n_queries, int32_t k, const int32_t* input_ids,
                          int32_t n_ids, freddy_row3* out, int32_t* n_rows);
int analogy_3cosadd_in_ivpq_batch(freddy_session_t* s, const int32_t* triples /*[n][3]*/, int32_t n, const int32_t* input_ids, int32_t n_ids,
                                  int32_t* results /*[n]*/);

#ifdef __cplusplus
}
#endif
#endif /* FREDDY_UDF_IVPQ_H */
