/*
 * freddy_gpu.h -- C ABI of the MI355X (gfx950) search library behind the FREDDY UDFs.
 *
 * This is the drop-in boundary for the reference's hot path: the bodies of the
 * PostgreSQL SRFs in freddy_extension/freddy.c and freddy_extension/ivpq_search_in.c
 * stop scanning SPI tuples and call these entry points instead (INTEGRATION.md shows
 * the binding).  Plain pointers and sizes only; caller allocates every host buffer;
 * the library never retains a host pointer after a call returns, never throws and
 * never longjmps.  Every function returns 0 on success and a negative FREDDY_E_* code
 * on failure, with a message available from freddy_gpu_last_error().
 *
 * Threading: one caller thread per process (a PostgreSQL backend is single threaded,
 * SURVEY 8b).  HIP is initialised lazily on the first pin call -- never at library
 * load -- so a postmaster can dlopen() the extension and fork() safely.
 *
 * Numerics: all distances are IEEE binary32, computed with separately rounded
 * sub/mul/add in the reference's summation order (index_utils.c:500-508, :1126-1133);
 * result lists follow the reference's insertion rule including its tie behaviour
 * (index_utils.c:19-33), with the canonical scan order "ascending id".
 */
#ifndef FREDDY_GPU_H
#define FREDDY_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FREDDY_OK 0
#define FREDDY_E_ARG (-1)      /* bad argument (NULL, shape mismatch, unsupported size) */
#define FREDDY_E_HIP (-2)      /* HIP runtime / device failure */
#define FREDDY_E_NOMEM (-3)    /* host or device allocation failed */
#define FREDDY_E_KIND (-4)     /* index handle of the wrong kind for this call */
#define FREDDY_E_LIMIT (-5)    /* parameter beyond what this build supports (see message): k > 4096, W > 512 probes per round,
                                * k * pvf > 8192 (or k > 512) in the kNN-join, k * pvf > 4096 in the post verification, n_cand > 4096 in the approximate analogies, Q > 65536 in the assign calls, K > 32767, d > 1024 for training */

/* found_rule for freddy_gpu_ivfadc_search */
#define FREDDY_FOUND_ROWS 0      /* ivfadc_search:       found += rows retrieved  (freddy.c:377) */
#define FREDDY_FOUND_ACCEPTED 1  /* found += insertions (freddy.c:971) over ivfadc_search's cell choice */
#define FREDDY_FOUND_BATCH_UDF 2 /* ivfadc_batch_search itself: found += insertions (freddy.c:971) AND its cell choice --
                                  * argmin by strict "<" from minDist = 1000 (freddy.c:853-866), where ivfadc_search's cell
                                  * list never admits a cell at distance >= 100 (freddy.c:266-283).  W must be 1. */

/* calculationMethod, index_utils.h:111 */
#define FREDDY_METHOD_PQ 0
#define FREDDY_METHOD_EXACT 1
#define FREDDY_METHOD_PQ_PV 2

typedef struct freddy_gpu_index freddy_gpu_index_t; /* opaque, library-owned, HBM-resident */

/* ---- what gets pinned: the tables the reference re-reads through SPI on EVERY call ----- */

/* pq_codebook + pq_quantization.  Replaces getCodebook(CODEBOOK) (freddy.c:69,
 * index_utils.c:577-630) and "SELECT id, vector FROM pq_quantization" (freddy.c:96-100). */
typedef struct freddy_pq_desc {
  int32_t d;             /* vector dimensionality (300) */
  int32_t m;             /* sub-quantizers = codebook positions */
  int32_t K;             /* codes per sub-quantizer */
  int64_t N;             /* rows */
  const float* codebook; /* [m][K][d/m]  entry (pos, code) -> its centroid */
  const int32_t* ids;    /* [N] row ids, rows in canonical scan order (ascending id, unique) */
  const int16_t* codes;  /* [N][m] as stored in the bytea column (int16, index_utils.c:1088) */
} freddy_pq_desc;

/* coarse_quantization + residual_codebook + fine_quantization.  Replaces getCodebook +
 * getCoarseQuantizer (freddy.c:239-241,746-749; index_utils.c:531-575) and the per-round
 * "SELECT id, vector, coarse_id FROM fine_quantization WHERE coarse_id IN (...)"
 * (freddy.c:324-342, 915-935).  Rows are grouped into inverted lists by coarse id. */
typedef struct freddy_ivf_desc {
  int32_t d, m, K;
  int32_t C;               /* coarse cells; coarse id == array index (freddy.c:309,873) */
  int64_t N;
  const float* coarse;     /* [C][d] */
  const float* codebook;   /* [m][K][d/m] residual codebook */
  const int32_t* list_off; /* [C+1] CSR offsets into ids/codes */
  const int32_t* ids;      /* [N] ascending and unique inside each list, unique overall, >= 0 */
  const int16_t* codes;    /* [N][m] */
} freddy_ivf_desc;

/* codebook_ivpq + coarse_quantization_ivpq (2-position multi index) +
 * fine_quantization_ivpq (+ the normalised vectors the reference JOINs in for methods
 * 1 and 2) + the stat_* table.  Replaces getCodebook x2, getStatistics
 * (ivpq_search_in.c:218-232) and the per-iteration SELECT (ivpq_search_in.c:352-401). */
typedef struct freddy_ivpq_desc {
  int32_t d, m, K;
  int32_t coarse_positions; /* must be 2 (index_utils.c:322) */
  int32_t coarse_codes;     /* cells = coarse_codes^2, cell = code0 + coarse_codes*code1 */
  int64_t N;
  const float* codebook;    /* [m][K][d/m] */
  const float* coarse;      /* [2][coarse_codes][d/2] */
  const int32_t* ids;       /* [N] ascending, unique */
  const int32_t* coarse_id; /* [N] */
  const int16_t* codes;     /* [N][m] */
  const float* vectors;     /* [N][d] row-aligned with ids; NULL if methods 1/2 are never used */
  const float* stats;       /* [cells+1] coarse_freq; last = total count (freddy--0.0.1.sql:158-168) */
} freddy_ivpq_desc;

/* Copy the tables into HBM once (layouts re-organised for the kernels).  The host
 * arrays may be freed as soon as the call returns. */
int freddy_gpu_pin_pq(const freddy_pq_desc* desc, int device, freddy_gpu_index_t** out);
int freddy_gpu_pin_ivf(const freddy_ivf_desc* desc, int device, freddy_gpu_index_t** out);
int freddy_gpu_pin_ivpq(const freddy_ivpq_desc* desc, int device, freddy_gpu_index_t** out);
int freddy_gpu_unpin(freddy_gpu_index_t* index);

/* ---- searches (host buffers in, host buffers out, synchronous) --------------------------- */

/* Body of pq_search (freddy.c:28-152), pq_search_in (freddy.c:1028-1157) and
 * pq_search_in_batch (freddy.c:414-653): exhaustive ADC over all rows
 * (subset_ids == NULL) or over the rows whose id is in subset_ids ("WHERE id IN (...)":
 * duplicates and unknown ids are ignored), for Q query vectors at once.
 * sentinel: 100.0 for pq_search, 1000.0 for the _in variants.
 * out_ids/out_dist: [Q][k]; unfilled slots hold (-1, sentinel). */
int freddy_gpu_pq_search(freddy_gpu_index_t* pq, const float* queries, int32_t Q, int32_t k,
                         float sentinel, const int32_t* subset_ids, int64_t n_subset,
                         int32_t* out_ids, float* out_dist);

/* Body of ivfadc_search (freddy.c:174-393) for Q independent queries; with W == 1,
 * sentinel 100.0 and FREDDY_FOUND_BATCH_UDF it is the body of ivfadc_batch_search
 * (freddy.c:679-999).  Each round probes the W nearest not-yet-used cells; rounds repeat
 * while found < k (found_rule).  out_*: [Q][k]. */
int freddy_gpu_ivfadc_search(freddy_gpu_index_t* ivf, const float* queries, int32_t Q, int32_t k,
                             int32_t W, float sentinel, int32_t found_rule, int32_t* out_ids,
                             float* out_dist);

/* How the host-buffer IVFADC call runs (the reference makes one synchronous call per batch, freddy.c:679-999): a batch
 * larger than `pipeline_batch` (2048) queries is cut into equal sub-batches that go round-robin to up to four
 * library-owned streams ("lanes", two sub-batches queued on each), with pinned staging buffers: host copy of the
 * sub-batch's queries into pinned memory -> a copy kernel reads them over PCIe -> round one of the search, the lanes'
 * persistent scans sharing the CUs -> a copy kernel writes the lists into pinned memory.  The host waits only when it
 * needs a staging slot again and once per slot at the end.  Queries that round one leaves unfinished (their first W
 * cells hold fewer than k rows: rare) are searched again from the start with all their rounds where the host waits for
 * their sub-batch -- the search is deterministic, so that is the list the round-by-round continuation gives.  Results
 * do not depend on how a batch is cut.
 *
 * Query buffers obtained from freddy_gpu_host_alloc (pinned host memory) skip the staging copy: a host that decodes
 * its bytea / array arguments can write the floats straight into such a buffer.  freddy_gpu_host_free releases it. */
int freddy_gpu_host_alloc(void** out, size_t bytes);
int freddy_gpu_host_free(void* p);

/* Product-level multi-GPU (north_star: "partition queries across the 8 MI355X with a replicated index"): the ivf tables
 * pinned on EVERY device of devices[0 .. n_devices) behind one handle.  freddy_gpu_ivfadc_search on such a handle splits
 * the host batch contiguously over the devices (sizes differ by at most one; one host thread per device inside the
 * call) -- queries are independent (freddy.c:835-982 keeps no cross-query state) and the lists land in the caller's
 * host buffers, so no collective is needed.  The same device may be listed more than once (tests).  append_rows /
 * update_codebook / set_option / the self-check counters act on every replica; the *_dev entry point, the profile and
 * the freddy_gpu_last_* diagnostics act on devices[0] only.  freddy_gpu_replica_count: number of devices behind a handle. */
int freddy_gpu_pin_ivf_multi(const freddy_ivf_desc* desc, const int* devices, int n_devices, freddy_gpu_index_t** out);
int freddy_gpu_replica_count(const freddy_gpu_index_t* index);

/* Body of ivpq_search_in (ivpq_search_in.c:61-699), the kNN-join.  Arguments are the
 * SRF's own (ivpq_search_in.c:168-208).  iterations_out (may be NULL) receives the
 * number of alpha-doubling rounds.  out_*: [Q][k], sentinel 1000.0.
 * Bounds, refused with FREDDY_E_LIMIT before any device work (the message names the value): method 0 (ADC) and method 1
 * (exact) take k <= 4096 -- up to k = 512 one workgroup selects and replays a query's 2k candidates, beyond that the 2k keys are
 * selected 1024 per pass over the query's target rows and a second launch writes the lists in closed form (bigk.h; a workspace
 * of 16 k bytes per scanned query: 328 MB at 5 000 queries and k = 4096); method 2 (post verification) takes k * pvf <= 8192.
 * The lists are the reference's at every k: ids, ranks and distance bits. */
int freddy_gpu_knn_join(freddy_gpu_index_t* ivpq, const float* queries, int32_t Q, int32_t k,
                        const int32_t* target_ids, int64_t n_targets, int32_t alpha, int32_t pvf,
                        int32_t method, int32_t use_target_lists, float confidence,
                        int32_t double_threshold, int32_t* out_ids, float* out_dist,
                        int32_t* iterations_out);

/* ---- next row after the PQ / IVFADC / kNN-join path: exact brute-force kNN --------
 * google_vecs_norm pinned as raw vectors.  Replaces the SQL of k_nearest_neighbour
 * (freddy--0.0.1.sql:426-454) and knn_in_exact (:991-1084):
 *   ORDER BY cosine_similarity_bytea(q, v.vector) DESC FETCH FIRST k ROWS ONLY
 * with cosine_similarity_bytea = the binary32 chain "scalar += v1[i] * v2[i]"
 * (core_functions.c:67-81), reproduced bit for bit.  Equal similarities are returned in
 * ascending id (PostgreSQL leaves their order unspecified). */
typedef struct freddy_vec_desc {
  int32_t d;
  int64_t N;
  const int32_t* ids;     /* [N] strictly ascending */
  const float* vectors;   /* [N][d] */
} freddy_vec_desc;
int freddy_gpu_pin_vectors(const freddy_vec_desc* desc, int device, freddy_gpu_index_t** out);
/* subset_ids == NULL: all rows; else "id = ANY(subset_ids)" (duplicates / unknown ids ignored).
 * out_ids/out_sim: [Q][k]; slots beyond the number of rows hold (-1, -inf). */
int freddy_gpu_exact_search(freddy_gpu_index_t* vecs, const float* queries, int32_t Q, int32_t k,
                            const int32_t* subset_ids, int64_t n_subset, int32_t* out_ids, float* out_sim);

/* ---- exact word analogies on the same handle (analogy.h) ------------------------------------------------------------
 * The bodies of analogy_3cosadd, analogy_3cosadd_in (freddy--0.0.1.sql:1270-1315) and analogy_3cosmul (:1231-1249), batched:
 * for every triple (w1, w2, w3) of row ids the k rows v4 with the largest score, v4 not one of the three input rows
 * ("v4.word NOT IN (...)"; another row with an identical vector is not excluded), ordered by score DESC, id ASC.
 *   3CosAdd: cosine_similarity_bytea(vec_plus_bytea(vec_minus_bytea(v3, v1), v2), v4) -- binary32, reported widened to double
 *   3CosMul: ((c3 + 1)/2) * ((c2 + 1.0)/2.0) / (((c1 + 1.0)/2.0) + 0.001), c_i = cosine_similarity_bytea(v4, v_i), all in
 *            float8 (PostgreSQL's float48pl: the binary32 c_i widened, constants the doubles nearest 1, 2, 0.001)
 * subset_ids == NULL: all rows; else "id = ANY(subset_ids)" (the _in form: duplicates / unknown ids ignored; the inputs may lie
 * outside the set).  An unknown input id (the SQL's empty INNER JOIN, NULL) and slots beyond the rows hold (-1, -inf).
 * Any Q (processed in passes); k <= 32 (FREDDY_E_LIMIT above).  Argument errors are reported before any device work. */
#define FREDDY_ANALOGY_3COSADD 0
#define FREDDY_ANALOGY_3COSMUL 1
/* analogy_pair_direction (freddy--0.0.1.sql:1212-1229): score = cosine_similarity_bytea(vec_normalize(v1 - v2), vec_normalize(v3 - v4)),
 * every operation in binary32 as core_functions.c does it, the float widened.  The reference runs it on the ORIGINAL table
 * (get_vecs_name_original()); any freddy_gpu_pin_vectors handle is accepted.  A row with v3's vector under another id scores NaN
 * and comes first; w1 == w2 makes every score NaN (the k lowest ids that are not inputs).  Always the all-exact scan: no filter
 * passes are reported, exact_filter and check_brackets have no effect. */
#define FREDDY_ANALOGY_PAIR_DIRECTION 2
int freddy_gpu_exact_analogy(freddy_gpu_index_t* vecs, int32_t method, const int32_t* triples /*[Q][3] ids w1,w2,w3*/,
                             int32_t Q, int32_t k, const int32_t* subset_ids, int64_t n_subset,
                             int32_t* out_ids /*[Q][k]*/, double* out_score /*[Q][k]; 3CosAdd: the float widened*/);
/* What the last freddy_gpu_exact_analogy call on this handle did: passes of (up to 32) analogies the filter + refine path ran
 * over the whole table (0: the all-exact path answered everything -- subsets, small or non-finite tables, exact_filter = 0,
 * 3CosMul with d > 416), the candidates those passes refined (summed over their analogies), and how many of them were redone on
 * the all-exact path (a candidate buffer overflowed or the pass's vectors were not finite).  NULL pointers are skipped. */
int freddy_gpu_last_analogy_stats(const freddy_gpu_index_t* vecs, int64_t* filter_passes, int64_t* candidates, int64_t* redone_passes);

/* ---- the exact kNN-join on the same handle (exact_join.h) -------------------------------------------------------------
 * knn_search_in_batch (freddy--0.0.1.sql:456-501), the reference's default knn_join(): one knn_in_exact per query over the
 * target set "id = ANY(target_ids)" (duplicates / unknown ids ignored).  For every input the lists are bit for bit those of
 * freddy_gpu_exact_search(vecs, queries, Q, k, target_ids, n_targets, ...): ORDER BY cosine_similarity_bytea DESC, id ASC, the
 * similarity bits of the binary32 chain, (-1, -inf) beyond the rows.  n_targets == 0 is the EMPTY set (every slot empty);
 * target_ids == NULL with n_targets > 0 is FREDDY_E_ARG.  Any Q, k <= 4096; argument and limit errors are reported before any
 * device work.  Filter + refine on the matrix cores over the target set, one gather and five launches per pass of >= 10 880 queries, when k <= 32, d % 4 == 0,
 * 16 <= d <= 512, table and queries finite, option exact_filter != 0 and the set has >= 8000 known rows (exact_filter = 1: any
 * size); the all-exact subset path otherwise, and for every single query whose candidate buffer overflowed. */
int freddy_gpu_exact_join(freddy_gpu_index_t* vecs, const float* queries /*[Q][d]*/, int32_t Q, int32_t k,
                          const int32_t* target_ids, int64_t n_targets, int32_t* out_ids /*[Q][k]*/, float* out_sim /*[Q][k]*/);
/* What the last freddy_gpu_exact_join call on this handle did: queries the filter + refine path ran for (0: the all-exact path
 * answered the call), the candidates it refined (summed over the queries it answered), and the queries answered again on the
 * all-exact path because their candidate buffer overflowed.  NULL pointers are skipped. */
int freddy_gpu_last_exact_join_stats(const freddy_gpu_index_t* vecs, int64_t* filter_queries, int64_t* candidates, int64_t* redone_queries);

/* ---- the assignment step of the clustering functions (assign.h) ---------------------------------------------------------
 * generic_cluster (freddy--0.0.1.sql:1086-1170; cluster_exact :1172-1183, cluster_pq :1198-1209) sends every token to the centroid
 * that lists it with the highest similarity (:1115-1127): it asks knn_search_in_batch (:480-501) resp. knn_in_pq_batch (:846-867
 * over pq_search_in_batch :386-387) for ALL n tokens per centroid, orders the kc * n rows by similarity DESC and keeps the first
 * row of every token.  These two calls return what that keeps, for any number of targets: per target the first query under
 * "similarity DESC, query index ASC", i.e. the lists of freddy_gpu_exact_join / freddy_gpu_pq_search at k = n_targets reduced per
 * target -- without the lists and without their k <= 4096.
 * Outputs are POSITIONAL: slot i answers target_ids[i]; a duplicated id gets its answer in every slot (the INNER JOIN of the
 * tokens with the rows, :1119).
 * freddy_gpu_exact_assign, for a target with a row v in `vecs`:
 *   sim(q) = the binary32 chain "scalar += q[j] * v[j]", j ascending, no contraction (core_functions.c:67-81) -- the bits
 *   freddy_gpu_exact_join returns; out_query[i] = the q that comes first under sim DESC, q ASC, DESC being PostgreSQL's float4
 *   order (a NaN above every number, all NaNs equal, +-Inf as numbers); out_sim[i] = that similarity.  A target id without a row:
 *   (-1, -inf).
 * freddy_gpu_pq_assign, for a target with a row in `pq`:
 *   dist(q) = the ADC distance freddy_gpu_pq_search computes (the same LUT entries, positions summed in order); q is a candidate
 *   iff dist(q) < sentinel (strict: a NaN distance never is); its key is freddy_similarity_of(dist) (include/freddy_similarity.h:
 *   the "%f" text round trip of the SRF, then (float)(1.0 - y / 2.0), freddy--0.0.1.sql:862 -- what the host mirror's
 *   similarity_of() computes with snprintf / strtof); out_query[i] = the candidate that comes first under key DESC, q ASC -- the
 *   ROUNDED key is compared, so of two distances the round trip merges the lower query index wins; out_sim[i] = that key.
 *   (-1, -inf) when no query is a candidate or the id is not in the table.
 *   That key is defined for 0 <= dist < 2^24, and only distances below the sentinel are evaluated (an ADC distance is a sum of
 *   squares, never negative): a sentinel above 2^24 (16777216) or NaN is refused with FREDDY_E_ARG.
 * Errors, all before any device work and the scalars before the handle: FREDDY_E_ARG for Q < 0, n_targets < 0, a NULL buffer
 * when Q > 0 and n_targets > 0, the sentinel above; FREDDY_E_LIMIT for Q > 65536 (the message names the value); FREDDY_E_ARG for a
 * NULL handle, FREDDY_E_KIND for one of the wrong kind.  Q == 0 or n_targets == 0 succeeds and writes nothing.  Any n_targets
 * (passes of 2^22 targets); only n_targets integers and floats leave the device. */
int freddy_gpu_exact_assign(freddy_gpu_index_t* vecs, const float* queries /*[Q][d]*/, int32_t Q, const int32_t* target_ids,
                            int64_t n_targets, int32_t* out_query /*[n_targets]*/, float* out_sim /*[n_targets]*/);
int freddy_gpu_pq_assign(freddy_gpu_index_t* pq, const float* queries /*[Q][d]*/, int32_t Q, float sentinel,
                         const int32_t* target_ids, int64_t n_targets, int32_t* out_query /*[n_targets]*/,
                         float* out_sim /*[n_targets]*/);

/* ---- the whole k-means of cluster_exact / cluster_pq in one call (cluster.h) ----------------------------------------------
 * generic_cluster (freddy--0.0.1.sql:1086-1209) with the draws of random() supplied by the caller; pq == NULL: cluster_exact,
 * else cluster_pq.  The semantics, bit for bit those of the host mirror's loop around the two assign calls above:
 *   pick(u, r) = min(max(rint(r * u + 0.5), 1), u)  in binary64, the product rounded before the sum, rint half to even
 *                (include/freddy_pick.h).
 *   Start.   clusters[n] = 0, lens[kc] = 0; centroid[I] = the row in `vecs` of token_ids[pick(n, draws[I]) - 1], I = 0 .. kc - 1.
 *   Round J = 1 .. rounds.   (best, sim) = what freddy_gpu_exact_assign(vecs, centroids, kc, token_ids, n) returns, resp.
 *            freddy_gpu_pq_assign(pq, centroids, kc, sentinel, token_ids, n) -- the same kernels, the same bits.  Every position i
 *            with best[i] >= 0: clusters[i] = best[i] + 1 and lens[best[i]] += 1.  A position no centroid claims keeps its cluster:
 *            it then counts as a member but not in lens.
 *   If J < rounds, for every I, with base = kc + ((J - 1) * kc + I) * 10:
 *            lens[I] == 0: the centroid stays (its ten draws are not used, but they are counted).
 *            Otherwise members = the positions i with clusters[i] == I + 1, ascending; for t = 0 .. 9: x = pick(lens[I], draws[base + t]),
 *            and if x <= |members| the row of token members[x - 1] is a sample (repeats allowed).  With ns > 0 samples in draw
 *            order: c = 0, then c[j] = c[j] + (row[j] / (float)ns) -- every operation binary32, the division the correctly rounded
 *            one, never a reciprocal multiply (centroid_bytea, core_functions.c:371-379).  lens[I] = 0.
 *   Outputs. out_cluster[i] = 1 .. kc, or 0 for a position no round claimed; out_sim[i] (may be NULL) = the last round's similarity,
 *            -inf where the last round claimed nothing; out_centroids (may be NULL) = the centroids the last assignment used.
 * Outputs are positional: a repeated id is a token per position.  Ids are resolved on the device against the handle's current
 * ids, so a call sees every append_rows / update_rows / remove_rows made before it.
 * Errors, all before any device work and the scalars before the handles: FREDDY_E_ARG for n <= 0, kc <= 0, rounds <= 0, a NULL
 * token_ids / draws / out_cluster, n_draws < kc + 10 * kc * (rounds - 1) (the message names both numbers), a NaN among the draws
 * the call would use, the sentinel rule of freddy_gpu_pq_assign (pq != NULL only); FREDDY_E_LIMIT for kc > 65536 and n > 2^31 - 1;
 * FREDDY_E_ARG for a NULL vecs, FREDDY_E_KIND for handles of the wrong kind, FREDDY_E_ARG for handles on different devices or of
 * different d.  A token id without a row in `vecs` is the reference's "token id %d has no vector": FREDDY_E_ARG naming the first
 * such id by position (found on the device: a flag word, no host search); a refused call writes none of the outputs.  A failed
 * allocation gives FREDDY_E_NOMEM, leaves the handles as they were, and the call may be repeated.
 * One call enqueues everything on the vector handle's stream: ids and draws go up, the outputs come down, and the host does not
 * wait for the device between the rounds.  The assignment takes 2^22 targets per pass (option "cluster_pass", 64 at least). */
int freddy_gpu_cluster(freddy_gpu_index_t* vecs, freddy_gpu_index_t* pq /* NULL: cluster_exact */, float sentinel /* pq only */,
                       const int32_t* token_ids, int64_t n, int32_t kc, int32_t rounds, const double* draws, int64_t n_draws,
                       int32_t* out_cluster /*[n]*/, float* out_sim /*[n] or NULL*/, float* out_centroids /*[kc][d] or NULL*/);

/* ---- similarities by row id: pairs, matrices, joins (similarity.h) --------------------------------------------------------
 * cosine_similarity(token1, token2) (freddy--0.0.1.sql:946-959) finds two rows of google_vecs_norm and runs
 * cosine_similarity_bytea (core_functions.c:67-81) on them; cosine_similarity_bytea(vector, token) (:961-974) takes the first
 * operand from the caller.  The usual query calls them once per row of a join, often under "WHERE cosine_similarity(..) > t".
 * These calls are the batched forms on the pinned vector handle: they return the VALUES, with no ranking around them.
 *   A similarity is the binary32 chain "scalar = 0; scalar += v1[i] * v2[i]", i ascending, every product and sum rounded on
 *   its own -- bit for bit cosine_similarity_bytea of the two rows (so the matrix cores cannot be used: the order is fixed).
 *   Ids are resolved on the device against the handle's ascending ids: a table with gaps needs no lookup by the caller, and a
 *   call sees every append_rows / update_rows / remove_rows made before it.
 * freddy_gpu_similarity_pairs: out_sim[i] = the chain over the rows of ids_a[i] (v1) and ids_b[i] (v2); out_known[i] = 1 when
 *   both ids have a row, else 0 and out_sim[i] = 0.0f (the SQL's NULL).  Any n >= 0 (passes of 2^22 pairs).
 * freddy_gpu_similarity_matrix: exactly one of a_ids / a_vectors is non-NULL -- the A side is na rows named by id, or [na][d]
 *   floats of the caller's (the vector overload).  out[i][j] = the chain with v1 = A row i, v2 = the row of b_ids[j]; entries of
 *   an id without a row are 0.0f, known_a[na] / known_b[nb] say which (known_a is all 1 for vectors).  Either side may repeat
 *   an id.  nb <= 2^22 (FREDDY_E_LIMIT above, the message names the value), any na: A is walked in passes whose device result
 *   block stays within 256 MiB (option "similarity_pass_bytes"; a multiple of 16 rows of A, 16 at least), one D2H copy per pass.
 * freddy_gpu_similarity_join: "WHERE cosine_similarity(a, b) > threshold": every (i, j) with both rows known and
 *   sim > threshold in PostgreSQL's float4 order (float4gt: a NaN similarity is greater than every non-NaN threshold, nothing is
 *   greater than a NaN threshold, -0.0 is not greater than +0.0).  out_a / out_b are 0-based POSITIONS in the A / B arguments
 *   (not ids), out_sim the value; the order is i ascending, then j ascending -- always.  *n_pairs = the number of matches
 *   whatever max_pairs is; the first min(*n_pairs, max_pairs) in that order are written.  max_pairs = 0 (the outputs may be
 *   NULL) only counts.  Every chain is computed once, and only the matches that are written leave the device.
 * Errors, all before any device work and the scalars before the handle: FREDDY_E_ARG for a negative size, for both or neither
 * of a_ids / a_vectors, for a NULL buffer that would be read or written (n > 0; na > 0 and nb > 0; the join's outputs when
 * max_pairs > 0; n_pairs always), max_pairs < 0; FREDDY_E_LIMIT for nb > 2^22; FREDDY_E_ARG for a NULL handle, FREDDY_E_KIND
 * for one of the wrong kind.  A refused call writes nothing, *n_pairs included.  A zero size succeeds with no device work
 * (*n_pairs = 0), and so does a call in which no id has a row (zeros, known = 0, *n_pairs = 0: nothing is launched). */
int freddy_gpu_similarity_pairs(freddy_gpu_index_t* vecs, const int32_t* ids_a /*[n]*/, const int32_t* ids_b /*[n]*/, int64_t n,
                                float* out_sim /*[n]*/, uint8_t* out_known /*[n]*/);
int freddy_gpu_similarity_matrix(freddy_gpu_index_t* vecs, const int32_t* a_ids /*[na] or NULL*/, const float* a_vectors /*[na][d] or NULL*/,
                                 int32_t na, const int32_t* b_ids /*[nb]*/, int64_t nb, float* out /*[na][nb]*/,
                                 uint8_t* known_a /*[na]*/, uint8_t* known_b /*[nb]*/);
int freddy_gpu_similarity_join(freddy_gpu_index_t* vecs, const int32_t* a_ids /*[na] or NULL*/, const float* a_vectors /*[na][d] or NULL*/,
                               int32_t na, const int32_t* b_ids /*[nb]*/, int64_t nb, float threshold, int64_t max_pairs,
                               int32_t* out_a /*[max_pairs]*/, int32_t* out_b /*[max_pairs]*/, float* out_sim /*[max_pairs]*/,
                               int64_t* n_pairs);

/* ---- batched post verification: the ANN handles and the raw-vector handle in one call (pv.h) ----------------------------
 * k_nearest_neighbour_ivfadc_pv / k_nearest_neighbour_pq_pv (freddy--0.0.1.sql:556-662) for Q queries: fetch k * pvf candidates
 * with the approximate search, re-rank them by cosine_similarity_bytea against the raw vectors, keep the first k.
 * Contract: for every query q let L be the list freddy_gpu_ivfadc_search (freddy_gpu_pq_search) returns for the same arguments with
 * k * pvf in place of k -- stage one IS that entry point: every path, every probing round, the passes of k * pvf > 512.  The
 * output row is bit for bit that of freddy_gpu_exact_search(vecs, q, 1, k, the ids of L that are >= 0, ...): ORDER BY similarity
 * DESC, id ASC (non-finite values as that call orders them: the same key); the similarity bits of the binary32 chain
 * "scalar += v1[i] * v2[i]", i ascending, no contraction; (-1, -inf) in the slots beyond the rows.  The (-1, sentinel) fillers of L
 * are dropped; a candidate id with no row in vecs is dropped; an empty candidate set gives a row of (-1, -inf), never a search of
 * the whole table.  Candidate vectors never travel to the host: ids are resolved to rows, similarities computed and the k best
 * selected on the device (kernel pv_rerank: one workgroup per query, one lane per candidate); the host receives [Q][k] only.
 * Errors, all before any device work: FREDDY_E_ARG for bad sizes (k < 1, pvf < 1, Q < 0, W < 1, n_subset < 0) and NULL buffers;
 * FREDDY_E_LIMIT for k * pvf > 4096 (the message names the product); FREDDY_E_KIND for handles of the wrong kinds; FREDDY_E_ARG
 * for vecs on another device or of another d, and for an ivf handle with replicas (freddy_gpu_replica_count > 1; the message
 * says so).  Q == 0 succeeds and does nothing.  Any Q (passes of queries whose lists hold at most 8 M entries). */
int freddy_gpu_ivfadc_search_pv(freddy_gpu_index_t* ivf, freddy_gpu_index_t* vecs, const float* queries, int32_t Q, int32_t k,
                                int32_t pvf, int32_t W, float sentinel, int32_t found_rule, int32_t* out_ids /*[Q][k]*/,
                                float* out_sim /*[Q][k]*/);
int freddy_gpu_pq_search_pv(freddy_gpu_index_t* pq, freddy_gpu_index_t* vecs, const float* queries, int32_t Q, int32_t k,
                            int32_t pvf, float sentinel, const int32_t* subset_ids, int64_t n_subset, int32_t* out_ids,
                            float* out_sim);
/* The last post-verification call on this pq / ivf handle: list entries with id >= 0, summed over the queries, and how many of
 * them had a vector row (were scored).  NULL pointers are skipped. */
int freddy_gpu_last_pv_stats(const freddy_gpu_index_t* ann, int64_t* candidates, int64_t* scored);

/* ---- searches by row id: the queries are rows of a pinned vector handle, gathered on the device (query_ids.h) ---------------
 * The reference's callers start from ids, not floats: ivfadc_batch_search(int[] ids, k) selects "id, vector FROM <vecs> WHERE id IN
 * (...)" itself (freddy.c:767-804), and the token forms resolve words to rows of the same table first.  These four calls take the
 * ids; the vectors never cross PCIe: 4 bytes per query go up, and a kernel (query_gather) copies the rows of `vecs` into the
 * search's query block.  From there everything the existing entry point runs, runs unchanged.
 * Which ids are searched is decided by id_rule; let sel[0..Q) be the ids it selects and v[j] the row of `vecs` with id sel[j]:
 *   FREDDY_QIDS_TABLE_ORDER  the SELECT above: Q = the distinct ids of query_ids that have a row, in ascending id order (duplicates
 *                            collapse, ids without a row vanish).  Output slots >= Q are not written.  Q == 0 succeeds and launches
 *                            nothing.
 *   FREDDY_QIDS_POSITIONAL   Q = n_ids and sel = query_ids: slot j answers query_ids[j], a repeated id is answered again.  A slot
 *                            whose id has no row holds k fillers -- (-1, sentinel), or (-1, -inf) for the _pv forms -- and is not
 *                            searched: such slots are compacted away before anything is launched (as the approximate analogies do
 *                            with unknown triples), cost nothing and disturb no neighbour; a batch of only such ids launches nothing.
 * Contract: *n_queries = Q, out_query_ids[0..Q) = sel, and for every j with a row, list j is bit for bit (ids, ranks, distance or
 * similarity bits) what freddy_gpu_ivfadc_search / freddy_gpu_pq_search / freddy_gpu_ivfadc_search_pv / freddy_gpu_pq_search_pv
 * returns for the query v[j] with the same remaining arguments: every path (one launch, small batch, pipelined sub-batches, every
 * scan, the passes of k > 512), every probing round, and the re-search of the queries round one leaves unfinished.  The query row
 * need not be a row of the ANN index: `vecs` may hold more or fewer ids than ivf / pq.
 * Errors, all before any device work and in this order: FREDDY_E_ARG for a NULL handle, n_ids < 0, a bad id_rule, a NULL n_queries,
 * a NULL buffer with n_ids > 0; then what the entry point underneath refuses (k, W, found_rule, the subset, k * pvf), with its
 * messages; FREDDY_E_KIND for handles of the wrong kinds; FREDDY_E_ARG for vecs on another device or of another d, and for an ivf
 * handle with replicas; a poisoned handle of either kind is refused as everywhere.  n_ids == 0 succeeds with *n_queries = 0.
 * Concurrency as for the _pv calls: synchronous, on the library's own streams; `vecs` is read while the call runs, so a mutation of
 * `vecs` must not run beside it.  A mutation BEFORE the call is seen: after freddy_gpu_update_rows / append_rows / remove_rows on
 * vecs a search by id answers as if the host had read the new table. */
#define FREDDY_QIDS_TABLE_ORDER 0
#define FREDDY_QIDS_POSITIONAL 1
int freddy_gpu_ivfadc_search_ids(freddy_gpu_index_t* ivf, freddy_gpu_index_t* vecs, const int32_t* query_ids, int32_t n_ids,
                                 int32_t id_rule, int32_t k, int32_t W, float sentinel, int32_t found_rule,
                                 int32_t* out_query_ids /*[n_ids]*/, int32_t* n_queries, int32_t* out_ids /*[n_ids][k]*/,
                                 float* out_dist /*[n_ids][k]*/);
int freddy_gpu_pq_search_ids(freddy_gpu_index_t* pq, freddy_gpu_index_t* vecs, const int32_t* query_ids, int32_t n_ids,
                             int32_t id_rule, int32_t k, float sentinel, const int32_t* subset_ids, int64_t n_subset,
                             int32_t* out_query_ids, int32_t* n_queries, int32_t* out_ids, float* out_dist);
int freddy_gpu_ivfadc_search_pv_ids(freddy_gpu_index_t* ivf, freddy_gpu_index_t* vecs, const int32_t* query_ids, int32_t n_ids,
                                    int32_t id_rule, int32_t k, int32_t pvf, int32_t W, float sentinel, int32_t found_rule,
                                    int32_t* out_query_ids, int32_t* n_queries, int32_t* out_ids, float* out_sim);
int freddy_gpu_pq_search_pv_ids(freddy_gpu_index_t* pq, freddy_gpu_index_t* vecs, const int32_t* query_ids, int32_t n_ids,
                                int32_t id_rule, int32_t k, int32_t pvf, float sentinel, const int32_t* subset_ids,
                                int64_t n_subset, int32_t* out_query_ids, int32_t* n_queries, int32_t* out_ids, float* out_sim);

/* ---- exact kNN and the exact kNN-join by row id; id sets resolved on the device (resolve.h) --------------------------------
 * The exact defaults of the SQL surface start from words, i.e. from row ids of the vector table: k_nearest_neighbour(token)
 * (freddy--0.0.1.sql:426-454), knn_in_exact, knn_search_in_batch (:480-501) and grouping_func.  These two calls take the ids on
 * both sides: the queries are rows of `vecs` (id_rule, out_query_ids, n_queries, the fillers (-1, -inf) and the compaction of
 * slots without a row exactly as for the four calls above), and the id set -- subset_ids / target_ids -- is turned into ascending,
 * distinct table rows by three kernels over a bitmap of the table's rows instead of one binary search per id, a sort and a copy on
 * the host: N / 8 bytes cleared and read, 4 n bytes of ids read, 4 nT bytes of rows written, one synchronisation to learn nT.
 * Contract: for every selected id with a row v, list j is bit for bit (ids, ranks, similarity bits) what freddy_gpu_exact_search /
 * freddy_gpu_exact_join returns for the query v with the same k and the same set -- on every path: filter + refine, all-exact, the
 * passes of k > 1024, the redo of overflowed queries, the fall-back for a non-finite query, more queries than one pass.
 * subset_ids == NULL: the whole table (no bitmap); n_targets == 0: the empty set (every list is fillers).
 * freddy_gpu_last_exact_join_stats reports for freddy_gpu_exact_join_ids as for freddy_gpu_exact_join.
 * Errors, all before any device work and in this order: the front checks of the calls above (NULL handle, n_ids < 0, a bad id_rule,
 * a NULL n_queries, a NULL buffer with n_ids > 0); what the entry point underneath refuses (FREDDY_E_ARG for k < 1, a negative set
 * size or a NULL set of positive size; FREDDY_E_LIMIT for k > 4096); FREDDY_E_KIND; a poisoned handle.  Concurrency and mutations
 * as above: a mutation before the call is seen, none may run beside it.
 * Option "exact_resolve" = 1 makes freddy_gpu_exact_search (subset), freddy_gpu_exact_join and freddy_gpu_exact_analogy (subset)
 * resolve their sets the same way (default 0: on the host, as before; no result changes); these two calls always do. */
int freddy_gpu_exact_search_ids(freddy_gpu_index_t* vecs, const int32_t* query_ids, int32_t n_ids, int32_t id_rule, int32_t k,
                                const int32_t* subset_ids, int64_t n_subset, int32_t* out_query_ids /*[n_ids]*/,
                                int32_t* n_queries, int32_t* out_ids /*[n_ids][k]*/, float* out_sim /*[n_ids][k]*/);
int freddy_gpu_exact_join_ids(freddy_gpu_index_t* vecs, const int32_t* query_ids, int32_t n_ids, int32_t id_rule, int32_t k,
                              const int32_t* target_ids, int64_t n_targets, int32_t* out_query_ids /*[n_ids]*/,
                              int32_t* n_queries, int32_t* out_ids /*[n_ids][k]*/, float* out_sim /*[n_ids][k]*/);
/* Test hook: the device resolve alone.  out_rows[0..*n_rows) = the table rows of ids[0..n) that have one, ascending and distinct
 * (unknown ids vanish, duplicates collapse); out_rows holds min(n, N) entries. */
int freddy_gpu_debug_resolve_ids(freddy_gpu_index_t* vecs, const int32_t* ids, int64_t n, int32_t* out_rows /*[min(n, N)]*/,
                                 int64_t* n_rows);

/* ---- batched approximate analogies: 3CosAdd over the candidates of an approximate search (approx_analogy.h) ----------------
 * analogy_3cosadd_ivfadc (freddy--0.0.1.sql:1428-1460), analogy_3cosadd_pq (:1317-1346) and, with subset_ids, analogy_3cosadd_in_pq
 * (:1348-1384) for Q triples of row ids (w1, w2, w3) at once; the reference calls them with n_cand = get_pvf() + 3 and k = 1.
 * Contract, per triple whose three ids have a row (v1, v2, v3) in `vecs`:
 *   raw[i] = (v3[i] - v1[i]) + v2[i], both rounded binary32; unit = vec_normalize_bytea(raw): sq += raw[i] * raw[i] in ascending i,
 *   length = (float)sqrt((double)sq), unit[i] = raw[i] / length (a correctly rounded division);
 *   L = the list freddy_gpu_ivfadc_search(ivf, unit, 1, n_cand, W, sentinel, found_rule) (freddy_gpu_pq_search(pq, unit, 1, n_cand,
 *   sentinel, subset_ids, n_subset)) returns -- stage one IS that entry point, every path of it;
 *   the output row is bit for bit freddy_gpu_exact_search(vecs, raw, 1, k, S) with S = the ids of L that are >= 0, have a row in
 *   vecs and are none of w1, w2, w3: similarity (the binary32 chain against RAW, not unit) DESC, id ASC, (-1, -inf) beyond its
 *   rows, and a row of (-1, -inf) for an empty S (never a search of the table).
 * A triple with an id that has no row in vecs is the SQL's empty join: its row is all (-1, -inf), it is not searched and does not
 * disturb its neighbours (the other triples are compacted before stage one); a batch of such triples launches nothing.  Nothing
 * is special-cased: raw == 0 makes unit all NaN and the search does what it does for a NaN query; ids may repeat inside a triple.
 * Errors, all before any device work: FREDDY_E_ARG for Q < 0, k < 1, n_cand < k, W < 1, a bad found_rule, a bad subset, NULL
 * buffers with Q > 0; FREDDY_E_LIMIT for n_cand > 4096 (the message names the value); FREDDY_E_KIND for handles of the wrong kinds;
 * FREDDY_E_ARG for vecs on another device or of another d, and for an ivf handle with replicas.  Q == 0 succeeds and does nothing.
 * Any Q (passes of triples whose lists hold at most 8 M entries; option "analogy_pass" sets the triples per pass).
 * analogy_3cosadd_in_ivpq goes through the kNN-join (the literal k = 4): freddy_gpu_ivpq_analogy below. */
int freddy_gpu_ivfadc_analogy(freddy_gpu_index_t* ivf, freddy_gpu_index_t* vecs, const int32_t* triples /*[Q][3] ids w1,w2,w3*/,
                              int32_t Q, int32_t k, int32_t n_cand, int32_t W, float sentinel, int32_t found_rule,
                              int32_t* out_ids /*[Q][k]*/, float* out_sim /*[Q][k]*/);
int freddy_gpu_pq_analogy(freddy_gpu_index_t* pq, freddy_gpu_index_t* vecs, const int32_t* triples, int32_t Q, int32_t k,
                          int32_t n_cand, float sentinel, const int32_t* subset_ids, int64_t n_subset,
                          int32_t* out_ids, float* out_sim);
/* analogy_3cosadd_in_ivpq (freddy--0.0.1.sql:1383-1425) for Q triples at once: the contract above word for word, with another
 * stage one.  Per pass of triples (the same pass rule and option "analogy_pass", set on the ivpq handle) the lists L are the list
 * block of ONE freddy_gpu_knn_join(ivpq, <the unit rows of the pass's live triples>, nq, n_cand, target_ids, n_targets, alpha, pvf,
 * method, use_target_lists, confidence, double_threshold, ...); the reference passes the literal n_cand = 4.  The join's fillers
 * (-1, 1000.0) are no candidates.  `vecs` is required: it supplies v1 .. v3 and the candidates' rows, as google_vecs_norm does in the
 * SQL.  The unit rows are written by aa_query straight into the join's query block and the join starts behind it on the same stream
 * with no host synchronisation in between: they never reach the host.  "aa_query" and "aa_rerank" are recorded in the ivpq handle's
 * profile, once per pass; freddy_gpu_last_approx_analogy_stats reports for this call on the ivpq handle.
 * Errors, all before any device work: the scalars above (Q, k, n_cand, NULL buffers, FREDDY_E_LIMIT for n_cand > 4096), then what
 * freddy_gpu_knn_join refuses at k = n_cand (with its messages), then the handles as above. */
int freddy_gpu_ivpq_analogy(freddy_gpu_index_t* ivpq, freddy_gpu_index_t* vecs, const int32_t* triples /*[Q][3]*/, int32_t Q,
                            int32_t k, int32_t n_cand, const int32_t* target_ids, int64_t n_targets, int32_t alpha, int32_t pvf,
                            int32_t method, int32_t use_target_lists, float confidence, int32_t double_threshold,
                            int32_t* out_ids /*[Q][k]*/, float* out_sim /*[Q][k]*/);
/* The last approximate-analogy call on this pq / ivf / ivpq handle: triples that reached stage one, their list entries with id >= 0,
 * and how many of those had a vector row and were not an input of their triple (were scored).  NULL pointers are skipped. */
int freddy_gpu_last_approx_analogy_stats(const freddy_gpu_index_t* ann, int64_t* searched, int64_t* candidates, int64_t* scored);

/* ---- text vectors from token ids, and searches over them (tokenize.h) ---------------------------------------------------------
 * tokenize(text) = vec_normalize_bytea(centroid_bytea(ARRAY(SELECT vector FROM google_vecs_norm WHERE word = ANY(tokens)))) and
 * tokenize_raw (the same over google_vecs, without the normalisation; freddy--0.0.1.sql:1512-1536) for n_texts texts at once, each a
 * list of row ids of `vecs`: token_ids[offsets[n_texts]] and offsets[n_texts + 1] (non-decreasing, offsets[0] == 0).  At most
 * FREDDY_TOK_MAX_LEN ids per text.  The rows never leave the device; bit for bit, no tolerance anywhere:
 *   row list     FREDDY_QIDS_TABLE_ORDER (the SQL above): the DISTINCT table rows of the ids that have one, in ascending row order --
 *                unknown ids vanish, duplicates collapse, as for every id set of this library (PostgreSQL leaves the order of "= ANY"
 *                unspecified).  FREDDY_QIDS_POSITIONAL (centroid_bytea(ARRAY[...]) of an explicit array): the rows of the ids that have
 *                one in the given order, duplicates kept.
 *   centroid     n = the length of the row list; core_functions.c:371-379: out[j] = 0, then for i ascending
 *                out[j] = out[j] + row_i[j] / (float)n -- every division (correctly rounded, never a reciprocal) and every addition
 *                rounded to binary32, no FMA.
 *   normalize    != 0: vec_normalize_bytea -- sq = sq + out[j] * out[j] for j ascending (one chain), len = (float)sqrt((double)sq),
 *                out[j] / len.  Nothing is special-cased: a zero centroid gives a row of NaN.
 *   n == 0       (an empty text, or no id with a row; the reference returns a zero-length bytea that no search accepts):
 *                out_count[t] = 0 and the vector is all zeros; in the search forms the text's list holds the entry point's fillers,
 *                (-1, sentinel) or (-1, -inf) for the exact form, costs no search work and disturbs no neighbour.
 * The three *_search_texts forms: for every text with out_count > 0 the list is bit for bit (ids, ranks, distance or similarity
 * bits) what freddy_gpu_ivfadc_search / freddy_gpu_pq_search / freddy_gpu_exact_search returns for the vector freddy_gpu_tokenize
 * returns for that text, with the same remaining arguments.  The approximate forms always normalise (tokenize is the only producer
 * of their queries); the exact form takes the flag (tokenize_raw).  The texts with a row list are compacted and searched in passes
 * (option "tokenize_pass", set on `vecs`: texts per pass); the vectors of a pass are written by the kernels into a pinned block
 * that the public search reads, and never reach the caller's memory.
 * Errors, all before any device work and in this order: FREDDY_E_ARG for the scalars (k < 1, W, found_rule, the subset, n_texts < 0,
 * a bad id_rule), for a NULL buffer with work to do, offsets[0] != 0 and decreasing offsets; FREDDY_E_LIMIT for a text of more than
 * FREDDY_TOK_MAX_LEN ids (the message names the text and its length) and for k > 4096; then the handles as for the searches by id
 * (NULL, kinds, devices, d, replicas) and a poisoned handle.  n_texts == 0 succeeds and launches nothing.  A failed allocation is
 * FREDDY_E_NOMEM and leaves the handles' tables as they were.  Concurrency and mutations as for the searches by id: a mutation of
 * `vecs` before the call is seen (the ids are resolved against the handle's device id column), none may run beside it.  The
 * launches are recorded as "tok_resolve", "tok_rows", "tok_centroid" and "tok_unit" in the profile of `vecs`. */
#define FREDDY_TOK_MAX_LEN 4096
int freddy_gpu_tokenize(freddy_gpu_index_t* vecs, const int32_t* token_ids, const int64_t* offsets /*[n_texts + 1]*/, int32_t n_texts,
                        int32_t id_rule, int32_t normalize, float* out_vectors /*[n_texts][d]*/, int32_t* out_count /*[n_texts]*/);
int freddy_gpu_ivfadc_search_texts(freddy_gpu_index_t* ivf, freddy_gpu_index_t* vecs, const int32_t* token_ids, const int64_t* offsets,
                                   int32_t n_texts, int32_t id_rule, int32_t k, int32_t W, float sentinel, int32_t found_rule,
                                   int32_t* out_count /*[n_texts]*/, int32_t* out_ids /*[n_texts][k]*/, float* out_dist /*[n_texts][k]*/);
int freddy_gpu_pq_search_texts(freddy_gpu_index_t* pq, freddy_gpu_index_t* vecs, const int32_t* token_ids, const int64_t* offsets,
                               int32_t n_texts, int32_t id_rule, int32_t k, float sentinel, const int32_t* subset_ids, int64_t n_subset,
                               int32_t* out_count, int32_t* out_ids, float* out_dist);
int freddy_gpu_exact_search_texts(freddy_gpu_index_t* vecs, const int32_t* token_ids, const int64_t* offsets, int32_t n_texts,
                                  int32_t id_rule, int32_t normalize, int32_t k, const int32_t* subset_ids, int64_t n_subset,
                                  int32_t* out_count, int32_t* out_ids, float* out_sim);

/* ---- the kNN-join by row id (join_run.h JoinQueries, join_kernels.h sub_dist_rows_kernel) -----------------------------------
 * The kNN-join's SQL callers start from ids: knn_in_ivpq_batch(query_set varchar[], ...) selects "word, vector, id FROM
 * google_vecs_norm WHERE word = ANY(...)" and hands the vectors over (freddy--0.0.1.sql:720-761, 797-814).  This call takes the ids:
 * the queries are the rows of `vecs` -- or, with vecs == NULL, of the ivpq handle's own pinned vectors -- with these ids.  id_rule,
 * out_query_ids and n_queries exactly as for the calls above; the ids are looked up in the id column of the table the rows come from.
 * Contract: let R be the selected ids that have a row, in order, and V their rows.  The lists of R and *iterations_out are bit for
 * bit (ids, ranks, distance bits) what ONE call freddy_gpu_knn_join(ivpq, V, |R|, k, <the same remaining arguments>) returns.  A
 * positional slot whose id has no row holds k fillers (-1, 1000.0f) and is compacted away before anything is launched; |R| == 0
 * launches nothing and gives *iterations_out = 0; TABLE_ORDER leaves the slots >= Q unwritten.  freddy_gpu_last_track reports as
 * for freddy_gpu_knn_join, and the cache of the previous call's target array is shared with it.
 * 4 bytes per query go up; ONE kernel ("join_front_rows" in the ivpq handle's profile) gathers the rows into the join's query block
 * and computes their sub-distances, where freddy_gpu_knn_join's front pulls the caller's floats over PCIe.  Option
 * "join_front_gather" = 0 (default 1), and d / 2 > 512, take two launches instead: "query_gather", then the sub-distance kernel.
 * Errors, all before any device work and in this order: the front checks of the calls above; what freddy_gpu_knn_join refuses
 * (k <= 0, n_targets < 0, NULL target ids, the method, the limits of k and k * pvf, pair codes), with its messages; FREDDY_E_KIND
 * and a poisoned handle; vecs on another device or of another d; vecs == NULL on a handle pinned without vectors (FREDDY_E_ARG, the
 * message says so).  A mutation of either handle BEFORE the call is seen; none may run beside it. */
int freddy_gpu_knn_join_ids(freddy_gpu_index_t* ivpq, freddy_gpu_index_t* vecs /* NULL: the ivpq handle's own vectors */,
                            const int32_t* query_ids, int32_t n_ids, int32_t id_rule, int32_t k, const int32_t* target_ids,
                            int64_t n_targets, int32_t alpha, int32_t pvf, int32_t method, int32_t use_target_lists,
                            float confidence, int32_t double_threshold, int32_t* out_query_ids /*[n_ids]*/, int32_t* n_queries,
                            int32_t* out_ids /*[n_ids][k]*/, float* out_dist /*[n_ids][k]*/, int32_t* iterations_out);

/* ---- next row: grouping_pq ---------------------------------------------------------
 * Body of grouping_pq (freddy.c:1176-1401): for every row of the PQ table (subset_ids == NULL) or of
 * "id IN (subset_ids)" the nearest of G group vectors by ADC distance -- one LUT per group from the PQ
 * codebook (:1288-1299), positions summed in order (:1346-1351), strict "<" from minDist = 100 so the
 * first of equally near groups wins (:1337,1353-1356).  group_vectors: [G][d] in the order the caller
 * wants the ties broken (the reference: ascending group id).  out_ids / out_group: caller-allocated,
 * one slot per requested row (n_subset, or N); rows come back in table order, out_group[i] is the
 * group's index or -1 if no group is nearer than 100 (the reference leaves that case undefined).
 * *n_out receives the number of rows. */
int freddy_gpu_grouping_pq(freddy_gpu_index_t* pq, const float* group_vectors, int32_t G, const int32_t* subset_ids,
                           int64_t n_subset, int32_t* out_ids, int32_t* out_group, int64_t* n_out);

/* ---- next row: index build, encoding step --------------------------------------------
 * What index_creation/pq_index.py:65-92 (create_index / create_index_with_faiss) and ivfadc.py do once
 * the quantizers are trained: every vector's coarse cell (nearest of C centroids, all d dimensions) and
 * its PQ code (per position the nearest codeword of the -- residual, if coarse != NULL -- sub-vector),
 * by squareDistance with the lowest index on ties.  Standalone: no index handle, tables and vectors are
 * host arrays, results are host arrays.  out_cell may be NULL when coarse is NULL. */
typedef struct freddy_encode_desc {
  int32_t d, m, K;
  const float* codebook;   /* [m][K][d/m] */
  int32_t C;               /* 0: flat PQ (no coarse quantizer) */
  const float* coarse;     /* [C][d] or NULL */
} freddy_encode_desc;
int freddy_gpu_encode(const freddy_encode_desc* desc, int device, const float* vectors, int64_t N, int32_t* out_cell,
                      int16_t* out_codes);

/* Quantizer training (index_creation/quantizer_creation.py:13-52: scipy k-means for the coarse quantizer, per
 * sub-vector position for the PQ codebooks): Lloyd's algorithm on the device.  Initial centroids =
 * vectors[init_rows[c]] (NULL: vectors[c mod n]); every iteration assigns each vector to its nearest centroid by
 * squareDistance (lowest index on ties) and replaces each centroid by the binary32 mean of its members, summed
 * in index order; an empty cluster keeps its centroid.  centroids [k][d]; assign_out [n] (may be NULL) = the
 * assignment under the final centroids.  Deterministic: equals oracle/fo_kmeans bit for bit.  (The reference
 * seeds scipy randomly, so its own output is not reproducible; d <= 1024.) */
int freddy_gpu_kmeans(int device, const float* vectors, int64_t n, int32_t d, int32_t k, int32_t iters,
                      const int32_t* init_rows, float* centroids, int32_t* assign_out);

/* ---- next row: insert_batch --------------------------------------------------------------
 * Quantisation of NEW vectors as insert_batch does it (freddy.c:1557-1623): per vector the PQ code, the coarse
 * cell (argmin from minDistCoarse = 100, :1568-1575) with the code of the residual, the ivpq code, and the
 * two multi-index coarse codes (argmin from MAX_DIST = 1000, :1588-1597); codes = exact 1-NN by squareDistance
 * from minDist = 100 with the first entry winning ties (updateCodebook, index_utils.c:925-939).  A codebook
 * pointer that is NULL skips its part.  FREDDY_E_ARG if some (vector, position) has no centroid nearer than
 * 100 (undefined behaviour in the reference).  The codebook update itself (index_utils.c:940-956: a few
 * sequential float / double operations per new vector) and the table rows stay with the host. */
typedef struct freddy_insert_desc {
  int32_t d;
  int32_t pq_m, pq_K;       const float* pq_codebook;         /* [pq_m][pq_K][d/pq_m]   pq_codebook */
  int32_t res_m, res_K;     const float* residual_codebook;   /* residual_codebook */
  int32_t C;                const float* coarse;              /* [C][d] coarse_quantization */
  int32_t ivpq_m, ivpq_K;   const float* ivpq_codebook;       /* codebook_ivpq */
  int32_t multi_positions, multi_codes; const float* coarse_multi;   /* [positions][codes][d/positions] coarse_quantization_ivpq */
} freddy_insert_desc;
int freddy_gpu_insert_quantize(const freddy_insert_desc* desc, int device, const float* vectors, int64_t n,
                               int16_t* pq_codes /*[n][pq_m]*/, int32_t* coarse_id /*[n]*/, int16_t* residual_codes /*[n][res_m]*/,
                               int16_t* ivpq_codes /*[n][ivpq_m]*/, int16_t* coarse_multi_codes /*[n][multi_positions]*/);
/* ---- index mutation: append_rows, remove_rows, update_rows, update_codebook, set_statistics, create_statistics ------------
 * THE CONTRACT OF A FAILED CALL, for all of them: after a non-zero return the handle is AS IT WAS, or POISONED.
 *   as it was:  every entry point answers as before the call, freddy_gpu_index_bytes has not moved, and the same call may simply
 *               be made again.  This is what a refused argument leaves, and what a failed allocation (FREDDY_E_NOMEM) leaves
 *               wherever the new arrays are built beside the old ones and swapped in last: append_rows and remove_rows on pq,
 *               ivf and ivpq handles, update_codebook on every kind, set_statistics, create_statistics.
 *   poisoned:   arrays had been rewritten in place when the call failed (update_rows after its first write; append_rows /
 *               remove_rows on a vector handle once the rows are in and the exact filter's statistics, which are rewritten in
 *               place, could not follow; a replica that failed after another device had changed).  Every entry point that reads
 *               the tables then refuses with FREDDY_E_HIP ("unpin it and pin again") without launching anything, and
 *               freddy_gpu_unpin frees it as usual.
 * There is no third state: no call returns an error and leaves a table that a search would read past its end. */
/* Append rows to a pinned index in HBM (the INSERTs of updateProductQuantizationRelation /
 * updateWordVectorsRelation, index_utils.c:993-1074): ids must be larger than every id already pinned and
 * ascending.  pq: (ids, codes); ivf: (ids, coarse_id, codes) -- each row joins the end of its cell's inverted
 * list, the block layout is rebuilt on the device; ivpq: (ids, coarse_id, codes[, vectors]); vectors: (ids, vectors). */
int freddy_gpu_append_rows(freddy_gpu_index_t* index, int64_t n, const int32_t* ids, const int32_t* coarse_id,
                           const int16_t* codes, const float* vectors);
/* Remove rows from a pinned index in HBM (a DELETE on the table behind it): every pinned row whose id is one of ids[0..n)
 * leaves, on every handle kind (pq, ivf with its replicas, ivpq, vectors).  Afterwards every entry point that takes the handle
 * answers bit for bit as a fresh pin of the same table without those rows; the rows that stay keep their order (inside its
 * list, for an ivf row), and a later append_rows may start above the largest id that is LEFT, as on a fresh pin.  ids may come
 * in any order; an id listed twice counts once; an id that no pinned row has is skipped; *removed (may be NULL) receives the
 * number of rows that left.  Emptying a cell or the whole handle is allowed.  Refused with FREDDY_E_ARG before anything has
 * changed: a negative id (-1 is the filler of the result lists; the message names the id and its position), n < 0, ids == NULL
 * with n > 0, a NULL handle.  n == 0 changes nothing.
 * Like append_rows the call synchronises the handle's own stream first and rebuilds the layouts on the device beside the old
 * ones: it must NOT run beside *_dev searches the caller has in flight on other streams -- drain them first.  Replicas follow
 * append_rows' rule: the primary first; a failure after the first device has changed poisons the handle.
 * freddy_gpu_index_bytes afterwards equals a fresh pin's for pq, ivf and ivpq; a vector handle's fragment-order copy keeps
 * its capacity (at least a fresh pin's figure, at most the figure before the call).  A compacted ivf list loses part of the
 * bank-conflict arrangement a fresh pin gives it: speed only, never a result. */
int freddy_gpu_remove_rows(freddy_gpu_index_t* index, int64_t n, const int32_t* ids, int64_t* removed /* may be NULL */);
/* Update rows of a pinned index in HBM (an UPDATE of rows of the table behind it: a row keeps its id and gets a new vector, and
 * with it new codes and possibly a new coarse cell).  For every i whose ids[i] is the id of a pinned row, that row's payload
 * becomes the i-th one given; its id stays.  The payload arrays are those append_rows takes for the handle's kind -- pq: codes;
 * ivf (with its replicas): coarse_id, codes; ivpq: coarse_id, codes, and vectors if the handle was pinned with vectors; a vector
 * handle: vectors.  Afterwards every entry point that takes the handle answers bit for bit as a fresh pin of the same table with
 * those rows replaced, served by the same kernels.  N, the ids and the largest pinned id do not change: a later append_rows must
 * still start above the same id.  ids may come in any order; an id that no pinned row has is skipped (its payload is still
 * validated); *updated (may be NULL) receives the number of rows that changed.  n == 0 succeeds and changes nothing; a call in
 * which no id is known changes nothing, the footprint included.
 * Refused with FREDDY_E_ARG before anything on the device has changed (the message names the value and its position): an id
 * listed twice (which payload would win is undefined), a negative id, n < 0, ids == NULL with n > 0, a NULL handle, a payload
 * array the kind needs but did not get, a coarse_id outside the cells, a code outside [0, K); n above INT32_MAX is refused with
 * FREDDY_E_LIMIT at the same point.  *updated is written on success only (with replicas: once every one has followed).  Vectors are accepted whatever
 * their values, as a fresh pin accepts them: the exact filter's statistics are taken again over all rows (the filter goes off
 * when a row turns non-finite and comes back when the only such row turns finite).
 * pq: the row's code words are rewritten in its slot; ivf: in its slot while the cell stays, else the row leaves its list
 * (a stable compaction, as remove_rows) and joins the end of the new one (as append_rows) -- the order inside a list affects
 * speed only, never a result; ivpq and vectors: the rows are overwritten in place.
 * Like append_rows and remove_rows the call synchronises the handle's own stream first; it must NOT run beside *_dev searches
 * the caller has in flight on other streams -- drain them first.  Replicas follow append_rows' rule: the primary first; a
 * failure after the first device has changed poisons the handle.  Once the arguments have passed, arrays are written in
 * place: a HIP failure after the first write poisons the handle too.  freddy_gpu_index_bytes afterwards equals a fresh pin's
 * for pq, ivf and ivpq; a vector handle's figure does not move unless the filter's state does. */
int freddy_gpu_update_rows(freddy_gpu_index_t* index, int64_t n, const int32_t* ids, const int32_t* coarse_id,
                           const int16_t* codes, const float* vectors, int64_t* updated /* may be NULL */);
/* Replace the codebook of a pinned pq / ivf / ivpq index (updateCodebookRelation, index_utils.c:959-991) and
 * re-derive everything on the device that depends on it. */
int freddy_gpu_update_codebook(freddy_gpu_index_t* index, const float* codebook /*[m][K][d/m]*/);

/* ---- the statistics row of a pinned ivpq handle (freddy_ivpq_desc::stats, [cells + 1] floats) ----------------------------
 * In the reference the statistics are a setting, not part of the index: getStatistics (index_utils.c:632-665) reads the table
 * set_statistics_table (freddy--0.0.1.sql:70) names on every ivpq_search_in call, and create_statistics(table, column,
 * coarse_table) (:150-171) builds such a table for any column of tokens.  The row decides how many cells a query of the
 * kNN-join probes for a given confidence.  append_rows / remove_rows / update_rows / update_codebook leave it alone, and
 * nothing here is ever installed implicitly: the caller decides when the row follows its table.
 * All three calls take an ivpq handle: a NULL handle is FREDDY_E_ARG, a handle of another kind FREDDY_E_KIND, and argument
 * errors are reported before any device work.  Like the mutation calls they synchronise the handle's own stream first and
 * must NOT run beside searches the caller has in flight on other streams.
 *
 * set_statistics: the device side of set_statistics_table.  n_stats must be cells + 1 (else FREDDY_E_ARG; the message names
 * both numbers); the values are accepted whatever they are, as a fresh pin accepts them.  The device copy of the row is
 * overwritten in place and only then the host copy, so the two never disagree after a failure.  Afterwards
 * freddy_gpu_knn_join answers bit for bit as a fresh pin of the same tables with that row (lists, iterations_out, the cells
 * each query took).  freddy_gpu_index_bytes does not move, and the target list cached from the previous join stays valid (it
 * does not depend on the statistics).
 *
 * get_statistics: the row the DEVICE holds, copied into out[n_stats]; n_stats must be cells + 1.
 *
 * create_statistics: create_statistics() over the pinned rows.  ids[0..n) is the multiset of row ids of the column's tokens
 * (the host resolves words to ids as for every other call); ids == NULL with n == 0 means every pinned row once, the default
 * stat_google_vecs_norm_word.  An id that no pinned row has is skipped; an id listed r times counts r times (the SQL is an
 * INNER JOIN with the column, not IN).  With count[c] = entries whose row lies in cell c and total = entries that have a row:
 *     stats[c]     = (float)((double)count[c] / (double)total)   for c < cells  ("count(*)::float / total_amount": float8, stored float4)
 *     stats[cells] = (float)total                                               (bigint -> float4, round to nearest even)
 * Counts are 64-bit integers on the device: a count above 2^24 is not rounded before the division and n above 2^31 does not
 * wrap.  The reference takes total over the VECTOR table, not the ivpq table; the two are equal whenever the ivpq table covers
 * the vector table, which index creation guarantees.
 * out_stats ([cells + 1], may be NULL) receives the row, *matched (may be NULL) the total.  install != 0 makes the row the
 * handle's row exactly as set_statistics would (a device-to-device copy; the host copy is filled from the floats that come
 * back).  total == 0 is the SQL's division by zero: FREDDY_E_ARG, nothing is installed and nothing is written.  ids == NULL
 * with n > 0, and n < 0, are FREDDY_E_ARG.  Any n is accepted: the ids are staged in passes, and only the row and the total
 * leave the device. */
int freddy_gpu_set_statistics(freddy_gpu_index_t* ivpq, const float* stats, int32_t n_stats);
int freddy_gpu_get_statistics(const freddy_gpu_index_t* ivpq, float* out, int32_t n_stats);
int freddy_gpu_create_statistics(freddy_gpu_index_t* ivpq, const int32_t* ids, int64_t n, int32_t install,
                                 float* out_stats /*[cells+1], may be NULL*/, int64_t* matched /* may be NULL */);

/* ---- device-resident variant used for throughput measurement ----------------------------
 * Same as freddy_gpu_ivfadc_search, but queries / outputs are DEVICE pointers on the
 * index's device and all work is enqueued on `hip_stream` (a hipStream_t; NULL = the
 * library's own stream) without synchronising.  d_status[0] is set non-zero by the
 * device if some query needs a further probing round (rare: its first W cells hold
 * fewer than k rows); such queries keep partial results and the caller should re-run
 * them through freddy_gpu_ivfadc_search.  Single round only.
 *
 * The status word, as tests/test_gpu_dev_contract.py pins it:
 *   - d_status[0] becomes non-zero iff at least one query of the call has found < k after the first probing round (found by
 *     the call's found_rule: rows retrieved, or accepted insertions).  The library only ever WRITES NON-ZERO and never clears
 *     the word: the caller zeroes it, on the same stream, before the call (or outside a captured graph before a replay).
 *   - A call that is cut into chunks (option lut_budget_mb) shares the one word among its chunks: it is set if a query of any
 *     chunk is unfinished, and every chunk's lists land at the chunk's offset of the output buffers.
 *   - d_status == NULL is allowed: the same lists, no report.
 *   - "Partial results" are defined: the list of an unfinished query is the reference's list after its FIRST probing round
 *     (freddy.c:262-377 stopped after one pass of its loop; oracle/freddy_oracle.h fo_ivfadc_search_capped with
 *     max_rounds = 1), unfilled slots (-1, sentinel).  A finished query's list is its final list.  Re-running the unfinished
 *     queries through freddy_gpu_ivfadc_search gives their final lists.
 *   - With W >= C (W is cut to C) on a table of fewer than k rows every query has found < k after round one although no cell
 *     is left to probe: the word IS set, every row is listed and the other slots hold (-1, sentinel); the host-buffer call
 *     returns the same lists.
 *   - Q == 0 succeeds, writes nothing and leaves the word alone.  A refused call (FREDDY_E_ARG / _KIND / _LIMIT: k < 1,
 *     k > 4096, W < 1, more than 512 probes after the cut to C, a bad found_rule, a NULL buffer with Q > 0, a handle of another
 *     kind) allocates nothing and enqueues nothing.  freddy_gpu_pq_search_dev has no status word: a flat scan is one round.
 *
 * Concurrency: everything a search writes besides its outputs lives in a workspace that belongs to the stream
 * the search is enqueued on (twelve slots per handle; with all taken a new stream takes over the least recently
 * used one after the device has drained).  Searches enqueued on DIFFERENT streams may therefore be in flight
 * together on one handle -- bench.py keeps four batches going that way.  The caller states how many with option
 * "scan_share" (an explicit contract; the library does not guess it): a batch's persistent scan then takes
 * n_cus / scan_share CUs so that the scans run side by side and the small kernels fit in between.  Searches on the
 * same stream are ordered by it.  Host threads may call concurrently as long as they do not share a stream (the
 * slot table and the profile map are locked).  The synchronous calls above use the library's own streams.
 * freddy_gpu_last_* report on the most recent call. */
int freddy_gpu_ivfadc_search_dev(freddy_gpu_index_t* ivf, const float* d_queries, int32_t Q,
                                 int32_t k, int32_t W, float sentinel, int32_t found_rule,
                                 int32_t* d_out_ids, float* d_out_dist, int32_t* d_status,
                                 void* hip_stream);
int freddy_gpu_pq_search_dev(freddy_gpu_index_t* pq, const float* d_queries, int32_t Q, int32_t k,
                             float sentinel, int32_t* d_out_ids, float* d_out_dist,
                             void* hip_stream);

/* ---- diagnostics ------------------------------------------------------------------------ */

/* Stage timers of the most recent freddy_gpu_knn_join call on this handle, in seconds, under the names the
 * reference reports with elog(INFO, "TRACK <stage> %f") (ivpq_search_in.c:234-697; scraped off the
 * connection by evaluation/tracking.py).  The PostgreSQL host re-emits them with the same elog lines. */
typedef struct freddy_track {
  double precomputation_time;                /* :294  here: coarse sub-distances + side sorts (the LUTs are built inside the join kernel) */
  double determine_coarse_quantization_time; /* :341  multi-index traversal, summed over the alpha rounds */
  double query_construction_time;            /* :397  per-query cell lists */
  double data_retrieval_time;                /* :403  "fq.id IN (targets)": ids resolved and bucketed by cell on the device */
  double computation_time;                   /* :632  the join kernel: ADC / exact distances, selection, replay */
  double pv_computation_time;                /* :627  0: post verification happens inside the join kernel */
  double recalculate_query_indices_time;     /* :671 */
  double total_time;                         /* :697 */
  double join_kernel_time;                   /* HIP-event time of the join kernel launches alone (inside computation_time) */
  int64_t candidate_rows;                    /* sum over queries of the target rows in their selected cells (what the kernel scans) */
  int32_t iterations;                        /* alpha-doubling rounds */
  int32_t replay_us;                         /* HIP-event time, in microseconds, of the list-writing launches behind the join kernels of a call
                                              * with methods 0 / 1 and k > 512 (inside join_kernel_time); 0 otherwise (was: reserved, always 0) */
  int64_t host_traversals;                   /* (query, round) pairs whose multi-index traversal ran on the host heap: every one with more than
                                              * 1024 cells; with the device traversal only those it hands back (equal keys in the taken prefix,
                                              * or the host's libm disagreeing with the proposed stop) */
  int64_t libm_checks;                       /* evaluations of getConfidenceHyp by the host's libm on device-proposed stops (only where the device's
                                              * own value lies within 1e-5 of the confidence) */
} freddy_track;
int freddy_gpu_last_track(const freddy_gpu_index_t* ivpq, freddy_track* out);
/* The same with the caller's idea of the struct's size: at most `out_size` bytes are written (a host built against an older
 * header, whose freddy_track ends earlier, gets the fields it knows); returns the number of bytes written, or < 0.  Hosts
 * that are built separately from the library (the PostgreSQL extension) call this one. */
int freddy_gpu_last_track_sized(const freddy_gpu_index_t* ivpq, void* out, size_t out_size);

/* The allocation seam: every device and pinned-host allocation of the library passes one counter, and a test can make one of
 * them fail.  Process-wide, for tests and diagnosis only; nothing reads the environment, and with nothing armed and tracking off
 * an allocation costs one relaxed atomic add.
 *   alloc_fail_nth(n, real): the n-th allocation from now fails ONCE (whichever thread makes it), then the seam is disarmed;
 *     n <= 0 disarms.  real = 0: the failure is injected -- hipErrorOutOfMemory without a call into the runtime.  real != 0: the
 *     runtime itself is made to fail, by a request for 2^60 bytes, so that its own error state is that of a real failure.
 *     The caller sees what any failed allocation gives: FREDDY_E_NOMEM from the entry point that made it.
 *   alloc_track(on): on != 0 starts tracking from an EMPTY live set (what was allocated before is unknown to it and never
 *     counted); 0 stops it and drops the set.
 *   alloc_stats(out, out_size): at most out_size bytes of the record; returns the number written.  calls = allocations requested
 *     since the library was loaded, failed = those that returned an error; live / live_bytes = allocations made while tracking
 *     and not yet freed; digest = a 64-bit value that depends on the live set {(address, bytes)} alone, not on the order in
 *     which it came about (0 when it is empty). */
typedef struct freddy_alloc_stats {
  int64_t calls, failed, live, live_bytes;
  uint64_t digest;
} freddy_alloc_stats;
int freddy_gpu_debug_alloc_fail_nth(int64_t n, int32_t real);
int freddy_gpu_debug_alloc_track(int32_t on);
int freddy_gpu_debug_alloc_stats(freddy_alloc_stats* out, size_t out_size);

/* ABI version of the library: bumped whenever a struct of this header grows or an entry point changes meaning.  A host
 * compares it with the FREDDY_GPU_ABI_VERSION it was compiled against before its first other call into the library
 * (pg/freddy_gpu_glue.c: ensure_exit_hook(), at the top of every freddy_glue_* entry) and refuses a mismatch instead of
 * overrunning a stack variable. */
#define FREDDY_GPU_ABI_VERSION 4
int freddy_gpu_abi_version(void);

/* Options of a pinned index (the FREDDY_GPU_* environment variables of the same names are read once, at pin time).  No setting
 * changes a result.
 *   deployment:  "scan_share" (the batches that share the chip with one of this handle's: the batches the caller keeps in flight
 *                through the *_dev entry points, one stream each, or the other BACKENDS searching at the same time -- a persistent
 *                scan takes at least n_cus / scan_share workgroups, one per CU, and with "scan_elastic" further ones while CUs are
 *                free; default 0 = auto: the whole chip, or half of it for a host-buffer call that
 *                starts while another backend (process) of the same GPU is searching: the library keeps a registry of live backends per
 *                physical GPU in /dev/shm and also picks GPU_MAX_HW_QUEUES from it before its first HIP call -- 6 alone, 2 beside
 *                others),
 *                "scan_elastic" (IVFADC batches with scan_share > 1 through the six-phase scan, i.e. not the whole-slab scan of
 *                K <= 256 and not batches over a flat PQ table: 1 = a scan also launches extra workgroups, up to
 *                n_cus - scan_elastic_reserve - reserve_cus * scan_share scan workgroups alive over all streams of the handle; an
 *                extra takes work entries only while no other batch's scan is announced, and leaves when one is; 2 = every
 *                extra leaves after its first entry (tests); 0 = off, the default: exactly n_cus / scan_share workgroups),
 *                "scan_elastic_reserve" (CUs the elastic scans together leave to the other kernels of the batches in flight; 64),
 *                "reserve_cus" (CUs a persistent scan leaves free), "pipeline_batch" / "pipeline_lanes" (host-buffer IVFADC calls:
 *                queries per sub-batch, 2048; sub-batches in flight, 1..4), "coarse_pieces" (1: a call of one sub-batch launches its
 *                cell selection per staged piece of the queries), "lut_budget_mb" (workspace cap per call)
 *   paths (each has GPU tests of its own):  "fused" (-1 auto, 0 generic kernels, 1 cell-grouped scans always), "fused_kernel"
 *                (5 filter + refine on int16 slabs, 3 the reference's arithmetic for every row), "coarse_approx" (1: cell selection
 *                as filter + refine, 0: every coarse distance exact), "one_launch" (1: a host-buffer call with ONE query -- the
 *                reference's own call shape -- is a single launch, pq_one_kernel / ivf_one_kernel, the host polls the kernel's
 *                completion word; 0: the multi-launch path.  A handle whose grid once failed to meet within the kernel's bounded
 *                polls switches itself to 0), "pq_fused" (batches over the flat PQ table through the cell-grouped scan over
 *                pseudo-lists of 4096 rows: -1 = from 16 queries on, 0 never, 1 always), "sparse_items" (cells that at most this
 *                many queries of a batch probe are scanned item by item; default 2, 0 = never, a negative value forces it for
 *                cells of up to that many items whatever the batch), "running_bound" (1: the scan's work entries share a
 *                per-query bound of the L-th smallest cheap distance), "codes_u8" (1: indexes with K <= 256 are scanned from one
 *                byte per code by the kernel that keeps a whole work entry's slab in LDS; 2: one byte per code, the six-phase kernel;
 *                0: the int16 layout), "exact_filter" (exact brute-force kNN as f16-split MFMA filter + exact
 *                refine: -1 = tables of >= 8192 rows and k <= 32, 0 never -- and no fragment copy of a table pinned with it --,
 *                1 always), "exact_join_tile" (queries per workgroup of the exact join's filter: 0 = 128 when Q > 64 and
 *                d <= 320, else 64; 64 = never 128), "analogy_pass" (triples per pass of the approximate analogies: 0 = as many as
 *                keep a pass's lists within 8 M entries), "similarity_pass_bytes" (the device result block of one pass of A rows of
 *                freddy_gpu_similarity_matrix / _join: 0 = 256 MiB, at most 4 GiB; always 16 rows of A at least), "cluster_pass" (targets
 *                per assignment pass of freddy_gpu_cluster: 0 = 2^22; 64 at least), "cluster_walk" (how freddy_gpu_cluster finds a
 *                cluster's sampled members: 1 = by walking all positions, as it does beyond 1024 clusters; 2 = from per-block counts;
 *                0 = auto: 2 from n > 32768 tokens on), "exact_resolve" (where freddy_gpu_exact_search / _exact_join /
 *                _exact_analogy turn their id set into table rows: 0 = on the host, the default; 1 = on the device, as the
 *                *_exact_*_ids calls always do), "resolve_block" (bitmap words per block of the device resolve: 0 = 256, at most
 *                2^20; tests make a small table span many blocks), "tokenize_pass" (on a vector handle: texts per pass of the
 *                *_search_texts calls: 0 = as many as a pinned block of 256 MiB holds), "tokenize_unit" (the normalisation of
 *                text vectors: 1 = a wave per text, lane 0 walking the chain of squares; 2 = one chain per lane over 64 texts;
 *                0 = auto, the default: 1 below 16384 texts, 2 from there on)
 *   self-checks (tests):  "check_brackets" (bit 0: the scan keeps and the merge refines EVERY probed row, bit 1: the cell
 *                selection refines every cell, bit 2: exact kNN and the exact join refine every row -- each with its proven bracket compared with
 *                the reference's value: freddy_gpu_filter_bound_violations / _checked; bit 3: the exact analogy refines
 *                every row for every analogy, counted the same way), "join_host_traversal", "join_front_gather" (1, the
 *                default: freddy_gpu_knn_join_ids gathers its queries in the sub-distance launch; 0: a gather launch, then the
 *                sub-distance kernel -- the same lists either way),
 *                "join_libm_margin_ppm", "grid_cus" (the CU count that every grid sized from the chip is planned with, and every
 *                choice of a kernel made from it -- csrc/grid_plan.h: v <= 0 = the device's count, the default; otherwise
 *                min(v, the device's count).  It can only shrink grids, never grow them: the workgroups of the one-launch kernels
 *                wait for each other and must be co-resident.  With a small value every workgroup loops over many pieces of work
 *                where at the device's count it takes one and leaves; also what a compute partition of the card would see.  It
 *                reaches the replicas and a PQ handle's views, and holds across append_rows, remove_rows, update_rows and
 *                update_codebook) */
int freddy_gpu_set_option(freddy_gpu_index_t* index, const char* name, int64_t value);

/* Thread-local message of the last failing call; valid until the next call. */
const char* freddy_gpu_last_error(void);

/* Per-kernel timing with HIP events on the launch stream.  enable=1 starts recording
 * (and clears earlier records); freddy_gpu_profile_read() synchronises, then reports up
 * to `cap` kernels: name, number of launches, total milliseconds.  Returns the number
 * of distinct kernels (or <0). */
int freddy_gpu_profile_enable(freddy_gpu_index_t* index, int32_t enable);
int freddy_gpu_profile_read(freddy_gpu_index_t* index, int32_t cap, char (*names)[64],
                            int64_t* launches, double* total_ms);

/* Sizes the caller may want for roofline arithmetic. */
int64_t freddy_gpu_index_bytes(const freddy_gpu_index_t* index);   /* HBM footprint of the pinned index */
/* Sum of list lengths the last ivfadc call scanned (all queries, all probes). */
int64_t freddy_gpu_last_scanned_rows(const freddy_gpu_index_t* index);
/* Distinct cells the last probing round touched (cell-grouped scans) and the rows of their lists: the bytes a
 * scan that reads every probed list once per batch must move, as the reference's loop does (freddy.c:939-974). */
int freddy_gpu_last_probed_cells(const freddy_gpu_index_t* index, int64_t* n_cells, int64_t* rows);
/* Self-check of the filter + refine IVFADC scan: every row that reaches the exact stage
 * has both its proven bracket [d_lo, d_lo + E] and the reference's distance d in hand; this returns how
 * many such rows had d outside the bracket since the index was pinned (0 unless the error analysis is
 * wrong for some input; <0 on a HIP error).  Synchronises the device. */
int64_t freddy_gpu_filter_bound_violations(const freddy_gpu_index_t* index);
/* How many rows that check has seen -- counted only in the tests' refine-every-row mode
 * (option check_brackets, bit 0), where it is the number of probed rows; 0 otherwise. */
int64_t freddy_gpu_filter_bound_checked(const freddy_gpu_index_t* index);
/* The coarse-cell selection is a filter + refine too (MFMA distances with a proven bracket, the reference's
 * squareDistance for the candidate cells): refined cells whose distance left the bracket are
 * INCLUDED in freddy_gpu_filter_bound_violations; this returns how many cells the tests' refine-every-cell mode
 * (option check_brackets, bit 1) has checked. */
int64_t freddy_gpu_coarse_bound_checked(const freddy_gpu_index_t* index);
/* The elastic scan's four device words (option "scan_elastic") after synchronising the device: out[0] = scan workgroups alive,
 * out[1] = guaranteed workgroups announced and not yet started (both 0 once every search has finished), out[2] = extra
 * workgroups that took work since the index was pinned, out[3] = extras that left because another scan was announced.  The
 * words only steer speed: no result depends on them.  All 0 for a handle that is not an IVF index. */
int freddy_gpu_scan_elastic_stats(const freddy_gpu_index_t* index, int64_t out[4]);

#ifdef __cplusplus
}
#endif
#endif /* FREDDY_GPU_H */
