/*
 * ref_driver.c -- plain-array entry points into the FREDDY reference's own C code, in the style of
 * oracle/freddy_oracle.h.  Test infrastructure only: compiled together with the reference's sources and the
 * stand-in runtime (pgshim_rt.c) into oracle/_ref/libfreddy_ref.so, which is never committed.
 *
 *   fr_<function>   calls one reference function on caller-provided arrays;
 *   fr_srf_<name>   runs a set-returning function of the reference to exhaustion over the tables registered
 *                   with fr_add_*, and returns the rows it emitted (as text, exactly as emitted) and the
 *                   entries behind them (read from the SRF's user_fctx).
 *
 * Every entry point returns 0, or FR_ERROR after the reference raised an ERROR (fr_last_error() has the text).
 * Nothing here guards the reference's undefined cases: the tests filter their inputs instead.
 */
#include "pgshim_rt.h"

#include "catalog/pg_type.h"
#include "cosine_similarity.h"
#include "index_utils.h"
#include "output_utils.h"

#define FR_ERROR (-100)
#define FR_STRLEN 24

#define FR_BEGIN                        \
  pgshim_error_armed = 1;               \
  if (setjmp(pgshim_error_jmp)) {       \
    pgshim_reset_memory();              \
    return FR_ERROR;                    \
  }
#define FR_END              \
  pgshim_error_armed = 0;   \
  pgshim_reset_memory();    \
  return 0;

const char* fr_last_error(void) { return pgshim_last_error(); }
long fr_statement_count(void) { return pgshim_statement_count(); }

/* ======================================================================================================== */
/* function level                                                                                           */
/* ======================================================================================================== */

int fr_sqdist(const float* a, const float* b, int n, float* out) {
  FR_BEGIN
  *out = squareDistance((float*)a, (float*)b, n);
  FR_END
}

static Codebook make_codebook(int n_entries, int s, const int32_t* pos, const int32_t* code, const float* vectors) {
  Codebook cb = palloc(sizeof(CodebookEntry) * (size_t)n_entries);
  for (int e = 0; e < n_entries; e++) {
    cb[e].pos = pos[e];
    cb[e].code = code[e];
    cb[e].vector = palloc(sizeof(float) * (size_t)s);
    memcpy(cb[e].vector, vectors + (size_t)e * s, sizeof(float) * (size_t)s);
  }
  return cb;
}

/* lut [m*K]; the entries (pos, code, vector) in any order */
int fr_lut(float* lut, int m, int K, int s, const float* q, const int32_t* pos, const int32_t* code,
           const float* vectors) {
  FR_BEGIN
  getPrecomputedDistances(lut, m, K, s, (float*)q, make_codebook(m * K, s, pos, code, vectors));
  FR_END
}

/* lut2 [(m/2)*K*K]; the entries position-major, any code order inside a position */
int fr_lut_double(float* lut2, int m, int K, int s, const float* q, const int32_t* pos, const int32_t* code,
                  const float* vectors) {
  FR_BEGIN
  getPrecomputedDistancesDouble(lut2, m, K, s, (float*)q, make_codebook(m * K, s, pos, code, vectors));
  FR_END
}

int fr_adc(const float* lut, const int16_t* codes, int m, int K, float* out) {
  FR_BEGIN
  *out = computePQDistanceInt16((float*)lut, (int16*)codes, m, K);
  FR_END
}

/* initTopK(s) + the call sites' guard: if (dist < maxDist) { updateTopK; maxDist = tk[k-1].distance; } */
int fr_topk_stream(int k, float sentinel, int n, const float* dists, const int32_t* ids, int use_init_many,
                   TopKEntry* out) {
  FR_BEGIN
  TopK tk;
  float maxDist;
  if (use_init_many) {
    TopK* tks;
    float* maxDists;
    initTopKs(&tks, &maxDists, 3, k, sentinel);
    tk = tks[2];
    maxDist = maxDists[2];
  } else {
    initTopK(&tk, k, sentinel);
    maxDist = sentinel;
  }
  for (int i = 0; i < n; i++) {
    if (dists[i] < maxDist) {
      updateTopK(tk, dists[i], ids[i], k, maxDist);
      maxDist = tk[k - 1].distance;
    }
  }
  memcpy(out, tk, sizeof(TopKEntry) * (size_t)k);
  FR_END
}

/* the same over updateTopKPV / initTopKPV(s); out_vec_index[i] = the stream position whose vector sits in slot i, -1 if none */
int fr_topkpv_stream(int k, float sentinel, int n, const float* dists, const int32_t* ids, int dim,
                     int use_init_many, TopKEntry* out, int32_t* out_vec_index) {
  FR_BEGIN
  TopKPV tk;
  float maxDist;
  float4* vecs = palloc(sizeof(float4) * (size_t)(n ? n : 1));
  if (use_init_many) {
    TopKPV* tks;
    float* maxDists;
    initTopKPVs(&tks, &maxDists, 2, k, sentinel, dim);
    tk = tks[1];
    maxDist = maxDists[1];
  } else {
    initTopKPV(&tk, k, sentinel, dim);
    maxDist = sentinel;
  }
  for (int i = 0; i < n; i++) {
    if (dists[i] < maxDist) {
      updateTopKPV(tk, dists[i], ids[i], k, maxDist, vecs + i, dim);
      maxDist = tk[k - 1].distance;
    }
  }
  for (int i = 0; i < k; i++) {
    out[i].id = tk[i].id;
    out[i].distance = tk[i].distance;
    out_vec_index[i] = tk[i].vector ? (int32_t)(tk[i].vector - vecs) : -1;
  }
  FR_END
}

/* qsort with cmpTopKEntry / cmpTopKPVEntry */
int fr_sort_entries(TopKEntry* entries, int n, int pv) {
  FR_BEGIN
  if (pv) {
    TopKPVEntry* e = palloc(sizeof(TopKPVEntry) * (size_t)(n ? n : 1));
    for (int i = 0; i < n; i++) {
      e[i].id = entries[i].id;
      e[i].distance = entries[i].distance;
      e[i].vector = NULL;
    }
    qsort(e, (size_t)n, sizeof(TopKPVEntry), cmpTopKPVEntry);
    for (int i = 0; i < n; i++) {
      entries[i].id = e[i].id;
      entries[i].distance = e[i].distance;
    }
  } else {
    qsort(entries, (size_t)n, sizeof(TopKEntry), cmpTopKEntry);
  }
  FR_END
}

int fr_cmp_entries(float a, float b, int pv, int* out) {
  FR_BEGIN
  if (pv) {
    TopKPVEntry x = {0, a, NULL}, y = {1, b, NULL};
    *out = cmpTopKPVEntry(&x, &y);
  } else {
    TopKEntry x = {0, a}, y = {1, b};
    *out = cmpTopKEntry(&x, &y);
  }
  FR_END
}

/* postverify for one query: k*pvf candidates in buffer order (id -1 = hole), cand_vecs [k*pvf][d] */
int fr_postverify(const float* q, int d, int k, int pvf, const int32_t* cand_ids, const float* cand_vecs,
                  float sentinel, TopKEntry* out) {
  FR_BEGIN
  int n = k * pvf;
  TopKPV pv;
  TopK tk;
  int index = 0;
  float4* qv = (float4*)q;
  initTopKPV(&pv, n, sentinel, d);
  initTopK(&tk, k, sentinel);
  for (int j = 0; j < n; j++) {
    pv[j].id = cand_ids[j];
    pv[j].vector = (float4*)(cand_vecs + (size_t)j * d);
  }
  postverify(&index, 1, k, pvf, &pv, &tk, &qv, d, sentinel);
  memcpy(out, tk, sizeof(TopKEntry) * (size_t)k);
  FR_END
}

/* determineCoarseIdsMultiWithStatisticsMulti (multi != 0) over a two-position coarse codebook [2][Kc][d/2], or
 * determineCoarseIdsMultiWithStatistics over a flat coarse quantizer [cells][d]; stats [cells+1].
 * cells_out [n_active][cells], counts_out [n_active], *last_out = lastIteration. */
int fr_multi_index_select(int multi, const float* coarse, int Kc, int d, const float* stats, const float* queries, int Q,
                          const int32_t* active, int n_active, int n_targets, int min_target_count,
                          float confidence, int32_t* cells_out, int32_t* counts_out, int* last_out) {
  FR_BEGIN
  const int cells = multi ? Kc * Kc : Kc, sub = d / 2;
  int** cqIds;
  int** cqTableIds;
  int* cqTableIdCounts;
  float4** qv = palloc(sizeof(float4*) * (size_t)Q);
  for (int i = 0; i < Q; i++) qv[i] = (float4*)(queries + (size_t)i * d);
  bool last;
  if (multi) {
    Codebook cq = palloc(sizeof(CodebookEntry) * (size_t)(2 * Kc));
    for (int e = 0; e < 2 * Kc; e++) {
      cq[e].pos = e / Kc;
      cq[e].code = e % Kc;
      cq[e].vector = (float*)(coarse + (size_t)e * sub);
    }
    last = determineCoarseIdsMultiWithStatisticsMulti(&cqIds, &cqTableIds, &cqTableIdCounts, (int*)active, n_active, Q,
                                                      1000.0, cq, cells, 2, Kc, qv, d, (float*)stats, n_targets,
                                                      min_target_count, confidence);
  } else {
    CoarseQuantizer cq = palloc(sizeof(CoarseQuantizerEntry) * (size_t)cells);
    for (int e = 0; e < cells; e++) {
      cq[e].id = e;
      cq[e].vector = (float*)(coarse + (size_t)e * d);
    }
    last = determineCoarseIdsMultiWithStatistics(&cqIds, &cqTableIds, &cqTableIdCounts, (int*)active, n_active, Q,
                                                 1000.0, cq, cells, qv, d, (float*)stats, n_targets, min_target_count,
                                                 confidence);
  }
  /* the number of cells of a query = its occurrences in the cell -> queries table */
  for (int x = 0; x < n_active; x++) counts_out[x] = 0;
  for (int c = 0; c < cells; c++)
    for (int j = 0; j < cqTableIdCounts[c]; j++)
      for (int x = 0; x < n_active; x++)
        if (active[x] == cqTableIds[c][j]) counts_out[x]++;
  for (int x = 0; x < n_active; x++)
    memcpy(cells_out + (size_t)x * cells, cqIds[active[x]], sizeof(int) * (size_t)counts_out[x]);
  *last_out = last ? 1 : 0;
  FR_END
}

int fr_confidence(int hyp, int expect, int size, float p, int stat_size, float* out) {
  FR_BEGIN
  *out = hyp ? getConfidenceHyp(expect, size, p, stat_size) : getConfidenceBin(expect, size, p);
  FR_END
}

/* updateCodebook over the tuples in the given order (order[j] = pos*K + code of tuple j).  codebook [m][K][s] and
 * counts [m*K] receive the in-memory CodebookWithCounts afterwards; codes [n][m]; count_incs [m*K]. */
int fr_update_codebook(float* codebook, int32_t* counts, int m, int K, int s, const float* vecs, int n,
                       const int32_t* order, int32_t* codes, int32_t* count_incs) {
  FR_BEGIN
  const int E = m * K, d = m * s;
  CodebookWithCounts cb = palloc(sizeof(CodebookEntryComplete) * (size_t)E);
  for (int j = 0; j < E; j++) {
    int slot = order[j];
    cb[j].pos = slot / K;
    cb[j].code = slot % K;
    cb[j].vector = codebook + (size_t)slot * s;
    cb[j].count = counts[slot];
  }
  float** raw = palloc(sizeof(float*) * (size_t)(n ? n : 1));
  for (int i = 0; i < n; i++) raw[i] = (float*)(vecs + (size_t)i * d);
  int** nearest = palloc(sizeof(int*) * (size_t)(n ? n : 1));
  updateCodebook(raw, n, s, cb, m, K, nearest, count_incs);
  for (int i = 0; i < n; i++)
    for (int j = 0; j < m; j++) codes[(size_t)i * m + j] = nearest[i][j];
  for (int j = 0; j < E; j++) counts[order[j]] = cb[j].count;
  FR_END
}

/* addToTargetList: the ids in call order go to query 0's chain of lists of `list_size`; returns the chain
 * flattened (out_ids [n]), the size of every list (out_sizes [n / list_size + 1]) and their number. */
int fr_target_list(const int32_t* ids, int n, int list_size, int method, int32_t* out_ids, int32_t* out_sizes,
                   int* out_lists) {
  FR_BEGIN
  TargetListElem* lists = palloc(sizeof(TargetListElem));
  int16 dummy_codes[1] = {0};
  float4 dummy_vector[1] = {0};
  lists[0].codes = palloc(sizeof(int16*) * (size_t)list_size);
  lists[0].ids = palloc(sizeof(int) * (size_t)list_size);
  lists[0].vectors = palloc(sizeof(float4*) * (size_t)list_size);
  lists[0].size = 0;
  lists[0].next = NULL;
  lists[0].last = &lists[0];
  for (int i = 0; i < n; i++) addToTargetList(lists, 0, list_size, method, dummy_codes, dummy_vector, ids[i]);
  int w = 0, l = 0;
  for (TargetListElem* e = &lists[0]; e; e = e->next) {
    out_sizes[l++] = e->size;
    for (int i = 0; i < e->size; i++) out_ids[w++] = e->ids[i];
  }
  *out_lists = l;
  FR_END
}

/* addToBlacklist for every id of `add` in order, then inBlacklist for every id of `ask` */
int fr_blacklist(const int32_t* add, int n_add, const int32_t* ask, int n_ask, int32_t* out) {
  FR_BEGIN
  Blacklist bl;
  bl.isValid = false;
  for (int i = 0; i < n_add; i++) {
    Blacklist* fresh = palloc(sizeof(Blacklist));
    fresh->isValid = false;
    addToBlacklist(add[i], &bl, fresh);
  }
  for (int i = 0; i < n_ask; i++) out[i] = inBlacklist(ask[i], &bl) ? 1 : 0;
  FR_END
}

/* convert_<type>_bytea then convert_bytea_<type>: type 0 float4, 1 int32, 2 int16; `bytes` of payload.
 * preallocated != 0 takes the "size given, memory provided" branch.  out receives the payload back. */
int fr_bytea_roundtrip(int type, const void* in, int n, int preallocated, void* out, int* out_n, int* out_varsize) {
  FR_BEGIN
  bytea* b;
  int size = preallocated ? n : 0;
  if (type == 0) {
    float4* o = preallocated ? (float4*)out : NULL;
    convert_float4_bytea((float4*)in, &b, n);
    convert_bytea_float4(b, &o, &size);
    if (!preallocated && size) memcpy(out, o, sizeof(float4) * (size_t)size);
  } else if (type == 1) {
    int32* o = preallocated ? (int32*)out : NULL;
    convert_int32_bytea((int32*)in, &b, n);
    convert_bytea_int32(b, &o, &size);
    if (!preallocated && size) memcpy(out, o, sizeof(int32) * (size_t)size);
  } else {
    int16* o = preallocated ? (int16*)out : NULL;
    convert_int16_bytea((int16*)in, &b, n);
    convert_bytea_int16(b, &o, &size);
    if (!preallocated && size) memcpy(out, o, sizeof(int16) * (size_t)size);
  }
  *out_n = size;
  *out_varsize = VARSIZE(b);
  FR_END
}

int fr_cosine_simple(const float* a, const float* b, int n, int norm, double* out) {
  FR_BEGIN
  Datum* da = palloc(sizeof(Datum) * (size_t)(n ? n : 1));
  Datum* db = palloc(sizeof(Datum) * (size_t)(n ? n : 1));
  for (int i = 0; i < n; i++) {
    da[i] = Float4GetDatum(a[i]);
    db[i] = Float4GetDatum(b[i]);
  }
  *out = norm ? cosine_similarity_simple_norm(da, db, n) : cosine_similarity_simple(da, db, n);
  FR_END
}

#ifdef FR_HAVE_CORE_FUNCTIONS
Datum cosine_similarity_bytea(PG_FUNCTION_ARGS);
Datum vec_minus_bytea(PG_FUNCTION_ARGS);
Datum vec_plus_bytea(PG_FUNCTION_ARGS);
Datum vec_normalize_bytea(PG_FUNCTION_ARGS);

/* op 0 cosine_similarity_bytea (out[0]), 1 vec_minus_bytea, 2 vec_plus_bytea, 3 vec_normalize_bytea (a only) */
int fr_core_bytea(int op, const float* a, const float* b, int n, float* out) {
  FR_BEGIN
  FunctionCallInfoBaseData fc;
  memset(&fc, 0, sizeof fc);
  fc.nargs = op == 3 ? 1 : 2;
  fc.args[0] = PointerGetDatum(pgshim_make_bytea(a, n * (int)sizeof(float)));
  if (op != 3) fc.args[1] = PointerGetDatum(pgshim_make_bytea(b, n * (int)sizeof(float)));
  if (op == 0) {
    out[0] = DatumGetFloat4(cosine_similarity_bytea(&fc));
  } else {
    Datum r = op == 1 ? vec_minus_bytea(&fc) : op == 2 ? vec_plus_bytea(&fc) : vec_normalize_bytea(&fc);
    bytea* v = DatumGetByteaP(r);
    if (VARSIZE(v) - VARHDRSZ != n * (int)sizeof(float)) elog(ERROR, "fr_core_bytea: result of %d bytes", VARSIZE(v) - VARHDRSZ);
    if (n) memcpy(out, VARDATA(v), sizeof(float) * (size_t)n);
  }
  FR_END
}
int fr_have_core_functions(void) { return 1; }
#else
int fr_have_core_functions(void) { return 0; }
#endif

/* ======================================================================================================== */
/* tables                                                                                                   */
/* ======================================================================================================== */

static void name_function(const char* function, const char* table) {
  static const char* const col[] = {"name"};
  static const int type[] = {PGSHIM_TEXT};
  pgshim_table* t = pgshim_create_table(function, 1, col, type);
  Datum cell = PointerGetDatum(table);
  pgshim_add_row(t, &cell, NULL);
}

/* drops every table and registers the functions that name them */
int fr_reset_tables(void) {
  pgshim_drop_tables();
  name_function("get_vecs_name_original()", "vecs_original");
  name_function("get_vecs_name()", "vecs_norm");
  name_function("get_vecs_name_pq_quantization()", "pq_quantization");
  name_function("get_vecs_name_codebook()", "pq_codebook");
  name_function("get_vecs_name_residual_quantization()", "fine_quantization");
  name_function("get_vecs_name_coarse_quantization()", "coarse_quantization");
  name_function("get_vecs_name_residual_codebook()", "residual_codebook");
  return 0;
}

int fr_set_parameter(const char* function, int value) {
  static const char* const col[] = {"value"};
  static const int type[] = {PGSHIM_INT4};
  pgshim_table* t = pgshim_create_table(function, 1, col, type);
  if (!t) return FR_ERROR;
  Datum cell = Int32GetDatum(value);
  pgshim_add_row(t, &cell, NULL);
  return 0;
}

/* a codebook table (id, pos, code, vector, count): the entries in the given (stored) order */
int fr_add_codebook(const char* table, int n_entries, int s, const int32_t* pos, const int32_t* code,
                    const float* vectors) {
  static const char* const col[] = {"id", "pos", "code", "vector", "count"};
  static const int type[] = {PGSHIM_INT4, PGSHIM_INT4, PGSHIM_INT4, PGSHIM_BYTEA, PGSHIM_INT4};
  pgshim_table* t = pgshim_create_table(table, 5, col, type);
  if (!t) return FR_ERROR;
  for (int e = 0; e < n_entries; e++) {
    Datum cells[5] = {Int32GetDatum(e), Int32GetDatum(pos[e]), Int32GetDatum(code[e]),
                      PointerGetDatum(vectors + (size_t)e * s), Int32GetDatum(1)};
    int bytes[5] = {0, 0, 0, s * (int)sizeof(float), 0};
    pgshim_add_row(t, cells, bytes);
  }
  return 0;
}

/* (id, vector): float vectors (vecs_norm, coarse_quantization) when codes == NULL, else int16 codes (pq_quantization) */
int fr_add_id_vector(const char* table, int64_t n, int width, const int32_t* ids, const float* vectors,
                     const int16_t* codes) {
  static const char* const col[] = {"id", "vector"};
  static const int type[] = {PGSHIM_INT4, PGSHIM_BYTEA};
  pgshim_table* t = pgshim_create_table(table, 2, col, type);
  if (!t) return FR_ERROR;
  for (int64_t r = 0; r < n; r++) {
    Datum cells[2] = {Int32GetDatum(ids[r]), codes ? PointerGetDatum(codes + r * width) : PointerGetDatum(vectors + r * width)};
    int bytes[2] = {0, width * (int)(codes ? sizeof(int16_t) : sizeof(float))};
    pgshim_add_row(t, cells, bytes);
  }
  return 0;
}

/* fine_quantization (id, coarse_id, vector) */
int fr_add_fine(const char* table, int64_t n, int m, const int32_t* ids, const int32_t* coarse_id,
                const int16_t* codes) {
  static const char* const col[] = {"id", "coarse_id", "vector"};
  static const int type[] = {PGSHIM_INT4, PGSHIM_INT4, PGSHIM_BYTEA};
  pgshim_table* t = pgshim_create_table(table, 3, col, type);
  if (!t) return FR_ERROR;
  for (int64_t r = 0; r < n; r++) {
    Datum cells[3] = {Int32GetDatum(ids[r]), Int32GetDatum(coarse_id[r]), PointerGetDatum(codes + r * m)};
    int bytes[3] = {0, 0, m * (int)sizeof(int16_t)};
    pgshim_add_row(t, cells, bytes);
  }
  return 0;
}

/* any statement through SPI_exec: the number of rows, for the tests of the stand-in itself */
int fr_spi_count(const char* command, int64_t* rows, int32_t* first_col, int max_rows) {
  FR_BEGIN
  SPI_connect();
  SPI_exec(command, 0);
  *rows = (int64_t)SPI_processed;
  for (uint64 i = 0; i < SPI_processed && (int)i < max_rows; i++) {
    bool isnull;
    first_col[i] = DatumGetInt32(SPI_getbinval(SPI_tuptable->vals[i], SPI_tuptable->tupdesc, 1, &isnull));
  }
  SPI_finish();
  FR_END
}

/* ======================================================================================================== */
/* SRF level                                                                                                */
/* ======================================================================================================== */

Datum pq_search(PG_FUNCTION_ARGS);
Datum pq_search_in(PG_FUNCTION_ARGS);
Datum ivfadc_search(PG_FUNCTION_ARGS);
Datum ivfadc_batch_search(PG_FUNCTION_ARGS);
Datum grouping_pq(PG_FUNCTION_ARGS);

/* calls the SRF until it is done; row r, column c of the emitted text goes to strs[(r*ncols + c) * FR_STRLEN] */
static int64_t run_srf(Datum (*fn)(PG_FUNCTION_ARGS), FunctionCallInfo fc, int ncols, char* strs, int64_t max_rows) {
  int64_t rows = 0;
  for (;;) {
    Datum r = fn(fc);
    if (fc->srf_done) break;
    HeapTuple t = (HeapTuple)DatumGetPointer(r);
    if (rows >= max_rows) elog(ERROR, "ref_driver: the SRF emitted more than %ld rows", (long)max_rows);
    if (t->natts != ncols) elog(ERROR, "ref_driver: the SRF emitted %d columns, %d expected", t->natts, ncols);
    for (int c = 0; c < ncols; c++) snprintf(strs + (rows * ncols + c) * FR_STRLEN, FR_STRLEN, "%s", t->cstrings[c]);
    rows++;
  }
  return rows;
}

static void copy_single(FunctionCallInfo fc, int k, TopKEntry* out) {
  UsrFctx* u = (UsrFctx*)((FuncCallContext*)fc->srf_ctx)->user_fctx;
  if (u->k != k) elog(ERROR, "ref_driver: user_fctx holds k = %d", u->k);
  memcpy(out, u->tk, sizeof(TopKEntry) * (size_t)k);
}

/* strs [k][2][FR_STRLEN], out [k] */
int fr_srf_pq_search(const float* q, int d, int k, TopKEntry* out, char* strs, int64_t* rows) {
  FR_BEGIN
  FunctionCallInfoBaseData fc;
  memset(&fc, 0, sizeof fc);
  fc.nargs = 2;
  fc.args[0] = PointerGetDatum(pgshim_make_bytea(q, d * (int)sizeof(float)));
  fc.args[1] = Int32GetDatum(k);
  *rows = run_srf(pq_search, &fc, 2, strs, k);
  copy_single(&fc, k, out);
  FR_END
}

int fr_srf_pq_search_in(const float* q, int d, int k, const int32_t* ids, int n_ids, TopKEntry* out, char* strs,
                        int64_t* rows) {
  FR_BEGIN
  FunctionCallInfoBaseData fc;
  memset(&fc, 0, sizeof fc);
  fc.nargs = 3;
  fc.args[0] = PointerGetDatum(pgshim_make_bytea(q, d * (int)sizeof(float)));
  fc.args[1] = Int32GetDatum(k);
  fc.args[2] = PointerGetDatum(pgshim_make_int4_array(ids, n_ids));
  *rows = run_srf(pq_search_in, &fc, 2, strs, k);
  copy_single(&fc, k, out);
  FR_END
}

int fr_srf_ivfadc_search(const float* q, int d, int k, TopKEntry* out, char* strs, int64_t* rows) {
  FR_BEGIN
  FunctionCallInfoBaseData fc;
  memset(&fc, 0, sizeof fc);
  fc.nargs = 2;
  fc.args[0] = PointerGetDatum(pgshim_make_bytea(q, d * (int)sizeof(float)));
  fc.args[1] = Int32GetDatum(k);
  *rows = run_srf(ivfadc_search, &fc, 2, strs, k);
  copy_single(&fc, k, out);
  FR_END
}

/* out_query_ids [n_ids] in fetch order, out [n_ids][k], strs [n_ids*k][3][FR_STRLEN]; *n_queries = vectors found */
int fr_srf_ivfadc_batch_search(const int32_t* query_ids, int n_ids, int k, int32_t* out_query_ids, TopKEntry* out,
                               char* strs, int64_t* rows, int* n_queries) {
  FR_BEGIN
  FunctionCallInfoBaseData fc;
  memset(&fc, 0, sizeof fc);
  fc.nargs = 2;
  fc.args[0] = PointerGetDatum(pgshim_make_int4_array(query_ids, n_ids));
  fc.args[1] = Int32GetDatum(k);
  *rows = run_srf(ivfadc_batch_search, &fc, 3, strs, (int64_t)n_ids * k);
  UsrFctxBatch* u = (UsrFctxBatch*)((FuncCallContext*)fc.srf_ctx)->user_fctx;
  if (u->k != k || u->queryIdsSize > n_ids) elog(ERROR, "ref_driver: user_fctx holds k = %d, %d queries", u->k, u->queryIdsSize);
  *n_queries = u->queryIdsSize;
  for (int i = 0; i < u->queryIdsSize; i++) {
    out_query_ids[i] = u->queryIds[i];
    memcpy(out + (size_t)i * k, u->tk[i], sizeof(TopKEntry) * (size_t)k);
  }
  FR_END
}

/* out_ids / out_group_index [n_ids] (index into the sorted group ids), out_sorted_groups [n_groups],
 * strs [n_ids][2][FR_STRLEN] */
int fr_srf_grouping_pq(const int32_t* ids, int n_ids, const int32_t* group_ids, int n_groups, int32_t* out_ids,
                       int32_t* out_group_index, int32_t* out_sorted_groups, char* strs, int64_t* rows) {
  FR_BEGIN
  FunctionCallInfoBaseData fc;
  memset(&fc, 0, sizeof fc);
  fc.nargs = 2;
  fc.args[0] = PointerGetDatum(pgshim_make_int4_array(ids, n_ids));
  fc.args[1] = PointerGetDatum(pgshim_make_int4_array(group_ids, n_groups));
  *rows = run_srf(grouping_pq, &fc, 2, strs, n_ids);
  UsrFctxGrouping* u = (UsrFctxGrouping*)((FuncCallContext*)fc.srf_ctx)->user_fctx;
  if (u->size != *rows || u->groupsSize != n_groups) elog(ERROR, "ref_driver: user_fctx holds %d rows, %d groups", u->size, u->groupsSize);
  for (int i = 0; i < u->size; i++) {
    out_ids[i] = u->ids[i];
    out_group_index[i] = u->nearestGroup[i];
  }
  for (int i = 0; i < n_groups; i++) out_sorted_groups[i] = u->groups[i];
  FR_END
}
