/* stub_gpu.c -- a recording stand-in for the 26 device functions the host mirror (postgres-word2vec_amd/host) calls.
 *
 * No GPU, no HIP: every call appends one line to stdout -- its name, the handle as the ordinal it was pinned with, every
 * scalar argument, every pointer that is NULL and one 64-bit hash over the bytes of all its input arrays (each with the length the
 * arguments imply) -- and fills its outputs deterministically from those hashes and the ids the handle holds.  The pin calls hash
 * the tables they are given, so the trace shows what the host tables held at every (re-)pin.
 * Argument names are shortened: q = queries, fill = sentinel, in / n_in = subset_ids / n_subset, to / n_to = target_ids /
 * n_targets, found = found_rule, cb = codebook, cq = the multi-index coarse quantizer.  tests/test_host_trace_cpu.py links
 * this file with trace_main.cpp and the host mirror and compares the output with tests/golden/host_trace.txt. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/freddy_gpu.h"

enum { KIND_PQ = 0, KIND_IVF = 1, KIND_IVPQ = 2, KIND_VEC = 3 };
static const char* const kKind[4] = {"pq", "ivf", "ivpq", "vec"};

/* a handle: kind, shape, and a copy of its ids in pinned order */
struct freddy_gpu_index {
  int kind, ordinal, has_vec;
  int64_t N;
  int32_t d, m, K, C;
  int32_t* ids;
};

#define MAX_LIVE 64
static freddy_gpu_index_t* g_live[MAX_LIVE];
static int g_n_live = 0, g_next_ordinal = 1;
static int g_quiet = 0;          /* stub_quiet(1): no trace lines (the timing mode; the set-up of the sweep sessions after the first) */
static long g_fail_in = 0;       /* > 0: the g_fail_in-th counted call from now fails */
static char g_err[128] = "";

#define T(...) do { if (!g_quiet) printf(__VA_ARGS__); } while (0)

static void report_live(void) { printf("live handles: %d\n", g_n_live); }
__attribute__((constructor)) static void report_live_at_exit(void) { atexit(report_live); }

static int is_live(const freddy_gpu_index_t* h) {
  for (int i = 0; i < g_n_live; ++i) if (g_live[i] == h) return 1;
  return 0;
}

static uint64_t fnv(const void* p, size_t bytes) {
  uint64_t h = 0xcbf29ce484222325ull;
  const unsigned char* b = (const unsigned char*)p;
  for (size_t i = 0; i < bytes; ++i) { h ^= b[i]; h *= 0x100000001b3ull; }
  return h;
}
static uint64_t mix(uint64_t h, uint64_t i) {
  uint64_t z = h + 0x9e3779b97f4a7c15ull * (i + 1);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
static uint32_t fbits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

/* An input array: " name=NULL" without one; else its bytes are hashed (64-bit FNV-1a) and folded, in argument order, into the one
 * hash that ends the call's line (" #<hash>") -- one hash over all input arrays of a call keeps the trace short. */
static uint64_t g_line_hash = 0;
static int g_line_arrays = 0;
static uint64_t arr(const char* name, const void* p, size_t bytes) {
  if (!p) { T(" %s=NULL", name); return 0; }
  const uint64_t h = fnv(p, bytes);
  g_line_hash = mix(g_line_hash ^ h, (uint64_t)++g_line_arrays);
  return h;
}
/* an output pointer: named only when it is NULL */
static void outp(const char* name, const void* p) { if (!p) T(" %s=NULL", name); }
static void hnd(const char* name, const freddy_gpu_index_t* h) {
  if (!h) T(" %s=NULL", name);
  else if (!is_live(h)) T(" %s=#dead", name);
  else T(" %s=#%d:%s", name, h->ordinal, kKind[h->kind]);
}

/* the end of every trace line: the injected failure if this is the call it was armed for, else `rc` */
static int done(int rc) {
  if (g_fail_in > 0 && --g_fail_in == 0) {
    snprintf(g_err, sizeof g_err, "stub: injected device failure");
    rc = FREDDY_E_HIP;
  }
  if (g_line_arrays) T(" #%016llx", (unsigned long long)g_line_hash);
  g_line_hash = 0; g_line_arrays = 0;
  T(" -> %d\n", rc);
  return rc;
}
/* armed for this call?  (outputs stay untouched then, and handles as they were) */
static int failing(void) { return g_fail_in == 1; }
static int usable(const freddy_gpu_index_t* h, int kind) { return h && is_live(h) && h->kind == kind; }
static int refuse(const char* why) { snprintf(g_err, sizeof g_err, "stub: %s", why); T(" !%s", why); return done(FREDDY_E_ARG); }

void stub_fail_after(long n) { g_fail_in = n; }
void stub_quiet(int on) { g_quiet = on; }

const char* freddy_gpu_last_error(void) { return g_err; }

static int has_id(const int32_t* ids, int64_t n, int32_t id) {
  for (int64_t i = 0; i < n; ++i) if (ids[i] == id) return 1;
  return 0;
}

/* One result list of k slots: the handle's ids walked DOWNWARDS from a start the seed chooses (so a higher id usually comes before
 * a lower one), kept if in `subset` (when given), in `vecs` (when given) and not one of `skip3` (when given); `may_be_short` lists
 * lose their last row for one seed in four; the rest is (-1, filler). */
static void fill_list(const freddy_gpu_index_t* h, uint64_t seed, int32_t k, float filler, const int32_t* subset, int64_t n_subset,
                      const freddy_gpu_index_t* vecs, const int32_t* skip3, int may_be_short, int32_t* out_ids, float* out_val) {
  int32_t n = 0;
  const int64_t N = h->N;
  const int64_t start = N ? (int64_t)(seed % (uint64_t)N) : 0;
  for (int64_t j = 0; j < N && n < k; ++j) {
    const int32_t id = h->ids[(start + N - j) % N];
    if (subset && !has_id(subset, n_subset, id)) continue;
    if (vecs && !has_id(vecs->ids, vecs->N, id)) continue;
    if (skip3 && has_id(skip3, 3, id)) continue;
    out_ids[n] = id;
    out_val[n] = (float)(mix(seed, (uint64_t)n) % 4096) / 2048.0f;
    ++n;
  }
  if (may_be_short && n > 0 && seed % 4 == 1) --n;
  for (; n < k; ++n) { out_ids[n] = -1; out_val[n] = filler; }
}

static freddy_gpu_index_t* new_handle(int kind, int64_t N, int32_t d, int32_t m, int32_t K, int32_t C, const int32_t* ids, int has_vec) {
  freddy_gpu_index_t* h = (freddy_gpu_index_t*)calloc(1, sizeof *h);
  h->kind = kind; h->ordinal = g_next_ordinal++; h->has_vec = has_vec;
  h->N = N; h->d = d; h->m = m; h->K = K; h->C = C;
  h->ids = (int32_t*)malloc(sizeof(int32_t) * (size_t)(N ? N : 1));
  if (N) memcpy(h->ids, ids, sizeof(int32_t) * (size_t)N);
  if (g_n_live >= MAX_LIVE) { fprintf(stderr, "stub: too many live handles\n"); abort(); }
  g_live[g_n_live++] = h;
  return h;
}

int freddy_gpu_pin_pq(const freddy_pq_desc* p, int device, freddy_gpu_index_t** out) {
  T("  gpu pin_pq device=%d d=%d m=%d K=%d N=%lld", device, p->d, p->m, p->K, (long long)p->N);
  arr("codebook", p->codebook, sizeof(float) * (size_t)p->K * p->d);
  arr("ids", p->ids, sizeof(int32_t) * (size_t)p->N);
  arr("codes", p->codes, sizeof(int16_t) * (size_t)p->N * p->m);
  if (failing()) return done(0);
  *out = new_handle(KIND_PQ, p->N, p->d, p->m, p->K, 0, p->ids, 0);
  T(" = #%d", (*out)->ordinal);
  return done(0);
}

int freddy_gpu_pin_ivf(const freddy_ivf_desc* p, int device, freddy_gpu_index_t** out) {
  T("  gpu pin_ivf device=%d d=%d m=%d K=%d C=%d N=%lld", device, p->d, p->m, p->K, p->C, (long long)p->N);
  arr("coarse", p->coarse, sizeof(float) * (size_t)p->C * p->d);
  arr("codebook", p->codebook, sizeof(float) * (size_t)p->K * p->d);
  arr("list_off", p->list_off, sizeof(int32_t) * ((size_t)p->C + 1));
  arr("ids", p->ids, sizeof(int32_t) * (size_t)p->N);
  arr("codes", p->codes, sizeof(int16_t) * (size_t)p->N * p->m);
  if (failing()) return done(0);
  *out = new_handle(KIND_IVF, p->N, p->d, p->m, p->K, p->C, p->ids, 0);
  T(" = #%d", (*out)->ordinal);
  return done(0);
}

int freddy_gpu_pin_ivpq(const freddy_ivpq_desc* p, int device, freddy_gpu_index_t** out) {
  const int32_t cells = p->coarse_codes * p->coarse_codes;
  T("  gpu pin_ivpq device=%d d=%d m=%d K=%d cq_m=%d cq_K=%d N=%lld", device, p->d, p->m, p->K, p->coarse_positions,
    p->coarse_codes, (long long)p->N);
  arr("codebook", p->codebook, sizeof(float) * (size_t)p->K * p->d);
  arr("coarse", p->coarse, sizeof(float) * (size_t)p->coarse_codes * p->d);
  arr("ids", p->ids, sizeof(int32_t) * (size_t)p->N);
  arr("coarse_id", p->coarse_id, sizeof(int32_t) * (size_t)p->N);
  arr("codes", p->codes, sizeof(int16_t) * (size_t)p->N * p->m);
  arr("vectors", p->vectors, sizeof(float) * (size_t)p->N * p->d);
  arr("stats", p->stats, sizeof(float) * ((size_t)cells + 1));
  if (failing()) return done(0);
  *out = new_handle(KIND_IVPQ, p->N, p->d, p->m, p->K, cells, p->ids, p->vectors != NULL);
  T(" = #%d", (*out)->ordinal);
  return done(0);
}

int freddy_gpu_pin_vectors(const freddy_vec_desc* p, int device, freddy_gpu_index_t** out) {
  T("  gpu pin_vectors device=%d d=%d N=%lld", device, p->d, (long long)p->N);
  arr("ids", p->ids, sizeof(int32_t) * (size_t)p->N);
  arr("vectors", p->vectors, sizeof(float) * (size_t)p->N * p->d);
  if (failing()) return done(0);
  *out = new_handle(KIND_VEC, p->N, p->d, 0, 0, 0, p->ids, 1);
  T(" = #%d", (*out)->ordinal);
  return done(0);
}

/* not counted by stub_fail_after: the host ignores its result */
int freddy_gpu_unpin(freddy_gpu_index_t* h) {
  for (int i = 0; i < g_n_live; ++i)
    if (g_live[i] == h) {
      T("  gpu unpin(#%d:%s) -> 0\n", h->ordinal, kKind[h->kind]);
      g_live[i] = g_live[--g_n_live];
      free(h->ids);
      free(h);
      return 0;
    }
  printf("  gpu unpin: DOUBLE UNPIN of a handle that is not live\n");
  return FREDDY_E_ARG;
}

int freddy_gpu_pq_search(freddy_gpu_index_t* pq, const float* queries, int32_t Q, int32_t k, float sentinel, const int32_t* subset_ids,
                         int64_t n_subset, int32_t* out_ids, float* out_dist) {
  T("  gpu pq_search");
  hnd("pq", pq);
  if (!usable(pq, KIND_PQ)) return refuse("handle");
  T(" Q=%d k=%d fill=%08x n_in=%lld", Q, k, fbits(sentinel), (long long)n_subset);
  arr("q", queries, sizeof(float) * (size_t)Q * pq->d);
  arr("in", subset_ids, sizeof(int32_t) * (size_t)n_subset);
  outp("out_ids", out_ids); outp("out_dist", out_dist);
  if (failing()) return done(0);
  for (int32_t q = 0; q < Q; ++q)
    fill_list(pq, fnv(queries + (size_t)q * pq->d, sizeof(float) * pq->d), k, sentinel, subset_ids, n_subset, NULL, NULL, 0,
              out_ids + (size_t)q * k, out_dist + (size_t)q * k);
  return done(0);
}

int freddy_gpu_ivfadc_search(freddy_gpu_index_t* ivf, const float* queries, int32_t Q, int32_t k, int32_t W, float sentinel, int32_t found_rule,
                             int32_t* out_ids, float* out_dist) {
  T("  gpu ivfadc_search");
  hnd("ivf", ivf);
  if (!usable(ivf, KIND_IVF)) return refuse("handle");
  T(" Q=%d k=%d W=%d fill=%08x found=%d", Q, k, W, fbits(sentinel), found_rule);
  arr("q", queries, sizeof(float) * (size_t)Q * ivf->d);
  outp("out_ids", out_ids); outp("out_dist", out_dist);
  if (failing()) return done(0);
  for (int32_t q = 0; q < Q; ++q)
    fill_list(ivf, fnv(queries + (size_t)q * ivf->d, sizeof(float) * ivf->d) + (uint64_t)W, k, sentinel, NULL, 0, NULL, NULL, 0,
              out_ids + (size_t)q * k, out_dist + (size_t)q * k);
  return done(0);
}

int freddy_gpu_knn_join(freddy_gpu_index_t* ivpq, const float* queries, int32_t Q, int32_t k, const int32_t* target_ids, int64_t n_targets,
                        int32_t alpha, int32_t pvf, int32_t method, int32_t use_target_lists, float confidence, int32_t double_threshold,
                        int32_t* out_ids, float* out_dist, int32_t* iterations_out) {
  T("  gpu knn_join");
  hnd("ivpq", ivpq);
  if (!usable(ivpq, KIND_IVPQ)) return refuse("handle");
  T(" Q=%d k=%d n_to=%lld alpha=%d pvf=%d method=%d lists=%d conf=%08x dbl=%d", Q, k, (long long)n_targets,
    alpha, pvf, method, use_target_lists, fbits(confidence), double_threshold);
  arr("q", queries, sizeof(float) * (size_t)Q * ivpq->d);
  arr("to", target_ids, sizeof(int32_t) * (size_t)n_targets);
  outp("out_ids", out_ids); outp("out_dist", out_dist); outp("iterations", iterations_out);
  if (failing()) return done(0);
  static const int32_t none = -1;
  for (int32_t q = 0; q < Q; ++q)
    fill_list(ivpq, fnv(queries + (size_t)q * ivpq->d, sizeof(float) * ivpq->d), k, 1000.0f, target_ids ? target_ids : &none,
              target_ids ? n_targets : 1, NULL, NULL, 0, out_ids + (size_t)q * k, out_dist + (size_t)q * k);
  if (iterations_out) *iterations_out = 1;
  return done(0);
}

int freddy_gpu_exact_search(freddy_gpu_index_t* vecs, const float* queries, int32_t Q, int32_t k, const int32_t* subset_ids, int64_t n_subset,
                            int32_t* out_ids, float* out_sim) {
  T("  gpu exact_search");
  hnd("vecs", vecs);
  if (!usable(vecs, KIND_VEC)) return refuse("handle");
  T(" Q=%d k=%d n_in=%lld", Q, k, (long long)n_subset);
  arr("q", queries, sizeof(float) * (size_t)Q * vecs->d);
  arr("in", subset_ids, sizeof(int32_t) * (size_t)n_subset);
  outp("out_ids", out_ids); outp("out_sim", out_sim);
  if (failing()) return done(0);
  for (int32_t q = 0; q < Q; ++q)
    fill_list(vecs, fnv(queries + (size_t)q * vecs->d, sizeof(float) * vecs->d), k, -__builtin_inff(), subset_ids, n_subset, NULL, NULL, 0,
              out_ids + (size_t)q * k, out_sim + (size_t)q * k);
  return done(0);
}

int freddy_gpu_exact_analogy(freddy_gpu_index_t* vecs, int32_t method, const int32_t* triples, int32_t Q, int32_t k, const int32_t* subset_ids,
                             int64_t n_subset, int32_t* out_ids, double* out_score) {
  T("  gpu exact_analogy");
  hnd("vecs", vecs);
  if (!usable(vecs, KIND_VEC)) return refuse("handle");
  T(" method=%d Q=%d k=%d n_in=%lld", method, Q, k, (long long)n_subset);
  arr("triples", triples, sizeof(int32_t) * 3 * (size_t)Q);
  arr("in", subset_ids, sizeof(int32_t) * (size_t)n_subset);
  outp("out_ids", out_ids); outp("out_score", out_score);
  if (failing()) return done(0);
  float* val = (float*)malloc(sizeof(float) * (size_t)(k > 0 ? k : 1));
  for (int32_t q = 0; q < Q; ++q) {
    const int32_t* t = triples + 3 * (size_t)q;
    const int known = has_id(vecs->ids, vecs->N, t[0]) && has_id(vecs->ids, vecs->N, t[1]) && has_id(vecs->ids, vecs->N, t[2]);
    /* an unknown word: the SQL's cross join is empty (an empty list: a subset nothing is in) */
    static const int32_t none = -1;
    fill_list(vecs, fnv(t, 12) + (uint64_t)method, k, 0.0f, known ? subset_ids : &none, known ? n_subset : 1, NULL, t, 0, out_ids + (size_t)q * k, val);
    for (int32_t r = 0; r < k; ++r) out_score[(size_t)q * k + r] = val[r];
  }
  free(val);
  return done(0);
}

int freddy_gpu_exact_join(freddy_gpu_index_t* vecs, const float* queries, int32_t Q, int32_t k, const int32_t* target_ids, int64_t n_targets,
                          int32_t* out_ids, float* out_sim) {
  T("  gpu exact_join");
  hnd("vecs", vecs);
  if (!usable(vecs, KIND_VEC)) return refuse("handle");
  T(" Q=%d k=%d n_to=%lld", Q, k, (long long)n_targets);
  arr("q", queries, sizeof(float) * (size_t)Q * vecs->d);
  arr("to", target_ids, sizeof(int32_t) * (size_t)n_targets);
  outp("out_ids", out_ids); outp("out_sim", out_sim);
  if (failing()) return done(0);
  static const int32_t none = -1;
  for (int32_t q = 0; q < Q; ++q)
    fill_list(vecs, fnv(queries + (size_t)q * vecs->d, sizeof(float) * vecs->d), k, -__builtin_inff(), n_targets ? target_ids : &none,
              n_targets ? n_targets : 1, NULL, NULL, 1, out_ids + (size_t)q * k, out_sim + (size_t)q * k);
  return done(0);
}

static void fill_assign(uint64_t seed, int32_t Q, int64_t n_targets, int32_t* out_query, float* out_sim) {
  for (int64_t i = 0; i < n_targets; ++i) {
    const uint64_t z = mix(seed, (uint64_t)i);
    out_query[i] = (int32_t)(z % (uint64_t)(Q + 1)) - 1;   /* -1: no query lists the target */
    out_sim[i] = out_query[i] < 0 ? -__builtin_inff() : (float)((z >> 20) % 4096) / 4096.0f;
  }
}

int freddy_gpu_exact_assign(freddy_gpu_index_t* vecs, const float* queries, int32_t Q, const int32_t* target_ids, int64_t n_targets,
                            int32_t* out_query, float* out_sim) {
  T("  gpu exact_assign");
  hnd("vecs", vecs);
  if (!usable(vecs, KIND_VEC)) return refuse("handle");
  T(" Q=%d n_to=%lld", Q, (long long)n_targets);
  const uint64_t hq = arr("q", queries, sizeof(float) * (size_t)Q * vecs->d);
  const uint64_t ht = arr("to", target_ids, sizeof(int32_t) * (size_t)n_targets);
  outp("out_query", out_query); outp("out_sim", out_sim);
  if (failing()) return done(0);
  fill_assign(hq ^ ht, Q, n_targets, out_query, out_sim);
  return done(0);
}

int freddy_gpu_pq_assign(freddy_gpu_index_t* pq, const float* queries, int32_t Q, float sentinel, const int32_t* target_ids, int64_t n_targets,
                         int32_t* out_query, float* out_sim) {
  T("  gpu pq_assign");
  hnd("pq", pq);
  if (!usable(pq, KIND_PQ)) return refuse("handle");
  T(" Q=%d fill=%08x n_to=%lld", Q, fbits(sentinel), (long long)n_targets);
  const uint64_t hq = arr("q", queries, sizeof(float) * (size_t)Q * pq->d);
  const uint64_t ht = arr("to", target_ids, sizeof(int32_t) * (size_t)n_targets);
  outp("out_query", out_query); outp("out_sim", out_sim);
  if (failing()) return done(0);
  fill_assign(hq ^ ht ^ 1, Q, n_targets, out_query, out_sim);
  return done(0);
}

int freddy_gpu_ivfadc_search_pv(freddy_gpu_index_t* ivf, freddy_gpu_index_t* vecs, const float* queries, int32_t Q, int32_t k, int32_t pvf, int32_t W,
                                float sentinel, int32_t found_rule, int32_t* out_ids, float* out_sim) {
  T("  gpu ivfadc_search_pv");
  hnd("ivf", ivf); hnd("vecs", vecs);
  if (!usable(ivf, KIND_IVF) || !usable(vecs, KIND_VEC)) return refuse("handle");
  T(" Q=%d k=%d pvf=%d W=%d fill=%08x found=%d", Q, k, pvf, W, fbits(sentinel), found_rule);
  arr("q", queries, sizeof(float) * (size_t)Q * ivf->d);
  outp("out_ids", out_ids); outp("out_sim", out_sim);
  if (failing()) return done(0);
  for (int32_t q = 0; q < Q; ++q)
    fill_list(ivf, fnv(queries + (size_t)q * ivf->d, sizeof(float) * ivf->d) + (uint64_t)W, k, -__builtin_inff(), NULL, 0, vecs, NULL, 1,
              out_ids + (size_t)q * k, out_sim + (size_t)q * k);
  return done(0);
}

int freddy_gpu_pq_search_pv(freddy_gpu_index_t* pq, freddy_gpu_index_t* vecs, const float* queries, int32_t Q, int32_t k, int32_t pvf, float sentinel,
                            const int32_t* subset_ids, int64_t n_subset, int32_t* out_ids, float* out_sim) {
  T("  gpu pq_search_pv");
  hnd("pq", pq); hnd("vecs", vecs);
  if (!usable(pq, KIND_PQ) || !usable(vecs, KIND_VEC)) return refuse("handle");
  T(" Q=%d k=%d pvf=%d fill=%08x n_in=%lld", Q, k, pvf, fbits(sentinel), (long long)n_subset);
  arr("q", queries, sizeof(float) * (size_t)Q * pq->d);
  arr("in", subset_ids, sizeof(int32_t) * (size_t)n_subset);
  outp("out_ids", out_ids); outp("out_sim", out_sim);
  if (failing()) return done(0);
  for (int32_t q = 0; q < Q; ++q)
    fill_list(pq, fnv(queries + (size_t)q * pq->d, sizeof(float) * pq->d), k, -__builtin_inff(), subset_ids, n_subset, vecs, NULL, 1,
              out_ids + (size_t)q * k, out_sim + (size_t)q * k);
  return done(0);
}

/* out_ids[q] lists for triples: nothing (-1) when a word of the triple has no vector row */
static void fill_analogy(const freddy_gpu_index_t* ann, const freddy_gpu_index_t* vecs, const int32_t* triples, int32_t Q, int32_t k,
                         const int32_t* subset_ids, int64_t n_subset, int32_t* out_ids, float* out_sim) {
  static const int32_t none = -1;
  for (int32_t q = 0; q < Q; ++q) {
    const int32_t* t = triples + 3 * (size_t)q;
    const int known = has_id(vecs->ids, vecs->N, t[0]) && has_id(vecs->ids, vecs->N, t[1]) && has_id(vecs->ids, vecs->N, t[2]);
    fill_list(ann, fnv(t, 12), k, -__builtin_inff(), known ? subset_ids : &none, known ? n_subset : 1, vecs, t, 0, out_ids + (size_t)q * k,
              out_sim + (size_t)q * k);
  }
}

int freddy_gpu_ivfadc_analogy(freddy_gpu_index_t* ivf, freddy_gpu_index_t* vecs, const int32_t* triples, int32_t Q, int32_t k, int32_t n_cand, int32_t W,
                              float sentinel, int32_t found_rule, int32_t* out_ids, float* out_sim) {
  T("  gpu ivfadc_analogy");
  hnd("ivf", ivf); hnd("vecs", vecs);
  if (!usable(ivf, KIND_IVF) || !usable(vecs, KIND_VEC)) return refuse("handle");
  T(" Q=%d k=%d n_cand=%d W=%d fill=%08x found=%d", Q, k, n_cand, W, fbits(sentinel), found_rule);
  arr("triples", triples, sizeof(int32_t) * 3 * (size_t)Q);
  outp("out_ids", out_ids); outp("out_sim", out_sim);
  if (failing()) return done(0);
  fill_analogy(ivf, vecs, triples, Q, k, NULL, 0, out_ids, out_sim);
  return done(0);
}

int freddy_gpu_pq_analogy(freddy_gpu_index_t* pq, freddy_gpu_index_t* vecs, const int32_t* triples, int32_t Q, int32_t k, int32_t n_cand, float sentinel,
                          const int32_t* subset_ids, int64_t n_subset, int32_t* out_ids, float* out_sim) {
  T("  gpu pq_analogy");
  hnd("pq", pq); hnd("vecs", vecs);
  if (!usable(pq, KIND_PQ) || !usable(vecs, KIND_VEC)) return refuse("handle");
  T(" Q=%d k=%d n_cand=%d fill=%08x n_in=%lld", Q, k, n_cand, fbits(sentinel), (long long)n_subset);
  arr("triples", triples, sizeof(int32_t) * 3 * (size_t)Q);
  arr("in", subset_ids, sizeof(int32_t) * (size_t)n_subset);
  outp("out_ids", out_ids); outp("out_sim", out_sim);
  if (failing()) return done(0);
  fill_analogy(pq, vecs, triples, Q, k, subset_ids, n_subset, out_ids, out_sim);
  return done(0);
}

int freddy_gpu_grouping_pq(freddy_gpu_index_t* pq, const float* group_vectors, int32_t G, const int32_t* subset_ids, int64_t n_subset, int32_t* out_ids,
                           int32_t* out_group, int64_t* n_out) {
  T("  gpu grouping_pq");
  hnd("pq", pq);
  if (!usable(pq, KIND_PQ)) return refuse("handle");
  T(" G=%d n_in=%lld", G, (long long)n_subset);
  const uint64_t hg = arr("groups", group_vectors, sizeof(float) * (size_t)G * pq->d);
  arr("in", subset_ids, sizeof(int32_t) * (size_t)n_subset);
  outp("out_ids", out_ids); outp("out_group", out_group); outp("n_out", n_out);
  if (failing()) return done(0);
  int64_t n = 0;   /* the rows of the table with id IN subset, table order; group -1: none is nearer than the sentinel */
  for (int64_t i = 0; i < pq->N; ++i)
    if (!subset_ids || has_id(subset_ids, n_subset, pq->ids[i])) {
      out_ids[n] = pq->ids[i];
      out_group[n] = (int32_t)(mix(hg, (uint64_t)pq->ids[i]) % (uint64_t)(G + 1)) - 1;
      ++n;
    }
  *n_out = n;
  return done(0);
}

int freddy_gpu_insert_quantize(const freddy_insert_desc* p, int device, const float* vectors, int64_t n, int16_t* pq_codes, int32_t* coarse_id,
                               int16_t* residual_codes, int16_t* ivpq_codes, int16_t* coarse_multi_codes) {
  T("  gpu insert_quantize device=%d d=%d n=%lld pq_m=%d pq_K=%d res_m=%d res_K=%d C=%d ivpq_m=%d ivpq_K=%d cq_m=%d cq_K=%d", device, p->d,
    (long long)n, p->pq_m, p->pq_K, p->res_m, p->res_K, p->C, p->ivpq_m, p->ivpq_K, p->multi_positions, p->multi_codes);
  arr("pq_cb", p->pq_codebook, sizeof(float) * (size_t)p->pq_K * p->d);
  arr("res_cb", p->residual_codebook, sizeof(float) * (size_t)p->res_K * p->d);
  arr("coarse", p->coarse, sizeof(float) * (size_t)p->C * p->d);
  arr("ivpq_cb", p->ivpq_codebook, sizeof(float) * (size_t)p->ivpq_K * p->d);
  arr("cq", p->coarse_multi, sizeof(float) * (size_t)p->multi_codes * p->d);
  arr("vectors", vectors, sizeof(float) * (size_t)n * p->d);
  outp("pq_codes", pq_codes); outp("coarse_id", coarse_id); outp("residual_codes", residual_codes); outp("ivpq_codes", ivpq_codes);
  outp("coarse_multi_codes", coarse_multi_codes);
  if (failing()) return done(0);
  for (int64_t i = 0; i < n; ++i) {
    const uint64_t h = fnv(vectors + (size_t)i * p->d, sizeof(float) * p->d);
    if (pq_codes) for (int j = 0; j < p->pq_m; ++j) pq_codes[i * p->pq_m + j] = (int16_t)(mix(h, 100 + j) % (uint64_t)p->pq_K);
    if (coarse_id) coarse_id[i] = (int32_t)(mix(h, 200) % (uint64_t)p->C);
    if (residual_codes) for (int j = 0; j < p->res_m; ++j) residual_codes[i * p->res_m + j] = (int16_t)(mix(h, 300 + j) % (uint64_t)p->res_K);
    if (ivpq_codes) for (int j = 0; j < p->ivpq_m; ++j) ivpq_codes[i * p->ivpq_m + j] = (int16_t)(mix(h, 400 + j) % (uint64_t)p->ivpq_K);
    if (coarse_multi_codes)
      for (int j = 0; j < p->multi_positions; ++j) coarse_multi_codes[i * p->multi_positions + j] = (int16_t)(mix(h, 500 + j) % (uint64_t)p->multi_codes);
  }
  return done(0);
}

int freddy_gpu_append_rows(freddy_gpu_index_t* h, int64_t n, const int32_t* ids, const int32_t* coarse_id, const int16_t* codes, const float* vectors) {
  T("  gpu append_rows");
  hnd("index", h);
  if (!h || !is_live(h)) return refuse("handle");
  T(" n=%lld", (long long)n);
  arr("ids", ids, sizeof(int32_t) * (size_t)n);
  arr("coarse_id", coarse_id, sizeof(int32_t) * (size_t)n);
  arr("codes", codes, sizeof(int16_t) * (size_t)n * h->m);
  arr("vectors", vectors, sizeof(float) * (size_t)n * h->d);
  if (failing()) return done(0);
  h->ids = (int32_t*)realloc(h->ids, sizeof(int32_t) * (size_t)(h->N + n ? h->N + n : 1));
  memcpy(h->ids + h->N, ids, sizeof(int32_t) * (size_t)n);
  h->N += n;
  return done(0);
}

int freddy_gpu_remove_rows(freddy_gpu_index_t* h, int64_t n, const int32_t* ids, int64_t* removed) {
  T("  gpu remove_rows");
  hnd("index", h);
  if (!h || !is_live(h)) return refuse("handle");
  T(" n=%lld", (long long)n);
  arr("ids", ids, sizeof(int32_t) * (size_t)n);
  outp("removed", removed);
  if (failing()) return done(0);
  int64_t w = 0;
  for (int64_t r = 0; r < h->N; ++r)
    if (!has_id(ids, n, h->ids[r])) h->ids[w++] = h->ids[r];
  if (removed) *removed = h->N - w;
  T(" removed=%lld", (long long)(h->N - w));
  h->N = w;
  return done(0);
}

int freddy_gpu_update_rows(freddy_gpu_index_t* h, int64_t n, const int32_t* ids, const int32_t* coarse_id, const int16_t* codes, const float* vectors,
                           int64_t* updated) {
  T("  gpu update_rows");
  hnd("index", h);
  if (!h || !is_live(h)) return refuse("handle");
  T(" n=%lld", (long long)n);
  arr("ids", ids, sizeof(int32_t) * (size_t)n);
  arr("coarse_id", coarse_id, sizeof(int32_t) * (size_t)n);
  arr("codes", codes, sizeof(int16_t) * (size_t)n * h->m);
  arr("vectors", vectors, sizeof(float) * (size_t)n * h->d);
  outp("updated", updated);
  if (failing()) return done(0);
  int64_t hit = 0;
  for (int64_t i = 0; i < n; ++i) hit += has_id(h->ids, h->N, ids[i]);
  if (updated) *updated = hit;
  T(" updated=%lld", (long long)hit);
  return done(0);
}

int freddy_gpu_update_codebook(freddy_gpu_index_t* h, const float* codebook) {
  T("  gpu update_codebook");
  hnd("index", h);
  if (!h || !is_live(h)) return refuse("handle");
  arr("codebook", codebook, sizeof(float) * (size_t)h->K * h->d);
  return done(0);
}

int freddy_gpu_set_statistics(freddy_gpu_index_t* ivpq, const float* stats, int32_t n_stats) {
  T("  gpu set_statistics");
  hnd("ivpq", ivpq);
  if (!usable(ivpq, KIND_IVPQ)) return refuse("handle");
  T(" n_stats=%d", n_stats);
  arr("stats", stats, sizeof(float) * (size_t)n_stats);
  return done(0);
}

int freddy_gpu_create_statistics(freddy_gpu_index_t* ivpq, const int32_t* ids, int64_t n, int32_t install, float* out_stats, int64_t* matched) {
  T("  gpu create_statistics");
  hnd("ivpq", ivpq);
  if (!usable(ivpq, KIND_IVPQ)) return refuse("handle");
  T(" n=%lld install=%d", (long long)n, install);
  const uint64_t h = arr("ids", ids, sizeof(int32_t) * (size_t)n);
  outp("out_stats", out_stats); outp("matched", matched);
  if (failing()) return done(0);
  if (out_stats) for (int32_t c = 0; c <= ivpq->C; ++c) out_stats[c] = (float)(mix(h, (uint64_t)c) % 1024) / 1024.0f;
  if (matched) *matched = ids ? n : ivpq->N;
  return done(0);
}
