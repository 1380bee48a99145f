// trace_main.cpp -- drives every function of include/freddy_udf.h against the recording device stub (stub_gpu.c) and prints, after
// each call, its return code, the error text on failure and its outputs (floats as their 32 bits in hex).  Together with the
// stub's own lines this is the trace tests/golden/host_trace.txt holds: everything the host mirror does, without a GPU.
//   trace_main            the trace, on stdout (index files are written to the current directory and removed again)
//   trace_main --time N   no trace: N calls each of three entry points against the silent stub, ns per call
#include "../../include/freddy_udf.h"

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

extern "C" void stub_fail_after(long n);   // the n-th device call from now fails (0: none)
extern "C" void stub_quiet(int on);        // no trace lines from the stub (timing mode only)

namespace {

uint32_t g_lcg = 12345u;
uint32_t lcg() { g_lcg = g_lcg * 1664525u + 1013904223u; return g_lcg >> 8; }
float lcg_float() { return (float)((int)(lcg() % 2001u) - 1000) / 1000.0f; }

uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

// N = 48, d = 8, m = 4, K = 4, C = 3, multi-index 2 x 2: the smallest shapes that still reach every branch
struct Tables {
  int N = 48, d = 8, m = 4, K = 4, C = 3;
  std::vector<int32_t> norm_ids, pq_ids, fine_ids, fine_cell, ivpq_ids, ivpq_cell;
  std::vector<float> norm, orig;
  std::vector<int32_t> cb_pos, cb_code;
  std::vector<float> pq_cb, res_cb, ivpq_cb;
  std::vector<int16_t> pq_codes, fine_codes, ivpq_codes;
  std::vector<int32_t> coarse_ids;
  std::vector<float> coarse;
  std::vector<int32_t> cq_pos, cq_code;
  std::vector<float> cq_vec;
  std::vector<int32_t> stat_id;
  std::vector<float> stat_freq;
  std::vector<int32_t> counts;

  Tables() {
    // ids 1, 3, .., 95, handed over in descending order (the loaders sort); rows 39, 41 and 43 hold the same vector
    for (int i = N - 1; i >= 0; --i) norm_ids.push_back(1 + 2 * i);
    norm.resize((size_t)N * d); orig.resize((size_t)N * d);
    for (int i = 0; i < N; ++i) {
      float sq = 0;
      for (int j = 0; j < d; ++j) { orig[(size_t)i * d + j] = 3.0f * lcg_float(); sq += orig[(size_t)i * d + j] * orig[(size_t)i * d + j]; }
      const float len = sqrtf(sq);
      for (int j = 0; j < d; ++j) norm[(size_t)i * d + j] = orig[(size_t)i * d + j] / len;
    }
    for (int32_t dup : {41, 43}) {
      memcpy(row(norm, dup), row(norm, 39), sizeof(float) * d);
      memcpy(row(orig, dup), row(orig, 39), sizeof(float) * d);
    }
    for (int p = 0; p < m; ++p) for (int c = 0; c < K; ++c) { cb_pos.push_back(p); cb_code.push_back(c); }
    for (std::vector<float>* cb : {&pq_cb, &res_cb, &ivpq_cb}) for (int i = 0; i < m * K * (d / m); ++i) cb->push_back(lcg_float());
    pq_ids = norm_ids; pq_ids.push_back(200);   // one id google_vecs_norm does not have
    fine_ids = norm_ids; ivpq_ids = norm_ids;
    for (size_t i = 0; i < pq_ids.size() * m; ++i) pq_codes.push_back((int16_t)(lcg() % K));
    for (int i = 0; i < N * m; ++i) { fine_codes.push_back((int16_t)(lcg() % K)); ivpq_codes.push_back((int16_t)(lcg() % K)); }
    for (int i = 0; i < N; ++i) { fine_cell.push_back((int32_t)(lcg() % C)); ivpq_cell.push_back((int32_t)(lcg() % 4)); }
    coarse_ids = {2, 0, 1};
    for (int i = 0; i < C * d; ++i) coarse.push_back(lcg_float());
    cq_pos = {0, 0, 1, 1}; cq_code = {0, 1, 0, 1};
    for (int i = 0; i < 4 * (d / 2); ++i) cq_vec.push_back(lcg_float());
    stat_id = {4, 0, 1, 2, 3};
    stat_freq = {1.0f, 0.25f, 0.25f, 0.125f, 0.375f};
    for (int i = 0; i < m * K; ++i) counts.push_back(2 + (int32_t)(lcg() % 50));
  }
  float* row(std::vector<float>& t, int32_t id) {
    for (int i = 0; i < N; ++i) if (norm_ids[i] == id) return &t[(size_t)i * d];
    return nullptr;
  }
};
Tables T;

int g_rc = 0;
// one line per call, after the stub's lines for it: the call, its return code, the error text, then what `show` adds
void report(const char* call, int rc) {
  g_rc = rc;
  std::string text(call);   // the call as written, without what every call repeats
  for (const char* noise : {".data()", "T.", ", out2, &n_rows", ", out3, &n_rows", ", outg, &n_rows", ", &result"})
    for (size_t at; (at = text.find(noise)) != std::string::npos;) text.erase(at, strlen(noise));
  if (rc) printf("> %s = %d [%s]", text.c_str(), rc, freddy_udf_last_error());
  else printf("> %s = 0", text.c_str());
}
#define CALL_(expr, show) do { report(#expr, expr); show; printf("\n"); } while (0)
#define CALL(expr) CALL_(expr, (void)0)
// the call with the n-th device call from now failing
#define FAIL(n, expr) do { stub_fail_after(n); CALL(expr); stub_fail_after(0); } while (0)

freddy_row2 out2[8192];
freddy_row3 out3[8192];
freddy_group_row outg[512];
int32_t n_rows = -7;

// a list of result rows: up to three in full; a longer one as its first two and a 64-bit FNV-1a hash of all rows' bytes
template <class Row, class Print>
void show_rows(const Row* rows, Print print) {
  if (g_rc) return;
  printf(" : %d rows", n_rows);
  for (int i = 0; i < n_rows && i < (n_rows > 3 ? 2 : 3); ++i) print(rows[i]);
  if (n_rows > 3) {
    uint64_t h = 0xcbf29ce484222325ull;
    const unsigned char* b = reinterpret_cast<const unsigned char*>(rows);
    for (size_t i = 0; i < sizeof(Row) * (size_t)n_rows; ++i) { h ^= b[i]; h *= 0x100000001b3ull; }
    printf(" ... all: %016llx", (unsigned long long)h);
  }
}
void show2() { show_rows(out2, [](const freddy_row2& r) { printf(" (%d,%08x)", r.id, bits(r.distance)); }); }
void show3() { show_rows(out3, [](const freddy_row3& r) { printf(" (%d,%d,%08x)", r.query_id, r.id, bits(r.distance)); }); }
void showg() { show_rows(outg, [](const freddy_group_row& r) { printf(" (%d,%d)", r.id, r.group_id); }); }
void showi(const char* what, const int32_t* v, int n) {
  if (g_rc) return;
  printf(" : %s", what);
  for (int i = 0; i < n; ++i) printf(" %d", v[i]);
}
#define R2(expr) do { n_rows = -7; CALL_(expr, show2()); } while (0)
#define R3(expr) do { n_rows = -7; CALL_(expr, show3()); } while (0)
#define RG(expr) do { n_rows = -7; CALL_(expr, showg()); } while (0)
#define R1(expr) do { result = -7; CALL_(expr, showi("result", &result, 1)); } while (0)

void handles(freddy_session_t* s) {
  printf("    handles:");
  for (const char* t : {"pq", "ivfadc", "ivpq", "vecs"}) printf(" %s=%s", t, freddy_session_gpu_index(s, t) ? "set" : "NULL");
  printf("\n");
}

int load_norm(freddy_session_t* s) { return freddy_load_vecs_norm(s, T.norm_ids.data(), T.norm.data(), T.N, T.d); }
int load_orig(freddy_session_t* s) { return freddy_load_vecs_original(s, T.norm_ids.data(), T.orig.data(), T.N, T.d); }
int load_pq(freddy_session_t* s) {
  return freddy_load_pq(s, T.cb_pos.data(), T.cb_code.data(), T.pq_cb.data(), T.m * T.K, T.d / T.m, T.pq_ids.data(), T.pq_codes.data(), (int64_t)T.pq_ids.size());
}
int load_ivfadc(freddy_session_t* s) {
  return freddy_load_ivfadc(s, T.coarse_ids.data(), T.coarse.data(), T.C, T.cb_pos.data(), T.cb_code.data(), T.res_cb.data(), T.m * T.K, T.d / T.m,
                            T.fine_ids.data(), T.fine_cell.data(), T.fine_codes.data(), T.N);
}
int load_ivpq(freddy_session_t* s) {
  return freddy_load_ivpq(s, T.cb_pos.data(), T.cb_code.data(), T.ivpq_cb.data(), T.m * T.K, T.d / T.m, T.cq_pos.data(), T.cq_code.data(), T.cq_vec.data(), 4,
                          T.ivpq_ids.data(), T.ivpq_cell.data(), T.ivpq_codes.data(), T.N, T.stat_id.data(), T.stat_freq.data(), 5);
}
freddy_session_t* full_session(const char* label) {
  printf("---- session %s: every table\n", label);
  freddy_session_t* s = nullptr;
  CALL(freddy_session_open(0, &s));
  CALL(load_norm(s)); CALL(load_orig(s)); CALL(load_pq(s)); CALL(load_ivfadc(s)); CALL(load_ivpq(s));
  return s;
}

const int32_t kIn[] = {3, 9, 200, 41, 39, 43, 77, 500};              // an IN-list: known ids, the pq-only id, an unknown one
const int32_t kQids[] = {7, 3, 7, 1000, 95, 41};                      // query ids: a duplicate and an unknown one
const int32_t kTokens[] = {1, 5, 9, 13, 17, 21, 25, 29, 33, 37, 39, 41};
const int32_t kGroups[] = {11, 3, 59};
const int32_t kTriples[] = {1, 3, 5, 5, 5, 39, 7, 1000, 9};           // the third names an unknown word
double g_draws[40];

// every search entry point once, with arguments that are themselves valid; `dim` is what the caller claims for q
// (`lean`: without the calls that never look at google_vecs_norm -- sessions that differ from A only in that table)
// (cluster_pq / cluster_ivpq do not compare the dimension of google_vecs_norm with their code table's: with tables of different
// dimensions they hand the device centroids of the wrong width, so session D, which has such tables, leaves the two out)
void every_search(freddy_session_t* s, int32_t dim, bool same_dims = true, bool lean = false) {
  const float* q = T.row(T.norm, 9);
  const float* q2 = T.row(T.norm, 11);   // two queries: the rows 11 and 9 (the table is handed over in descending id order)
  const int32_t two[] = {70, 80};
  int32_t result = 0;
  if (!lean) R2(pq_search(s, q, dim, 5, out2, &n_rows));
  if (!lean) R2(pq_search_in(s, q, dim, 5, kIn, 8, out2, &n_rows));
  if (!lean) R2(ivfadc_search(s, q, dim, 5, out2, &n_rows));
  if (!lean) R3(pq_search_in_batch(s, q2, 2, dim, two, 2, 5, kIn, 8, 1, out3, &n_rows));
  R3(ivfadc_batch_search(s, kQids, 6, 5, out3, &n_rows));
  if (!lean) R3(ivpq_search_in(s, q2, 2, dim, two, 2, 5, kIn, 8, 2, 7, 1, 0, 0.5f, 1000, out3, &n_rows));
  if (!lean) R3(knn_join(s, q2, 2, dim, two, 5, kIn, 8, out3, &n_rows));
  R2(k_nearest_neighbour(s, q, dim, 5, out2, &n_rows));
  R2(knn_in_exact(s, q, dim, 5, kIn, 8, out2, &n_rows));
  RG(grouping_pq(s, kIn, 8, kGroups, 3, outg, &n_rows));
  R1(analogy_3cosadd_pq(s, 1, 3, 5, &result));
  R1(analogy_3cosadd_ivfadc(s, 1, 3, 5, &result));
  if (!lean) R2(k_nearest_neighbour_pq(s, q, dim, 5, out2, &n_rows));
  if (!lean) R2(k_nearest_neighbour_ivfadc(s, q, dim, 5, out2, &n_rows));
  R2(k_nearest_neighbour_pq_pv(s, q, dim, 5, out2, &n_rows));
  R2(k_nearest_neighbour_ivfadc_pv(s, q, dim, 5, out2, &n_rows));
  if (!lean) R2(knn_in_pq(s, q, dim, 5, kIn, 8, out2, &n_rows));
  R3(k_nearest_neighbour_ivfadc_batch(s, kQids, 6, 5, out3, &n_rows));
  R3(k_nearest_neighbour_ivfadc_pv_batch(s, kQids, 6, 5, out3, &n_rows));
  R3(k_nearest_neighbour_pq_pv_batch(s, kQids, 6, 5, out3, &n_rows));
  R3(knn_batch(s, kQids, 6, 5, out3, &n_rows));
  R1(analogy_3cosadd_in_pq(s, 1, 3, 5, kIn, 8, &result));
  R1(analogy_3cosadd_in_ivpq(s, 1, 3, 5, kIn, 8, &result));
  int32_t res3[3] = {-7, -7, -7};
  CALL_(analogy_3cosadd_pq_batch(s, kTriples, 3, res3), showi("results", res3, 3));
  CALL_(analogy_3cosadd_ivfadc_batch(s, kTriples, 3, res3), showi("results", res3, 3));
  CALL_(analogy_3cosadd_in_pq_batch(s, kTriples, 3, kIn, 8, res3), showi("results", res3, 3));
  int32_t cl[12];
  CALL_(cluster_exact(s, kTokens, 12, 3, g_draws, 40, cl), showi("clusters", cl, 12));
  if (same_dims) {
    CALL_(cluster_pq(s, kTokens, 12, 3, g_draws, 40, cl), showi("clusters", cl, 12));
    CALL_(cluster_ivpq(s, kTokens, 12, 3, g_draws, 40, cl), showi("clusters", cl, 12));
  }
  int32_t aq[12]; float as[12];
  CALL_(exact_assign(s, q2, 2, dim, kTokens, 12, aq, as), showi("out_query", aq, 12));
  if (!g_rc) { printf("    out_sim:"); for (float v : as) printf(" %08x", bits(v)); printf("\n"); }
  CALL_(pq_assign(s, q2, 2, dim, kTokens, 12, aq, as), showi("out_query", aq, 12));
  if (!g_rc) { printf("    out_sim:"); for (float v : as) printf(" %08x", bits(v)); printf("\n"); }
  R1(analogy_pair_direction(s, 1, 3, 5, &result));
  R1(analogy_3cosadd(s, 1, 3, 5, &result));
  R1(analogy_3cosmul(s, 1, 3, 5, &result));
  R1(analogy_3cosadd_in(s, 1, 3, 5, kIn, 8, &result));
  R1(analogy(s, 1, 3, 5, &result));
  R1(analogy_in(s, 1, 3, 5, kIn, 8, &result));
  R3(knn_search_in_batch(s, q2, 2, dim, 5, kIn, 8, out3, &n_rows));
  R3(knn_search_in_batch_ids(s, kQids, 6, 5, kIn, 8, out3, &n_rows));
  RG(grouping_func(s, kTokens, 12, kGroups, 3, outg, &n_rows));
  RG(groups(s, kTokens, 12, kGroups, 3, outg, &n_rows));
  float stats[5];
  CALL(freddy_set_statistics_table(s, T.stat_id.data(), T.stat_freq.data(), 5));
  CALL(create_statistics(s, kTokens, 12, stats));
  if (!g_rc) { printf("    stats:"); for (float v : stats) printf(" %08x", bits(v)); printf("\n"); }
  printf("    freddy_statistics_rows = %d\n", freddy_statistics_rows(s));
}

// the three mutations once: one new row, two rows updated, two rows deleted
void every_mutation(freddy_session_t* s, int32_t dim) {
  int32_t new_ids[2] = {-7, -7};
  int64_t cnt = -7;
  const int32_t upd[] = {9, 1000};
  const int32_t del[] = {9, 13, 9, 1000};
  CALL_(insert_batch(s, T.row(T.norm, 21), 1, dim, new_ids), showi("new_ids", new_ids, 1));
  CALL(update_rows(s, upd, T.row(T.norm, 31), 2, dim, &cnt)); if (!g_rc) printf("    updated = %lld\n", (long long)cnt);
  cnt = -7;
  CALL(delete_rows(s, del, 4, &cnt)); if (!g_rc) printf("    removed = %lld\n", (long long)cnt);
}

void after_failure(freddy_session_t* s) {
  int32_t result = 0;
  handles(s);
  R2(pq_search(s, T.row(T.norm, 9), T.d, 1, out2, &n_rows));
  R2(k_nearest_neighbour(s, T.row(T.norm, 9), T.d, 1, out2, &n_rows));
  R1(analogy_pair_direction(s, 1, 3, 5, &result));
}

// ---- index files ---------------------------------------------------------------------------------------------------
const char* kFile = "host_trace_tmp.idx";
std::vector<freddy_file_array> file_arrays(bool counts) {
  std::vector<freddy_file_array> a;
  auto add = [&](const char* name, int dtype, int ndim, int64_t d0, int64_t d1, const void* data) { a.push_back({name, dtype, ndim, {d0, d1}, data}); };
  const int E = T.m * T.K, sub = T.d / T.m;
  add("google_vecs_norm.id", 1, 1, T.N, 0, T.norm_ids.data());
  add("google_vecs_norm.vector", 0, 2, T.N, T.d, T.norm.data());
  add("pq_codebook.pos", 1, 1, E, 0, T.cb_pos.data());
  add("pq_codebook.code", 1, 1, E, 0, T.cb_code.data());
  add("pq_codebook.vector", 0, 2, E, sub, T.pq_cb.data());
  add("pq_quantization.id", 1, 1, (int64_t)T.pq_ids.size(), 0, T.pq_ids.data());
  add("pq_quantization.vector", 2, 2, (int64_t)T.pq_ids.size(), T.m, T.pq_codes.data());
  add("coarse_quantization.id", 1, 1, T.C, 0, T.coarse_ids.data());
  add("coarse_quantization.vector", 0, 2, T.C, T.d, T.coarse.data());
  add("residual_codebook.pos", 1, 1, E, 0, T.cb_pos.data());
  add("residual_codebook.code", 1, 1, E, 0, T.cb_code.data());
  add("residual_codebook.vector", 0, 2, E, sub, T.res_cb.data());
  add("fine_quantization.id", 1, 1, T.N, 0, T.fine_ids.data());
  add("fine_quantization.coarse_id", 1, 1, T.N, 0, T.fine_cell.data());
  add("fine_quantization.vector", 2, 2, T.N, T.m, T.fine_codes.data());
  add("codebook_ivpq.pos", 1, 1, E, 0, T.cb_pos.data());
  add("codebook_ivpq.code", 1, 1, E, 0, T.cb_code.data());
  add("codebook_ivpq.vector", 0, 2, E, sub, T.ivpq_cb.data());
  add("coarse_quantization_ivpq.pos", 1, 1, 4, 0, T.cq_pos.data());
  add("coarse_quantization_ivpq.code", 1, 1, 4, 0, T.cq_code.data());
  add("coarse_quantization_ivpq.vector", 0, 2, 4, T.d / 2, T.cq_vec.data());
  add("fine_quantization_ivpq.id", 1, 1, T.N, 0, T.ivpq_ids.data());
  add("fine_quantization_ivpq.coarse_id", 1, 1, T.N, 0, T.ivpq_cell.data());
  add("fine_quantization_ivpq.vector", 2, 2, T.N, T.m, T.ivpq_codes.data());
  add("stat.coarse_id", 1, 1, 5, 0, T.stat_id.data());
  add("stat.coarse_freq", 0, 1, 5, 0, T.stat_freq.data());
  if (counts) {
    add("pq_codebook.count", 1, 1, E, 0, T.counts.data());
    add("residual_codebook.count", 1, 1, E, 0, T.counts.data());
    add("codebook_ivpq.count", 1, 1, E, 0, T.counts.data());
  }
  return a;
}
freddy_file_array* named(std::vector<freddy_file_array>& a, const char* name) {
  for (freddy_file_array& f : a) if (!strcmp(f.name, name)) return &f;
  return nullptr;
}
void raw_file(const std::string& bytes) {
  FILE* f = fopen(kFile, "wb");
  fwrite(bytes.data(), 1, bytes.size(), f);
  fclose(f);
}
// write `a`, import it into a fresh session, insert one row (its codebook update shows the count columns in force)
void import_and_insert(const char* label, std::vector<freddy_file_array>& a, bool insert) {
  printf("---- index file: %s\n", label);
  freddy_session_t* s = nullptr;
  CALL(freddy_index_file_write(kFile, a.data(), (int32_t)a.size()));
  CALL(freddy_session_open(0, &s));
  CALL(freddy_import_index(s, kFile));
  handles(s);
  if (insert && !g_rc) { int32_t id = -7; CALL_(insert_batch(s, T.row(T.norm, 21), 1, T.d, &id), showi("new_ids", &id, 1)); }
  CALL(freddy_session_close(s));
}

void index_files() {
  std::vector<freddy_file_array> a = file_arrays(true);
  import_and_insert("every table, with the .count arrays", a, true);
  a = file_arrays(false);
  import_and_insert("every table, without the .count arrays", a, true);
  a = file_arrays(true);
  named(a, "pq_codebook.count")->dims[0] = 3;   // a count column of another length is passed over
  import_and_insert("a .count array of the wrong length", a, true);
  a = file_arrays(false);
  a.resize(7);
  import_and_insert("google_vecs_norm and the pq tables only", a, false);
  for (const char* shorter : {"google_vecs_norm.vector", "pq_quantization.vector", "fine_quantization.coarse_id", "stat.coarse_freq"}) {
    a = file_arrays(false);
    named(a, shorter)->dims[0] -= 1;
    import_and_insert(shorter, a, false);
  }
  std::vector<int32_t> neg = T.cb_pos; neg[3] = -1;   // a loader that refuses its tables ends the import
  for (const char* cb : {"pq_codebook.pos", "residual_codebook.pos", "codebook_ivpq.pos"}) {
    a = file_arrays(false);
    named(a, cb)->data = neg.data();
    import_and_insert(cb, a, false);
  }
  a = file_arrays(false);
  named(a, "google_vecs_norm.id")->dtype = 0;
  import_and_insert("google_vecs_norm.id as float32", a, false);
  a = file_arrays(false);
  a.resize(1);
  import_and_insert("no complete table group", a, false);
  printf("---- index file: refusals of the writer and the reader\n");
  freddy_session_t* s = nullptr;
  CALL(freddy_session_open(0, &s));
  a = file_arrays(false);
  CALL(freddy_index_file_write(nullptr, a.data(), 1));
  CALL(freddy_index_file_write(kFile, nullptr, 1));
  CALL(freddy_index_file_write("no_such_directory/x.idx", a.data(), 1));
  CALL(freddy_index_file_write("/dev/full", a.data(), 2));
  a[1].ndim = 3;
  CALL(freddy_index_file_write(kFile, a.data(), 2));
  a[0].name = "";
  CALL(freddy_index_file_write(kFile, a.data(), 2));
  CALL(freddy_index_file_write(kFile, a.data(), 0));
  CALL(freddy_import_index(s, kFile));
  CALL(freddy_import_index(nullptr, kFile));
  CALL(freddy_import_index(s, nullptr));
  CALL(freddy_import_index(s, "no_such_file.idx"));
  const std::string head("FRDYIDX1\1\0\0\0", 12), pad7(7, '\0');
  auto rec = [](char dtype, char ndim, uint64_t rows) {   // the header of a one-dimensional array "a"
    std::string r("\1\0a", 3);
    r += dtype; r += ndim;
    r.append(reinterpret_cast<const char*>(&rows), 8);
    return r;
  };
  raw_file("FRDYIDX2"); CALL(freddy_import_index(s, kFile));
  raw_file(std::string("FRDYIDX1\x89\x13\0\0", 12)); CALL(freddy_import_index(s, kFile));
  raw_file(head + std::string("\0\0", 2)); CALL(freddy_import_index(s, kFile));
  raw_file(head + std::string("\5\0ab", 4)); CALL(freddy_import_index(s, kFile));
  raw_file(head + rec(7, 1, 2)); CALL(freddy_import_index(s, kFile));
  raw_file(head + rec(1, 1, 2).substr(0, 7)); CALL(freddy_import_index(s, kFile));
  raw_file(head + rec(1, 1, 2)); CALL(freddy_import_index(s, kFile));
  raw_file(head + rec(1, 1, 1ull << 48) + pad7); CALL(freddy_import_index(s, kFile));
  raw_file(head + rec(1, 1, 2) + pad7 + "abcd"); CALL(freddy_import_index(s, kFile));
  raw_file(std::string("FRDYIDX1\2\0\0\0", 12) + rec(1, 1, 1) + pad7 + "abcd" + "\0"); CALL(freddy_import_index(s, kFile));
  remove(kFile);
  CALL(freddy_session_close(s));
}

// ---- the refusals of the loaders -------------------------------------------------------------------------------------
void loader_refusals() {
  printf("---- loaders: refusals\n");
  freddy_session_t* s = nullptr;
  CALL(freddy_session_open(0, nullptr));
  CALL(freddy_session_open(0, &s));
  printf("    gpu_index(NULL, pq) = %p, gpu_index(s, NULL) = %p, gpu_index(s, nothing) = %p\n", freddy_session_gpu_index(nullptr, "pq"),
         freddy_session_gpu_index(s, nullptr), freddy_session_gpu_index(s, "nothing"));
  CALL(freddy_session_close(nullptr));
  CALL(freddy_load_vecs_norm(s, nullptr, T.norm.data(), T.N, T.d));
  CALL(freddy_load_vecs_norm(s, T.norm_ids.data(), T.norm.data(), T.N, 0));
  CALL(freddy_load_vecs_original(s, T.norm_ids.data(), nullptr, T.N, T.d));
  CALL(freddy_load_vecs_original(s, T.norm_ids.data(), T.orig.data(), -1, T.d));
  const int E = T.m * T.K, sub = T.d / T.m;
  std::vector<int32_t> neg = T.cb_pos; neg[3] = -1;
  CALL(freddy_load_pq(s, T.cb_pos.data(), T.cb_code.data(), T.pq_cb.data(), E, sub, nullptr, T.pq_codes.data(), 49));
  CALL(freddy_load_pq(s, T.cb_pos.data(), T.cb_code.data(), T.pq_cb.data(), 0, sub, T.pq_ids.data(), T.pq_codes.data(), 49));
  CALL(freddy_load_pq(s, neg.data(), T.cb_code.data(), T.pq_cb.data(), E, sub, T.pq_ids.data(), T.pq_codes.data(), 49));
  CALL(freddy_load_pq(s, T.cb_pos.data(), T.cb_code.data(), T.pq_cb.data(), E - 1, sub, T.pq_ids.data(), T.pq_codes.data(), 49));
  FAIL(1, load_pq(s));
  handles(s);
  // freddy_load_ivfadc / freddy_load_ivpq with one argument at a time replaced by a bad one
  auto ivfadc = [&](const int32_t* coarse_ids, int32_t C, int32_t sub_dim, const int32_t* cell) {
    return freddy_load_ivfadc(s, coarse_ids, T.coarse.data(), C, T.cb_pos.data(), T.cb_code.data(), T.res_cb.data(), E, sub_dim, T.fine_ids.data(), cell,
                              T.fine_codes.data(), T.N);
  };
  auto ivpq = [&](int32_t n_entries, int32_t n_cq, const int32_t* ids, const int32_t* stat_id, int32_t n_stat) {
    return freddy_load_ivpq(s, T.cb_pos.data(), T.cb_code.data(), T.ivpq_cb.data(), n_entries, sub, T.cq_pos.data(), T.cq_code.data(), T.cq_vec.data(), n_cq, ids,
                            T.ivpq_cell.data(), T.ivpq_codes.data(), T.N, stat_id, T.stat_freq.data(), n_stat);
  };
  const int32_t twice[] = {2, 0, 2}, far[] = {4, 0, 1, 2, 5};
  std::vector<int32_t> cell = T.fine_cell; cell[5] = 3;
  CALL(ivfadc(nullptr, T.C, sub, T.fine_cell.data()));
  CALL(ivfadc(T.coarse_ids.data(), 0, sub, T.fine_cell.data()));
  CALL(ivfadc(T.coarse_ids.data(), T.C, 0, T.fine_cell.data()));
  CALL(ivfadc(twice, T.C, sub, T.fine_cell.data()));
  CALL(ivfadc(T.coarse_ids.data(), T.C, sub, cell.data()));
  FAIL(1, load_ivfadc(s));
  CALL(ivpq(E, 4, T.ivpq_ids.data(), nullptr, 5));
  CALL(ivpq(E - 1, 4, T.ivpq_ids.data(), T.stat_id.data(), 5));
  CALL(ivpq(E, 2, T.ivpq_ids.data(), T.stat_id.data(), 5));   // one position only
  CALL(ivpq(E, 3, T.ivpq_ids.data(), T.stat_id.data(), 5));   // two positions, not positions * codes entries
  CALL(ivpq(E, 4, T.ivpq_ids.data(), T.stat_id.data(), 4));
  CALL(ivpq(E, 4, T.ivpq_ids.data(), far, 5));
  printf("    (without google_vecs_norm the ivpq handle is pinned without vectors)\n");
  CALL(load_ivpq(s));
  CALL(load_norm(s));
  std::vector<int32_t> ids = T.ivpq_ids; ids[7] = 300;
  CALL(ivpq(E, 4, ids.data(), T.stat_id.data(), 5));
  FAIL(1, load_ivpq(s));
  handles(s);
  printf("    (an empty pq_quantization: max(id) + 1 starts from 0)\n");
  CALL(freddy_load_pq(s, T.cb_pos.data(), T.cb_code.data(), T.pq_cb.data(), E, sub, T.pq_ids.data(), T.pq_codes.data(), 0));
  CALL(freddy_session_close(s));
}

// ---- refusals of the entry points on a fully loaded session -----------------------------------------------------------
void argument_refusals(freddy_session_t* s) {
  printf("---- entry points: argument refusals, and which of two wins\n");
  const float* q = T.row(T.norm, 9);
  const int32_t two[] = {70, 80};
  int32_t result = 0, cl[12];
  int64_t cnt = 0;
  CALL(freddy_set_w(nullptr, 1));
  CALL(freddy_set_knn_batch_function(s, nullptr));
  CALL(freddy_set_analogy_function(nullptr, "x"));
  CALL(freddy_set_analogy_in_function(s, nullptr));
  CALL(freddy_set_groups_function(nullptr, nullptr));
  R2(pq_search(s, q, 7, 0, out2, &n_rows));             // dimension before k
  R2(pq_search(s, q, 8, 0, out2, &n_rows));
  R2(pq_search(s, nullptr, 8, 5, out2, &n_rows));
  R2(pq_search_in(s, q, 7, 5, kIn, -1, out2, &n_rows));
  R2(pq_search_in(s, q, 8, 5, kIn, -1, out2, &n_rows));
  R2(ivfadc_search(s, q, 9, 0, out2, &n_rows));
  R2(ivfadc_search(s, q, 8, 5, nullptr, &n_rows));
  R3(pq_search_in_batch(s, q, 2, 7, two, 1, 5, kIn, 8, 1, out3, &n_rows));   // the count of query ids before the dimension
  R3(pq_search_in_batch(s, q, 2, 7, two, 2, 0, kIn, 8, 1, out3, &n_rows));
  R3(pq_search_in_batch(s, q, 2, 8, two, 2, 0, kIn, 8, 1, out3, &n_rows));
  R3(ivfadc_batch_search(s, kQids, -1, 5, out3, &n_rows));
  R3(ivpq_search_in(s, q, 2, 7, two, 1, 5, kIn, 8, 2, 7, 1, 0, 0.5f, 1000, out3, &n_rows));
  R3(ivpq_search_in(s, q, 2, 7, two, 2, 0, kIn, 8, 2, 7, 1, 0, 0.5f, 1000, out3, &n_rows));
  R3(ivpq_search_in(s, q, 2, 8, two, 2, 0, kIn, 8, 2, 7, 1, 0, 0.5f, 1000, out3, &n_rows));
  R3(knn_join(nullptr, q, 2, 8, two, 5, kIn, 8, out3, &n_rows));
  R2(k_nearest_neighbour(s, q, 7, 0, out2, &n_rows));
  R2(k_nearest_neighbour(s, q, 8, 0, out2, &n_rows));
  R2(knn_in_exact(s, q, 8, 5, kIn, -1, out2, &n_rows));
  RG(grouping_pq(s, kIn, 8, kGroups, 0, outg, &n_rows));
  RG(grouping_pq(s, nullptr, 8, kGroups, 3, outg, &n_rows));
  const int32_t gdup[] = {11, 3, 11}, gunk[] = {11, 3, 500};
  RG(grouping_pq(s, kIn, 8, gdup, 3, outg, &n_rows));
  RG(grouping_pq(s, kIn, 8, gunk, 3, outg, &n_rows));
  RG(grouping_pq(s, kIn, 0, kGroups, 3, outg, &n_rows));   // no input ids: no rows, no device call
  CALL(analogy_3cosadd_pq(s, 1, 3, 5, nullptr));
  CALL(analogy_3cosadd_pq(nullptr, 1, 3, 5, &result));
  R2(k_nearest_neighbour_pq(s, q, 7, 0, out2, &n_rows));
  R2(k_nearest_neighbour_ivfadc(s, q, 8, 0, out2, &n_rows));
  R2(k_nearest_neighbour_pq_pv(s, q, 7, 0, out2, &n_rows));   // "google_vecs_norm is not loaded" for a query of another dimension
  R2(k_nearest_neighbour_ivfadc_pv(s, q, 8, 0, out2, &n_rows));
  R2(knn_in_pq(s, q, 8, 0, kIn, 8, out2, &n_rows));
  R2(knn_in_pq(s, q, 7, 5, kIn, 8, out2, &n_rows));
  R3(k_nearest_neighbour_ivfadc_batch(s, kQids, 6, 0, out3, &n_rows));
  R3(k_nearest_neighbour_pq_pv_batch(s, nullptr, 6, 5, out3, &n_rows));
  R3(knn_batch(nullptr, kQids, 6, 5, out3, &n_rows));
  const int32_t one = 0;
  CALL(freddy_set_codebook_counts(s, 0, nullptr, &one, &one, 1));
  CALL(freddy_set_codebook_counts(s, 3, &one, &one, &one, 1));
  const int32_t four = 4;
  CALL(freddy_set_codebook_counts(s, 1, &four, &one, &one, 1));
  CALL(freddy_set_codebook_counts(s, 2, &one, &four, &one, 1));
  CALL(insert_batch(s, nullptr, 1, 8, nullptr));
  CALL(insert_batch(s, q, -1, 8, nullptr));
  CALL(insert_batch(s, q, 1, 7, nullptr));
  CALL(insert_batch(s, q, 0, 7, nullptr));     // the dimension before "nothing to do"
  CALL(insert_batch(s, q, 0, 8, nullptr));
  const int32_t negid[] = {3, -5}, dupid[] = {9, 7, 9};
  CALL(delete_rows(s, nullptr, 1, &cnt));
  CALL(delete_rows(s, negid, 2, &cnt));
  CALL(delete_rows(s, negid, 0, &cnt));
  CALL(update_rows(s, negid, nullptr, 2, 8, &cnt));
  CALL(update_rows(s, negid, q, 2, 8, &cnt));
  CALL(update_rows(s, dupid, q, 3, 8, &cnt));
  CALL(update_rows(s, dupid, q, 2, 7, &cnt));
  CALL(update_rows(s, dupid, q, 0, 7, &cnt));   // "nothing to do" before the dimension
  CALL(analogy_3cosadd_in_pq(s, 1, 3, 5, nullptr, 8, &result));
  CALL(analogy_3cosadd_in_ivpq(s, 1, 3, 5, kIn, -1, &result));
  CALL(analogy_3cosadd_pq_batch(s, nullptr, 3, &result));
  CALL(analogy_3cosadd_in_pq_batch(s, kTriples, 3, nullptr, 8, &result));
  CALL(analogy_3cosadd_pq_batch(s, kTriples, 0, &result));
  CALL(analogy_3cosadd(s, 1, 3, 5, nullptr));
  CALL(analogy_3cosadd_in(s, 1, 3, 5, nullptr, 8, &result));
  CALL(analogy_pair_direction(s, 1, 3, 5, nullptr));
  CALL(analogy(s, 1, 3, 5, nullptr));
  CALL(analogy_in(nullptr, 1, 3, 5, kIn, 8, &result));
  R3(knn_search_in_batch(s, q, 2, 7, 0, kIn, 8, out3, &n_rows));
  R3(knn_search_in_batch(s, nullptr, 2, 8, 5, kIn, 8, out3, &n_rows));
  R3(knn_search_in_batch(s, q, 2, 8, 4097, kIn, 8, out3, &n_rows));
  R3(knn_search_in_batch(s, q, 0, 8, 5, kIn, 8, out3, &n_rows));
  R3(knn_search_in_batch_ids(s, nullptr, 6, 5, kIn, 8, out3, &n_rows));
  RG(grouping_func(s, kTokens, 12, nullptr, 3, outg, &n_rows));
  RG(groups(nullptr, kTokens, 12, kGroups, 3, outg, &n_rows));
  CALL(cluster_exact(s, nullptr, 12, 3, g_draws, 40, cl));
  CALL(cluster_pq(s, kTokens, 12, 0, g_draws, 40, cl));
  const int32_t unk[] = {1, 5, 1000};
  CALL(cluster_exact(s, unk, 3, 2, g_draws, 40, cl));
  CALL(exact_assign(s, q, 2, 7, kTokens, 12, cl, nullptr));
  CALL(pq_assign(s, q, 2, 7, kTokens, 12, cl, nullptr));
  CALL(freddy_set_statistics_table(s, nullptr, T.stat_freq.data(), 5));
  CALL(freddy_set_statistics_table(s, T.stat_id.data(), T.stat_freq.data(), 6));
  CALL(create_statistics(s, nullptr, 3, nullptr));
  CALL(create_statistics(s, nullptr, 0, nullptr));
  CALL(create_statistics(nullptr, nullptr, 0, nullptr));
}

// ---- k, pvf, W, lists, dispatcher names ----------------------------------------------------------------------------------
void parameters(freddy_session_t* s) {
  printf("---- parameters: k, pvf, w, duplicate and unknown ids, empty IN-lists, the dispatchers' names\n");
  const float* q = T.row(T.norm, 9);
  const float* q2 = T.row(T.norm, 11);
  const int32_t two[] = {70, 80};
  int32_t result = 0, res3[3];
  printf("  k = 1\n");
  R2(pq_search(s, q, 8, 1, out2, &n_rows));
  R2(k_nearest_neighbour(s, q, 8, 1, out2, &n_rows));
  R3(knn_search_in_batch(s, q2, 2, 8, 1, kIn, 8, out3, &n_rows));
  for (int k : {60}) {   // k above N: (-1, sentinel) filler rows
    printf("  k = %d\n", k);
    R2(pq_search(s, q, 8, k, out2, &n_rows));
    R2(pq_search_in(s, q, 8, k, kIn, 8, out2, &n_rows));
    R2(ivfadc_search(s, q, 8, k, out2, &n_rows));
    R3(ivfadc_batch_search(s, kQids, 6, k, out3, &n_rows));
    R2(k_nearest_neighbour(s, q, 8, k, out2, &n_rows));
    R2(k_nearest_neighbour_pq(s, q, 8, k, out2, &n_rows));
    R2(k_nearest_neighbour_ivfadc(s, q, 8, k, out2, &n_rows));
    R2(knn_in_pq(s, q, 8, k, kIn, 8, out2, &n_rows));
    R3(k_nearest_neighbour_ivfadc_batch(s, kQids, 6, k, out3, &n_rows));
    R3(knn_search_in_batch(s, q2, 2, 8, k, kIn, 8, out3, &n_rows));
    R3(knn_join(s, q2, 2, 8, two, k, kIn, 8, out3, &n_rows));
  }
  printf("  empty lists\n");
  R2(pq_search_in(s, q, 8, 5, nullptr, 0, out2, &n_rows));
  R3(pq_search_in_batch(s, q2, 2, 8, two, 2, 5, nullptr, 0, 0, out3, &n_rows));
  R3(pq_search_in_batch(s, q2, 0, 8, two, 0, 5, kIn, 8, 0, out3, &n_rows));
  R2(knn_in_exact(s, q, 8, 5, nullptr, 0, out2, &n_rows));
  R2(knn_in_pq(s, q, 8, 5, nullptr, 0, out2, &n_rows));
  R1(analogy_3cosadd_in_pq(s, 1, 3, 5, nullptr, 0, &result));
  R1(analogy_3cosadd_in_ivpq(s, 1, 3, 5, nullptr, 0, &result));
  R1(analogy_3cosadd_in(s, 1, 3, 5, nullptr, 0, &result));
  CALL_(analogy_3cosadd_in_pq_batch(s, kTriples, 3, nullptr, 0, res3), showi("results", res3, 3));
  R3(ivfadc_batch_search(s, kQids, 0, 5, out3, &n_rows));
  const int32_t unknown[] = {1000, 2000};
  R3(ivfadc_batch_search(s, unknown, 2, 5, out3, &n_rows));
  R3(k_nearest_neighbour_ivfadc_pv_batch(s, unknown, 2, 5, out3, &n_rows));
  R3(k_nearest_neighbour_ivfadc_batch(s, kQids, 0, 5, out3, &n_rows));
  R3(knn_search_in_batch(s, q2, 2, 8, 5, nullptr, 0, out3, &n_rows));
  R3(knn_search_in_batch_ids(s, unknown, 2, 5, kIn, 8, out3, &n_rows));
  RG(grouping_func(s, unknown, 2, kGroups, 3, outg, &n_rows));
  RG(grouping_func(s, kTokens, 12, nullptr, 0, outg, &n_rows));
  const int32_t toks[] = {9, 5, 9, 1000, 1};   // duplicated and unknown tokens and groups
  const int32_t gdup[] = {11, 3, 11, 500};
  RG(grouping_func(s, toks, 5, gdup, 4, outg, &n_rows));
  R1(analogy_3cosadd_pq(s, 1, 1000, 5, &result));   // an unknown word: NULL, no device call
  R1(analogy_3cosadd_in_pq(s, 1000, 3, 5, kIn, 8, &result));
  R1(analogy_3cosadd(s, 1, 1000, 5, &result));
  R1(analogy_pair_direction(s, 1, 1000, 5, &result));
  printf("  pvf = 2, w = 1\n");
  CALL(freddy_set_pvf(s, 2)); CALL(freddy_set_w(s, 1));
  R2(k_nearest_neighbour_pq_pv(s, q, 8, 5, out2, &n_rows));
  R2(k_nearest_neighbour_ivfadc_pv(s, q, 8, 5, out2, &n_rows));
  R3(k_nearest_neighbour_pq_pv_batch(s, kQids, 6, 5, out3, &n_rows));
  R3(k_nearest_neighbour_ivfadc_pv_batch(s, kQids, 6, 5, out3, &n_rows));
  R2(ivfadc_search(s, q, 8, 5, out2, &n_rows));
  R1(analogy_3cosadd_pq(s, 1, 3, 5, &result));
  R1(analogy_3cosadd_ivfadc(s, 1, 3, 5, &result));
  R1(analogy_3cosadd_in_pq(s, 1, 3, 5, kIn, 8, &result));
  CALL_(analogy_3cosadd_ivfadc_batch(s, kTriples, 3, res3), showi("results", res3, 3));
  printf("  pvf = 0 counts as 1\n");
  CALL(freddy_set_pvf(s, 0));
  R2(k_nearest_neighbour_pq_pv(s, q, 8, 5, out2, &n_rows));
  R3(k_nearest_neighbour_pq_pv_batch(s, kQids, 6, 5, out3, &n_rows));
  printf("  pvf = 50: every row is a candidate -- the rows 39, 41, 43 are equal, the lowest id decides; pvf * k above 4096\n");
  CALL(freddy_set_pvf(s, 50)); CALL(freddy_set_w(s, 3));
  R1(analogy_3cosadd_pq(s, 5, 5, 39, &result));
  R1(analogy_3cosadd_ivfadc(s, 5, 5, 39, &result));
  R1(analogy_3cosadd_in_pq(s, 5, 5, 39, kIn, 8, &result));
  R1(analogy_3cosadd_in_ivpq(s, 5, 5, 39, kIn, 8, &result));
  R2(k_nearest_neighbour_pq_pv(s, T.row(T.norm, 39), 8, 4, out2, &n_rows));
  R2(k_nearest_neighbour_ivfadc_pv(s, T.row(T.norm, 39), 8, 4, out2, &n_rows));
  R2(k_nearest_neighbour_pq_pv(s, q, 8, 100, out2, &n_rows));
  R2(k_nearest_neighbour_ivfadc_pv(s, q, 8, 82, out2, &n_rows));
  R3(k_nearest_neighbour_pq_pv_batch(s, kQids, 6, 82, out3, &n_rows));
  CALL(freddy_set_pvf(s, 20));
  printf("  configuration\n");
  CALL(freddy_set_alpha(s, 5)); CALL(freddy_set_confidence_value(s, 0.25f)); CALL(freddy_set_long_codes_threshold(s, 77)); CALL(freddy_set_method_flag(s, 2));
  CALL(freddy_set_use_targetlist(s, 0));
  printf("    w=%d pvf=%d alpha=%d confidence=%08x long_codes_threshold=%d method_flag=%d use_targetlist=%d\n", freddy_get_w(s), freddy_get_pvf(s),
         freddy_get_alpha(s), bits(freddy_get_confidence_value(s)), freddy_get_long_codes_threshold(s), freddy_get_method_flag(s), freddy_get_use_targetlist(s));
  R3(knn_join(s, q2, 2, 8, two, 5, kIn, 8, out3, &n_rows));
  R1(analogy_3cosadd_in_ivpq(s, 1, 3, 5, kIn, 8, &result));
  int32_t cl[6];
  const int32_t dtok[] = {1, 5, 5, 9, 1, 13};   // duplicated tokens; the caller's draws run out and the internal generator goes on
  CALL_(cluster_ivpq(s, dtok, 6, 2, g_draws, 5, cl), showi("clusters", cl, 6));
  printf("  dispatchers\n");
  for (const char* f : {"k_nearest_neighbour_ivfadc_batch", "k_nearest_neighbour_ivfadc_pv_batch", "k_nearest_neighbour_pq_pv_batch", "k_nearest_neighbour_pq_batch"}) {
    CALL(freddy_set_knn_batch_function(s, f));
    printf("    knn_batch_function = %s\n", freddy_get_knn_batch_function(s));
    R3(knn_batch(s, kQids, 6, 2, out3, &n_rows));
  }
  for (const char* f : {"analogy_3cosadd", "analogy_3cosmul", "analogy_pair_direction", "analogy_3cosadd_pq", "analogy_3cosadd_ivfadc", "analogy_3cosadd_in"}) {
    CALL(freddy_set_analogy_function(s, f));
    printf("    analogy_function = %s\n", freddy_get_analogy_function(s));
    R1(analogy(s, 1, 3, 5, &result));
  }
  for (const char* f : {"analogy_3cosadd_in", "analogy_3cosadd_in_pq", "analogy_3cosadd_in_ivpq", "analogy_pair_direction"}) {
    CALL(freddy_set_analogy_in_function(s, f));
    printf("    analogy_in_function = %s\n", freddy_get_analogy_in_function(s));
    R1(analogy_in(s, 1, 3, 5, kIn, 8, &result));
  }
  for (const char* f : {"grouping_func", "grouping_func_pq", "grouping_pq"}) {
    CALL(freddy_set_groups_function(s, f));
    printf("    groups_function = %s\n", freddy_get_groups_function(s));
    RG(groups(s, kTokens, 12, kGroups, 3, outg, &n_rows));
  }
  char v2[2][16], v3[3][16];
  const freddy_row2 r2 = {41, 0.123456789f};
  const freddy_row3 r3 = {7, -1, 1000.0f};
  freddy_emit_row2(&r2, v2); freddy_emit_row3(&r3, v3);
  printf("    emit_row2 = '%s' '%s', emit_row3 = '%s' '%s' '%s'\n", v2[0], v2[1], v3[0], v3[1], v3[2]);
}

// ---- a device call that fails, for every entry point ----------------------------------------------------------------------
void device_failures() {
  freddy_session_t* s = full_session("F (a device call fails: the lazy pins, and one entry point of each kind)");
  const float* q = T.row(T.norm, 9);
  const float* q2 = T.row(T.norm, 11);
  const int32_t two[] = {70, 80};
  int32_t result = 0, res3[3], cl[12];
  float as[12], stats[5];
  FAIL(1, k_nearest_neighbour(s, q, 8, 5, out2, &n_rows));   // the pin of google_vecs_norm
  handles(s);
  FAIL(2, k_nearest_neighbour(s, q, 8, 5, out2, &n_rows));   // pinned, then the search
  handles(s);
  FAIL(1, analogy_pair_direction(s, 1, 3, 5, &result));
  FAIL(2, analogy_pair_direction(s, 1, 3, 5, &result));
  FAIL(1, analogy_pair_direction(s, 1, 3, 5, &result));
  FAIL(1, pq_search(s, q, 8, 5, out2, &n_rows));
  FAIL(1, pq_search_in(s, q, 8, 5, kIn, 8, out2, &n_rows));
  FAIL(1, ivfadc_search(s, q, 8, 5, out2, &n_rows));
  FAIL(1, analogy_3cosadd(s, 1, 3, 5, &result));
  FAIL(1, pq_search_in_batch(s, q2, 2, 8, two, 2, 5, kIn, 8, 1, out3, &n_rows));
  FAIL(1, ivfadc_batch_search(s, kQids, 6, 5, out3, &n_rows));
  FAIL(1, knn_join(s, q2, 2, 8, two, 5, kIn, 8, out3, &n_rows));
  FAIL(1, grouping_pq(s, kIn, 8, kGroups, 3, outg, &n_rows));
  FAIL(1, analogy_3cosadd_ivfadc(s, 1, 3, 5, &result));
  FAIL(1, k_nearest_neighbour_ivfadc_pv(s, q, 8, 5, out2, &n_rows));
  FAIL(1, k_nearest_neighbour_pq_pv_batch(s, kQids, 6, 5, out3, &n_rows));
  FAIL(1, analogy_3cosadd_in_ivpq(s, 1, 3, 5, kIn, 8, &result));
  FAIL(1, analogy_3cosadd_in_pq_batch(s, kTriples, 3, kIn, 8, res3));
  FAIL(3, cluster_exact(s, kTokens, 12, 3, g_draws, 40, cl));
  FAIL(3, cluster_pq(s, kTokens, 12, 3, g_draws, 40, cl));
  FAIL(3, cluster_ivpq(s, kTokens, 12, 3, g_draws, 40, cl));
  FAIL(1, pq_assign(s, q2, 2, 8, kTokens, 12, cl, as));
  FAIL(1, knn_search_in_batch(s, q2, 2, 8, 5, kIn, 8, out3, &n_rows));
  FAIL(1, freddy_set_statistics_table(s, T.stat_id.data(), T.stat_freq.data(), 5));
  FAIL(1, create_statistics(s, nullptr, 0, stats));
  CALL(freddy_session_close(s));
}

// ---- insert_batch / delete_rows / update_rows with each device call of the sequence failing in turn ---------------------
void failure_sweep() {
  int32_t result = 0, id[2] = {0, 0};
  int64_t cnt = 0;
  const int32_t upd[] = {9, 1000, 21, 3, 5, 7, 11, 13};
  const int32_t del[] = {9, 13, 9, 1000};
  for (int which = 0; which < 3; ++which) {
    const int calls = which == 0 ? 8 : 5;
    for (int f = 1; f <= calls; ++f) {
      printf("---- failure sweep: %s, device call %d of %d fails\n", which == 0 ? "insert_batch" : which == 1 ? "delete_rows" : "update_rows", f, calls);
      freddy_session_t* s = nullptr;
      stub_quiet(which != 0 || f != 1);   // the set-up, five loads and the two lazy pins, is the same every time: traced once
      freddy_session_open(0, &s);
      load_norm(s); load_orig(s); load_pq(s); load_ivfadc(s); load_ivpq(s);
      k_nearest_neighbour(s, T.row(T.norm, 9), T.d, 1, out2, &n_rows);
      analogy_pair_direction(s, 1, 3, 5, &result);
      stub_quiet(0);
      stub_fail_after(f);
      if (which == 0) CALL(insert_batch(s, T.row(T.norm, 21), 2, T.d, id));
      if (which == 1) CALL(delete_rows(s, del, 4, &cnt));
      if (which == 2) CALL(update_rows(s, upd, T.row(T.norm, 31), 8, T.d, &cnt));
      stub_fail_after(0);
      after_failure(s);
      CALL(freddy_session_close(s));
    }
  }
}

int timing(long n) {
  stub_quiet(1);
  freddy_session_t* s = nullptr;
  freddy_session_open(0, &s);
  if (load_norm(s) || load_orig(s) || load_pq(s) || load_ivfadc(s) || load_ivpq(s)) return 1;
  int32_t qids[16], upd[8];
  for (int i = 0; i < 16; ++i) qids[i] = 1 + 4 * i;
  for (int i = 0; i < 8; ++i) upd[i] = 3 + 6 * i;
  int64_t cnt = 0;
  long bad = 0;
  auto run = [&](const char* name, auto&& call) {
    for (long i = 0; i < n / 10 + 1; ++i) bad += call() != 0;
    const auto t0 = std::chrono::steady_clock::now();
    for (long i = 0; i < n; ++i) bad += call() != 0;
    const double ns = std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0).count();
    fprintf(stderr, "%s %.1f ns/call\n", name, ns / (double)n);
  };
  run("ivfadc_batch_search(16)", [&] { return ivfadc_batch_search(s, qids, 16, 5, out3, &n_rows); });
  run("k_nearest_neighbour_pq_pv", [&] { return k_nearest_neighbour_pq_pv(s, T.row(T.norm, 9), T.d, 5, out2, &n_rows); });
  run("update_rows(8)", [&] { return update_rows(s, upd, T.row(T.norm, 31), 8, T.d, &cnt); });
  freddy_session_close(s);
  return bad != 0;
}

}  // namespace

int main(int argc, char** argv) {
  for (double& v : g_draws) v = (double)(lcg() % 100000u) / 100000.0;
  if (argc == 3 && !strcmp(argv[1], "--time")) return timing(atol(argv[2]));
  freddy_session_t* s = nullptr;

  printf("---- session E: nothing loaded\n");
  CALL(freddy_session_open(0, &s));
  every_search(s, 8);
  every_mutation(s, 8);
  CALL(freddy_session_close(s));

  printf("---- session P: the three code tables, no google_vecs_norm\n");
  CALL(freddy_session_open(0, &s));
  CALL(load_pq(s)); CALL(load_ivfadc(s)); CALL(load_ivpq(s));
  every_search(s, 8, true, true);
  every_mutation(s, 8);
  CALL(freddy_session_close(s));

  printf("---- session D: google_vecs_norm with 4 dimensions, code tables with 8\n");
  CALL(freddy_session_open(0, &s));
  CALL(freddy_load_vecs_norm(s, T.norm_ids.data(), T.norm.data(), T.N, 4));
  CALL(load_pq(s)); CALL(load_ivfadc(s)); CALL(load_ivpq(s));
  every_search(s, 8, false, true);
  every_mutation(s, 8);
  CALL(freddy_session_close(s));

  printf("---- session V: google_vecs_norm and the pq tables only (update_rows and delete_rows skip what is not loaded)\n");
  CALL(freddy_session_open(0, &s));
  CALL(load_norm(s)); CALL(load_pq(s));
  every_mutation(s, 8);
  CALL(freddy_session_close(s));

  s = full_session("A");
  every_search(s, 8);
  argument_refusals(s);
  parameters(s);
  printf("---- mutations on session A: counts set before an insert; insert -> delete -> insert (max(id) + 1 of what is left)\n");
  {
    int32_t new_ids[3] = {-7, -7, -7}, result = 0;
    int64_t cnt = -7;
    CALL(freddy_set_codebook_counts(s, 0, T.cb_pos.data(), T.cb_code.data(), T.counts.data(), T.m * T.K));
    CALL(freddy_set_codebook_counts(s, 1, T.cb_pos.data(), T.cb_code.data(), T.counts.data(), 3));
    CALL_(insert_batch(s, T.row(T.norm, 21), 3, 8, new_ids), showi("new_ids", new_ids, 3));
    const int32_t del[] = {new_ids[2], new_ids[1], 200, 95, 9, 9};   // the two largest ids of every table, the pq-only id, a duplicate
    CALL(delete_rows(s, del, 6, &cnt)); if (!g_rc) printf("    removed = %lld\n", (long long)cnt);
    CALL_(insert_batch(s, T.row(T.norm, 21), 2, 8, new_ids), showi("new_ids", new_ids, 2));
    const int32_t upd[] = {new_ids[0], 3, 9};
    CALL(update_rows(s, upd, T.row(T.norm, 31), 3, 8, &cnt)); if (!g_rc) printf("    updated = %lld\n", (long long)cnt);
    CALL(update_rows(s, upd, T.row(T.norm, 31), 3, 8, nullptr));
    CALL(delete_rows(s, upd, 1, nullptr));
    R1(analogy_pair_direction(s, 1, new_ids[1], 5, &result));   // insert_batch does not extend google_vecs
    CALL(load_norm(s));                                          // loading the table again drops its handle
    handles(s);
    CALL(load_orig(s));
    R2(k_nearest_neighbour(s, T.row(T.norm, 9), 8, 1, out2, &n_rows));
    CALL(load_pq(s)); CALL(load_ivfadc(s)); CALL(load_ivpq(s));   // ... and a reload replaces the pinned handle
  }
  CALL(freddy_session_close(s));

  loader_refusals();
  index_files();
  device_failures();
  failure_sweep();
  return 0;
}
