// session.h -- what a session of the host mirror holds and how it gets there: the error text, one record per table, the handles
// and who drops them, and the freddy_load_* entry points.  Included by freddy_udf.cpp only (one translation unit, as csrc/).
#pragma once
#include "../../include/freddy_udf.h"
#include "../../include/freddy_udf_ivpq.h"

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include "../../include/freddy_gpu.h"

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}
int gpu_fail(int rc) { return fail(rc, "%s", freddy_gpu_last_error()); }

}  // namespace

// CodebookCompound from an entry list: slot from each entry's own (pos, code); positions and
// codeSize are max+1 as in getCodebook (index_utils.c:577-630)
struct Codebook {
  int m = 0, K = 0, s = 0;
  std::vector<float> dense;   // [m][K][s]
  int build(const int32_t* pos, const int32_t* code, const float* vec, int n, int sub) {
    if (n <= 0 || sub <= 0 || !pos || !code || !vec) return fail(-1, "empty codebook");
    m = 0; K = 0; s = sub;
    for (int i = 0; i < n; ++i) {
      if (pos[i] < 0 || code[i] < 0) return fail(-1, "negative pos/code in codebook");
      m = std::max(m, pos[i] + 1);
      K = std::max(K, code[i] + 1);
    }
    if ((int64_t)m * K != n) return fail(-1, "codebook has %d entries, expected positions*codes = %d*%d", n, m, K);
    dense.assign((size_t)m * K * s, 0.0f);
    for (int i = 0; i < n; ++i)
      memcpy(&dense[((size_t)pos[i] * K + code[i]) * s], vec + (size_t)i * s, sizeof(float) * s);
    return 0;
  }
};

namespace {

// permutation that sorts row ids ascending (table scan order = canonical order)
std::vector<int64_t> order_by_id(const int32_t* ids, int64_t N) {
  std::vector<int64_t> ord((size_t)N);
  std::iota(ord.begin(), ord.end(), 0);
  std::stable_sort(ord.begin(), ord.end(), [&](int64_t a, int64_t b) { return ids[a] < ids[b]; });
  return ord;
}

// a column in the order `ord`: dst row i = src row ord[i], rows of `width` elements
template <class T>
std::vector<T> gather(const T* src, const std::vector<int64_t>& ord, size_t width = 1) {
  std::vector<T> dst(ord.size() * width);
  for (size_t i = 0; i < ord.size(); ++i) memcpy(&dst[i * width], src + (size_t)ord[i] * width, sizeof(T) * width);
  return dst;
}

// getStatistics (index_utils.c:632-665): result[coarse_id] = coarse_freq, from the (coarse_id, coarse_freq) rows of a stat table
int stat_row(int cells, const int32_t* stat_coarse_id, const float* stat_freq, int32_t n_stat, std::vector<float>& stats) {
  if (n_stat != cells + 1) return fail(-1, "statistics table has %d rows, expected %d", n_stat, cells + 1);
  stats.assign((size_t)cells + 1, 0.0f);
  for (int i = 0; i < n_stat; ++i) {
    if (stat_coarse_id[i] < 0 || stat_coarse_id[i] > cells) return fail(-1, "statistics coarse_id out of range");
    stats[stat_coarse_id[i]] = stat_freq[i];
  }
  return 0;
}

void drop(freddy_gpu_index_t*& h) {
  if (h) { freddy_gpu_unpin(h); h = nullptr; }
}

}  // namespace

// A code table with its codebook: pq_quantization + pq_codebook, fine_quantization + residual_codebook, fine_quantization_ivpq +
// codebook_ivpq -- numbered as freddy_set_codebook_counts numbers them.  What insert_batch reads and writes besides the rows
// (freddy.c:1545-1560): the codebook with its count column and the ids, whose largest is where the next insert goes on.
enum { PQ = 0, IVF = 1, IVPQ = 2 };
const char* const kNotLoaded[3] = {"pq_quantization / pq_codebook are not loaded",
                                   "coarse_quantization / residual_codebook / fine_quantization are not loaded", "the ivpq tables are not loaded"};
struct CodeTable {
  freddy_gpu_index_t* h = nullptr;   // pinned by its loader; NULL: not loaded (or dropped after a failed mutation)
  int d = 0;
  Codebook cb;
  std::vector<int32_t> counts;       // count column; 1 unless freddy_set_codebook_counts was called
  std::vector<int32_t> ids;          // ascending; delete_rows takes ids out
  // "SELECT max(id) + 1" of insert_batch sees the rows that are left (0 for an empty table)
  int32_t max_id() const { return ids.empty() ? 0 : ids.back(); }
  void loaded(const Codebook& book, std::vector<int32_t>&& ascending_ids) {
    d = book.m * book.s;
    cb = book;
    counts.assign((size_t)book.m * book.K, 1);
    ids = std::move(ascending_ids);
  }
};

// A table of raw vectors: google_vecs_norm, and google_vecs (get_vecs_name_original()), the un-normalised table
// analogy_pair_direction scans.  Rows by ascending id; pinned as a vector handle by the first function that needs it.
struct VecTable {
  int d = 0;
  std::vector<int32_t> ids;     // ascending
  std::vector<float> rows;      // [N][d] in that order
  freddy_gpu_index_t* h = nullptr;
  bool empty() const { return ids.empty(); }
  int64_t row_of(int32_t id) const {   // -1: no such row
    auto it = std::lower_bound(ids.begin(), ids.end(), id);
    return it == ids.end() || *it != id ? -1 : it - ids.begin();
  }
  const float* find(int32_t id) const {
    const int64_t r = row_of(id);
    return r < 0 ? nullptr : rows.data() + (size_t)r * d;
  }
  int load(const int32_t* in_ids, const float* vectors, int64_t N, int32_t dim) {
    if (!in_ids || !vectors || N < 0 || dim <= 0) return fail(-1, "bad argument");
    const std::vector<int64_t> ord = order_by_id(in_ids, N);
    d = dim;
    ids = gather(in_ids, ord);
    rows = gather(vectors, ord, (size_t)dim);
    drop(h);
    return 0;
  }
  int pinned(int device) {
    if (h) return 0;
    freddy_vec_desc desc = {d, (int64_t)ids.size(), ids.data(), rows.data()};
    if (int rc = freddy_gpu_pin_vectors(&desc, device, &h)) return gpu_fail(rc);
    return 0;
  }
  // "SELECT id, vector FROM <table> WHERE id IN (...)": the rows in table order, duplicates collapse, unknown ids vanish
  // (freddy.c:767-804) -> their ids and, row-aligned, their vectors
  void select_in(const int32_t* in_ids, int n, std::vector<int32_t>& out_ids, std::vector<float>& out_rows) const {
    std::vector<int64_t> at;
    for (int i = 0; i < n; ++i)
      if (const int64_t r = row_of(in_ids[i]); r >= 0) at.push_back(r);
    std::sort(at.begin(), at.end());
    at.erase(std::unique(at.begin(), at.end()), at.end());
    out_ids = gather(ids.data(), at);
    out_rows = gather(rows.data(), at, (size_t)d);
  }
};

struct freddy_session {
  int device = 0;
  // config functions, defaults from freddy--0.0.1.sql:188-194
  int w = 3, pvf = 20, alpha = 3, long_codes_threshold = 10000000, method_flag = 0, use_targetlist = 1;
  float confidence = 0.8f;
  VecTable norm, orig;               // google_vecs_norm, google_vecs
  CodeTable code[3];                 // [PQ], [IVF], [IVPQ]
  std::vector<float> coarse;         // coarse_quantization [C][d]
  int C = 0;
  Codebook cq_multi;                 // coarse_quantization_ivpq
  // set_analogy_function / set_analogy_in_function / set_groups_function / set_knn_batch_function (freddy--0.0.1.sql:197-200)
  std::string analogy_fn = "analogy_3cosadd", analogy_in_fn = "analogy_3cosadd_in", groups_fn = "grouping_func",
              knn_batch_fn = "k_nearest_neighbour_ivfadc_batch";
};

namespace {

// Which handles a session gives up, and when -- said here and nowhere else:
//   freddy_session_close          all five.
//   a failed delete_rows          all five: remove_rows runs on every pinned handle, and any of them may have lost part of the rows.
//   a failed insert_batch or      the three code tables and google_vecs_norm, NOT google_vecs: neither call touches the original
//   update_rows                   table (insert_batch receives only normalised vectors, update_rows leaves it as it is), so that
//                                 handle still equals its host table.
// The host tables stay as they were in every case; searches then fail loudly with "not loaded" (google_vecs_norm and google_vecs
// are pinned again on their next use) until the tables are loaded again.
void drop_handles(freddy_session* s, bool original_too) {
  for (CodeTable& t : s->code) drop(t.h);
  drop(s->norm.h);
  if (original_too) drop(s->orig.h);
}
// a device mutation failed midway with `rc`: its message is kept first (unpinning may overwrite the library's), then the handles go
int device_failed(freddy_session* s, int rc, bool original_too) {
  const int code = gpu_fail(rc);
  drop_handles(s, original_too);
  return code;
}

}  // namespace

extern "C" {

const char* freddy_udf_last_error(void) { return g_err; }

int freddy_session_open(int device, freddy_session_t** out) {
  if (!out) return fail(-1, "NULL argument");
  freddy_session* s = new freddy_session();
  s->device = device;
  *out = s;
  return 0;
}

void* freddy_session_gpu_index(const freddy_session_t* s, const char* table) {
  if (!s || !table) return nullptr;
  const std::string t(table);
  return t == "pq" ? s->code[PQ].h : t == "ivfadc" ? s->code[IVF].h : t == "ivpq" ? s->code[IVPQ].h : t == "vecs" ? s->norm.h : nullptr;
}

int freddy_session_close(freddy_session_t* s) {
  if (!s) return 0;
  drop_handles(s, true);
  delete s;
  return 0;
}

int freddy_load_vecs_norm(freddy_session_t* s, const int32_t* ids, const float* vectors, int64_t N, int32_t d) {
  return s ? s->norm.load(ids, vectors, N, d) : fail(-1, "bad argument");
}
int freddy_load_vecs_original(freddy_session_t* s, const int32_t* ids, const float* vectors, int64_t N, int32_t d) {
  return s ? s->orig.load(ids, vectors, N, d) : fail(-1, "bad argument");
}

int freddy_load_pq(freddy_session_t* s, const int32_t* cb_pos, const int32_t* cb_code, const float* cb_vectors,
                   int32_t n_entries, int32_t sub_dim, const int32_t* ids, const int16_t* codes, int64_t N) {
  if (!s || !ids || !codes) return fail(-1, "bad argument");
  Codebook cb;
  if (int rc = cb.build(cb_pos, cb_code, cb_vectors, n_entries, sub_dim)) return rc;
  const std::vector<int64_t> ord = order_by_id(ids, N);
  std::vector<int32_t> sid = gather(ids, ord);
  const std::vector<int16_t> scodes = gather(codes, ord, (size_t)cb.m);
  freddy_pq_desc desc = {cb.m * cb.s, cb.m, cb.K, N, cb.dense.data(), sid.data(), scodes.data()};
  CodeTable& t = s->code[PQ];
  drop(t.h);
  if (int rc = freddy_gpu_pin_pq(&desc, s->device, &t.h)) return gpu_fail(rc);
  t.loaded(cb, std::move(sid));
  return 0;
}

int freddy_load_ivfadc(freddy_session_t* s, const int32_t* coarse_ids_tbl, const float* coarse_vectors, int32_t C,
                       const int32_t* cb_pos, const int32_t* cb_code, const float* cb_vectors, int32_t n_entries,
                       int32_t sub_dim, const int32_t* ids, const int32_t* coarse_id, const int16_t* codes, int64_t N) {
  if (!s || !coarse_ids_tbl || !coarse_vectors || C <= 0 || !ids || !coarse_id || !codes) return fail(-1, "bad argument");
  Codebook cb;
  if (int rc = cb.build(cb_pos, cb_code, cb_vectors, n_entries, sub_dim)) return rc;
  const int d = cb.m * cb.s;
  // coarse ids must be 0..C-1: the C code indexes the array by id (freddy.c:309,367,873,908)
  std::vector<float> coarse((size_t)C * d);
  std::vector<char> seen((size_t)C, 0);
  for (int i = 0; i < C; ++i) {
    const int id = coarse_ids_tbl[i];
    if (id < 0 || id >= C || seen[id]) return fail(-1, "coarse_quantization ids must be exactly 0..%d", C - 1);
    seen[id] = 1;
    memcpy(&coarse[(size_t)id * d], coarse_vectors + (size_t)i * d, sizeof(float) * d);
  }
  // "ORDER BY coarse_id, id": inverted lists with ascending ids inside
  std::vector<int64_t> ord((size_t)N);
  std::iota(ord.begin(), ord.end(), 0);
  for (int64_t i = 0; i < N; ++i)
    if (coarse_id[i] < 0 || coarse_id[i] >= C) return fail(-1, "coarse_id %d out of range at row %lld", coarse_id[i], (long long)i);
  std::stable_sort(ord.begin(), ord.end(), [&](int64_t a, int64_t b) {
    return coarse_id[a] != coarse_id[b] ? coarse_id[a] < coarse_id[b] : ids[a] < ids[b];
  });
  std::vector<int32_t> list_off((size_t)C + 1, 0);
  for (int64_t i = 0; i < N; ++i) list_off[coarse_id[i] + 1]++;
  for (int c = 0; c < C; ++c) list_off[c + 1] += list_off[c];
  const std::vector<int32_t> sid = gather(ids, ord);
  const std::vector<int16_t> scodes = gather(codes, ord, (size_t)cb.m);
  freddy_ivf_desc desc = {d, cb.m, cb.K, C, N, coarse.data(), cb.dense.data(), list_off.data(), sid.data(), scodes.data()};
  CodeTable& t = s->code[IVF];
  drop(t.h);
  if (int rc = freddy_gpu_pin_ivf(&desc, s->device, &t.h)) return gpu_fail(rc);
  std::vector<int32_t> ascending(ids, ids + N);
  std::sort(ascending.begin(), ascending.end());
  t.loaded(cb, std::move(ascending));
  s->coarse = coarse;
  s->C = C;
  return 0;
}

int freddy_load_ivpq(freddy_session_t* s, const int32_t* cb_pos, const int32_t* cb_code, const float* cb_vectors,
                     int32_t n_entries, int32_t sub_dim, const int32_t* cq_pos, const int32_t* cq_code,
                     const float* cq_vectors, int32_t n_cq_entries, const int32_t* ids, const int32_t* coarse_id,
                     const int16_t* codes, int64_t N, const int32_t* stat_coarse_id, const float* stat_freq,
                     int32_t n_stat) {
  if (!s || !ids || !coarse_id || !codes || !stat_coarse_id || !stat_freq) return fail(-1, "bad argument");
  Codebook cb;
  if (int rc = cb.build(cb_pos, cb_code, cb_vectors, n_entries, sub_dim)) return rc;
  const int d = cb.m * cb.s;
  int cpos = 0;
  for (int i = 0; i < n_cq_entries; ++i) cpos = std::max(cpos, cq_pos[i] + 1);
  if (cpos != 2) return fail(-1, "the multi-index coarse quantizer must have 2 positions (index_utils.c:322)");
  Codebook cq;
  if (int rc = cq.build(cq_pos, cq_code, cq_vectors, n_cq_entries, d / 2)) return rc;
  const int cells = cq.K * cq.K;
  std::vector<float> stats;
  if (int rc = stat_row(cells, stat_coarse_id, stat_freq, n_stat, stats)) return rc;
  const std::vector<int64_t> ord = order_by_id(ids, N);
  std::vector<int32_t> sid = gather(ids, ord);
  const std::vector<int32_t> scell = gather(coarse_id, ord);
  const std::vector<int16_t> scodes = gather(codes, ord, (size_t)cb.m);
  std::vector<float> svec;
  const bool have_vecs = !s->norm.empty() && s->norm.d == d;
  if (have_vecs) {   // "INNER JOIN vecs ON fq.id = vecs.id" (ivpq_search_in.c:361-371)
    svec.resize((size_t)N * d);
    for (int64_t i = 0; i < N; ++i) {
      const float* v = s->norm.find(sid[i]);
      if (!v) return fail(-1, "id %d of fine_quantization_ivpq has no vector", sid[i]);
      memcpy(&svec[(size_t)i * d], v, sizeof(float) * d);
    }
  }
  freddy_ivpq_desc desc = {d, cb.m, cb.K, 2, cq.K, N, cb.dense.data(), cq.dense.data(), sid.data(), scell.data(),
                           scodes.data(), have_vecs ? svec.data() : nullptr, stats.data()};
  CodeTable& t = s->code[IVPQ];
  drop(t.h);
  if (int rc = freddy_gpu_pin_ivpq(&desc, s->device, &t.h)) return gpu_fail(rc);
  t.loaded(cb, std::move(sid));
  s->cq_multi = cq;
  return 0;
}

}  // extern "C"
