// cluster.h -- cluster_exact / cluster_pq / cluster_ivpq = generic_cluster (freddy--0.0.1.sql:1086-1209): the reference's plpgsql
// k-means.  cluster_exact and cluster_pq are ONE device call (freddy_gpu_cluster: the ten rounds stay in HBM); cluster_ivpq keeps the
// loop below with its assignment from the kNN-join's lists.  Included by freddy_udf.cpp only, after similarity_of.
#pragma once
#include <cmath>

#include "session.h"

namespace {
struct SimRow { float sim; int qid; int tid; };
}

// The ABI version did not move with freddy_gpu_cluster (no struct grew, no entry point changed meaning), so this mirror may be loaded
// beside a library that does not have it yet: the symbol is bound weakly, and without it the loop around the two assign calls runs.
extern "C" int freddy_gpu_cluster(freddy_gpu_index_t*, freddy_gpu_index_t*, float, const int32_t*, int64_t, int32_t, int32_t, const double*, int64_t,
                                  int32_t*, float*, float*) __attribute__((weak));

// cluster_ivpq: (query, target, similarity) rows of knn_in_ivpq_batch (bytea[] overload: query = 1-based centroid index) for
// k = all tokens; target as 1-based token index.  Its lists are the kNN-join's approximation, not "all tokens", so the rows
// themselves are needed; cluster_exact and cluster_pq take cluster_assign below.
static int cluster_knn(freddy_session_t* s, const std::vector<float>& centroids, int kc, const int32_t* token_ids, int n,
                       std::vector<SimRow>& rows) {
  rows.clear();
  std::vector<int32_t> ids((size_t)kc * n); std::vector<float> val((size_t)kc * n);
  // ivpq_search_in through knn_in_iv_batch (:754-795)
  if (!s->code[IVPQ].h) return fail(-1, "%s", kNotLoaded[IVPQ]);
  REQUIRE(session_knn_join(s, centroids.data(), kc, n, token_ids, n, ids.data(), val.data()));
  // token id -> 1-based token index (INNER JOIN unnest(token_ids, tokens) ON token = target; duplicates: every index)
  std::vector<std::pair<int32_t, int>> by_id((size_t)n);
  for (int i = 0; i < n; ++i) by_id[(size_t)i] = {token_ids[i], i + 1};
  std::sort(by_id.begin(), by_id.end());
  for (int qi = 0; qi < kc; ++qi)
    for (int r = 0; r < n; ++r) {
      const int32_t id = ids[(size_t)qi * n + r];
      if (id < 0) continue;   // the joins drop the (-1, sentinel) filler rows
      const float sim = similarity_of(val[(size_t)qi * n + r]);
      auto it = std::lower_bound(by_id.begin(), by_id.end(), std::make_pair(id, 0));
      for (; it != by_id.end() && it->first == id; ++it) rows.push_back({sim, qi + 1, it->second});
    }
  // ORDER BY similarity DESC (ties are unspecified in SQL: query, then token position)
  std::stable_sort(rows.begin(), rows.end(), [](const SimRow& a, const SimRow& b) {
    if (a.sim != b.sim) return a.sim > b.sim;
    if (a.qid != b.qid) return a.qid < b.qid;
    return a.tid < b.tid;
  });
  return 0;
}

// cluster_exact (method 0) and cluster_pq (method 1): what the loop over such sorted rows of ALL tokens keeps -- per token the first
// centroid under "similarity DESC, centroid ASC" -- straight from the device (freddy_gpu_exact_assign / freddy_gpu_pq_assign, csrc/assign.h), for any n.
// best[i] = 0-based centroid of token i, -1: no centroid lists it.
static int cluster_assign(freddy_session_t* s, int method, const std::vector<float>& centroids, int kc, const int32_t* token_ids, int n,
                          std::vector<int32_t>& best, std::vector<float>& sim) {
  best.resize((size_t)n); sim.resize((size_t)n);
  if (method == 0) {   // knn_search_in_batch (freddy--0.0.1.sql:480-501)
    if (int rc = s->norm.pinned(s->device)) return rc;
    if (int rc = freddy_gpu_exact_assign(s->norm.h, centroids.data(), kc, token_ids, n, best.data(), sim.data())) return gpu_fail(rc);
  } else {             // knn_in_pq_batch over pq_search_in_batch (:846-867)
    if (!s->code[PQ].h) return fail(-1, "%s", kNotLoaded[PQ]);
    if (int rc = freddy_gpu_pq_assign(s->code[PQ].h, centroids.data(), kc, 1000.0f, token_ids, n, best.data(), sim.data())) return gpu_fail(rc);
  }
  return 0;
}

static int generic_cluster(freddy_session_t* s, int method, const int32_t* token_ids, int32_t n, int32_t k, const double* draws,
                           int32_t n_draws, int32_t* cluster_out) {
  if (!s || !token_ids || n <= 0 || k <= 0 || !cluster_out) return fail(-1, "bad argument");
  if (s->norm.empty()) return fail(-1, "google_vecs_norm is not loaded");
  const int d = s->norm.d;
  int used = 0;
  uint64_t state = 0x9E3779B97F4A7C15ull;
  auto rnd = [&]() -> double {   // random(): the caller's sequence first (reproducible runs), then an xorshift
    if (draws && used < n_draws) return draws[used++];
    state ^= state << 13; state ^= state >> 7; state ^= state << 17;
    return (double)(state >> 11) / 9007199254740992.0;
  };
  auto pick = [&](int upper) -> int {   // round(random() * upper + 0.5): 1..upper
    const int v = (int)std::nearbyint(rnd() * upper + 0.5);   // float8 round() is rint()
    return v < 1 ? 1 : (v > upper ? upper : v);
  };
  if (method != 2 && freddy_gpu_cluster) {   // the whole k-means on the device: the draw sequence in full, then one call
    if (int rc = s->norm.pinned(s->device)) return rc;
    if (method == 1 && !s->code[PQ].h) return fail(-1, "%s", kNotLoaded[PQ]);
    std::vector<double> all((size_t)k + (size_t)90 * k);
    for (double& r : all) r = rnd();
    if (int rc = freddy_gpu_cluster(s->norm.h, method == 1 ? s->code[PQ].h : nullptr, 1000.0f, token_ids, n, k, 10, all.data(), (int64_t)all.size(),
                                    cluster_out, nullptr, nullptr))
      return gpu_fail(rc);
    return 0;
  }
  std::vector<const float*> tok((size_t)n);
  for (int i = 0; i < n; ++i) {
    tok[(size_t)i] = s->norm.find(token_ids[i]);
    if (!tok[(size_t)i]) return fail(-1, "token id %d has no vector", token_ids[i]);
  }
  std::vector<float> centroids((size_t)k * d);
  std::vector<int> clusters((size_t)n, 0), lens((size_t)k, 0);
  std::vector<char> processed((size_t)n, 0);
  for (int I = 0; I < k; ++I) memcpy(&centroids[(size_t)I * d], tok[(size_t)pick(n) - 1], sizeof(float) * d);   // :1107-1112
  std::vector<SimRow> rows;
  std::vector<int32_t> best;
  std::vector<float> best_sim;
  for (int J = 1; J <= 10; ++J) {                                                                                  // :1114
    if (method == 2) {
      if (int rc = cluster_knn(s, centroids, k, token_ids, n, rows)) return rc;
      for (const SimRow& r : rows)                                                                                 // :1122-1128
        if (!processed[(size_t)r.tid - 1]) {
          clusters[(size_t)r.tid - 1] = r.qid;
          lens[(size_t)r.qid - 1] += 1;
          processed[(size_t)r.tid - 1] = 1;
        }
    } else {   // the first row of every token, from the device; a token no centroid lists keeps its cluster
      if (int rc = cluster_assign(s, method, centroids, k, token_ids, n, best, best_sim)) return rc;
      for (int i = 0; i < n; ++i)
        if (best[(size_t)i] >= 0) {
          clusters[(size_t)i] = best[(size_t)i] + 1;
          lens[(size_t)best[(size_t)i]] += 1;
          processed[(size_t)i] = 1;
        }
    }
    if (J < 10) {
      for (int I = 1; I <= k; ++I) {                                                                               // :1131-1156
        if (lens[(size_t)I - 1] == 0) {
          for (int t = 0; t < 10; ++t) (void)pick(n);   // ten samples are drawn and thrown away: the centroid keeps its value (:1133-1142)
        } else {
          std::vector<int> members;   // tokens of cluster I, in token order
          for (int i = 0; i < n; ++i) if (clusters[(size_t)i] == I) members.push_back(i);
          const int len = lens[(size_t)I - 1];
          std::vector<const float*> samples;
          for (int t = 0; t < 10; ++t) {   // r.x INNER JOIN x.id: ten draws with replacement (draws beyond the members vanish)
            const int x = pick(len);
            if (x <= (int)members.size()) samples.push_back(tok[(size_t)members[(size_t)x - 1]]);
          }
          if (!samples.empty()) {   // centroid_bytea: output[j] += data[i][j] / (float) n   core_functions.c:371-379
            float* c = &centroids[(size_t)(I - 1) * d];
            for (int j = 0; j < d; ++j) c[j] = 0;
            for (size_t i = 0; i < samples.size(); ++i)
              for (int j = 0; j < d; ++j) c[j] += samples[i][j] / (float)samples.size();
          }
          lens[(size_t)I - 1] = 0;
        }
      }
      std::fill(processed.begin(), processed.end(), 0);                                                            // :1158-1160
    }
  }
  for (int i = 0; i < n; ++i) cluster_out[i] = clusters[(size_t)i];
  return 0;
}
