// join_host.h -- the host side of the multi-index traversal (index_utils.c:252-443): the reference's heap, pop by pop
// (join_select_cells), for the queries the device traversal does not decide -- more than 1024 cells, option
// join_host_traversal, equal keys, a stop the host's libm does not confirm -- and the worker pool that runs it.
#pragma once

#include "join_traverse.h"

namespace freddy {

struct JoinSide { float dist; int code; };
static_assert(sizeof(JoinSide) == 8, "side_sort_kernel writes JoinSide records");

// What side_sort_kernel produces for one query, on the host: its two sides in stable ascending order (equal distances keep
// their code order, index_utils.c:306-320) by the kernel's key -- the distance's bit pattern, then the code.
static inline void join_sort_sides_host(const float* sub, int Kc, JoinSide* out) {
  for (int sd = 0; sd < 2; ++sd, sub += Kc, out += Kc) {
    for (int c = 0; c < Kc; ++c) { out[c].dist = sub[c]; out[c].code = c; }
    std::stable_sort(out, out + Kc, [](const JoinSide& u, const JoinSide& v) {
      uint32_t ub, vb; memcpy(&ub, &u.dist, 4); memcpy(&vb, &v.dist, 4); return ub < vb; });
  }
}
struct JoinNode { float key; int cell, p0, p1; };

// per-query scratch reused between calls of one worker thread
struct JoinTraversal {
  std::vector<JoinNode> heap;
  std::vector<uint32_t> traversed, queued;
  std::vector<float> cell_dist;
};

// sides: the query's two sub-distance arrays stably sorted ascending (qsort + cmpTopKEntry,
// index_utils.c:104-116,317-319; stable as glibc <= 2.36).  Appends visited cells to `out`.
// Returns true iff the query exhausted every cell.
static inline bool join_select_cells(const JoinSide* s0, const JoinSide* s1, const float* d0, const float* d1, int Kc,
                                     const float* stats, int n_targets, int min_target, float confidence,
                                     JoinTraversal& w, std::vector<int32_t>& out) {
  const int cells = Kc * Kc;
  w.cell_dist.resize(cells);
  for (int c = 0; c < cells; ++c) {        // 0 + D0[c0] + D1[c1], index_utils.c:306-313
    float acc = 0;
    acc += d0[c % Kc];
    acc += d1[c / Kc];
    w.cell_dist[c] = acc;
  }
  w.traversed.assign(cells / 32 + 1, 0u);
  w.queued.assign(cells / 32 + 1, 0u);
  w.heap.resize(cells + 1);
  JoinNode* h = w.heap.data();
  int len = 1;
  h[0].p0 = 0; h[0].p1 = 0;
  h[0].cell = s0[0].code + Kc * s1[0].code;
  h[0].key = w.cell_dist[h[0].cell];
  float prob = 0.0f;
  int emitted = 0;
  const int stat_size = (int)stats[cells];
  auto push = [&](const JoinNode& nd) {     // index_utils.c:118-131
    int i = len, parent = (i - 1) / 2;
    while (i > 0 && h[parent].key > nd.key) { h[i] = h[parent]; i = parent; parent = (parent - 1) / 2; }
    h[i] = nd;
    ++len;
  };
  auto pop = [&]() {                        // index_utils.c:133-155
    JoinNode top = h[0];
    h[0] = h[len - 1];
    --len;
    const int n = len;
    int i = 0;
    while (i != n) {
      int pick = n;
      const int child = 1 + 2 * i;
      if (child <= n - 1 && h[child].key < h[pick].key) pick = child;
      if (child <= n - 1 && h[child + 1].key < h[pick].key) pick = child + 1;
      h[i] = h[pick];
      i = pick;
    }
    return top;
  };
  while (join_confidence_expr(min_target, n_targets, prob, stat_size) < confidence && emitted < cells) {
    const JoinNode cur = pop();
    const int here = cur.p0 + Kc * cur.p1;
    w.traversed[here / 32] |= 1u << (here % 32);
    int diag = cur.p0 + 1 + Kc * (cur.p1 - 1);
    if (cur.p0 < Kc - 1 && (cur.p1 == 0 || (w.traversed[diag / 32] & (1u << (diag % 32))))) {
      const int np0 = cur.p0 + 1, np1 = cur.p1, npi = np0 + Kc * np1;
      if (!(w.queued[npi / 32] & (1u << (npi % 32)))) {
        JoinNode nd; nd.p0 = np0; nd.p1 = np1; nd.cell = s0[np0].code + Kc * s1[np1].code; nd.key = w.cell_dist[nd.cell];
        push(nd);
        w.queued[npi / 32] |= 1u << (npi % 32);
      }
    }
    diag = cur.p0 - 1 + Kc * (cur.p1 + 1);
    if (cur.p1 < Kc - 1 && (cur.p0 == 0 || (w.traversed[diag / 32] & (1u << (diag % 32))))) {
      const int np0 = cur.p0, np1 = cur.p1 + 1, npi = np0 + Kc * np1;
      if (!(w.queued[npi / 32] & (1u << (npi % 32)))) {
        JoinNode nd; nd.p0 = np0; nd.p1 = np1; nd.cell = s0[np0].code + Kc * s1[np1].code; nd.key = w.cell_dist[nd.cell];
        push(nd);
        w.queued[npi / 32] |= 1u << (npi % 32);
      }
    }
    prob += stats[cur.cell];
    out.push_back(cur.cell);
    ++emitted;
  }
  return emitted >= cells;
}

// Host worker pool for the per-query traversals.  The workers are created on first use (never at
// library load, so a forking host stays safe) and parked on a condition variable; spawning threads per
// call cost ~1 ms per join_parallel_for on the GPU box (32 x std::thread), more than the work itself.
class JoinPool {
 public:
  static JoinPool& get() { static JoinPool p; return p; }
  int size() const { return (int)workers_.size(); }
  // runs fn(t) for t = 0..n_chunks-1 (n_chunks <= size()+1; chunk 0 runs on the caller)
  void run(int n_chunks, const std::function<void(int)>& fn) {
    if (n_chunks <= 1) { if (n_chunks == 1) fn(0); return; }
    {
      std::lock_guard<std::mutex> g(mu_);
      fn_ = &fn; chunks_ = n_chunks; pending_ = n_chunks - 1; ++generation_;
    }
    cv_.notify_all();
    fn(0);
    std::unique_lock<std::mutex> g(mu_);
    done_.wait(g, [&] { return pending_ == 0; });
    fn_ = nullptr;
  }
 private:
  JoinPool() {
    static const int cap = getenv("FREDDY_GPU_JOIN_THREADS") ? atoi(getenv("FREDDY_GPU_JOIN_THREADS")) : 32;
    const unsigned hw = std::thread::hardware_concurrency();
    const int n = std::max(0, (int)std::min<unsigned>(hw ? hw : 1, (unsigned)std::max(cap, 1)) - 1);
    for (int i = 0; i < n; ++i) workers_.emplace_back([this, i] { loop(i + 1); });
  }
  ~JoinPool() {
    { std::lock_guard<std::mutex> g(mu_); stop_ = true; ++generation_; }
    cv_.notify_all();
    for (auto& t : workers_) t.join();
  }
  void loop(int id) {
    unsigned long seen = 0;
    for (;;) {
      const std::function<void(int)>* fn = nullptr;
      {
        std::unique_lock<std::mutex> g(mu_);
        cv_.wait(g, [&] { return generation_ != seen; });
        seen = generation_;
        if (stop_) return;
        if (id < chunks_) fn = fn_;
      }
      if (fn) {
        (*fn)(id);
        std::lock_guard<std::mutex> g(mu_);
        if (--pending_ == 0) done_.notify_one();
      }
    }
  }
  std::vector<std::thread> workers_;
  std::mutex mu_;
  std::condition_variable cv_, done_;
  const std::function<void(int)>* fn_ = nullptr;
  int chunks_ = 0, pending_ = 0;
  unsigned long generation_ = 0;
  bool stop_ = false;
};

template <class F>
static inline void join_parallel_for(int n, F&& f) {
  if (n < 256) { f(0, n, 0); return; }
  JoinPool& pool = JoinPool::get();
  const int nt = std::min(pool.size() + 1, (n + 63) / 64);
  if (nt <= 1) { f(0, n, 0); return; }
  const int per = (n + nt - 1) / nt;
  const int chunks = (n + per - 1) / per;
  pool.run(chunks, [&](int t) {
    const int lo = t * per, hi = std::min(n, lo + per);
    if (lo < hi) f(lo, hi, t);
  });
}

}  // namespace freddy
