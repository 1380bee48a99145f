// join_index.h -- the pinned ivpq index (JoinIndex), its workspaces and error buffer: what the handle holds.  The kNN-join
// itself: join.h (overview), join_kernels.h, join_traverse.h, join_host.h, join_run.h.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include <condition_variable>
#include <functional>
#include <mutex>
#include <stdint.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#include "../../include/freddy_gpu.h"
#include "pinned.h"
#include "wave_topk.h"

namespace freddy {

static constexpr float JOIN_MAX_DIST = 1000.0f;   // ivpq_search_in.c:62
static constexpr int JOIN_CELL_CHUNK = 256;    // cells of a query whose target rows are laid out as ONE index space at a time
static constexpr int JOIN_WG = 256;
static constexpr int JOIN_WAVES = JOIN_WG / 64;

static thread_local char g_join_err[384] = "";
static inline const char* join_error() { return g_join_err; }
static inline int join_fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_join_err, sizeof(g_join_err), fmt, ap);
  va_end(ap);
  return code;
}
#define JOIN_HIP(expr)                                                                          \
  do {                                                                                          \
    hipError_t e_ = (expr);                                                                     \
    if (e_ != hipSuccess)                                                                       \
      return join_fail(e_ == hipErrorOutOfMemory ? FREDDY_E_NOMEM : FREDDY_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)

// The device workspaces of a call (JoinIndex::w), grown on demand and kept between calls.  Every one is a buffer of its own:
// JW_SCAN and JW_ACTIVE, JW_QCELLS and JW_QCELLS_FLAT are live at the same time in stream order.
enum JoinSlot {
  JW_QUERIES,      // float [Q][d]        the queries
  JW_SUB,          // float [Q][2][Kc]    their sub-distances to the multi-index centroids
  JW_TCELL_OFF,    // int32 [cells + 1]   target buckets by cell   } kept for the next call with the same target array
  JW_TROW,         // int32 [n_targets]   target rows by bucket    } (JoinIndex::tl_valid)
  JW_SCAN,         // int32 [Q]           the round's scan list (before it: the `only` list of a partial side sort)
  JW_QCELL_OFF,    // int32 [Q + 1]       host-traversed queries: offsets into JW_QCELLS_FLAT
  JW_QCELLS_FLAT,  // int32               host-traversed queries: their cells, back to back
  JW_WIN,          // int32 [n_targets]   mark kernel: the row a target id won (-1: unknown or duplicate)
  JW_CELL_CNT,     // int32 [2][cells]    targets per cell, fill cursors of the place kernel
  JW_SORTED,       // JoinSide [Q][2][Kc] the sides in stable ascending order (host heap)
  JW_ACTIVE,       // int32 [Q]           the round's active list
  JW_QCELLS,       // int32 [Q][cells]    device traversal: row q = the cells query q takes
  JW_QCELL_CNT,    // int32 [Q]           device traversal: how many
  JW_BIG_KEYS,     // u64   [n_scan][L]   BIG: the candidates (post verification's, or the 2k keys of methods 0 / 1) ...
  JW_BIG_EXACT,    // float [n_scan][L]   ... and, for post verification, their exact distances
  JW_STAT,         // u64 [cells] + float [cells + 1]   create_statistics: the counts per cell, then the row they give
  JW_SLOTS
};

struct JoinIndex {
  int d = 0, m = 0, K = 0, S = 0, Kc = 0, cells = 0;
  int MP = 0;                 // pitch of a code row in int16: m rounded up to a multiple of 8 (16-byte aligned rows, zero padded)
  int64_t N = 0;
  bool has_vectors = false;
  // device
  float* cbT = nullptr;       // [m][S][K]
  float* coarseT = nullptr;   // [2][d/2][Kc]
  int32_t* ids = nullptr;     // [N]
  int16_t* codes = nullptr;   // [N][MP] -- a lane fetches a row with 16-byte loads
  float* vectors = nullptr;   // [N][d]
  int32_t* cell = nullptr;    // [N] coarse cell of each row
  uint32_t* markbits = nullptr;  // [ceil(N/32)] scratch bitmap of the "id IN (targets)" resolution
  float* d_stats = nullptr;      // [cells+1] the statistics row (device traversal)
  PinnedBuf h_q;                 // staging of the query batch (read by a copy kernel: no SDMA ordering hops)
  PinnedBuf h_sum;               // per-round traversal summaries and result lists come back here
  // host
  std::vector<int32_t> h_ids, h_cell;
  std::vector<float> h_stats;
  bool ids_affine = false;       // ids[r] == ids[0] + r: O(1) id -> row
  // "fq.id IN (targets)" of the previous call: the same target array (compared word for word) finds its rows resolved,
  // de-duplicated and bucketed by cell already (JW_TCELL_OFF and JW_TROW stay as they are); invalidated when rows are appended
  // (kept in ONE pinned block: [cells + 1] bucket offsets, written by the offsets kernel, then the target array, which the mark
  // kernel reads over PCIe -- no SDMA copy in either direction, and the copy the next call is compared with is the staging copy)
  PinnedBuf h_tl;
  // create_statistics: [cells + 1] floats and the exact total as the finish kernel writes them, then two halves of a pass of
  // ids each (the count kernel reads a half over PCIe while the host fills the other); an event per half
  PinnedBuf h_stat;
  hipEvent_t ev_stat[2] = {nullptr, nullptr};
  int64_t tl_n = -1;
  int tl_cells = -1;
  bool tl_valid = false;
  // workspaces
  void* w[JW_SLOTS] = {nullptr};
  size_t wcap[JW_SLOTS] = {0};
  float libm_margin = 1e-5f;     // option join_libm_margin_ppm: device confidences this close to the threshold are re-evaluated by the host's libm
  bool front_gather = true;      // option join_front_gather: a join by row id gathers its queries in the sub-distance launch (sub_dist_rows_kernel); 0 = query_gather_kernel, then sub_dist_kernel
  bool host_traversal = false;   // option join_host_traversal / FREDDY_GPU_JOIN_HOST_TRAVERSAL: every traversal on the host heap
  // stage timers of the last call under the reference's TRACK names (ivpq_search_in.c:234-697)
  freddy_track track;
  hipEvent_t ev0 = nullptr, ev1 = nullptr, ev_replay = nullptr;   // around the join launches; in front of the replay launch
};

template <class T>
static inline int join_buf(JoinIndex* j, JoinSlot slot, size_t count, T** out) {
  const size_t bytes = sizeof(T) * count;
  if (bytes > j->wcap[slot]) {
    if (j->w[slot]) (void)dev_free(j->w[slot]);
    j->w[slot] = nullptr;
    j->wcap[slot] = 0;
    size_t want = bytes + bytes / 4 + 256;
    if (dev_malloc(&j->w[slot], want) != hipSuccess) return join_fail(FREDDY_E_NOMEM, "workspace allocation of %zu bytes failed", want);
    j->wcap[slot] = want;
  }
  *out = static_cast<T*>(j->w[slot]);
  return 0;
}

static inline void join_free(JoinIndex* j) {
  void* ptrs[] = {j->cbT, j->coarseT, j->ids, j->codes, j->vectors, j->cell, j->markbits, j->d_stats};
  for (void* p : ptrs) if (p) (void)dev_free(p);
  for (PinnedBuf* b : {&j->h_q, &j->h_sum, &j->h_tl, &j->h_stat}) b->release();
  for (int i = 0; i < JW_SLOTS; ++i) if (j->w[i]) (void)dev_free(j->w[i]);
  if (j->ev0) (void)hipEventDestroy(j->ev0);
  if (j->ev1) (void)hipEventDestroy(j->ev1);
  if (j->ev_replay) (void)hipEventDestroy(j->ev_replay);
  for (hipEvent_t e : j->ev_stat) if (e) (void)hipEventDestroy(e);
  *j = JoinIndex();
}

static inline std::vector<int16_t> join_pad_codes(const int16_t* codes, int64_t n, int m, int MP) {
  std::vector<int16_t> out((size_t)std::max<int64_t>(n, 1) * MP, 0);
  for (int64_t r = 0; r < n; ++r) memcpy(&out[(size_t)r * MP], codes + (size_t)r * m, sizeof(int16_t) * m);
  return out;
}

}  // namespace freddy
