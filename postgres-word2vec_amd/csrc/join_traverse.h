// join_traverse.h -- the multi-index traversal on the device (join_traverse_kernel, TravArgs) and the confidence expression it
// shares with the host heap (join_host.h) and the host's check of the stops it proposes (join_run.h).
#pragma once

#include "join_kernels.h"

namespace freddy {

// ---------------------------------------------------------------------------------------
// device: a10 multi-index traversal for <= 1024 cells             index_utils.c:252-443
// ---------------------------------------------------------------------------------------
// getConfidenceHyp (index_utils.c:673-682) with the reference's types: float variables, double sub-expressions.
// One text for both sides: the host heap and the host's check of a proposed stop evaluate it with the host's libm, and the
// device's erf is not glibc's bit for bit -- which is why the host re-evaluates the expression at the proposed stop.
__host__ __device__ __forceinline__ float join_confidence_expr(int expect, int size, float p, int stat_size) {
  if (expect > size) return 0;
  float mu = size * p;
  float sig = sqrt(size * p * (1.0 - p)) * (((float)stat_size - size) / ((float)stat_size - 1.0));
  return 1.0 - 0.5 * (1.0 + erf((((float)expect) - 0.5 - mu) / (sig * sqrt(2.0))));
}

static constexpr int TRAV_SUM_DW = 8;   // per query: n, cells with targets, target rows, flags (1 tie, 2 exhausted), bits(P_n), bits(P_{n-1})
struct TravArgs {
  const float* sub;          // [Q][2][Kc]
  const int32_t* active;     // [n_active]
  const float* stats;        // [cells+1]
  const int32_t* tcell_off;  // [cells+1]
  int32_t* qcells;           // [Q][cells]: the taken cells that hold targets, in the order they are taken
  int32_t* qcell_cnt;        // [Q]
  int32_t* summary;          // [n_active][TRAV_SUM_DW]
  float* fb_sub;             // [n_active][2 * Kc] or NULL: the sub-distances of a query that is handed to the host (mapped host memory)
  int Kc, cells, n_targets, min_target;
  float confidence;
};

// One wave per query.  Most queries take a few dozen cells: the 64 smallest keys come from a streaming selection
// (WaveSelect) and decide the stop; only a query that needs more than 63 cells sorts all of them -- a bitonic sort in LDS
// with ROLLED loops: the fully unrolled register sort of 1024 keys is ~100 KB of straight-line code that every wave
// streamed through the 64 KB instruction cache once (380 us per launch for 5 000 queries, as long as the join itself).
// SMALL: only the smallest keys are ever held (1.5 instead of 17 KB of LDS for 1024 cells), found with ONE sort + merge (below);
// a query whose stop is not among them (at least its 31 nearest cells) is handed to the host heap like one with equal keys
// (flag 1).  The host picks SMALL when the expected number of cells is far below that.
template <int V, bool SMALL = false>
__global__ __launch_bounds__(64) void join_traverse_kernel(TravArgs a) {
  constexpr int NS = SMALL ? 64 : 64 * V;
  __shared__ u64 s_key[NS];            // (distance bits << 32) | cell, ascending from index 0 as far as they are sorted
  __shared__ float s_stat[NS];
  __shared__ float s_P[NS + 1];
  __shared__ u64 s_stage[64];
  const int lane = threadIdx.x, x = blockIdx.x;
  const int q = a.active[x];
  const int Kc = a.Kc, cells = a.cells;
  const float* d0 = a.sub + ((size_t)q * 2) * Kc;
  const float* d1 = d0 + Kc;
  auto cell_key = [&](int c) -> u64 {
    if (c >= cells) return KEY_INF;
    float acc = 0;            // 0 + D0[c0] + D1[c1], index_utils.c:306-313
    acc += d0[c % Kc];
    acc += d1[c / Kc];
    return make_key(acc, (uint32_t)c);
  };
  const int stat_size = (int)a.stats[cells];
  // ---- the 64 smallest keys, ascending
  int n_valid = 64;   // SMALL: how many of them are known to be the smallest (>= 32)
  if constexpr (SMALL) {
    // The kernel is bound by instruction issue (5 000 lone waves), and a streaming selection that starts without a threshold
    // pays a 64-bit sort + merge for every other batch of 64 keys.  Here: the lane's V keys stay in registers, the 32nd
    // smallest of the 64 lane minima (one 32-bit sort) bounds the 32nd smallest key, only keys up to it are offered (about
    // 40 of 1024): one sort + merge.  Every key below the bound is in the result, so its first n_valid entries are exactly the
    // n_valid smallest keys; a stop beyond them is handed to the host.
    u64 kk[V];
    uint32_t mn = 0xffffffffu;
#pragma unroll
    for (int v = 0; v < V; ++v) { kk[v] = cell_key(v * 64 + lane); mn = min(mn, (uint32_t)(kk[v] >> 32)); }
    const uint32_t dL = (uint32_t)__builtin_amdgcn_readlane((int)wave_sort32(mn), 31);
    WaveSelect<1> sel;
    sel.init(s_stage, ((u64)dL << 32) | 0xffffffffull, 64);
#pragma unroll
    for (int v = 0; v < V; ++v) sel.push(kk[v], kk[v] != KEY_INF);
    sel.finish();
    n_valid = (int)__popcll(__ballot(sel.acc[0] != KEY_INF));
    s_key[lane] = sel.acc[0];
    s_stat[lane] = (sel.acc[0] != KEY_INF) ? a.stats[key_pos(sel.acc[0])] : 0.0f;
  } else {
    WaveSelect<1> sel;
    sel.init(s_stage, KEY_INF, 64);
#pragma unroll 1
    for (int v = 0; v < V; ++v) {
      const u64 kk = cell_key(v * 64 + lane);
      sel.push(kk, kk != KEY_INF);
    }
    sel.finish();
    s_key[lane] = sel.acc[0];
    s_stat[lane] = (sel.acc[0] != KEY_INF) ? a.stats[key_pos(sel.acc[0])] : 0.0f;
  }
  if (lane == 0) s_P[0] = 0.0f;
  __syncthreads();
  // n = the first count whose confidence reaches the threshold ("while (conf(prob) < confidence && emitted < cells)"):
  // lane 0 extends the running sum by a chunk of 64 cells (prob += statistics[cell], :424, sequential binary32 adds),
  // then the 64 lanes test the chunk's 64 counts
  int n = cells;
  bool sorted_all = (V == 1);
  bool beyond = false;   // SMALL: the stop is not among the first 63 cells
  for (int base = 0; base < cells; base += 64) {
    if constexpr (SMALL) { if (base > 0) { beyond = true; n = 0; break; } }
    if (base > 0 && !sorted_all) {
     if constexpr (!SMALL) {
      // more than 63 cells: every key, sorted (rolled bitonic network over LDS; 64 V is a power of two)
#pragma unroll 1
      for (int v = 0; v < V; ++v) s_key[v * 64 + lane] = cell_key(v * 64 + lane);
      __syncthreads();
#pragma unroll 1
      for (int k = 2; k <= 64 * V; k <<= 1) {
#pragma unroll 1
        for (int j = k >> 1; j > 0; j >>= 1) {
#pragma unroll 1
          for (int t = lane; t < 32 * V; t += 64) {
            const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
            const int l = i | j;
            const u64 lo = s_key[i], hi = s_key[l];
            const bool up = (i & k) == 0;
            if ((lo > hi) == up) { s_key[i] = hi; s_key[l] = lo; }
          }
          __syncthreads();
        }
      }
#pragma unroll 1
      for (int v = 0; v < V; ++v) {
        const u64 kk = s_key[v * 64 + lane];
        s_stat[v * 64 + lane] = (kk != KEY_INF) ? a.stats[key_pos(kk)] : 0.0f;
      }
      sorted_all = true;
      __syncthreads();
     }
    }
    if (lane == 0) {
      float P = s_P[base];
      const int hi = base + 64 < cells ? base + 64 : cells;
      for (int i = base; i < hi; ++i) { P = P + s_stat[i]; s_P[i + 1] = P; }
    }
    __syncthreads();
    const int cnt = base + lane;
    const bool ok = cnt < cells && (!SMALL || cnt + 1 < n_valid) && !(join_confidence_expr(a.min_target, a.n_targets, s_P[cnt < cells ? cnt : 0], stat_size) < a.confidence);
    const u64 m = __ballot(ok);
    if (m != 0ull) { n = base + (int)__builtin_ctzll(m); break; }
  }
  // (n <= 63 when only the 64 smallest keys are sorted; n == cells needs all of them)
  // equal keys among the first n + 1 sorted cells: the heap's order is history-dependent there -> the host decides
  bool tie = false;
  for (int i = lane; i < n && i + 1 < cells; i += 64) tie = tie || ((uint32_t)(s_key[i] >> 32) == (uint32_t)(s_key[i + 1] >> 32));
  const bool any_tie = __ballot(tie) != 0ull;
  // the taken cells that hold targets, compacted in order; their rows
  int n_keep = 0, rows = 0;
  int32_t* dst = a.qcells + (size_t)q * cells;
  for (int base = 0; base < n; base += 64) {
    const int i = base + lane;
    int tc = 0, c = 0;
    if (i < n) { c = (int)key_pos(s_key[i]); tc = a.tcell_off[c + 1] - a.tcell_off[c]; }
    const u64 m = __ballot(tc > 0);
    if (tc > 0) dst[n_keep + lanes_below(m)] = c;
    n_keep += (int)__popcll(m);
    rows += tc;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) rows += __shfl_xor(rows, o, 64);
  // a query the host heap has to traverse: its 2 x Kc sub-distances go along with the summary (the host sorts the two sides
  // itself: a side-sort kernel, two small copies and a synchronisation per handed-back query cost 0.05 - 0.08 ms per call)
  if ((any_tie || beyond) && a.fb_sub)
    for (int i = lane; i < 2 * Kc; i += 64) a.fb_sub[(size_t)x * 2 * Kc + i] = d0[i];
  if (lane == 0) {
    a.qcell_cnt[q] = n_keep;
    int32_t* sm = a.summary + (size_t)x * TRAV_SUM_DW;
    sm[0] = n; sm[1] = n_keep; sm[2] = rows; sm[3] = ((any_tie || beyond) ? 1 : 0) | (n >= cells ? 2 : 0);
    sm[4] = (int32_t)__float_as_uint(s_P[n]);
    sm[5] = (int32_t)__float_as_uint(n > 0 ? s_P[n - 1] : 0.0f);
    // the device's own values of the expression at the stop and one step before it: the host re-evaluates with its
    // libm only where one of them is within 1e-5 of the confidence (the arguments of erf are IEEE-identical on both
    // sides -- float / double products, correctly rounded sqrt and division -- and the two erf implementations differ
    // by a few units in the last place of a double)
    sm[6] = (int32_t)__float_as_uint(join_confidence_expr(a.min_target, a.n_targets, s_P[n], stat_size));
    sm[7] = (int32_t)__float_as_uint(n > 0 ? join_confidence_expr(a.min_target, a.n_targets, s_P[n - 1], stat_size) : 0.0f);
  }
}

}  // namespace freddy
