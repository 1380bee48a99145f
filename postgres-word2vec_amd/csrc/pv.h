// pv.h -- batched post verification (freddy--0.0.1.sql:556-662: k_nearest_neighbour_pq_pv / k_nearest_neighbour_ivfadc_pv): the
// k * pvf candidates an approximate search returned per query are re-ranked by cosine_similarity_bytea against the raw vectors
// and the first k kept.  Stage one is the public search itself (freddy_gpu_ivfadc_search / freddy_gpu_pq_search at k * pvf, every
// path of it); this header is stage two: one workgroup per query
//   1. resolves the query's candidate ids to rows of the vector handle (row_of_id over its ascending device ids; the
//      (-1, sentinel) fillers and ids without a row drop out -- and, for the approximate analogies of approx_analogy.h, the three
//      ids of PvArgs::exclude),
//   2. scores the rows: similarity = the binary32 chain "scalar += v1[i] * v2[i]", i ascending (core_functions.c:67-81), one lane
//      per candidate.  A wave takes 64 candidates at a time through dot_chain.h's gather tile, one tile per wave, and every lane
//      walks its own column against the query in LDS with the accumulator carried in a register across the steps (chain1),
//   3. sorts the keys (ordered similarity, row) -- exact.h's sim_key, the order of freddy_gpu_exact_search: similarity DESC,
//      id ASC -- and writes the first k as (id, similarity), (-1, -inf) beyond the rows.
// So a row of the result is bit for bit freddy_gpu_exact_search(vecs, q, 1, k, candidate ids of q).
//
// LDS budget per workgroup: P keys of 8 bytes (P = candidates padded to a power of two, <= 4096: 32 KiB) + waves x 8 320 B of tiles
// (4 waves: 32.5 KiB) + the query (d floats) -- 66 KiB at d = 300 with 4096 candidates, 2.2 KiB with up to 64 (one wave).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dot_chain.h"
#include "exact.h"
#include "wave_topk.h"

namespace freddy {

static constexpr int PV_MAX_CAND = 4096;   // k * pvf

struct PvArgs {
  const int32_t* cand;       // [Q][n_cand] stage one's ids (-1: filler)
  const int32_t* vec_ids;    // [N] ascending ids of the vector handle
  const float* rows;         // [N][d] its row-major copy
  const float* queries;      // [Q][d]
  const int32_t* exclude;    // aa_rerank_kernel only: [Q][3] ids that are no candidates of their query (approx_analogy.h: the analogy's inputs)
  int32_t* out_ids;          // [Q][k]
  float* out_sim;            // [Q][k]
  int32_t* counts;           // [Q][2]: candidates with id >= 0, and how many of them have a row (and are not excluded)
  int64_t N;
  int n_cand, k, d, P;       // P: n_cand padded to a power of two >= 64
};

static inline int pv_pad(int n) {
  int p = 64;
  while (p < n) p <<= 1;
  return p;
}
static inline size_t pv_lds_bytes(int NW, int P, int d) { return (size_t)P * sizeof(u64) + (size_t)NW * TILE_FLOATS * sizeof(float) + (size_t)d * sizeof(float); }

// NW = 1: up to 64 candidates, the sort is wave_sort64; NW = 4: up to 4096, a bitonic sort in LDS.  EX: PvArgs::exclude is read
// (a compile-time switch, so that the post-verification kernels below stay instruction for instruction what they were before the
// exclusion came: the three ids and their pointer cost scalar registers, and tests/golden/pv_codegen_ceilings.json pins those).
template <int NW, bool EX>
__device__ __forceinline__ void pv_rerank_body(const PvArgs& a) {
  constexpr int T = NW * 64;
  extern __shared__ __attribute__((aligned(16))) unsigned char pv_smem[];
  u64* keys = reinterpret_cast<u64*>(pv_smem);                              // [P]: the row of every candidate, then its key
  float* tiles = reinterpret_cast<float*>(keys + a.P);                      // [NW][TILE_DCH][TILE_STRIDE]
  float* qs = tiles + NW * TILE_FLOATS;                                     // [d]
  __shared__ int sh_cnt[2];
  __shared__ int32_t sh_ex[3];
  const int q = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int d = a.d, P = a.P;
  if (tid < 2) sh_cnt[tid] = 0;
  if constexpr (EX) {
    if (tid < 3) sh_ex[tid] = a.exclude[(size_t)q * 3 + tid];
  }
  __syncthreads();
  // 1. ids -> rows
  int32_t ex0 = -1, ex1 = -1, ex2 = -1;   // (-1: no candidate that gets this far is negative)
  if constexpr (EX) { ex0 = sh_ex[0]; ex1 = sh_ex[1]; ex2 = sh_ex[2]; }
  int n_ids = 0, n_rows = 0;
  for (int i = tid; i < P; i += T) {
    int32_t row = -1;
    if (i < a.n_cand) {
      const int32_t id = a.cand[(size_t)q * a.n_cand + i];
      if (id >= 0) ++n_ids;
      if (id >= 0 && id != ex0 && id != ex1 && id != ex2) {
        const int32_t r = row_of_id(a.vec_ids, a.N, id);
        if (r >= 0) { row = r; ++n_rows; }
      }
    }
    keys[i] = (u64)(uint32_t)row;
  }
  if (n_ids) atomicAdd(&sh_cnt[0], n_ids);
  if (n_rows) atomicAdd(&sh_cnt[1], n_rows);
  for (int i = tid; i < d; i += T) qs[i] = a.queries[(size_t)q * d + i];
  __syncthreads();
  // 2. similarities: wave `wave` takes the candidates [64 g, 64 g + 64), g = wave, wave + NW, ...
  float* tile = tiles + wave * TILE_FLOATS;
  const bool vec4 = (d & 3) == 0;
  for (int g = wave; g < P / 64; g += NW) {
    const int c = g * 64 + lane;
    const int32_t row = (int32_t)(uint32_t)keys[c];
    if (__ballot(row >= 0) == 0ull) { keys[c] = KEY_INF; continue; }
    float acc = 0.0f;
    for (int c0 = 0; c0 < d; c0 += TILE_DCH) {
      const int nd = (d - c0 < TILE_DCH) ? d - c0 : TILE_DCH;
      float4 v[8];
#pragma unroll
      for (int it = 0; it < 8; ++it) v[it] = tile_row_piece(a.rows, row, it, lane, d, c0, nd, vec4);
#pragma unroll
      for (int it = 0; it < 8; ++it) tile_store_row_piece(tile, v[it], it, lane);
      wave_lds_sync();
      chain1<1, TILE_STRIDE>(acc, qs + c0, tile + lane, nd);   // v1: the query
      wave_lds_sync();
    }
    keys[c] = row >= 0 ? sim_key(acc, (uint32_t)row) : KEY_INF;
  }
  __syncthreads();
  // 3. order: similarity DESC, row ASC (keys are unique: a stage-one list holds an id once)
  if constexpr (NW == 1) {
    const u64 key = wave_sort64(keys[lane]);
    if (lane < a.k) {
      a.out_ids[(size_t)q * a.k + lane] = key == KEY_INF ? -1 : a.vec_ids[key_pos(key)];
      a.out_sim[(size_t)q * a.k + lane] = key == KEY_INF ? -__builtin_huge_valf() : key_sim(key);
    }
  } else {
    for (int size = 2; size <= P; size <<= 1) {
      for (int stride = size >> 1; stride > 0; stride >>= 1) {
        for (int t = tid; t < (P >> 1); t += T) {
          const int lo = 2 * t - (t & (stride - 1));
          const int hi = lo + stride;
          const bool up = (lo & size) == 0;
          const u64 u = keys[lo], w = keys[hi];
          if ((u > w) == up) { keys[lo] = w; keys[hi] = u; }
        }
        __syncthreads();
      }
    }
    for (int r = tid; r < a.k; r += T) {
      const u64 key = keys[r];
      a.out_ids[(size_t)q * a.k + r] = key == KEY_INF ? -1 : a.vec_ids[key_pos(key)];
      a.out_sim[(size_t)q * a.k + r] = key == KEY_INF ? -__builtin_huge_valf() : key_sim(key);
    }
  }
  if (tid < 2) a.counts[(size_t)q * 2 + tid] = sh_cnt[tid];
}

template <int NW>
__global__ __launch_bounds__(NW * 64) void pv_rerank_kernel(PvArgs a) { pv_rerank_body<NW, false>(a); }
// the re-rank of the approximate analogies (approx_analogy.h): a.exclude[q] holds the three input ids of query q
template <int NW>
__global__ __launch_bounds__(NW * 64) void aa_rerank_kernel(PvArgs a) { pv_rerank_body<NW, true>(a); }

}  // namespace freddy
