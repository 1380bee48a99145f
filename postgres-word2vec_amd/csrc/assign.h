// assign.h -- the assignment step of cluster_exact / cluster_pq (generic_cluster, freddy--0.0.1.sql:1086-1209): "every token goes
// to the centroid that lists it with the highest similarity" (:1115-1127) is, per token, an argmax over the centroids.  The SQL
// asks the kNN-join for a list of ALL n tokens per centroid (k = n), sorts the kc * n rows by similarity DESC and keeps the first
// row of every token; these kernels compute what that keeps -- one (centroid index, similarity) per token -- for any n:
//
//   assign_exact_kernel  (freddy_gpu_exact_assign, rows of knn_search_in_batch :480-501): similarity = the binary32 chain
//       "scalar += v1[i] * v2[i]", i ascending (core_functions.c:67-81), first under "similarity DESC (PostgreSQL's float4 order: a
//       NaN above every number, all NaNs equal), query index ASC".
//   assign_pq_kernel     (freddy_gpu_pq_assign, rows of pq_search_in_batch as knn_in_pq_batch :846-867 reads them): the ADC
//       distance of freddy_gpu_pq_search (LUT entry = squareDistance, index_utils.c:445-455, positions summed in order), a
//       candidate iff distance < sentinel, key = freddy_similarity_of(distance) (include/freddy_similarity.h: the SRF's "%f" round
//       trip, then 1 - y / 2), first under "key DESC, query index ASC".
//
// assign_exact_kernel: one lane per target, one wave per workgroup (64 targets; the waves share nothing, so nothing is gained by
// larger workgroups and a small set still spreads over n / 64 CUs).  Ids are resolved by row_of_id.  The rows are a gather of 4 d-byte
// rows: dot_chain.h's gather tile with its tile of 16 queries beside it, all ten loads of a step issued before the first store.
// LDS: 8 320 B + 2 048 B = 10 368 B static per workgroup of one wave (15 waves per CU by LDS); registers: 16 accumulators + 8
// float4 of row pieces + 2 of query pieces in flight.  No workgroup reads what another wrote.
//
// assign_pq_kernel: grouping_kernel's shape (kernels.h).  A workgroup of 256 threads owns RPT * 256 targets, one or four per
// thread, their code dwords in registers (M2 = 6: m = 12; M2 = 0: any m, the codes re-read per query), and walks the queries'
// LUTs (lut_build, the search's own entries), staging LT of them at a time in LDS (LT * m * K * 4 bytes: as many as fit 64 KiB,
// at least one -- a single LUT may take up to 156 KiB, check_pq_shape).  Per (target, query): the sum, then "dist < best distance
// so far" (which starts at the sentinel, so it is the sentinel test too); only then the key is computed and compared.  That skips
// no winner: freddy_similarity_of is monotone (a distance that is not smaller has a key that is not larger) and the queries come
// in ascending order, so a later query wins only with a strictly larger key, which needs a strictly smaller distance.  The state
// (best key, its query, the smallest distance) lives in out_sim / out_query / best_dist between the launches of a call whose LUTs
// do not fit the workspace at once.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dot_chain.h"
#include "freddy_similarity.h"

namespace freddy {

static constexpr int AS_MAX_Q = 65536;     // queries per assign call
static constexpr int AS_PQ_WG = 256;

// PostgreSQL's float4 order as an unsigned number: ascending with the float, every NaN the one largest value; never 0
__device__ __forceinline__ uint32_t assign_ord(float sim) {
  const uint32_t b = __float_as_uint(sim);
  if ((b & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

struct AssignExactArgs {
  const int32_t* targets;    // [n_targets] ids
  const int32_t* vec_ids;    // [N] ascending ids of the vector handle
  const float* rows;         // [N][d] its row-major copy
  const float* queries;      // [Q][d]
  int32_t* out_query;        // [n_targets]
  float* out_sim;            // [n_targets]
  int64_t N;
  int n_targets, Q, d;
};

// (static: the header is included by several units, cluster.hip launches it)
static __global__ __launch_bounds__(64) void assign_exact_kernel(AssignExactArgs a) {
  __shared__ __attribute__((aligned(16))) float tile[TILE_FLOATS];     // [TILE_DCH][TILE_STRIDE]
  __shared__ __attribute__((aligned(16))) float qs[TILE_QFLOATS];      // [TILE_DCH][TILE_QT]
  const int lane = threadIdx.x, d = a.d;
  const int i = blockIdx.x * 64 + lane;
  int32_t row = -1;
  if (i < a.n_targets) row = row_of_id(a.vec_ids, a.N, a.targets[i]);
  uint32_t best_ord = 0;   // (no similarity's image)
  int32_t best_q = -1;
  float best_sim = -__builtin_huge_valf();
  if (__ballot(row >= 0) != 0ull) {
    const bool vec4 = (d & 3) == 0;
    for (int q0 = 0; q0 < a.Q; q0 += TILE_QT) {
      float acc[TILE_QT];
#pragma unroll
      for (int t = 0; t < TILE_QT; ++t) acc[t] = 0.0f;
      for (int c0 = 0; c0 < d; c0 += TILE_DCH) {
        const int nd = (d - c0 < TILE_DCH) ? d - c0 : TILE_DCH;
        float4 v[8], qv[2];
#pragma unroll
        for (int it = 0; it < 8; ++it) v[it] = tile_row_piece(a.rows, row, it, lane, d, c0, nd, vec4);
#pragma unroll
        for (int it = 0; it < 2; ++it) qv[it] = tile_query_piece(a.queries, a.Q, q0, it, lane, d, c0, nd, vec4);
#pragma unroll
        for (int it = 0; it < 8; ++it) tile_store_row_piece(tile, v[it], it, lane);
#pragma unroll
        for (int it = 0; it < 2; ++it) tile_store_query_piece(qs, qv[it], it, lane);
        wave_lds_sync();
        const float* col = tile + lane;   // (the 16-accumulator walk, kept in place for registers: dot_chain.h)
        if (nd == TILE_DCH) {
#pragma unroll
          for (int j = 0; j < TILE_DCH; ++j) {
            const float x = col[j * TILE_STRIDE];
#pragma unroll
            for (int t4 = 0; t4 < TILE_QT / 4; ++t4) {
              const float4 qq = *reinterpret_cast<const float4*>(qs + tile_qrow(j) * TILE_QT + t4 * 4);
              float p;
              p = qq.x * x; acc[t4 * 4 + 0] = acc[t4 * 4 + 0] + p;   // core_functions.c:77: scalar += v1[i] * v2[i]
              p = qq.y * x; acc[t4 * 4 + 1] = acc[t4 * 4 + 1] + p;
              p = qq.z * x; acc[t4 * 4 + 2] = acc[t4 * 4 + 2] + p;
              p = qq.w * x; acc[t4 * 4 + 3] = acc[t4 * 4 + 3] + p;
            }
          }
        } else {
          for (int j = 0; j < nd; ++j) {
            const float x = col[j * TILE_STRIDE];
#pragma unroll
            for (int t4 = 0; t4 < TILE_QT / 4; ++t4) {
              const float4 qq = *reinterpret_cast<const float4*>(qs + tile_qrow(j) * TILE_QT + t4 * 4);
              float p;
              p = qq.x * x; acc[t4 * 4 + 0] = acc[t4 * 4 + 0] + p;
              p = qq.y * x; acc[t4 * 4 + 1] = acc[t4 * 4 + 1] + p;
              p = qq.z * x; acc[t4 * 4 + 2] = acc[t4 * 4 + 2] + p;
              p = qq.w * x; acc[t4 * 4 + 3] = acc[t4 * 4 + 3] + p;
            }
          }
        }
        wave_lds_sync();
      }
#pragma unroll
      for (int t = 0; t < TILE_QT; ++t) {   // ascending query index: only a strictly larger similarity replaces the best
        const uint32_t o = assign_ord(acc[t]);
        if (q0 + t < a.Q && o > best_ord) { best_ord = o; best_q = q0 + t; best_sim = acc[t]; }
      }
    }
  }
  if (i < a.n_targets) {
    a.out_query[i] = row >= 0 ? best_q : -1;
    a.out_sim[i] = row >= 0 ? best_sim : -__builtin_huge_valf();
  }
}

struct AssignPqArgs {
  const float* lut;          // [nq][m][K] the LUTs of queries q_base .. q_base + nq - 1
  const int32_t* targets;    // [n_targets] ids
  const int32_t* ids;        // [N] ascending ids of the pq handle (position -> id)
  const uint32_t* packed;    // [blocks][M2][64] its codes
  int32_t* out_query;        // [n_targets]  state between launches, and the result
  float* out_sim;            // [n_targets]
  float* best_dist;          // [n_targets]  the smallest candidate distance so far
  int64_t N;
  int n_targets, q_base, nq, m, K, LT, first;
  float sentinel;
};

template <int M2, int RPT>   // dwords of codes per row (0: read the codes from memory for every query, any m); targets per thread
__global__ __launch_bounds__(AS_PQ_WG) void assign_pq_kernel(AssignPqArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char as_smem[];
  float* sl = reinterpret_cast<float*>(as_smem);   // [LT][m][K]
  const int tid = threadIdx.x, m = a.m, K = a.K, lutN = m * K;
  const int m2 = M2 ? M2 : (m + 1) / 2;
  int32_t row[RPT], bq[RPT];
  uint32_t cw[RPT][M2 ? M2 : 1];
  float bkey[RPT], bdist[RPT];
#pragma unroll
  for (int r = 0; r < RPT; ++r) {
    const int i = (blockIdx.x * RPT + r) * AS_PQ_WG + tid;
    row[r] = -1; bq[r] = -1; bkey[r] = -__builtin_huge_valf(); bdist[r] = a.sentinel;
    if (i < a.n_targets) {
      row[r] = row_of_id(a.ids, a.N, a.targets[i]);
      if (!a.first) { bq[r] = a.out_query[i]; bkey[r] = a.out_sim[i]; bdist[r] = a.best_dist[i]; }
    }
#pragma unroll
    for (int j = 0; j < (M2 ? M2 : 1); ++j)
      cw[r][j] = (M2 && row[r] >= 0) ? a.packed[((size_t)(row[r] >> 6) * m2 + j) * 64 + (row[r] & 63)] : 0u;
  }
  for (int l0 = 0; l0 < a.nq; l0 += a.LT) {
    const int nl = (a.nq - l0 < a.LT) ? a.nq - l0 : a.LT;
    __syncthreads();
    const float* src = a.lut + (size_t)l0 * lutN;
    if ((lutN & 3) == 0) {
      const int n4 = nl * (lutN >> 2);
      for (int x = tid; x < n4; x += AS_PQ_WG) reinterpret_cast<float4*>(sl)[x] = reinterpret_cast<const float4*>(src)[x];
    } else {
      for (int x = tid; x < nl * lutN; x += AS_PQ_WG) sl[x] = src[x];
    }
    __syncthreads();
    for (int l = 0; l < nl; ++l) {
      const float* lt = sl + (size_t)l * lutN;
#pragma unroll
      for (int r = 0; r < RPT; ++r) {
        if (row[r] < 0) continue;
        float dist = 0.0f;
        if (M2) {
#pragma unroll
          for (int j = 0; j < (M2 ? M2 : 1); ++j) {
            const uint32_t w = cw[r][j];
            dist = dist + lt[(2 * j) * K + (int)(w & 0xffffu)];
            if (2 * j + 1 < m) dist = dist + lt[(2 * j + 1) * K + (int)(w >> 16)];
          }
        } else {
          for (int j = 0; j < m2; ++j) {
            const uint32_t w = a.packed[((size_t)(row[r] >> 6) * m2 + j) * 64 + (row[r] & 63)];
            dist = dist + lt[(2 * j) * K + (int)(w & 0xffffu)];
            if (2 * j + 1 < m) dist = dist + lt[(2 * j + 1) * K + (int)(w >> 16)];
          }
        }
        if (dist < bdist[r]) {   // (false for a NaN; bdist starts at the sentinel)
          bdist[r] = dist;
          const float key = freddy_similarity_of(dist);
          if (key > bkey[r]) { bkey[r] = key; bq[r] = a.q_base + l0 + l; }
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < RPT; ++r) {
    const int i = (blockIdx.x * RPT + r) * AS_PQ_WG + tid;
    if (i < a.n_targets) { a.out_query[i] = bq[r]; a.out_sim[i] = bkey[r]; a.best_dist[i] = bdist[r]; }
  }
}

}  // namespace freddy
