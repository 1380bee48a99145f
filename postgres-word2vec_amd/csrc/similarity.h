// similarity.h -- cosine_similarity(token1, token2) (freddy--0.0.1.sql:946-959: two rows of google_vecs_norm through
// cosine_similarity_bytea, core_functions.c:67-81) and its vector overload (:961-974) in their batched forms: the VALUES, with no
// ranking around them (include/freddy_gpu.h: freddy_gpu_similarity_pairs / _matrix / _join).  A similarity is always the binary32
// chain "scalar = 0; scalar += v1[i] * v2[i]", i ascending, every product and sum rounded on its own (-ffp-contract=off) -- one
// sequential chain per lane.  (The bit contract fixes the summation order, so the matrix cores cannot produce these values.)
// Ids are resolved on the device by binary search over the handle's ascending ids (row_of_id).  The tiles are dot_chain.h's.
//
//   sim_pairs_kernel   one lane per pair, 64 pairs per wave, one wave per workgroup.  Both rows of a pair are a gather of 4 d bytes:
//       the gather tile twice, one of the A rows and one of the B rows, all 16 loads of a step issued before the first store; every
//       lane then walks its own column of either tile with the accumulator in a register (chain1).  No instruction touches both
//       tiles.  LDS 2 x 8 320 B = 16 640 B per wave (9 waves per CU by LDS); registers: 16 float4 of row pieces in flight + one
//       accumulator.
//   sim_rows_kernel    ids -> rows (-1: none) and the `known` bytes of the B side of a matrix, once per call.
//   sim_matrix_kernel  assign_exact_kernel's tiles with the values kept: lanes are B rows (the gather tile), the query tile holds 16
//       A rows, 16 accumulators per lane; a B row piece is loaded once per 16 A rows.  For a fixed A row the 64 lanes
//       write 64 consecutive floats of out[a][.]: 16 stores of 256 contiguous bytes per A tile.  A workgroup (x: 64 B rows, y: a
//       range of A tiles -- the host splits A only as far as the chip needs workgroups) is still ONE wave: the waves share nothing
//       but the A tile (2 KiB per step beside 8 KiB of B pieces, and L2-resident), the 4 KiB of results per A tile leave through
//       plain stores that nothing waits for (one tile's arithmetic is 16 x 64 x d multiply-adds behind them), and a workgroup of four
//       waves would turn the two wave barriers per step into workgroup barriers.  LDS 8 320 B + 2 048 B = 10 368 B per wave (15 waves
//       per CU by LDS); registers: 16 accumulators + 8 float4 of row pieces + 2 of A pieces in flight.
//   sim_count_kernel / sim_scan_kernel / sim_fill_kernel   the join "WHERE cosine_similarity(a, b) > threshold" over the block the
//       matrix kernel wrote (every chain is computed once): one ballot + popcount per (A row, 64 B rows), an exclusive scan of the
//       counts in A-major order (per chunk of 1024 units: the count kernel also writes the chunk's sum, and every workgroup of the
//       scan adds up the sums of the chunks before its own -- two launches, no workgroup waits for another), and the matching lanes written at the scanned offset + the lane's rank in its ballot -- i ascending, then j ascending,
//       with no atomics.  The predicate is PostgreSQL's float4gt (sim_float4gt), not assign_ord, which separates the two zeros.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "assign.h"

namespace freddy {

static constexpr int64_t SIM_MAX_NB = (int64_t)1 << 22;   // B ids per matrix / join call
static constexpr int SIM_CHUNK = 1024;                     // units per workgroup of sim_count_kernel / sim_scan_kernel
static constexpr int SIM_COUNT_WAVES = 16;                 // waves per workgroup of sim_count_kernel

// PostgreSQL's float4gt (float4_cmp_internal > 0): a NaN is greater than every non-NaN and equal to a NaN, nothing is greater than a
// NaN, and -0.0 is not greater than +0.0
__host__ __device__ __forceinline__ bool sim_float4gt(float a, float b) {
  const bool an = a != a, bn = b != b;
  if (an) return !bn;
  if (bn) return false;
  return a > b;
}

struct SimPairsArgs {
  const int32_t* ids_a;      // [n]
  const int32_t* ids_b;      // [n]
  const int32_t* vec_ids;    // [N] ascending ids of the vector handle
  const float* rows;         // [N][d] its row-major copy
  float* out_sim;            // [n]
  uint8_t* out_known;        // [n]
  int64_t N;
  int n, d;
};

static __global__ __launch_bounds__(64) void sim_pairs_kernel(SimPairsArgs a) {
  __shared__ __attribute__((aligned(16))) float ta[TILE_FLOATS];   // [TILE_DCH][TILE_STRIDE] rows of ids_a
  __shared__ __attribute__((aligned(16))) float tb[TILE_FLOATS];   // the same of ids_b
  const int lane = threadIdx.x, d = a.d;
  const int i = blockIdx.x * 64 + lane;
  int32_t ra = -1, rb = -1;
  if (i < a.n) {
    ra = row_of_id(a.vec_ids, a.N, a.ids_a[i]);
    if (ra >= 0) rb = row_of_id(a.vec_ids, a.N, a.ids_b[i]);
    if (rb < 0) ra = -1;   // (a pair is known with both rows; none of an unknown pair's rows is read)
  }
  float acc = 0.0f;
  if (__ballot(ra >= 0) != 0ull) {
    const bool vec4 = (d & 3) == 0;
    for (int c0 = 0; c0 < d; c0 += TILE_DCH) {
      const int nd = (d - c0 < TILE_DCH) ? d - c0 : TILE_DCH;
      float4 va[8], vb[8];
#pragma unroll
      for (int it = 0; it < 8; ++it) {
        va[it] = tile_row_piece(a.rows, ra, it, lane, d, c0, nd, vec4);
        vb[it] = tile_row_piece(a.rows, rb, it, lane, d, c0, nd, vec4);
      }
#pragma unroll
      for (int it = 0; it < 8; ++it) {
        tile_store_row_piece(ta, va[it], it, lane);
        tile_store_row_piece(tb, vb[it], it, lane);
      }
      wave_lds_sync();
      chain1<TILE_STRIDE, TILE_STRIDE>(acc, ta + lane, tb + lane, nd);   // v1: the row of ids_a
      wave_lds_sync();
    }
  }
  if (i < a.n) {
    a.out_sim[i] = ra >= 0 ? acc : 0.0f;
    a.out_known[i] = ra >= 0 ? 1 : 0;
  }
}

// ids[n] -> rows[n] (-1: the id has no row) and known[n]
static __global__ __launch_bounds__(256) void sim_rows_kernel(const int32_t* __restrict__ ids, int n, const int32_t* __restrict__ vec_ids, int64_t N,
                                                              int32_t* __restrict__ rows, uint8_t* __restrict__ known) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int32_t r = row_of_id(vec_ids, N, ids[i]);
  rows[i] = r;
  known[i] = r >= 0 ? 1 : 0;
}

struct SimMatrixArgs {
  const int32_t* b_rows;     // [nb] rows of the B ids in the table, -1: none (sim_rows_kernel)
  const float* rows;         // [N][d] the table, row-major
  const float* a;            // [na][d] the A rows of this pass
  const uint8_t* known_a;    // [na], or NULL: every A row is known
  float* out;                // [na][nb]
  int na, nb, d;
  int tiles_per_wg;          // A tiles per workgroup: blockIdx.y owns the tiles [y * tiles_per_wg, ...)
};

static __global__ __launch_bounds__(64) void sim_matrix_kernel(SimMatrixArgs a) {
  __shared__ __attribute__((aligned(16))) float tile[TILE_FLOATS];    // [TILE_DCH][TILE_STRIDE]
  __shared__ __attribute__((aligned(16))) float qs[TILE_QFLOATS];     // [TILE_DCH][TILE_QT] A rows
  const int lane = threadIdx.x, d = a.d;
  const int j = blockIdx.x * 64 + lane;
  const int32_t row = j < a.nb ? a.b_rows[j] : -1;
  const bool any = __ballot(row >= 0) != 0ull;
  const bool vec4 = (d & 3) == 0;
  const int n_tiles = (a.na + TILE_QT - 1) / TILE_QT;
  const int t_begin = blockIdx.y * a.tiles_per_wg;
  const int t_end = (t_begin + a.tiles_per_wg < n_tiles) ? t_begin + a.tiles_per_wg : n_tiles;
  for (int tl = t_begin; tl < t_end; ++tl) {
    const int q0 = tl * TILE_QT;
    float acc[TILE_QT];
#pragma unroll
    for (int t = 0; t < TILE_QT; ++t) acc[t] = 0.0f;
    if (any) {
      for (int c0 = 0; c0 < d; c0 += TILE_DCH) {
        const int nd = (d - c0 < TILE_DCH) ? d - c0 : TILE_DCH;
        float4 v[8], qv[2];
#pragma unroll
        for (int it = 0; it < 8; ++it) v[it] = tile_row_piece(a.rows, row, it, lane, d, c0, nd, vec4);
#pragma unroll
        for (int it = 0; it < 2; ++it) qv[it] = tile_query_piece(a.a, a.na, q0, it, lane, d, c0, nd, vec4);
#pragma unroll
        for (int it = 0; it < 8; ++it) tile_store_row_piece(tile, v[it], it, lane);
#pragma unroll
        for (int it = 0; it < 2; ++it) tile_store_query_piece(qs, qv[it], it, lane);
        wave_lds_sync();
        const float* col = tile + lane;   // (the 16-accumulator walk, kept in place for registers: dot_chain.h)
        if (nd == TILE_DCH) {
#pragma unroll
          for (int jj = 0; jj < TILE_DCH; ++jj) {
            const float x = col[jj * TILE_STRIDE];
#pragma unroll
            for (int t4 = 0; t4 < TILE_QT / 4; ++t4) {
              const float4 qq = *reinterpret_cast<const float4*>(qs + tile_qrow(jj) * TILE_QT + t4 * 4);
              float p;
              p = qq.x * x; acc[t4 * 4 + 0] = acc[t4 * 4 + 0] + p;   // core_functions.c:77: scalar += v1[i] * v2[i] (v1: the A row)
              p = qq.y * x; acc[t4 * 4 + 1] = acc[t4 * 4 + 1] + p;
              p = qq.z * x; acc[t4 * 4 + 2] = acc[t4 * 4 + 2] + p;
              p = qq.w * x; acc[t4 * 4 + 3] = acc[t4 * 4 + 3] + p;
            }
          }
        } else {
          for (int jj = 0; jj < nd; ++jj) {
            const float x = col[jj * TILE_STRIDE];
#pragma unroll
            for (int t4 = 0; t4 < TILE_QT / 4; ++t4) {
              const float4 qq = *reinterpret_cast<const float4*>(qs + tile_qrow(jj) * TILE_QT + t4 * 4);
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
    }
    if (j < a.nb) {
#pragma unroll
      for (int t = 0; t < TILE_QT; ++t) {   // per A row: the wave's 64 lanes write 64 consecutive floats
        if (q0 + t < a.na) {
          const bool known = row >= 0 && (a.known_a == nullptr || a.known_a[q0 + t] != 0);
          a.out[(size_t)(q0 + t) * a.nb + j] = known ? acc[t] : 0.0f;
        }
      }
    }
  }
}

// The join over one block of the matrix.  A unit u = (A row u / nblk of the block, B rows 64 (u % nblk) ..) is one wave's ballot.
struct SimJoinArgs {
  const float* blk;          // [na][nb] the block sim_matrix_kernel wrote
  const uint8_t* known_a;    // [na] of the block's A rows, or NULL: all known
  const uint8_t* known_b;    // [nb]
  int32_t* cnt;              // [units] matches per unit
  int32_t* part;             // [chunks] matches per chunk of SIM_CHUNK units
  const int32_t* off;        // [units] their exclusive scan (sim_fill_kernel)
  int32_t* out_a;            // [cap] position in the A argument
  int32_t* out_b;            // [cap] position in the B argument
  float* out_sim;            // [cap]
  int64_t units;
  int na, nb, nblk;
  int a0;                    // position of the block's first A row in the A argument
  int32_t cap;               // matches of this block that are written: the first `cap` in (i, j) order
  float threshold;
};

__device__ __forceinline__ bool sim_join_match(const SimJoinArgs& a, int al, int j, float* v) {
  if (j >= a.nb || !a.known_b[j] || (a.known_a != nullptr && !a.known_a[al])) return false;
  *v = a.blk[(size_t)al * a.nb + j];
  return sim_float4gt(*v, a.threshold);
}

// Workgroup c (16 waves) owns the units [c * SIM_CHUNK, (c + 1) * SIM_CHUNK), 64 per wave; a wave takes eight units per step, their
// loads issued together.  cnt[u] = matches of unit u, part[c] = matches of the chunk.
static __global__ __launch_bounds__(SIM_COUNT_WAVES * 64) void sim_count_kernel(SimJoinArgs a) {
  __shared__ int32_t wave_sum[SIM_COUNT_WAVES];
  constexpr int PER_WAVE = SIM_CHUNK / SIM_COUNT_WAVES;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t u0 = (int64_t)blockIdx.x * SIM_CHUNK + w * PER_WAVE;
  int32_t sum = 0;
  int al = (int)(u0 / a.nblk), jb = (int)(u0 - (int64_t)al * a.nblk);   // unit u0 + t + k = (A row al, B rows 64 jb ..), advanced unit by unit
  for (int t = 0; t < PER_WAVE && u0 + t < a.units; t += 8) {   // (uniform over the wave)
    bool m[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      m[k] = false;
      if (u0 + t + k < a.units) {
        float v;
        m[k] = sim_join_match(a, al, jb * 64 + lane, &v);
      }
      if (++jb == a.nblk) { jb = 0; ++al; }
    }
    int32_t mine = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int32_t c = __popcll(__ballot(m[k]));
      sum += c;
      if (lane == k) mine = c;
    }
    if (lane < 8 && u0 + t + lane < a.units) a.cnt[u0 + t + lane] = mine;   // eight consecutive counts in one store
  }
  if (lane == 0) wave_sum[w] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    int32_t total = 0;
    for (int k = 0; k < SIM_COUNT_WAVES; ++k) total += wave_sum[k];
    a.part[blockIdx.x] = total;
  }
}

// off[i] = cnt[0] + .. + cnt[i - 1], off[n] = the total.  Workgroup c scans its chunk of SIM_CHUNK counts (four consecutive ones per
// thread: one 16-byte load and store where the chunk is whole; cnt and off come from the allocator and a chunk begins at a multiple of
// 1024) from the sum of the chunks before it, which it adds up from part[0 .. c) itself -- at most a few thousand values, and no
// workgroup waits for another.
static __global__ __launch_bounds__(256) void sim_scan_kernel(const int32_t* __restrict__ cnt, const int32_t* __restrict__ part, int64_t n,
                                                              int32_t* __restrict__ off) {
  __shared__ int32_t red[4], wave_sum[4];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  int32_t s = 0;
  for (int i = tid; i < (int)blockIdx.x; i += 256) s += part[i];
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (lane == 0) red[w] = s;
  const int64_t i0 = (int64_t)blockIdx.x * SIM_CHUNK + 4 * tid;
  int32_t c[4];
  if (i0 + 4 <= n) {
    const int4 v = *reinterpret_cast<const int4*>(cnt + i0);
    c[0] = v.x; c[1] = v.y; c[2] = v.z; c[3] = v.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) c[k] = (i0 + k < n) ? cnt[i0 + k] : 0;
  }
  const int32_t mine = c[0] + c[1] + c[2] + c[3];
  int32_t inc = mine;
  for (int o = 1; o < 64; o <<= 1) {
    const int32_t up = __shfl_up(inc, o, 64);
    if (lane >= o) inc += up;
  }
  if (lane == 63) wave_sum[w] = inc;
  __syncthreads();
  int32_t run = red[0] + red[1] + red[2] + red[3] + inc - mine;
  for (int k = 0; k < w; ++k) run += wave_sum[k];
  if (i0 + 4 <= n) {
    int4 v;
    v.x = run; v.y = run + c[0]; v.z = run + c[0] + c[1]; v.w = run + c[0] + c[1] + c[2];
    *reinterpret_cast<int4*>(off + i0) = v;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (i0 + k < n) off[i0 + k] = run;
      run += c[k];
    }
  }
  if (blockIdx.x == gridDim.x - 1 && tid == 0) off[n] = red[0] + red[1] + red[2] + red[3] + wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3];
}

static __global__ __launch_bounds__(256) void sim_fill_kernel(SimJoinArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * 4;
  for (int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); u < a.units; u += stride) {
    if (a.cnt[u] == 0) continue;   // (uniform over the wave)
    const int32_t first = a.off[u];
    if (first >= a.cap) continue;
    const int al = (int)(u / a.nblk), j = (int)(u - (int64_t)al * a.nblk) * 64 + lane;
    float v = 0.0f;
    const bool m = sim_join_match(a, al, j, &v);
    const unsigned long long mask = __ballot(m);
    if (m) {
      const int32_t p = first + (int32_t)__popcll(mask & ((1ull << lane) - 1ull));
      if (p < a.cap) { a.out_a[p] = a.a0 + al; a.out_b[p] = j; a.out_sim[p] = v; }
    }
  }
}

}  // namespace freddy
