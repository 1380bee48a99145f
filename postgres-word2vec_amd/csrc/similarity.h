// similarity.h -- cosine_similarity(token1, token2) (freddy--0.0.1.sql:946-959: two rows of google_vecs_norm through
// cosine_similarity_bytea, core_functions.c:67-81) and its vector overload (:961-974) in their batched forms: the VALUES, with no
// ranking around them (include/freddy_gpu.h: freddy_gpu_similarity_pairs / _matrix / _join).  A similarity is always the binary32
// chain "scalar = 0; scalar += v1[i] * v2[i]", i ascending, every product and sum rounded on its own (-ffp-contract=off) -- one
// sequential chain per lane.  (The bit contract fixes the summation order, so the matrix cores cannot produce these values.)
// Ids are resolved on the device by binary search over the handle's ascending ids (assign_row_of).
//
//   sim_pairs_kernel   one lane per pair, 64 pairs per wave, one wave per workgroup.  Both rows of a pair are a gather of 4 d bytes;
//       pv_rerank's staging, twice: per step 64 pairs x SIM_DCH = 32 dimensions of the A rows and of the B rows are read with 16-byte
//       loads (8 consecutive lanes = 128 contiguous bytes of one row; a scalar path for d % 4 != 0) and stored transposed into two
//       tiles [32][65]; every lane then walks its own column of either tile with the accumulator in a register.
//       LDS banks (ds_write_b32 / ds_read_b32: bank = (address / 4) mod 32 within each half of the wave): a store instruction writes,
//       per half, 4 pairs x 8 row pieces at tile[(4 * piece + j) * 65 + pair]: banks 4 * piece + pair (mod 32), all different; a read
//       is lane-consecutive.  The second tile begins 32 * 65 = 2080 floats after the first, a multiple of 32 banks, and no instruction
//       touches both tiles: the argument of pv.h holds for each tile by itself.  LDS 2 x 8 320 B = 16 640 B per wave (9 waves per CU
//       by LDS); registers: 16 float4 of row pieces in flight + one accumulator.
//   sim_rows_kernel    ids -> rows (-1: none) and the `known` bytes of the B side of a matrix, once per call.
//   sim_matrix_kernel  assign_exact_kernel's tile with the values kept: lanes are B rows (row tile [32][65], the banks as above), a
//       tile of SIM_AT = 16 A rows x 32 dimensions [32][16] is loaded as 16-byte pieces and stored with its rows permuted (as_qrow:
//       a store's 64 lanes write 64 consecutive floats), every lane reads the same 16 consecutive floats of a dimension (four
//       broadcast ds_read_b128) into 16 accumulators; a B row piece is loaded once per 16 A rows.  For a fixed A row the 64 lanes
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
static constexpr int SIM_AT = AS_QT;                       // A rows per tile of sim_matrix_kernel
static constexpr int SIM_DCH = AS_DCH;                     // dimensions per step
static constexpr int SIM_STRIDE = AS_STRIDE;               // floats per dimension of a row tile: 64 rows + 1
static constexpr int SIM_TILE = SIM_DCH * SIM_STRIDE;
static constexpr int SIM_ATILE = SIM_DCH * SIM_AT;
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

// the piece (dimensions c0 + dim0 .. + 3) of row r of a row-major table, zeros where the row (r < 0) or the dimension is missing
__device__ __forceinline__ float4 sim_piece(const float* __restrict__ rows, int32_t r, int d, int c0, int dim0, int nd, bool vec4) {
  float4 v = float4{0.0f, 0.0f, 0.0f, 0.0f};
  if (r >= 0 && dim0 < nd) {
    const float* src = rows + (size_t)r * d + c0 + dim0;
    if (vec4) v = *reinterpret_cast<const float4*>(src);
    else {
      v.x = src[0];
      if (dim0 + 1 < nd) v.y = src[1];
      if (dim0 + 2 < nd) v.z = src[2];
      if (dim0 + 3 < nd) v.w = src[3];
    }
  }
  return v;
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
  __shared__ __attribute__((aligned(16))) float ta[SIM_TILE];   // [SIM_DCH][SIM_STRIDE] rows of ids_a
  __shared__ __attribute__((aligned(16))) float tb[SIM_TILE];   // the same of ids_b
  const int lane = threadIdx.x, d = a.d;
  const int i = blockIdx.x * 64 + lane;
  int32_t ra = -1, rb = -1;
  if (i < a.n) {
    ra = assign_row_of(a.vec_ids, a.N, a.ids_a[i]);
    if (ra >= 0) rb = assign_row_of(a.vec_ids, a.N, a.ids_b[i]);
    if (rb < 0) ra = -1;   // (a pair is known with both rows; none of an unknown pair's rows is read)
  }
  float acc = 0.0f;
  if (__ballot(ra >= 0) != 0ull) {
    const bool vec4 = (d & 3) == 0;   // every row 16-byte aligned and no piece crosses the row's end
    for (int c0 = 0; c0 < d; c0 += SIM_DCH) {
      const int nd = (d - c0 < SIM_DCH) ? d - c0 : SIM_DCH;
      float4 va[8], vb[8];
#pragma unroll
      for (int it = 0; it < 8; ++it) {   // piece (it * 64 + lane): pair (it * 8 + lane / 8), dimensions c0 + 4 (lane % 8) ..
        const int cl = it * 8 + (lane >> 3), dim0 = (lane & 7) * 4;
        va[it] = sim_piece(a.rows, __shfl(ra, cl, 64), d, c0, dim0, nd, vec4);
        vb[it] = sim_piece(a.rows, __shfl(rb, cl, 64), d, c0, dim0, nd, vec4);
      }
#pragma unroll
      for (int it = 0; it < 8; ++it) {
        const int cl = it * 8 + (lane >> 3), dim0 = (lane & 7) * 4;
        float* da = ta + dim0 * SIM_STRIDE + cl;
        da[0] = va[it].x; da[SIM_STRIDE] = va[it].y; da[2 * SIM_STRIDE] = va[it].z; da[3 * SIM_STRIDE] = va[it].w;
        float* db = tb + dim0 * SIM_STRIDE + cl;
        db[0] = vb[it].x; db[SIM_STRIDE] = vb[it].y; db[2 * SIM_STRIDE] = vb[it].z; db[3 * SIM_STRIDE] = vb[it].w;
      }
      assign_wave_sync();
      const float* ca = ta + lane;
      const float* cb = tb + lane;
      if (nd == SIM_DCH) {
#pragma unroll
        for (int j = 0; j < SIM_DCH; ++j) {
          const float p = ca[j * SIM_STRIDE] * cb[j * SIM_STRIDE];   // core_functions.c:77: v1[i] * v2[i]
          acc = acc + p;                                             //                     scalar += ...
        }
      } else {
        for (int j = 0; j < nd; ++j) {
          const float p = ca[j * SIM_STRIDE] * cb[j * SIM_STRIDE];
          acc = acc + p;
        }
      }
      assign_wave_sync();
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
  const int32_t r = assign_row_of(vec_ids, N, ids[i]);
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
  __shared__ __attribute__((aligned(16))) float tile[SIM_TILE];    // [SIM_DCH][SIM_STRIDE]
  __shared__ __attribute__((aligned(16))) float qs[SIM_ATILE];     // [SIM_DCH][SIM_AT]
  const int lane = threadIdx.x, d = a.d;
  const int j = blockIdx.x * 64 + lane;
  const int32_t row = j < a.nb ? a.b_rows[j] : -1;
  const bool any = __ballot(row >= 0) != 0ull;
  const bool vec4 = (d & 3) == 0;   // every row of the table and of A 16-byte aligned and no piece crosses its end
  const int n_tiles = (a.na + SIM_AT - 1) / SIM_AT;
  const int t_begin = blockIdx.y * a.tiles_per_wg;
  const int t_end = (t_begin + a.tiles_per_wg < n_tiles) ? t_begin + a.tiles_per_wg : n_tiles;
  for (int tl = t_begin; tl < t_end; ++tl) {
    const int q0 = tl * SIM_AT;
    float acc[SIM_AT];
#pragma unroll
    for (int t = 0; t < SIM_AT; ++t) acc[t] = 0.0f;
    if (any) {
      for (int c0 = 0; c0 < d; c0 += SIM_DCH) {
        const int nd = (d - c0 < SIM_DCH) ? d - c0 : SIM_DCH;
        float4 v[8], qv[2];
#pragma unroll
        for (int it = 0; it < 8; ++it) {   // piece (it * 64 + lane): B row (it * 8 + lane / 8), dimensions c0 + 4 (lane % 8) ..
          const int cl = it * 8 + (lane >> 3), dim0 = (lane & 7) * 4;
          v[it] = sim_piece(a.rows, __shfl(row, cl, 64), d, c0, dim0, nd, vec4);
        }
#pragma unroll
        for (int it = 0; it < 2; ++it) {   // A row (q0 + lane % 16), dimensions c0 + 4 (it * 4 + lane / 16) ..
          const int t = lane & 15, dim0 = (it * 4 + (lane >> 4)) * 4;
          qv[it] = sim_piece(a.a, q0 + t < a.na ? q0 + t : -1, d, c0, dim0, nd, vec4);
        }
#pragma unroll
        for (int it = 0; it < 8; ++it) {
          const int cl = it * 8 + (lane >> 3), dim0 = (lane & 7) * 4;
          float* dst = tile + dim0 * SIM_STRIDE + cl;
          dst[0] = v[it].x; dst[SIM_STRIDE] = v[it].y; dst[2 * SIM_STRIDE] = v[it].z; dst[3 * SIM_STRIDE] = v[it].w;
        }
#pragma unroll
        for (int it = 0; it < 2; ++it) {   // piece p, element c (dimension 4 p + c) -> row as_qrow(4 p + c) = 8 c + p
          float* dst = qs + (it * 4 + (lane >> 4)) * SIM_AT + (lane & 15);
          dst[0] = qv[it].x; dst[8 * SIM_AT] = qv[it].y; dst[16 * SIM_AT] = qv[it].z; dst[24 * SIM_AT] = qv[it].w;
        }
        assign_wave_sync();
        const float* col = tile + lane;
        if (nd == SIM_DCH) {
#pragma unroll
          for (int jj = 0; jj < SIM_DCH; ++jj) {
            const float x = col[jj * SIM_STRIDE];
#pragma unroll
            for (int t4 = 0; t4 < SIM_AT / 4; ++t4) {
              const float4 qq = *reinterpret_cast<const float4*>(qs + as_qrow(jj) * SIM_AT + t4 * 4);
              float p;
              p = qq.x * x; acc[t4 * 4 + 0] = acc[t4 * 4 + 0] + p;   // core_functions.c:77: scalar += v1[i] * v2[i] (v1: the A row)
              p = qq.y * x; acc[t4 * 4 + 1] = acc[t4 * 4 + 1] + p;
              p = qq.z * x; acc[t4 * 4 + 2] = acc[t4 * 4 + 2] + p;
              p = qq.w * x; acc[t4 * 4 + 3] = acc[t4 * 4 + 3] + p;
            }
          }
        } else {
          for (int jj = 0; jj < nd; ++jj) {
            const float x = col[jj * SIM_STRIDE];
#pragma unroll
            for (int t4 = 0; t4 < SIM_AT / 4; ++t4) {
              const float4 qq = *reinterpret_cast<const float4*>(qs + as_qrow(jj) * SIM_AT + t4 * 4);
              float p;
              p = qq.x * x; acc[t4 * 4 + 0] = acc[t4 * 4 + 0] + p;
              p = qq.y * x; acc[t4 * 4 + 1] = acc[t4 * 4 + 1] + p;
              p = qq.z * x; acc[t4 * 4 + 2] = acc[t4 * 4 + 2] + p;
              p = qq.w * x; acc[t4 * 4 + 3] = acc[t4 * 4 + 3] + p;
            }
          }
        }
        assign_wave_sync();
      }
    }
    if (j < a.nb) {
#pragma unroll
      for (int t = 0; t < SIM_AT; ++t) {   // per A row: the wave's 64 lanes write 64 consecutive floats
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
