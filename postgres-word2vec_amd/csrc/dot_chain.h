// dot_chain.h -- the one copy of the loops every exact similarity here is made of.  cosine_similarity_bytea (core_functions.c:67-81)
// is "scalar = 0; scalar += v1[i] * v2[i]", i ascending, in binary32 with a separately rounded multiply and add (never an fma:
// -ffp-contract=off, and the chains below say "p = a * b; acc = acc + p").  The bit contract fixes the summation order: one
// sequential chain per lane, and the matrix cores cannot produce these values.  The kernels keep their own setup, selection and
// epilogue and call into this header for
//
//   row_of_id       the row of an id in a handle's ascending ids, by binary search.
//   the gather tile (assign_exact_kernel, sim_pairs_kernel, sim_matrix_kernel, pv_rerank_body): one wave, one lane per row, 64
//       arbitrary rows of a row-major table, TILE_DCH = 32 dimensions per step.  The step's 64 x 32 floats are eight 16-byte
//       pieces per lane (tile_row_piece; piece it * 64 + lane: row it * 8 + lane / 8, dimensions c0 + 4 (lane % 8) ..; 8 consecutive
//       lanes = 128 contiguous bytes of one row; a scalar path where d % 4 != 0, zeros for a missing row or dimension), and
//       tile_store_row_piece writes a piece transposed into the LDS tile [32][TILE_STRIDE = 65], dimension-major; between two
//       wave_lds_sync every lane then walks its own column, tile[j * 65 + lane].
//       LDS banks (ds_write_b32 / ds_read_b32: bank = (address / 4) mod 32 within each half of the wave): a store instruction
//       writes, per half, 4 rows x 8 pieces at tile[(4 * piece + j) * 65 + row]: banks 4 * piece + row (mod 32), all different; a
//       read is lane-consecutive.  Both are conflict free, which a stride of 64 would not be for the stores (8-way).  A tile is
//       8 320 B, a multiple of 32 banks, so the argument holds for each of several tiles by itself.
//       The helpers are per piece and hand a float4 over by value; the loops over the pieces stay in the kernels, which issue ALL
//       their loads of a step (8 row pieces + 2 query pieces, or 16 row pieces, A and B alternating) before the first store, so
//       that many are in flight.
//   the query tile (assign_exact_kernel, sim_matrix_kernel): TILE_QT = 16 queries x 32 dimensions beside the row tile, [32][16],
//       2 048 B.  Two 16-byte pieces per lane (tile_query_piece; 16 consecutive lanes = one piece of each of the 16 queries),
//       stored with the tile's rows permuted (tile_store_query_piece, tile_qrow) so that a store's 64 lanes write 64 consecutive
//       floats -- conflict free as well.  Every lane then reads the same 16 consecutive floats of a dimension (four broadcast
//       ds_read_b128), multiplies them by its own row element and adds into 16 accumulators in registers -- a row piece is
//       loaded once per 16 queries.  That walk is written out in its two kernels (kept in place for registers: profiles/HISTORY.md,
//       the dot_chain.h entry).  chain1 is the walk with one accumulator (sim_pairs_kernel, pv_rerank_body), both operands
//       given by the caller.
//   stream_row      a row of the blocked layout xb[block][dim][64] (lane = row; an_pair_scan_kernel), its values handed on in
//       ascending dimension with eight loads in flight ahead of their use.  (exact_scan_kernel and an_scan_kernel have the same
//       loop written out, for registers: the same entry.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace freddy {

static constexpr int TILE_DCH = 32;                       // dimensions per step
static constexpr int TILE_STRIDE = 65;                    // floats per dimension of a row tile: 64 rows + 1 (the banks, above)
static constexpr int TILE_FLOATS = TILE_DCH * TILE_STRIDE;
static constexpr int TILE_QT = 16;                        // queries per query tile
static constexpr int TILE_QFLOATS = TILE_DCH * TILE_QT;

// writes of this wave's lanes to its tiles become visible to its other lanes (the LDS executes a wave's accesses in order; the
// fences keep the compiler from moving them across)
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the row of `id` in a table of N ascending ids, -1 if it has none
__device__ __forceinline__ int32_t row_of_id(const int32_t* __restrict__ ids, int64_t N, int32_t id) {
  int64_t lo = 0, hi = N;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (ids[mid] < id) lo = mid + 1; else hi = mid;
  }
  return (lo < N && ids[lo] == id) ? (int32_t)lo : -1;
}

// the piece (dimensions c0 + dim0 .. + 3) of row r of a row-major table, zeros where the row (r < 0) or the dimension (>= c0 + nd)
// is missing.  vec4: d % 4 == 0, so every row is 16-byte aligned and no piece crosses its end
__device__ __forceinline__ float4 row_piece(const float* __restrict__ rows, int32_t r, int d, int c0, int dim0, int nd, bool vec4) {
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

// piece `it` (of eight) of this lane in the step [c0, c0 + nd) of the wave's 64 rows: piece it * 64 + lane is row it * 8 + lane / 8,
// dimensions c0 + 4 (lane % 8) ..; row_of_lane: the table row of the lane's own row (-1: none)
__device__ __forceinline__ float4 tile_row_piece(const float* __restrict__ rows, int32_t row_of_lane, int it, int lane, int d, int c0, int nd, bool vec4) {
  const int cl = it * 8 + (lane >> 3), dim0 = (lane & 7) * 4;
  return row_piece(rows, __shfl(row_of_lane, cl, 64), d, c0, dim0, nd, vec4);
}
// ... and its place in the transposed tile [TILE_DCH][TILE_STRIDE]
__device__ __forceinline__ void tile_store_row_piece(float* tile, float4 v, int it, int lane) {
  const int cl = it * 8 + (lane >> 3), dim0 = (lane & 7) * 4;
  float* dst = tile + dim0 * TILE_STRIDE + cl;
  dst[0] = v.x; dst[TILE_STRIDE] = v.y; dst[2 * TILE_STRIDE] = v.z; dst[3 * TILE_STRIDE] = v.w;
}

// The row of dimension j (of a step's 32) in the query tile: element c of the 16-byte piece p = j / 4 goes to row 8 c + p, so that
// the lanes of one store -- 16 queries x 4 pieces, c fixed -- write rows p, p + 1, p + 2, p + 3: 64 consecutive floats.
__device__ __forceinline__ constexpr int tile_qrow(int j) { return (j & 3) * 8 + (j >> 2); }

// piece `it` (of two) of this lane in the queries q0 .. q0 + 15 of queries[nq][d]: query q0 + lane % 16, dimensions
// c0 + 4 (it * 4 + lane / 16) ..; zeros beyond nq
__device__ __forceinline__ float4 tile_query_piece(const float* __restrict__ queries, int nq, int q0, int it, int lane, int d, int c0, int nd, bool vec4) {
  const int t = lane & 15, dim0 = (it * 4 + (lane >> 4)) * 4;
  return row_piece(queries, q0 + t < nq ? q0 + t : -1, d, c0, dim0, nd, vec4);
}
// ... and its place in the query tile [TILE_DCH][TILE_QT]: piece p, element c (dimension 4 p + c) -> row tile_qrow(4 p + c) = 8 c + p
__device__ __forceinline__ void tile_store_query_piece(float* qs, float4 qv, int it, int lane) {
  float* dst = qs + (it * 4 + (lane >> 4)) * TILE_QT + (lane & 15);
  dst[0] = qv.x; dst[8 * TILE_QT] = qv.y; dst[16 * TILE_QT] = qv.z; dst[24 * TILE_QT] = qv.w;
}

// a step of one chain: acc += a[j * SA] * b[j * SB], j ascending, the operands multiplied in this order
template <int SA, int SB>
__device__ __forceinline__ void chain1(float& acc, const float* a, const float* b, int nd) {
  if (nd == TILE_DCH) {
#pragma unroll
    for (int j = 0; j < TILE_DCH; ++j) {
      const float p = a[j * SA] * b[j * SB];   // core_functions.c:77: v1[i] * v2[i]
      acc = acc + p;                           //                     scalar += ...
    }
  } else {
    for (int j = 0; j < nd; ++j) {
      const float p = a[j * SA] * b[j * SB];
      acc = acc + p;
    }
  }
}

// A row's d values (lane = row of a 64-row block of xb[block][dim][64], xrow = the block's base + lane) handed to f(i, x) in
// ascending i, eight loads in flight ahead of their use.
template <class F>
__device__ __forceinline__ void stream_row(const float* __restrict__ xrow, int d, F&& f) {
  constexpr int DB = 8;
  float xn[DB];
#pragma unroll
  for (int u = 0; u < DB; ++u) xn[u] = (u < d) ? xrow[(size_t)u * 64] : 0.0f;
  for (int i0 = 0; i0 < d; i0 += DB) {
    float xc[DB];
#pragma unroll
    for (int u = 0; u < DB; ++u) xc[u] = xn[u];
#pragma unroll
    for (int u = 0; u < DB; ++u) xn[u] = (i0 + DB + u < d) ? xrow[(size_t)(i0 + DB + u) * 64] : 0.0f;
#pragma unroll
    for (int u = 0; u < DB; ++u)
      if (i0 + u < d) f(i0 + u, xc[u]);
  }
}

}  // namespace freddy
