// exact_join.h -- the exact kNN-join (knn_search_in_batch, freddy--0.0.1.sql:456-501: one knn_in_exact per query over a target
// set) as FILTER + REFINE on the matrix cores, all query tiles in a fixed number of launches.
//
// exact2.h ranks the rows of the WHOLE table with f16-split MFMA products a ~ x . q inside a proven bracket |a - s| <= eps(q)
// and evaluates the reference's binary32 chain only for the rows whose bracket reaches the k-th largest similarity.  A target
// set is a subset of the table's rows, so eps(q) = EXF_EPS X |q| with X the TABLE's largest row norm bounds its rows too: the
// bracket carries over unchanged.  What differs is the shape of the work: Q queries (thousands) against n_targets rows (a
// hundred thousand) instead of <= 64 queries against millions, so
//
//   exj_gather_kernel   the target rows (row-major copy, positions from rows_of_ids) -> a fragment-order f16 hi / lo copy in the
//                       workspace, the table's scale, last strip zero padded: n_targets d 4 bytes, written once per call
//   exf_prep_kernel     (exact2.h, one launch over all Q queries: its indexing is per query) norms, scales, B fragments, eps
//   exj_filter_kernel   <NT, SAMPLE = true>: a for the sample rows of every query; grid = (strip chunks, query tiles)
//   exf_threshold_kernel (exact2.h, one workgroup per query) tau -> the scaled threshold, candidate counters zeroed
//   exj_filter_kernel   <NT, false>: candidates (TABLE row, a) of every query into its own buffer
//   exf_refine_kernel   (exact2.h, one workgroup per query) the reference's chain, the bracket self-check, the list
//
// one gather and five launches per pass of queries (a pass holds 10 880 or more: exact.hip EXJ_PASS_BYTES; the five are exact kNN's chain, exact_host.h exf_chain).  A query whose
// candidate buffer overflowed is answered again by the all-exact subset path (the host reads the counters); nothing is dropped.
//
// Query-tile width: a workgroup's 8 waves share one LDS image of NT 32-column tiles and every wave streams its own 32-row
// strips past it.  The gathered copy is re-read once per query tile, so its traffic is (Q / 32 NT) n_targets d 4 bytes: at
// 5 000 x 100 000 x 300, 9.4 GB for NT = 2 and 4.7 GB for NT = 4 against 0.9 PFLOP-equivalents of MFMA work -- NT = 4 (128
// queries, 152 KiB of LDS at d = 300, one workgroup per CU) halves the bytes per flop.  NT = 4 needs T <= 20 (d <= 320).
#pragma once
#include "exact2.h"

namespace freddy {

// xf[strip][k-step t][hi / lo][lane]: exf_layout_kernel's layout for the rows map[0 .. n_targets) of the row-major table
__global__ __launch_bounds__(256) void exj_gather_kernel(const float* __restrict__ rows, const int32_t* __restrict__ map, int64_t n_targets,
                                                        int d, int T, int ex, h8v* __restrict__ xf) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;      // (strip, t, lane)
  const int64_t n_strips = (n_targets + 31) >> 5;
  if (i >= n_strips * T * 64) return;
  const int lane = (int)(i & 63);
  const int64_t st = i >> 6;
  const int t = (int)(st % T);
  const int64_t strip = st / T;
  const int64_t p = strip * 32 + (lane & 31);
  const int dim0 = 16 * t + 8 * (lane >> 5);
  float v[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  if (p < n_targets) {                                            // (d % 4 == 0: whole float4s)
    const float* x = rows + (size_t)map[p] * d + dim0;
    if (dim0 + 4 <= d) { const float4 a = *reinterpret_cast<const float4*>(x); v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; }
    if (dim0 + 8 <= d) { const float4 a = *reinterpret_cast<const float4*>(x + 4); v[4] = a.x; v[5] = a.y; v[6] = a.z; v[7] = a.w; }
  }
  h8v hi, lo;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float s = __builtin_ldexpf(v[e], ex);
    const _Float16 h = (_Float16)s;
    hi[e] = h;
    lo[e] = (_Float16)(s - (float)h);
  }
  xf[((size_t)(strip * T + t) * 2 + 0) * 64 + lane] = hi;
  xf[((size_t)(strip * T + t) * 2 + 1) * 64 + lane] = lo;
}

struct ExjArgs {
  const h8v* xf;            // the gathered target rows in fragment order
  const int32_t* map;       // [n_targets] position in the target set -> row of the table
  int64_t n_rows;           // rows of this launch (SAMPLE: whole strips)
  int64_t strip_stride;     // SAMPLE: strip i of the launch is strip i * strip_stride of the copy; 1 otherwise
  int T, nq;                // k-steps; queries of the call (columns beyond them never produce a candidate)
  const h8v* qfrag;         // [32-column tile][T][2][64]
  const float* qunscale;    // [padded Q]
  float* sample_out;        // SAMPLE: [padded Q][n_rows]
  const float* thr;         // [padded Q] scaled thresholds
  int32_t* cand_cnt;        // [padded Q]
  uint2* cand;              // [Q][cap] (table row, bits of the approximate similarity)
  int cap;
};

// blockIdx.y = the query tile (NT x 32 queries), blockIdx.x = the chunk of strips; a wave per strip.
template <int NT, bool SAMPLE>
__global__ __launch_bounds__(EXF_WG, NT <= 2 ? 2 : 1) void exj_filter_kernel(ExjArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  h8v* qf = reinterpret_cast<h8v*>(smem);                  // [NT][T][2][64]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int T = a.T;
  const int q0 = (int)blockIdx.y * 32 * NT;
  {
    const uint4* src = reinterpret_cast<const uint4*>(a.qfrag + (size_t)blockIdx.y * NT * T * 128);
    uint4* dst = reinterpret_cast<uint4*>(smem);
    const int n16 = NT * T * 2 * 64;
    for (int i = tid; i < n16; i += EXF_WG) dst[i] = src[i];
  }
  __syncthreads();
  const int i_row = lane & 31, g = lane >> 5;
  float thr[NT], unsc[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    thr[n] = SAMPLE ? 0.0f : a.thr[q0 + 32 * n + i_row];
    unsc[n] = a.qunscale[q0 + 32 * n + i_row];
  }
  const int64_t n_strips = (a.n_rows + 31) >> 5;
  for (int64_t strip = (int64_t)blockIdx.x * (EXF_WG / 64) + wave; strip < n_strips; strip += (int64_t)gridDim.x * (EXF_WG / 64)) {
    f16acc acc[NT];
    exf_strip_mfma<NT>(a.xf + (size_t)(SAMPLE ? strip * a.strip_stride : strip) * T * 128 + lane, qf, T, lane, acc);
    // C layout: register v of lane l = row (v & 3) + 8 (v >> 2) + 4 (l >> 5) of the strip, column l & 31
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      const int q = q0 + 32 * n + i_row;
      if constexpr (SAMPLE) {                              // (whole strips, n_rows % 32 == 0: four rows of a column are one 16-byte store)
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          const int64_t r = strip * 32 + 8 * w + 4 * g;
          float4 o;
          o.x = acc[n][4 * w + 0] * unsc[n]; o.y = acc[n][4 * w + 1] * unsc[n]; o.z = acc[n][4 * w + 2] * unsc[n]; o.w = acc[n][4 * w + 3] * unsc[n];
          if (r + 3 < a.n_rows) *reinterpret_cast<float4*>(a.sample_out + (size_t)q * a.n_rows + r) = o;
        }
      } else {
#pragma unroll
        for (int v = 0; v < 16; ++v) {
          const int64_t r = strip * 32 + (v & 3) + 8 * (v >> 2) + 4 * g;
          if (!(acc[n][v] < thr[n]) && r < a.n_rows && q < a.nq) {     // (a NaN passes: the refine stage decides)
            const int slot = atomicAdd(a.cand_cnt + q, 1);
            if (slot < a.cap) a.cand[(size_t)q * a.cap + slot] = uint2{(uint32_t)a.map[r], __float_as_uint(acc[n][v] * unsc[n])};
          }
        }
      }
    }
  }
}

}  // namespace freddy
