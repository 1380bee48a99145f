// stat_kernels.h -- the kernels of freddy_gpu_create_statistics (join.hip): create_statistics() of the reference
// (freddy--0.0.1.sql:150-171) over the rows a pinned ivpq handle holds.
//
// The SQL is `cells` three-way joins, one count per cell.  Here it is one histogram: every entry of the column (an id, with its
// multiplicity) is resolved to its row and counted in that row's cell; a second, one-workgroup kernel divides.  Counts are
// 64-bit INTEGERS everywhere, so the result does not depend on the order the atomics arrive in, a count above 2^24 is not
// rounded before the division, and a column of more than 2^31 entries does not wrap.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dot_chain.h"   // row_of_id

namespace freddy {

static constexpr int STAT_WG = 256;
// Up to this many cells a workgroup counts in a histogram of its own in LDS (32-bit bins: one launch gives a workgroup far
// fewer than 2^32 entries) and flushes the bins that are not zero with ONE 64-bit global atomic each.  16 KiB: ten such
// workgroups fit the 160 KiB of a CU, more than the eight (32 waves / 4) a CU runs at a time, so the histogram never limits
// occupancy; and a workgroup of a full pass has 4096 entries or more to count, so above 4096 cells it would clear and flush
// more bins than it counts entries, and the entries go to the global counters directly.
static constexpr int STAT_LDS_CELLS = 4096;
static constexpr int STAT_PER_LANE = 16;      // entries per lane the grid is sized for (grid-stride beyond that)
static constexpr int STAT_MAX_GRID = 1024;

// One lane per entry (grid-stride).  tids: the entries' ids, resolved to rows the way join_mark_kernel does -- ids[r] == ids[0]
// + r (affine) or a binary search over the ascending ids; an id no row has is skipped, and nothing is de-duplicated: an id listed
// r times counts r times (the SQL is an INNER JOIN with the column).  tids == NULL: entry i IS row row0 + i (every pinned row
// once).  count[cells]: zeroed by the caller before the first pass.
template <bool LDS_HIST>
__global__ __launch_bounds__(STAT_WG) void stat_count_kernel(const int32_t* __restrict__ tids, int64_t n, int64_t row0,
                                                            const int32_t* __restrict__ ids, int64_t N, int affine,
                                                            const int32_t* __restrict__ cell, int cells,
                                                            unsigned long long* __restrict__ count) {
  extern __shared__ uint32_t stat_bins[];   // [cells] (LDS_HIST)
  if (LDS_HIST) {
    for (int c = threadIdx.x; c < cells; c += STAT_WG) stat_bins[c] = 0u;
    __syncthreads();
  }
  const int64_t step = (int64_t)gridDim.x * STAT_WG;
  for (int64_t i = (int64_t)blockIdx.x * STAT_WG + threadIdx.x; i < n; i += step) {
    int64_t r = -1;
    if (!tids) {
      r = row0 + i;
      if (r >= N) r = -1;
    } else if (affine) {
      const int64_t c = (int64_t)tids[i] - ids[0];
      if (c >= 0 && c < N) r = c;
    } else {
      r = row_of_id(ids, N, tids[i]);
    }
    if (r < 0) continue;
    const int c = cell[r];
    if ((unsigned)c >= (unsigned)cells) continue;   // (pin / append / update refuse such a cell: never taken, and never out of bounds)
    if (LDS_HIST) atomicAdd(&stat_bins[c], 1u);
    else atomicAdd(&count[c], 1ull);
  }
  if (LDS_HIST) {
    __syncthreads();
    for (int c = threadIdx.x; c < cells; c += STAT_WG) {
      const uint32_t v = stat_bins[c];
      if (v) atomicAdd(&count[c], (unsigned long long)v);
    }
  }
}

// One workgroup.  total = the sum of the counts (the entries that have a row), then
//   row[c]     = (float)((double)count[c] / (double)total)     "count(*)::float / total_amount" (:166): float8, stored as float4
//   row[cells] = (float)total                                   (:168) bigint -> float4, round to nearest even
// in IEEE binary64 / binary32: counts below 2^53 convert to double exactly, the division is the correctly rounded one (this
// library is built without fast-math), and double -> float rounds once, to nearest even.  The row goes to the device (what an
// install copies into the handle's row) and to mapped host memory together with the exact total; total == 0 writes the total
// alone (the SQL's division by zero: the host refuses the call).
__global__ __launch_bounds__(STAT_WG) void stat_finish_kernel(const unsigned long long* __restrict__ count, int cells,
                                                             float* __restrict__ row, float* __restrict__ row_host,
                                                             unsigned long long* __restrict__ total_host) {
  __shared__ unsigned long long part[STAT_WG];
  const int tid = threadIdx.x;
  unsigned long long sum = 0;
  for (int c = tid; c < cells; c += STAT_WG) sum += count[c];
  part[tid] = sum;
  __syncthreads();
  for (int o = STAT_WG / 2; o > 0; o >>= 1) {
    if (tid < o) part[tid] += part[tid + o];
    __syncthreads();
  }
  const unsigned long long total = part[0];
  if (tid == 0) *total_host = total;
  if (total == 0) return;
  const double t = (double)total;
  for (int c = tid; c <= cells; c += STAT_WG) {
    const float v = (c < cells) ? (float)((double)count[c] / t) : (float)t;
    row[c] = v;
    row_host[c] = v;
  }
}

}  // namespace freddy
