// update_kernels.h -- the kernels of freddy_gpu_update_rows (mutate.h): rows of a pinned index that keep their id and get a new payload.
//   pq / ivf   64-row blocks [block][M2][64] + pos: where the rows of the update set sit (up_locate_kernel); their code words are
//              then rewritten in their slots (place_rows_kernel, mutate_kernels.h).  An ivf row that changes its cell leaves its list
//              (remove_kernels.h) and joins the end of the new one (append_packed_rows).
//   ivpq / vectors   row-major arrays: dst[row[j]] <- src[j] (up_scatter_rows_kernel), the mirror of rm_gather_rows_kernel; the
//              64-row blocks of a vector handle for a list of rows (up_place_vectors_kernel; place_vectors_kernel takes one run)
// Every index these kernels receive (rows, slots) was derived and bounds-checked on the host; nothing is allocated or resized.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// One wave per 64-row block: every slot looks its pos up in the n_upd ascending, distinct values of upd (ids for an ivf handle, row
// indices for the flat table).  A hit at entry j records slot[j] = block * 64 + lane and cell[j] = the block's list.  slot[] comes
// in as -1 everywhere: an entry that no slot holds stays -1.  (A pos occurs once in the layout, so no two lanes write one entry.)
static __global__ __launch_bounds__(256) void up_locate_kernel(const int32_t* __restrict__ pos, const int32_t* __restrict__ blk_cell, int64_t n_blocks,
                                                               const int32_t* __restrict__ upd, int n_upd, int64_t* __restrict__ slot,
                                                               int32_t* __restrict__ cell) {
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (b >= n_blocks) return;
  const int32_t p = pos[(size_t)b * 64 + lane];
  if (p < 0) return;
  int lo = 0, hi = n_upd;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (upd[mid] < p) lo = mid + 1; else hi = mid;
  }
  if (lo < n_upd && upd[lo] == p) {
    slot[lo] = b * 64 + lane;
    cell[lo] = blk_cell[b];
  }
}

// Row-major arrays of `wpr` 4-byte words per row: dst row rows[j] <- src row j, j < n.  rows[] holds distinct row indices inside dst.
static __global__ __launch_bounds__(256) void up_scatter_rows_kernel(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst,
                                                                     const int32_t* __restrict__ rows, int64_t n, int wpr) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n * wpr) return;
  const int64_t j = i / wpr;
  const int w = (int)(i - j * wpr);
  dst[(size_t)rows[j] * wpr + w] = src[i];
}

// raw vectors into the 64-row blocked layout, one workgroup per row: row rows[i] -> xb[r / 64][dim][r % 64]
static __global__ __launch_bounds__(256) void up_place_vectors_kernel(const float* __restrict__ src, const int32_t* __restrict__ rows, int64_t n,
                                                                      float* __restrict__ xb, int d) {
  const int64_t i = (int64_t)blockIdx.x;
  if (i >= n) return;
  const int64_t r = rows[i];
  for (int dim = threadIdx.x; dim < d; dim += 256) xb[((r >> 6) * d + dim) * 64 + (r & 63)] = src[(size_t)i * d + dim];
}
