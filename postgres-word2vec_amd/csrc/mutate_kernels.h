// mutate_kernels.h -- the kernels of freddy_gpu_append_rows (mutate.h): the 64-row block layout re-blocked on the device, new rows
// and raw vectors written into their slots.  freddy_gpu_update_rows rewrites rows in their slots with place_rows_kernel too.
// Everything but an update is written into fresh arrays beside the old ones; the host swaps them in once every launch has succeeded.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// new block j of list blk_cell[b] <- old block j of that list (or empty)
static __global__ __launch_bounds__(256) void repack_blocks_kernel(const uint32_t* __restrict__ old_packed, const int32_t* __restrict__ old_pos,
                                                           const int32_t* __restrict__ old_blk_off, const int32_t* __restrict__ new_blk_off,
                                                           const int32_t* __restrict__ new_blk_cell, uint32_t* __restrict__ packed,
                                                           int32_t* __restrict__ pos, int64_t n_new_blocks, int M2) {
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (b >= n_new_blocks) return;
  const int c = new_blk_cell[b];
  const int j = (int)(b - new_blk_off[c]);
  const bool have = j < old_blk_off[c + 1] - old_blk_off[c];
  const int64_t ob = (int64_t)old_blk_off[c] + j;
  for (int w = 0; w < M2; ++w) packed[((size_t)b * M2 + w) * 64 + lane] = have ? old_packed[((size_t)ob * M2 + w) * 64 + lane] : 0u;
  pos[(size_t)b * 64 + lane] = have ? old_pos[(size_t)ob * 64 + lane] : -1;
}
// new rows into their slots: slot[i] = row slot (block * 64 + lane) of new row i
static __global__ __launch_bounds__(256) void place_rows_kernel(const int64_t* __restrict__ slot, const int32_t* __restrict__ row_pos,
                                                        const int16_t* __restrict__ codes, int64_t n, uint32_t* __restrict__ packed,
                                                        int32_t* __restrict__ pos, int m, int M2) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t sl = slot[i], b = sl >> 6;
  const int lane = (int)(sl & 63);
  for (int w = 0; w < M2; ++w) {
    const uint32_t lo = (uint16_t)codes[(size_t)i * m + 2 * w];
    const uint32_t hi = (2 * w + 1 < m) ? (uint16_t)codes[(size_t)i * m + 2 * w + 1] : 0u;
    packed[((size_t)b * M2 + w) * 64 + lane] = lo | (hi << 16);
  }
  pos[(size_t)sl] = row_pos[i];
}
// raw vectors into the 64-row blocked layout: row r -> xb[r / 64][dim][r % 64]
static __global__ __launch_bounds__(256) void place_vectors_kernel(const float* __restrict__ src, int64_t first_row, int64_t n, float* __restrict__ xb, int d) {
  const int64_t i = (int64_t)blockIdx.x;
  if (i >= n) return;
  const int64_t r = first_row + i;
  for (int dim = threadIdx.x; dim < d; dim += 256) xb[((r >> 6) * d + dim) * 64 + (r & 63)] = src[(size_t)i * d + dim];
}
