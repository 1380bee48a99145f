// remove_kernels.h -- the kernels of freddy_gpu_remove_rows (mutate.h): a stable compaction of the pinned layouts on the device.
//   pq / ivf   64-row blocks [block][M2][64] + pos: keep mask and kept count per block (rm_mark_kernel), exclusive scan of the
//              counts inside every list (rm_list_scan_kernel), the kept lanes to their new slots (rm_scatter_kernel), code 0 /
//              pos -1 behind a list's last row (rm_fill_tail_kernel)
//   ivpq / vectors / the flat table's ids   row-major arrays: new row r reads old row r + (removed rows before it) (rm_gather_rows_kernel)
// Everything is written into fresh arrays beside the old ones; the host swaps them in once every launch has succeeded.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// is `v` one of the n ascending, distinct values of rm?
static __device__ __forceinline__ bool rm_contains(const int32_t* __restrict__ rm, int n, int32_t v) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (rm[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo < n && rm[lo] == v;
}

// One wave per 64-row block: which of its slots stay (pos >= 0 and not in the removal set -- ids for an ivf handle, row indices
// for the flat table), as a 64-bit mask and a count; the largest pos that stays goes into *max_pos (ivf: the new max_id).
static __global__ __launch_bounds__(256) void rm_mark_kernel(const int32_t* __restrict__ pos, int64_t n_blocks, const int32_t* __restrict__ rm, int n_rm,
                                                             unsigned long long* __restrict__ keep_mask, int32_t* __restrict__ keep_cnt,
                                                             int32_t* __restrict__ max_pos) {
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (b >= n_blocks) return;
  const int32_t p = pos[(size_t)b * 64 + lane];
  const bool keep = p >= 0 && !rm_contains(rm, n_rm, p);
  const unsigned long long mask = __ballot(keep);
  int32_t mx = keep ? p : -1;
  for (int o = 32; o > 0; o >>= 1) mx = max(mx, __shfl_xor(mx, o, 64));
  if (lane == 0) {
    keep_mask[b] = mask;
    keep_cnt[b] = __popcll(mask);
    if (mx >= 0) atomicMax(max_pos, mx);
  }
}

// One workgroup per list: prefix[b] = rows kept in the list's blocks before block b, list_keep[c] = rows kept in the list.  A list
// of more than 256 blocks is walked 256 blocks at a time with a running carry.
static __global__ __launch_bounds__(256) void rm_list_scan_kernel(const int32_t* __restrict__ blk_off, const int32_t* __restrict__ keep_cnt,
                                                                  int32_t* __restrict__ prefix, int32_t* __restrict__ list_keep) {
  __shared__ int32_t wave_sum[4];
  const int c = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int64_t b0 = blk_off[c], nb = (int64_t)blk_off[c + 1] - b0;
  int32_t carry = 0;
  for (int64_t base = 0; base < nb; base += 256) {
    const bool have = base + t < nb;
    const int32_t v = have ? keep_cnt[b0 + base + t] : 0;
    int32_t inc = v;
    for (int o = 1; o < 64; o <<= 1) {
      const int32_t u = __shfl_up(inc, o, 64);
      if (lane >= o) inc += u;
    }
    if (lane == 63) wave_sum[w] = inc;
    __syncthreads();
    int32_t before = 0, total = 0;
    for (int i = 0; i < 4; ++i) { if (i < w) before += wave_sum[i]; total += wave_sum[i]; }
    if (have) prefix[b0 + base + t] = carry + before + inc - v;
    carry += total;
    __syncthreads();
  }
  if (t == 0) list_keep[c] = carry;
}

// One wave per OLD block: every kept lane to slot new_blk_off[c] * 64 + prefix + (its rank among the block's kept lanes).
// renumber: the flat table -- pos is the row index, which is the new slot.
static __global__ __launch_bounds__(256) void rm_scatter_kernel(const uint32_t* __restrict__ old_packed, const int32_t* __restrict__ old_pos,
                                                                const int32_t* __restrict__ old_blk_cell, const int32_t* __restrict__ new_blk_off,
                                                                const unsigned long long* __restrict__ keep_mask, const int32_t* __restrict__ prefix,
                                                                int64_t n_old_blocks, int64_t n_new_slots, int M2, int renumber,
                                                                uint32_t* __restrict__ packed, int32_t* __restrict__ pos) {
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (b >= n_old_blocks) return;
  const unsigned long long mask = keep_mask[b];
  if (!((mask >> lane) & 1ull)) return;
  const int rank = __popcll(mask & ((1ull << lane) - 1ull));
  const int c = old_blk_cell[b];
  const int64_t first = (int64_t)new_blk_off[c] * 64;
  const int64_t slot = first + prefix[b] + rank;
  if (slot >= n_new_slots) return;   // (cannot happen with a consistent scan: never write past the fresh arrays)
  const int64_t nb = slot >> 6;
  const int nl = (int)(slot & 63);
  for (int w = 0; w < M2; ++w) packed[((size_t)nb * M2 + w) * 64 + nl] = old_packed[((size_t)b * M2 + w) * 64 + lane];
  pos[(size_t)slot] = renumber ? (int32_t)(slot - first) : old_pos[(size_t)b * 64 + lane];
}

// One wave per list: the free slots of its last block get code 0 / pos -1 (as pack_lists leaves them).
static __global__ __launch_bounds__(256) void rm_fill_tail_kernel(const int32_t* __restrict__ new_list_off, const int32_t* __restrict__ new_blk_off,
                                                                  int n_lists, int M2, uint32_t* __restrict__ packed, int32_t* __restrict__ pos) {
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (c >= n_lists) return;
  const int len = new_list_off[c + 1] - new_list_off[c];
  if ((len & 63) == 0 || lane < (len & 63)) return;
  const int64_t b = (int64_t)new_blk_off[c + 1] - 1;
  for (int w = 0; w < M2; ++w) packed[((size_t)b * M2 + w) * 64 + lane] = 0u;
  pos[(size_t)b * 64 + lane] = -1;
}

// Row-major arrays of `wpr` 4-byte words per row: new row r <- old row r + j, j = the number of removed rows before it.  rm_rows:
// the n_rm removed OLD row indices, ascending and distinct, so key[j] = rm_rows[j] - j does not decrease and j = the number of keys
// <= r.  One workgroup moves 64 rows: their source rows once, then every word with coalesced loads and stores.
static __global__ __launch_bounds__(256) void rm_gather_rows_kernel(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst,
                                                                    const int32_t* __restrict__ rm_rows, int n_rm, int64_t n_new, int wpr) {
  __shared__ int64_t src_row[64];
  const int64_t r0 = (int64_t)blockIdx.x * 64;
  if (threadIdx.x < 64) {
    const int64_t r = r0 + threadIdx.x;
    int lo = 0, hi = n_rm;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if ((int64_t)rm_rows[mid] - mid <= r) lo = mid + 1; else hi = mid;
    }
    src_row[threadIdx.x] = r + lo;
  }
  __syncthreads();
  const int rows = (int)(n_new - r0 < 64 ? n_new - r0 : 64);
  for (int i = threadIdx.x; i < rows * wpr; i += 256) {
    const int r = i / wpr, w = i - r * wpr;
    dst[(size_t)(r0 + r) * wpr + w] = src[(size_t)src_row[r] * wpr + w];
  }
}
