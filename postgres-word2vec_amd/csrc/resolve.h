// resolve.h -- "id = ANY(set)" on a pinned vector table, resolved where it is used: ids[n] -> the ascending, distinct table rows of
// the ids that have one, in device memory.  The result equals rows_of_ids (internal.h): unknown ids vanish, duplicates collapse,
// the order is table order -- but nothing is sorted: the set is a bitmap over the table's rows (bit r & 31 of word r >> 5), which is
// ordered and duplicate-free by construction.
//   resolve_mark_kernel    one lane per id: its row (the serial-id probe of row_of_near first, then row_of_id's binary search --
//                          the same row either way), and an atomicOr of the row's bit.  The bitmap was cleared by a memset.
//   resolve_count_kernel   one wave per block of `B` bitmap words (option resolve_block): the block's popcount -> cnt[b], and added
//                          to part[b / SIM_CHUNK], the sums sim_scan_kernel takes per chunk of 1024 counts (integer atomicAdd: the
//                          order of the additions changes nothing).  part lies behind the bitmap and is cleared with it.
//   sim_scan_kernel        (similarity.h, the join's own scan, unchanged) off[b] = rows before block b, off[n_blocks] = all rows.
//   resolve_place_kernel   one wave per block: 64 words per step, an exclusive prefix of their popcounts over the lanes, and every
//                          lane writes word * 32 + bit for its set bits, ascending, at off[b] + the prefix.  No atomics, no LDS.
//                          Its first thread also writes the total to a word of mapped host memory: all the host needs of the set.
// Three levels carry a row's position: the lanes' prefix inside a 64-word step (with the running sum of the steps before it, when
// B > 64), the block offsets of the scan, and the chunk sums behind the scan once a table has more than 1024 blocks (8.4 M rows at the
// default B = 256; a 40 000-row table at B = 1).
// Bounds: a row r < N sets a bit of word r >> 5 < ceil(N / 32); no bit at or beyond N is ever set, so the place kernel writes
// exactly popcount(bitmap) <= min(n, N) rows: what out_rows is sized for before anything is launched.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "similarity.h"

namespace freddy {

// Bitmap words per block (option resolve_block): four 64-word steps of a wave.  tools/exact_ids_timing.py (profiles/exact_ids_timing.txt)
// timed 64 and 256 over 3 M rows: 256 takes 10 us less for sets of up to 100 000 ids (a quarter of the counts, their additions to the
// chunk sums and the scan) and the same for 3 M ids; over 200 000 rows 64 was 7 us ahead at 100 000 ids.
static constexpr int RESOLVE_BLOCK = 256;

__device__ __forceinline__ int32_t resolve_row_of(const int32_t* __restrict__ vec_ids, int64_t N, int32_t id) {
  if (N <= 0) return -1;
  const int64_t g = (int64_t)id - (int64_t)vec_ids[0];   // serial ids: the row itself (strictly ascending ids: never less than the row)
  if (g < 0) return -1;
  if (g < N && vec_ids[g] == id) return (int32_t)g;
  return row_of_id(vec_ids, N, id);
}

static __global__ __launch_bounds__(256) void resolve_mark_kernel(const int32_t* __restrict__ ids, int64_t n, const int32_t* __restrict__ vec_ids,
                                                                  int64_t N, uint32_t* __restrict__ bitmap) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    const int32_t r = resolve_row_of(vec_ids, N, ids[i]);
    if (r >= 0) atomicOr(bitmap + (r >> 5), 1u << (r & 31));
  }
}

// n_words = ceil(N / 32) bitmap words in n_blocks = ceil(n_words / B) blocks
static __global__ __launch_bounds__(256) void resolve_count_kernel(const uint32_t* __restrict__ bitmap, int64_t n_words, int B, int64_t n_blocks,
                                                                   int32_t* __restrict__ cnt, int32_t* __restrict__ part) {
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * 4;
  for (int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); b < n_blocks; b += stride) {
    const int64_t w0 = b * B, w1 = (w0 + B < n_words) ? w0 + B : n_words;
    int32_t c = 0;
    for (int64_t w = w0 + lane; w < w1; w += 64) c += __popc(bitmap[w]);
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if (lane == 0) {
      cnt[b] = c;
      if (c) atomicAdd(part + b / SIM_CHUNK, c);
    }
  }
}

static __global__ __launch_bounds__(256) void resolve_place_kernel(const uint32_t* __restrict__ bitmap, int64_t n_words, int B, int64_t n_blocks,
                                                                   const int32_t* __restrict__ off, int32_t* __restrict__ out_rows,
                                                                   int32_t* __restrict__ total_out) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *total_out = off[n_blocks];
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * 4;
  for (int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); b < n_blocks; b += stride) {
    int32_t base = off[b];
    if (off[b + 1] == base) continue;   // (uniform over the wave: no row in this block)
    const int64_t w0 = b * B, w1 = (w0 + B < n_words) ? w0 + B : n_words;
    for (int64_t ws = w0; ws < w1; ws += 64) {
      const int64_t w = ws + lane;
      uint32_t v = w < w1 ? bitmap[w] : 0u;
      const int32_t mine = __popc(v);
      int32_t inc = mine;
      for (int o = 1; o < 64; o <<= 1) {
        const int32_t up = __shfl_up(inc, o, 64);
        if (lane >= o) inc += up;
      }
      int32_t p = base + inc - mine;
      const int32_t r0 = (int32_t)(w * 32);
      while (v) {
        out_rows[p++] = r0 + (__ffs(v) - 1);
        v &= v - 1;
      }
      base += __shfl(inc, 63, 64);
    }
  }
}

}  // namespace freddy
