// chunk_plan.h -- how many queries of a search call share one workspace (option lut_budget_mb), in plain C++: the chunk sizes of the
// IVFADC calls (ivfadc.hip, pipeline.hip) and of the flat PQ table's two paths (pq.hip) as functions of plain integers.  The
// callers pass their handle's fields and cut the call with for_chunks (ivf_run.h).  No HIP here: tests/test_chunk_plan_cpu.py builds
// it into a program of its own and compares it with the restatement in tests/chunk_inputs.py.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "ivf_sizes.h"   // FUSED_NW, FUSED_RMAX, FUSED_UNIT_BLOCKS: a survivor region; BIGK_PASS: the keys a selection pass keeps

namespace freddy {

// bytes of the survivor regions of one 4096-row unit: FUSED_NW gatherer waves x FUSED_RMAX x 64 keys of 8 bytes (32 KiB)
static constexpr size_t SURV_UNIT_BYTES = sizeof(uint64_t) * FUSED_NW * FUSED_RMAX * 64;
// the cell-grouped scans' per-cell item buckets ([cells or pseudo-lists][queries of the chunk], int32) stay within this
static constexpr size_t BUCKET_BYTES = (size_t)256 << 20;
// row blocks per chunk of the generic IVFADC scan once a round has many items (ivf_run.h generic_chunks: the coarse chunks)
static constexpr int GENERIC_MANY_BLOCKS = 256;

// ---- IVFADC: freddy_gpu_ivfadc_search_dev, the stragglers' re-search and the cap of a host-buffer call's sub-batches ----------------
// Workspace per query: the LUTs of its W items (generic path) or their survivor regions (cell-grouped scans).
//   upi               survivor units (4096-row chunks of the longest list) per (query, cell) item: units_per_item
//   special           the 300-d shape of fused5.h (fused_shape): LUTs OR survivor regions, whichever is larger; every other shape may
//                     take multi.h, which holds the LUTs of all items AND their survivor regions
//   max_list_blocks   row blocks of the longest list: the generic scan's chunks per item
static inline int max_queries_per_chunk(int64_t budget_mb, int m, int K, int W, int k, int upi, bool special, int C, int max_list_blocks) {
  size_t lut_bytes = sizeof(float) * (size_t)m * K * (size_t)W;
  if (2 * k > 64) {
    // lists beyond the cell-grouped scans' selection width take the generic kernels: one list of L keys per (item, chunk) beside
    // the LUTs, and from k = 513 on the passes' selected keys (bigk.h: ceil(2k / 1024) x 1024 per query)
    const size_t L = (size_t)std::min(2 * k, 1024);
    const size_t nchunk = (size_t)std::max(1, (max_list_blocks + GENERIC_MANY_BLOCKS - 1) / GENERIC_MANY_BLOCKS);
    lut_bytes += sizeof(uint64_t) * (size_t)W * nchunk * L;
    if (2 * k > 1024) lut_bytes += sizeof(uint64_t) * (size_t)((2 * k + BIGK_PASS - 1) / BIGK_PASS) * BIGK_PASS;
  }
  // (lists of more units than the cell-grouped scan of the shape takes: no survivor regions)
  const size_t surv_bytes = (size_t)upi <= (special ? 8u : 32u) ? (size_t)W * (size_t)upi * SURV_UNIT_BYTES : 0;
  const size_t per_query = special ? std::max(lut_bytes, surv_bytes) : lut_bytes + surv_bytes;
  size_t n = ((size_t)budget_mb << 20) / std::max<size_t>(per_query, 1);
  if (surv_bytes) n = std::min<size_t>(n, BUCKET_BYTES / (sizeof(int32_t) * (size_t)std::max(C, 1)));
  if (n < 1) n = 1;
  if (n > (1u << 20)) n = 1u << 20;
  return (int)n;
}

// ---- the flat PQ table through the cell-grouped scan (pq_fused_chunk) ------------------------------------------------------------------
// survivor regions: 32 KiB per (query, pseudo-list of 4096 rows) within the budget; the buckets [lists][queries] within 256 MiB;
// never fewer than 16 queries (a group of the records), never more than 2^16.  (pq_fused_shape keeps a table without row blocks off
// this path; counted as one pseudo-list here, so that nothing divides by zero)
static inline int pq_fused_queries_per_chunk(int64_t budget_mb, int64_t n_blocks) {
  const size_t lists = (size_t)std::max<int64_t>(1, (n_blocks + FUSED_UNIT_BLOCKS - 1) / FUSED_UNIT_BLOCKS);
  size_t n = ((size_t)budget_mb << 20) / (lists * SURV_UNIT_BYTES);
  n = std::min<size_t>(n, BUCKET_BYTES / (sizeof(int32_t) * lists));
  return (int)std::max<size_t>(16, std::min<size_t>(n, 1u << 16));
}

// ---- the flat PQ table through the generic scan (pq_chunk) ---------------------------------------------------------------------------
// a LUT per query, one list of L keys per (query, 4096-row chunk) -- the finest chunks pq_chunk may choose -- and, from k = 513 on,
// the keys the selection passes keep (bigk.h)
static inline int pq_queries_per_chunk(int64_t budget_mb, int m, int K, int64_t n_blocks, int k) {
  const size_t L = (size_t)std::min(2 * k, 1024), nchunk = (size_t)std::max<int64_t>(1, (n_blocks + 63) / 64);
  size_t per_query = sizeof(float) * (size_t)m * K + sizeof(uint64_t) * nchunk * L;
  if (2 * k > 1024) per_query += sizeof(uint64_t) * (size_t)((2 * k + BIGK_PASS - 1) / BIGK_PASS) * BIGK_PASS;
  const size_t n = ((size_t)budget_mb << 20) / per_query;
  return (int)std::min<size_t>(std::max<size_t>(n, 1), (size_t)1 << 20);
}

}  // namespace freddy
