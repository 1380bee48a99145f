// ivf_sizes.h -- what the IVFADC chunk driver (ivfadc.hip) and the host-buffer pipeline (pipeline.hip) need of the kernel headers
// without their kernels: the geometry constants its workspace sizes and path choices are made of, and the probe plan's argument
// record, which a round hands from the cell selection to its scan.  No __global__ function here or in what this includes; the
// kernel headers that own these names include this file (scan_common.h, multi.h, bigk.h, coarse.h, kernels.h).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace freddy {

// ---- scan_common.h: chunk geometry of the cell-grouped scans ----
static constexpr int FUSED_T = 512;
static constexpr int FUSED_NW = FUSED_T / 64;
static constexpr int FUSED_G = 16;                                 // (query, cell) items per workgroup
static constexpr int FUSED_RMAX = 8;
static constexpr int FUSED_E = 2;                                  // codes per lane: K <= 1024
static constexpr int FUSED_UNIT_BLOCKS = FUSED_RMAX * FUSED_NW;   // 64 row blocks = 4096 rows per chunk

// ---- multi.h ----
static constexpr int MULTI_G = 8;       // items per work entry
static inline size_t multi_lds_bytes(int m, int K) { return (size_t)m * K * MULTI_G * sizeof(float) + MULTI_G * 64 * 4 + MULTI_G * 4 + 64; }

// ---- bigk.h ----
static constexpr int BIGK_KMAX = 4096;   // largest k
static constexpr int BIGK_PASS = 1024;   // keys a selection pass adds

// ---- coarse.h ----
static constexpr int COARSE_MAX_CPAD = 1024;  // the plan keeps a query's approximate distances in registers: 16 per lane
static constexpr int COARSE_STREAM_MAX_CPAD = 16384;   // beyond 1024 cells the plan streams them twice (minima, then candidates as a bitmap)

// ---- kernels.h: probe_plan_kernel's arguments (the comment in front of the kernel says what it does with them) ----
struct PlanArgs {
  const float* dist;        // [Q][Cpad]
  const int32_t* active;    // [n_active] query indices (NULL = identity)
  const int32_t* list_off;  // [C+1]
  uint32_t* used;           // [Q][used_words] bitmap of cells already probed
  int32_t* item_cell;       // [n_active*W]
  int32_t* item_query;      // [n_active*W]
  float* item_dist;         // [n_active*W] or NULL: the item's coarse distance (the scan's bound on |r|^2)
  int32_t* round_rows;      // [n_active] rows retrieved this round, -1 = no cell was left
  int32_t* cell_count;      // [C] fused path only (NULL otherwise): += items probing each cell
  int32_t* cell_items;      // [C][cell_cap] fused path: the items of each cell, in arrival order (any order is fine)
  int cell_cap;             // >= number of active queries (a query probes a cell at most once)
  int n_active, Cpad, C, W, used_words;
  float cell_limit;         // a cell at this distance or beyond is never probed: 100.0 (ivfadc_search, the cell list's
                            // sentinel, freddy.c:266-283), 1000.0 (ivfadc_batch_search, minDist of its argmin, freddy.c:855)
};

}  // namespace freddy
