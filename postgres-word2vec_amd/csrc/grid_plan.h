// grid_plan.h -- every launch whose grid, or whose choice of kernel, comes from the handle's CU count (freddy_gpu_index::n_cus:
// the device's count, or less under option grid_cus): the formulas as pure functions of (n_cus, work sizes, options), one
// statement of each.  ivf_scan.hip, one.hip, pq.hip, exact.hip and its sibling units and exact_host.h call them; the kernels behind them loop over the work a
// smaller grid leaves (grid-stride loops, work counters, units dealt round G workgroups), so no value of n_cus >= 1 changes a
// result -- tests/test_gpu_grid_cus.py runs them at 1, 2, 3 and 7.
// Plain C++17, no HIP, so that tests/test_grid_inputs_cpu.py compiles this file on its own with g++ (as block_plan.h is).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

namespace freddy {

// Option grid_cus: v <= 0 = the device's count, else never above it (the one-launch kernels' workgroups wait for each other
// and must be co-resident: the option may only shrink grids).
inline int grid_cus_value(int64_t v, int device_cus) { return v <= 0 ? device_cus : (int)std::min<int64_t>(v, device_cus); }

// ---- the persistent scans of an IVFADC batch (ivf_scan.hip) ----
// CUs a batch's filter scan may take: its share of the chip (32 at least, where the chip has them), less the reserved ones.
// May be <= 0: the callers take max(1, .).
inline int scan_cus(int n_cus, int share, int reserve_cus) { return std::max(n_cus / std::max(1, share), std::min(n_cus, 32)) - reserve_cus; }
// the filter scan's guaranteed workgroups: one per CU of its share, never more than there are work entries
inline unsigned filter_scan_own(int n_cus, int share, int reserve_cus, size_t max_groups) {
  return (unsigned)std::min<size_t>(max_groups, (size_t)std::max(1, scan_cus(n_cus, share, reserve_cus)));
}
// scan workgroups that may be alive over all streams of a handle under option scan_elastic (negative: no extras)
inline int filter_scan_cap(int n_cus, int elastic_reserve, int reserve_cus, int share) { return n_cus - elastic_reserve - reserve_cus * share; }
// the filter scan's grid: the guaranteed workgroups, and with `elastic` the extras up to the cap
inline unsigned filter_scan_persist(bool elastic, unsigned n_own, int cap, size_t max_groups) {
  return elastic ? (unsigned)std::min<size_t>(max_groups, (size_t)std::max((int)n_own, cap)) : n_own;
}
// the item-wise scan of thin cells (sparse5.h): six workgroups of four waves per CU (three of the pair kernel), never more than units
inline unsigned sparse_grid(int n_cus, int share, int reserve_cus, size_t sp_cap, bool pairs) {
  return (unsigned)std::min<size_t>(sp_cap, (size_t)std::max(1, scan_cus(n_cus, share, reserve_cus)) * (pairs ? 3 : 6));
}
// ... which a batch takes by itself where thin cells are the rule (fewer than four items per cell on average) and there are
// enough items to fill the chip's workgroup slots several times
inline bool sparse_by_itself(int n_cus, int n_items, int C) { return (size_t)n_items < 4 * (size_t)C && n_items >= 16 * n_cus; }
// the reference-arithmetic scan (fused3.h): one persistent workgroup per CU
inline unsigned spec2_grid(int n_cus, size_t max_groups) { return (unsigned)std::min<size_t>(max_groups, (size_t)n_cus); }
// the scan of every other index shape (multi.h): as many workgroups per CU as fit (LDS, 8 waves of ~100 registers), two at most
inline int multi_per_cu(size_t lds) { return (int)std::max<size_t>(1, std::min<size_t>(2, (size_t)(150 * 1024) / lds)); }
inline unsigned multi_grid(int n_cus, size_t max_groups, size_t lds) { return (unsigned)std::min<size_t>(max_groups, (size_t)n_cus * multi_per_cu(lds)); }

// ---- one launch (one.h): G workgroups, one per CU at most (all co-resident), 256 at most (one_multiway4), and the last arriver
// stages every list in LDS: G * L keys within 56 KB.  pq_one_kernel: a workgroup per ONE_WAVES row blocks at most. ----
inline int ivf_one_groups(int n_cus, int L) { return (int)std::max<int64_t>(1, std::min<int64_t>({(int64_t)n_cus, (int64_t)256, (int64_t)(56 * 1024) / (8 * L)})); }
inline int pq_one_groups(int n_cus, int L, int64_t n_blocks, int waves) {
  return (int)std::max<int64_t>(1, std::min<int64_t>({(int64_t)n_cus, (int64_t)256, (n_blocks + waves - 1) / waves, (int64_t)(56 * 1024) / (8 * L)}));
}

// ---- assignment (assign.h): four targets per thread once that still gives every CU two workgroups of `wg` threads ----
inline int assign_pq_rpt(int n_cus, int64_t n, int wg) { return n >= (int64_t)n_cus * 2 * 4 * wg ? 4 : 1; }

// ---- exact kNN, analogies, join (exact2.h, analogy.h, exact_join.h) ----
// workgroups of a filter kernel over `rows` rows of the whole table: one per 256 rows, at most two per CU
inline unsigned filter_grid(int n_cus, int64_t rows) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((rows + 255) / 256, (int64_t)n_cus * 2)); }
// the exact join's strip chunks: a workgroup's 8 waves take 8 strips per step; with many query tiles every workgroup stays long
// enough (>= 64 strips) to pay for its LDS image of the tile
inline int64_t exact_join_gx(int n_cus, int64_t n_rows, int qtiles) {
  const int64_t wg_steps = (n_rows + 255) / 256;
  return std::max<int64_t>(1, std::min<int64_t>(wg_steps, std::max<int64_t>((int64_t)n_cus * 2 / qtiles, (wg_steps + 7) / 8)));
}
// the table's statistics (exf_table_stats_kernel): a thread group per 4 rows, eight workgroups per CU at most
inline unsigned table_stats_grid(int n_cus, int64_t n) { return (unsigned)std::min<int64_t>((n + 3) / 4, (int64_t)n_cus * 8); }

// ---- similarity (similarity.h): workgroups = nblk blocks of 64 B rows x ranges of A tiles; A is split only until the chip has
// about sixteen waves per CU to place ----
inline int sim_split(int n_cus, int n_tiles, int nblk) { return std::min(n_tiles, std::max(1, (16 * n_cus + nblk - 1) / nblk)); }
inline int sim_tiles_per_wg(int n_cus, int n_tiles, int nblk) { const int split = sim_split(n_cus, n_tiles, nblk); return (n_tiles + split - 1) / split; }
inline unsigned sim_grid_y(int n_cus, int n_tiles, int nblk) { const int t = sim_tiles_per_wg(n_cus, n_tiles, nblk); return (unsigned)((n_tiles + t - 1) / t); }

// ---- the device resolve of an id set (resolve.h): eight workgroups per CU at most; `wgs` = workgroups that would take the work in
// one go (256 ids each in the mark kernel, four blocks -- one per wave -- in the count and place kernels) ----
inline unsigned resolve_grid(int n_cus, int64_t wgs) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(wgs, (int64_t)n_cus * 8)); }

}  // namespace freddy
