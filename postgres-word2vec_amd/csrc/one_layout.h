// one_layout.h -- where the one-launch kernels (one.h) keep what: the regions of the hand-off buffer in global memory and of the
// dynamic LDS, from the call's shape (K, C, W, L, G).  The host (pq_one in pq.hip, ivf_one in one.hip) sizes the buffer and the
// launch with it, the kernels carve `smem` and nothing else with it: one statement of every offset.
// Plain C++17, no HIP, so that tests/test_one_layout_cpu.py compiles this file on its own with g++ (as block_plan.h is); the
// functions are constexpr, which is what lets device code call them.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace freddy {

static constexpr int ONE_WG = 512;
static constexpr int ONE_WAVES = ONE_WG / 64;
static constexpr int ONE_M = 12, ONE_D = 300;   // the shape the kernels are built for: 12 positions, 300 dimensions

struct OneRegion {
  size_t off, bytes;
  constexpr size_t end() const { return off + bytes; }
};

struct OneLayout {
  int K;   // codes per position
  int C;   // cells; 0: pq_one_kernel (no coarse stage, one table, no counts)
  int W;   // tables (cells probed); pq_one_kernel: 1
  int L;   // keys per published list (2k)
  int G;   // workgroups

  static constexpr size_t up(size_t n, size_t a) { return (n + a - 1) & ~(a - 1); }
  static constexpr size_t most(size_t a, size_t b) { return a < b ? b : a; }
  constexpr size_t lut_bytes() const { return sizeof(float) * (size_t)ONE_M * (size_t)K; }

  // ---- the hand-off buffer: coarse distances | the W tables | the workgroups' lists | their accepted-row counts ----
  constexpr size_t lut_off() const { return C ? up(sizeof(float) * ((size_t)C + 8), 256) : 0; }
  constexpr size_t part_off() const { return up(lut_off() + (size_t)W * lut_bytes(), 256); }
  constexpr size_t cnt_off() const { return up(part_off() + sizeof(uint64_t) * (size_t)G * (size_t)L, 256); }
  constexpr size_t handoff_bytes() const { return C ? cnt_off() + sizeof(uint32_t) * (size_t)G : part_off() + sizeof(uint64_t) * (size_t)G * (size_t)L; }

  // ---- dynamic LDS, stage by stage (every stage starts at 0: the stages before it are dead) ----
  // A (ivf): the centroid rows of a workgroup's n_mine <= cells_per_group() cells, then the query
  constexpr size_t cells_per_group() const { return ((size_t)C + (size_t)G - 1) / (size_t)G; }
  constexpr OneRegion coarse_rows(size_t n_mine) const { return {0, n_mine * ONE_D * sizeof(float)}; }
  constexpr OneRegion query(size_t n_mine) const { return {coarse_rows(n_mine).end(), ONE_D * sizeof(float)}; }
  // B (ivf): the C coarse distances (16-byte words), wave 0's staging row of 64 keys
  constexpr OneRegion cell_dist() const { return {0, sizeof(float) * up((size_t)C, 4)}; }
  constexpr OneRegion cell_row() const { return {((size_t)C * 4 + 63) & ~(size_t)15, 64 * sizeof(uint64_t)}; }
  // D: the table (16-byte words), a staging row of 64 keys per wave
  constexpr OneRegion table() const { return {0, lut_bytes()}; }
  constexpr OneRegion wave_rows() const { return {up(lut_bytes(), 16), (size_t)ONE_WAVES * 64 * sizeof(uint64_t)}; }
  // publish and, in workgroup 0, collect: the waves' lists [64 ranks][ONE_WAVES], behind them the G published lists [L][G]
  constexpr OneRegion lists() const { return {0, (size_t)ONE_WAVES * 64 * sizeof(uint64_t)}; }
  constexpr OneRegion all_lists() const { return {lists().end(), sizeof(uint64_t) * (size_t)G * (size_t)L}; }

  constexpr size_t lds_bytes() const {
    const size_t scan = most(wave_rows().end(), all_lists().end());
    // (stage B's figure keeps the slack it has always had: the row's offset rounded from above, 64 bytes behind it)
    return C ? most(most(query(cells_per_group()).end(), (size_t)C * 4 + 64 + 64 * sizeof(uint64_t) + 64), scan) : scan;
  }
};

}  // namespace freddy
