// block_plan.h -- from the lengths of the inverted lists to the 64-row block layout's index arrays: the one place
// that knows how lists become blocks.  pack_lists (pin.hip) and the append and the removal (mutate_host.h) all plan with it.
// Plain C++17, no HIP, so that tests/test_block_plan_cpu.py compiles this file on its own with g++ (as alloc_hook.h is).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace freddy {

constexpr int64_t kMaxRows = (int64_t)INT32_MAX - 64;   // row positions are 32-bit, and a list's last block may be padding

// An array per block holds one block at least: an empty table keeps one block of padding.
inline int64_t alloc_blocks(int64_t n_blocks) { return n_blocks > 0 ? n_blocks : 1; }

struct BlockPlan {
  std::vector<int32_t> list_off;   // [n_lists + 1] first row of every list
  std::vector<int32_t> blk_off;    // [n_lists + 1] first block of every list
  std::vector<int32_t> blk_cell;   // [alloc_blocks(n_blocks)] the list of every block
  int max_list_blocks = 0;
  int64_t n_blocks = 0;
  int64_t rows() const { return list_off.back(); }
};

enum { PLAN_OK = 0, PLAN_NEGATIVE_LENGTH = 1, PLAN_TOO_MANY_ROWS = 2 };

// len_of(c) = rows of list c.  *bad_list: the list a refusal is about.  A refused plan allocates nothing per block.
template <class LenOf>
inline int plan_blocks(int n_lists, LenOf len_of, BlockPlan& p, int* bad_list) {
  p.list_off.assign((size_t)n_lists + 1, 0);
  p.blk_off.assign((size_t)n_lists + 1, 0);
  p.max_list_blocks = 0;
  for (int c = 0; c < n_lists; ++c) {
    const int64_t len = len_of(c);
    *bad_list = c;
    if (len < 0) return PLAN_NEGATIVE_LENGTH;
    if (len > kMaxRows || (int64_t)p.list_off[(size_t)c] + len > kMaxRows) return PLAN_TOO_MANY_ROWS;
    const int nb = (int)((len + 63) / 64);
    p.list_off[(size_t)c + 1] = p.list_off[(size_t)c] + (int32_t)len;
    p.blk_off[(size_t)c + 1] = p.blk_off[(size_t)c] + nb;
    if (nb > p.max_list_blocks) p.max_list_blocks = nb;
  }
  p.n_blocks = p.blk_off[(size_t)n_lists];
  p.blk_cell.assign((size_t)alloc_blocks(p.n_blocks), 0);
  for (int c = 0; c < n_lists; ++c)
    for (int32_t b = p.blk_off[(size_t)c]; b < p.blk_off[(size_t)c + 1]; ++b) p.blk_cell[(size_t)b] = c;
  return PLAN_OK;
}

}  // namespace freddy
