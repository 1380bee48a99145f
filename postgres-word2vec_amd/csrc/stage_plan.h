// stage_plan.h -- the staging decisions of the host-buffer calls (pipeline.hip, pq.hip, one.hip) in plain C++: how a call is cut into
// sub-batches and lanes, how a sub-batch's queries reach the device, the pieces a chunk's queries cross in and the 16-byte words of
// a piece, and the layout of the pinned block the lists come back in.  No HIP here: tests/test_stage_plan_cpu.py builds it into a
// program of its own.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

namespace freddy {

// A handful of queries is read where it is staged, without a copy launch in front (and pq_search's lists of a handful are written
// straight into the pinned block): one launch less in a call that a PostgreSQL backend makes for a few rows.
static constexpr int IN_PLACE_QUERIES = 8;

// ---- one host-buffer IVFADC call: sub-batches and lanes --------------------------------------------------------------------------
// cap: queries a sub-batch may hold (the workspace's chunk limit and option pipeline_batch); equal sub-batches rather than full ones
// and a remainder; sub-batch j goes to lane j % n_lanes, slot (j / n_lanes) & 1.
struct PipeCuts {
  int cap, n_sub, per, n_lanes;
  int q0(int j) const { return j * per; }
  int n(int j, int Q) const { return std::min(per, Q - j * per); }
  int lane(int j) const { return j % n_lanes; }
  int slot(int j) const { return (j / n_lanes) & 1; }
};
static inline PipeCuts pipe_cuts(int Q, int max_chunk, int pipeline_batch, int pipeline_lanes, int max_lanes) {
  PipeCuts c;
  c.cap = std::max(1, std::min(max_chunk, pipeline_batch));
  c.n_sub = (Q + c.cap - 1) / c.cap;
  c.per = (Q + c.n_sub - 1) / c.n_sub;
  c.n_lanes = std::min(c.n_sub, std::min(pipeline_lanes, max_lanes));
  return c;
}

// ---- how the n queries of a sub-batch reach the device ---------------------------------------------------------------------------
// host: the caller's floats (else: rows of a device table, query_ids.h); pinned: the device address of the sub-batch's first query
// if the caller's buffer is pinned itself (0: pageable memory); row: bytes of a query.
//   in_place   no launch in front: a handful of host queries where they are staged (the lane's pinned block, or the caller's pinned
//              buffer); ONE query of a device table where its row lies
//   stage      host queries go through the lane's pinned block: pageable memory, or a pinned range that does not start and end on
//              a 16-byte word (the copy kernel moves whole words)
// Neither: the copy kernel reads the caller's pinned buffer (host), or a gather fills the block from staged row numbers (device).
struct QuerySource { bool in_place, stage; };
static inline QuerySource query_source(bool host, uintptr_t pinned, size_t row, int n) {
  QuerySource s;
  s.stage = host && (!pinned || pinned % 16 || (row * (size_t)n) % 16);
  s.in_place = host ? n <= IN_PLACE_QUERIES : n == 1;
  return s;
}

// ---- the pieces of a chunk (ivfadc_begin) and the words of a piece (stage_piece) --------------------------------------------------
// fn(q_lo, q_n) for the `pieces` pieces of a chunk of Q queries, until one fails: whole 32-query tiles (the MFMA cell selection's),
// the last one what is left; pieces == 1: the chunk.
template <class F>
static inline int for_pieces(int Q, int pieces, F&& fn) {
  const int per = ((Q + pieces - 1) / pieces + 31) & ~31;
  for (int q_lo = 0; q_lo < Q; q_lo += (pieces > 1 ? per : Q)) {
    const int q_n = pieces > 1 ? std::min(per, Q - q_lo) : Q;
    if (int rc = fn(q_lo, q_n)) return rc;
  }
  return 0;
}
// The bytes [b_lo, b_hi) and 16-byte words [w0, w1) of the queries [q_lo, q_hi) of a sub-batch of n (a range of whole queries; whole
// words except at the end of the sub-batch, whose buffers are padded), crossing as `cuts` copy launches of per16 words: without
// per-piece coarse launches (every path but one) a staged range of 512 KiB or more still crosses as four.
struct PieceWords {
  size_t b_lo, b_hi, w0, w1, per16;
  int cuts;
  bool aligned() const { return b_lo % 16 == 0; }
  size_t cut_lo(int ci) const { return w0 + (size_t)ci * per16; }
  size_t cut_hi(int ci) const { return std::min(w1, cut_lo(ci) + per16); }
};
static inline PieceWords piece_words(size_t row, int q_lo, int q_hi, int n, bool stage) {
  PieceWords p;
  p.b_lo = row * (size_t)q_lo; p.b_hi = row * (size_t)q_hi;
  p.w0 = p.b_lo / 16; p.w1 = (p.b_hi + 15) / 16;
  p.cuts = (q_lo == 0 && q_hi == n && stage && p.b_hi >= (size_t)512 * 1024) ? 4 : 1;
  p.per16 = (p.w1 - p.w0 + p.cuts - 1) / p.cuts;
  return p;
}

// ---- the pinned block a synchronous call's lists come back in (hio_out: ivf_one, pq_search) --------------------------------------
// [n_out ids][n_out distances][16 spare bytes, whose first word is the one-launch kernels' verdict]
struct HioOut {
  int32_t* ids;
  float* dist;
  int32_t* verdict;
  static size_t bytes(size_t n_out) { return n_out * 8 + 16; }
  HioOut(void* block, size_t n_out)
      : ids(static_cast<int32_t*>(block)), dist(reinterpret_cast<float*>(ids + n_out)), verdict(ids + 2 * n_out) {}
};

}  // namespace freddy
