// ivf_run.h -- the host-side facts of an IVFADC chain that need no kernel header: shape predicates and sizes, the query table's
// layout, the run state of a chain and its workspace, argument check, chunk loop.  ivfadc.hip (the chunk driver), pipeline.hip and
// one.hip include this alone; the units that launch the chain's kernels get it through ivf_host.h.
#pragma once

#include "internal.h"
#include "ivf_sizes.h"

// ---- shapes and sizes ----------------------------------------------------------------------------------------------------
// m = 12, S = 25, K <= 1024: what fused3.h / fused5.h / fused8.h / one.h are written for.  An IVF handle of these dimensions has
// the paired codebook cbP (pin.hip); a PQ handle never has it (pq_fused_shape asks for cbR and K <= FUSED_T * FUSED_E instead).
static bool fused_dims(const freddy_gpu_index* ix) { return ix->m == 12 && ix->S == 25 && ix->K <= 1024; }
static bool fused_shape(const freddy_gpu_index* ix) { return fused_dims(ix) && ix->cbP; }
// survivor units (4096-row chunks of the longest list) per (query, cell) item
static int units_per_item(const freddy_gpu_index* ix) { return std::max(1, (ix->max_list_blocks + FUSED_UNIT_BLOCKS - 1) / FUSED_UNIT_BLOCKS); }
// The generic scan: a workgroup per (item, chunk of `blocks` row blocks), `n` chunks over the longest list.  One per (query, probed cell)
// unless the list is huge -- but a handful of items would leave the chip to W workgroups: 32-block chunks then (30 instead of 10 workgroups)
static constexpr int GENERIC_FEW_ITEMS = 64;
struct Chunks { int blocks, n; };
static Chunks generic_chunks(const freddy_gpu_index* ix, size_t n_items) {
  const int blocks = n_items <= (size_t)GENERIC_FEW_ITEMS ? 32 : 256;
  return {blocks, std::max(1, (ix->max_list_blocks + blocks - 1) / blocks)};
}

// ---- the query x codebook table (fused5.h query_codebook5_body) ------------------------------------------------------------
// w_qc: [Q][m][512] dwords, then -- for the scan that keeps the whole entry's slab in LDS (fused8.h) -- a compact copy [Q][m][128];
// w_qn: the norms [Q][m], then the table scales [Q].  All query-major: a piece of the chunk (the pipeline's coarse launches) is an offset.
struct QueryTable { uint32_t* qc; uint32_t* qc8; float* qn; float* qscale; };   // qc8 NULL: no compact copy
static bool scan_whole_slab(const freddy_gpu_index* ix) { return ix->packed8 && ix->tune.codes_u8 == 1 && ix->K <= 256 && ix->m == 12; }
static int query_table_ensure(Workspace* ws, const freddy_gpu_index* ix, int Q) {
  return ws->w_qc.ensure(sizeof(uint32_t) * (size_t)Q * ix->m * (512 + 128)) || ws->w_qn.ensure(sizeof(float) * (size_t)Q * ix->m * 2);
}
static QueryTable query_table(const Workspace* ws, const freddy_gpu_index* ix, int Q) {
  uint32_t* qc = ws->w_qc.as<uint32_t>();
  float* qn = ws->w_qn.as<float>();
  return {qc, scan_whole_slab(ix) ? qc + (size_t)Q * ix->m * 512 : nullptr, qn, qn + (size_t)Q * ix->m};
}
static QueryTable query_table_piece(const QueryTable& t, const freddy_gpu_index* ix, int q_lo) {
  const size_t rows = (size_t)q_lo * ix->m;
  return {t.qc + rows * 512, t.qc8 ? t.qc8 + rows * 128 : nullptr, t.qn + rows, t.qscale + q_lo};
}

// ---- the run state of a chain ---------------------------------------------------------------------------------------------
// One chunk of Q queries with W items each before its first round: every query active, and what only a probing IVFADC chunk has
// (cell selection, found rule, running bounds: ivfadc_begin) off; pq_fused_chunk states fused, who wrote the records and the slices.
static IvfRun ivf_run(freddy_gpu_index* ix, Workspace* ws, hipStream_t s, int share, const float* d_q, int Q, int k, int W, float sentinel,
                      int32_t* d_out_ids, float* d_out_dist, int32_t* d_status) {
  IvfRun r{};
  r.ix = ix; r.ws = ws; r.s = s; r.share = std::max(1, share); r.d_q = d_q; r.Q = Q; r.k = k; r.W = W; r.L = std::min(2 * k, 64 * 16);
  r.Lt = std::min(k, r.L);
  r.sentinel = sentinel; r.d_out_ids = d_out_ids; r.d_out_dist = d_out_dist; r.d_status = d_status;
  r.upi = units_per_item(ix); r.scan_kernel = 5; r.n_active = Q;
  return r;
}
// survivor regions of `n_items` items (their counts are cleared before every round)
static size_t surv_regions(const IvfRun& r, size_t n_items) { return n_items * r.upi * FUSED_NW; }
// The workspace every chain writes: items, per-query state, counters; a cell-grouped scan's survivor regions; the filter + refine
// scan's query table.  Nonzero: an allocation failed (the caller's message names its shape).
static int ivf_run_ensure(IvfRun& r) {
  Workspace* ws = r.ws;
  const size_t Q = (size_t)r.Q, items = Q * r.W;
  if (ws->w_item_cell.ensure(sizeof(int32_t) * items) || ws->w_item_query.ensure(sizeof(int32_t) * items) ||
      ws->w_item_dist.ensure(sizeof(float) * items) || ws->w_rows.ensure(sizeof(int32_t) * Q) ||
      ws->w_cand.ensure(sizeof(int32_t) * 2 * Q) ||   // accepted-row counts, then the queries' running bounds (FilterArgs::tau_run)
      ws->w_found.ensure(sizeof(int32_t) * Q) || ws->w_act0.ensure(sizeof(int32_t) * Q) || ws->w_act1.ensure(sizeof(int32_t) * Q) ||
      ws->w_cnt.ensure(sizeof(int32_t) * 8))
    return -1;
  if (r.fused && (ws->w_surv.ensure(sizeof(u64) * surv_regions(r, items) * FUSED_RMAX * 64) || ws->w_surv_cnt.ensure(sizeof(int32_t) * surv_regions(r, items))))
    return -1;
  if (r.fused && r.scan_kernel == 5 && query_table_ensure(ws, r.ix, r.Q)) return -1;
  r.next = ws->w_act0.as<int32_t>();
  return 0;
}
// the accepted-rows rule counts the rows the scans accept; the rows rule needs no counter
static int32_t* rows_counter(const IvfRun& r) { return r.found_rule == 1 ? r.ws->w_cand.as<int32_t>() : nullptr; }
// a round's items (ivf_plan adds what the cell selection reads); a work table's counters in w_cnt, [0] = n_next (ivf_work_table adds the tables)
static PlanArgs plan_items(const IvfRun& r, int C) {
  PlanArgs pa{};
  pa.item_cell = r.ws->w_item_cell.as<int32_t>(); pa.item_query = r.ws->w_item_query.as<int32_t>(); pa.item_dist = r.ws->w_item_dist.as<float>();
  pa.round_rows = r.ws->w_rows.as<int32_t>(); pa.n_active = r.n_active; pa.C = C; pa.W = r.W;
  return pa;
}
static WorkTable work_counters(const Workspace* ws, size_t max_groups) {
  WorkTable wt{};
  int32_t* cnt = ws->w_cnt.as<int32_t>();
  wt.max_groups = max_groups; wt.n_groups = cnt + 1; wt.work_counter = cnt + 2; wt.sp_counter = cnt + 3; wt.n_sparse = cnt + 4;
  return wt;
}

// ---- entry points ---------------------------------------------------------------------------------------------------------
// what both IVFADC entry points ask of their arguments; W is cut to the number of cells
static int check_ivfadc_args(const freddy_gpu_index* ix, const void* q, int Q, int k, int32_t* W, int found_rule, const void* oi, const void* od) {
  if (int rc = check_search_args(ix, KIND_IVF, q, Q, k, oi, od)) return rc;
  if (int rc = check_probe_args(*W, found_rule)) return rc;
  if (*W > ix->C) *W = ix->C;
  return 0;
}
// fn(q0, n) for the chunks [q0, q0 + n) of at most `per` queries, until one fails
template <class F>
static int for_chunks(int Q, int per, F&& fn) {
  for (int q0 = 0; q0 < Q; q0 += per)
    if (int rc = fn(q0, std::min(per, Q - q0))) return rc;
  return 0;
}
