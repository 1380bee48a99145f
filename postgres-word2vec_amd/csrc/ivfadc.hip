// ivfadc.hip -- the IVFADC search (freddy.c:174-393, :679-999), chunk by chunk: one chunk of queries takes its path (ivfadc_begin),
// a probing round is cell selection (ivf_select.hip), then the scan + merge of that path (ivf_scan.hip, generic.hip), and the (rare)
// extra rounds of the reference's "while (foundInstances < k)" loop (freddy.c:262, :835) run with a host sync each; the *_dev entry
// point.  Host-side responsibilities only: size workspaces, order the launches on one HIP stream.  No arithmetic that influences a
// result happens on the host, and this unit launches nothing itself: it includes no header that holds a kernel.
#include "internal.h"

#include "ivf_run.h"
#include "stage_plan.h"

// One probing round of a chunk: cell selection, then the scan + merge of the path the chunk takes.
static int ivfadc_round(IvfRun& r) {
  PlanArgs pa;
  if (int rc = ivf_plan(r, pa)) return rc;
  if (r.fused) {
    WorkTable wt;
    if (int rc = ivf_work_table(r, wt)) return rc;
    return (r.scan_kernel == 5) ? ivf_scan_filter(r, pa, wt) : (r.scan_kernel == 2) ? ivf_scan_multi(r, pa, wt) : ivf_scan_exact(r, pa, wt);
  }
  return ivf_scan_generic(r, pa);
}

// One chunk of queries (device pointers): workspace, coarse distances and round one are enqueued on s, nothing is
// synchronised.  `share` = the batches in flight on this handle (the persistent scan takes n_cus / share CUs).  The
// state for further rounds stays in r (and in the stream's workspace): ivfadc_finish() runs them.
int ivfadc_begin(freddy_gpu_index* ix, hipStream_t s, int share, const float* d_q, int Q, int k, int W,
                 float sentinel, int found_rule, int32_t* d_out_ids, float* d_out_dist,
                 int32_t* d_status, IvfRun& r, const std::function<int(int, int)>* stage, bool by_pieces) {
  // stage(q_lo, q_hi) (host-buffer pipeline): brings the queries [q_lo, q_hi) of this chunk into d_q on stream s -- called once for
  // the whole chunk, or piece by piece with the piece's cell-selection / table launch right behind it
  Workspace* ws = workspace_for(ix, s);
  const int C = ix->C, m = ix->m, K = ix->K;
  if (2 * W > 1024) return fail(FREDDY_E_LIMIT, "W=%d exceeds this build's limit of 512 probes per round", W);
  r = ivf_run(ix, ws, s, share, d_q, Q, k, W, sentinel, d_out_ids, d_out_dist, d_status);
  // FREDDY_FOUND_BATCH_UDF = the accepted-rows rule + the batch UDF's cell limit (argmin from minDist = 1000,
  // freddy.c:853-866); ivfadc_search's cell list starts at 100.0 (freddy.c:266-283)
  r.found_rule = found_rule == FREDDY_FOUND_ROWS ? 0 : 1;
  r.cell_limit = found_rule == FREDDY_FOUND_BATCH_UDF ? 1000.0f : 100.0f;
  const size_t items = (size_t)Q * W;
  // Cell-grouped scans: residual PQ with m=12, S=25, K<=1024 and a selection width that one wave holds
  // (2k <= 64); lists longer than 8 chunks of 4096 rows would need survivor buffers out of proportion.  They
  // pay off once several (query, cell) items share a cell, i.e. for batches; option fused = 1 / 0 forces
  // them / the generic lut_build + adc_scan kernels (the tests run both).
  r.fused = ix->tune.fused != 0 && fused_shape(ix) && r.L <= 64 && r.upi <= 8 && (ix->tune.fused == 1 || items >= 256);
  r.scan_kernel = (ix->tune.scan_kernel == 3 || !ix->rterm) ? 3 : 5;
  if (!r.fused) {
    // every other shape whose interleaved LUT slab fits the LDS: the cell-grouped exact scan of multi.h (option fused = 0
    // keeps the generic kernels, fused = 1 takes it for small batches too)
    // (lists of up to 32 chunks: the reference's shipped 32-cell configuration has 37 000 rows per list)
    r.fused = ix->tune.fused != 0 && !fused_shape(ix) && multi_lds_bytes(m, K) <= (size_t)150 * 1024 && r.L <= 64 && r.upi <= 32 &&
              (ix->tune.fused == 1 || items >= 256);
    if (r.fused) r.scan_kernel = 2;
  }
  r.tiled = Q >= 32;
  r.zeroed = r.tiled || ix->d <= 1024;
  r.running_bound = ix->tune.running_bound != 0;
  // (the MFMA tile is 64 queries wide and the plan keeps a query's distances in registers: batches, <= 1024 cells)
  r.approx = ix->tune.coarse_approx != 0 && r.tiled && ix->Cpad <= COARSE_STREAM_MAX_CPAD && 2 * W <= 64 && ix->d <= 300 && ix->d % 4 == 0 && ix->coarseP;
  bool nomem = ivf_run_ensure(r) || ws->w_distT.ensure(sizeof(float) * (size_t)Q * ix->Cpad) ||
               ws->w_used.ensure(sizeof(uint32_t) * (size_t)Q * ((C + 31) / 32)) || ws->w_qn2.ensure(sizeof(float) * Q);
  if (r.fused) {
    // cell_count[C] + cursors; cell_items[C][Q]; work table: 3 arrays of (items/G + C + 1) * upi entries + the (item, chunk) units of sparse cells
    nomem = nomem || ws->w_cellcnt.ensure(sizeof(int32_t) * (size_t)C * 3) || ws->w_sorted.ensure(sizeof(int32_t) * (size_t)C * Q) ||
            ws->w_groups.ensure(sizeof(int32_t) * 3 * ((items / MULTI_G + (size_t)C + 1) * r.upi + items * r.upi)) ||
            (r.scan_kernel == 2 && ws->w_lut.ensure(sizeof(float) * items * (size_t)m * K));
  } else {
    // (a later probing round has fewer items and may take the finer chunks: room for either)
    const size_t parts = std::max(items * generic_chunks(ix, items).n, std::min<size_t>(items, GENERIC_FEW_ITEMS) * generic_chunks(ix, GENERIC_FEW_ITEMS).n);
    nomem = nomem || ws->w_resid.ensure(sizeof(float) * items * (size_t)ix->d) || ws->w_lut.ensure(sizeof(float) * items * (size_t)m * K) ||
            ws->w_part.ensure(sizeof(u64) * parts * r.L);   // (adc_scan_kernel leaves ONE list of L keys per (item, chunk): kernels.h)
  }
  if (nomem) return fail(FREDDY_E_NOMEM, "workspace allocation failed (Q=%d, W=%d)", Q, W);

  // pieces of whole 32-query tiles; a piece of fewer than 128 queries is not worth a launch of its own
  const int pieces = (stage && by_pieces && ix->tune.coarse_pieces && ivf_coarse_by_pieces(r) && Q >= 512) ? 4 : 1;
  if (int rc = for_pieces(Q, pieces, [&](int q_lo, int q_n) {   // (stage_plan.h)
        if (stage) if (int rc = (*stage)(q_lo, q_lo + q_n)) return rc;
        return ivf_coarse(r, q_lo, q_n);
      }))
    return rc;
  ix->last_Q = Q;
  return ivfadc_round(r);
}

// The extra rounds of the reference's "while (foundInstances < k)" loop (freddy.c:262, :835), one host sync per
// round.  n_next: the number of queries round one left unfinished if the caller has already read it back
// (ws->w_cnt[0], after the stream drained), -1 = read it here.
int ivfadc_finish(IvfRun& r, int n_next) {
  Workspace* ws = r.ws;
  freddy_gpu_index* ix = r.ix;
  hipStream_t s = r.s;
  const int max_rounds = (ix->C + r.W - 1) / r.W + 1;
  for (;;) {
    if (n_next < 0) {
      int32_t h = 0;
      HIP_TRY(hipMemcpyAsync(&h, ws->w_cnt.p, sizeof(int32_t), hipMemcpyDeviceToHost, s));
      HIP_TRY(hipStreamSynchronize(s));
      n_next = h;
    }
    if (n_next <= 0 || ++r.round >= max_rounds) break;
    HIP_TRY(hipMemsetAsync(ws->w_cnt.p, 0, sizeof(int32_t), s));
    r.active = r.next;
    r.next = (r.next == ws->w_act0.as<int32_t>()) ? ws->w_act1.as<int32_t>() : ws->w_act0.as<int32_t>();
    r.n_active = n_next;
    if (int rc = ivfadc_round(r)) return rc;
    n_next = -1;
  }
  return 0;
}

int max_queries_per_chunk(const freddy_gpu_index* ix, int W, int k) {
  // workspace per query: the LUTs of its W items (generic path) or their survivor regions (fused path)
  const size_t upi = (size_t)units_per_item(ix);
  size_t lut_bytes = sizeof(float) * (size_t)ix->m * ix->K * (size_t)W;
  if (2 * k > 64) {
    // lists beyond the cell-grouped scans' selection width take the generic kernels: one list of L keys per (item, chunk) beside
    // the LUTs, and from k = 513 on the passes' selected keys (bigk.h: ceil(2k / 1024) x 1024 per query)
    const size_t L = (size_t)std::min(2 * k, 1024), nchunk = (size_t)generic_chunks(ix, SIZE_MAX).n;   // (a chunk of many items: the coarse chunks)
    lut_bytes += sizeof(u64) * (size_t)W * nchunk * L;
    if (2 * k > 1024) lut_bytes += sizeof(u64) * (size_t)((2 * k + BIGK_PASS - 1) / BIGK_PASS) * BIGK_PASS;
  }
  const bool special = fused_shape(ix);
  const size_t surv_bytes = upi <= (special ? 8u : 32u) ? sizeof(u64) * (size_t)W * upi * FUSED_NW * FUSED_RMAX * 64 : 0;
  const size_t per_query = special ? std::max(lut_bytes, surv_bytes) : lut_bytes + surv_bytes;   // (multi.h: the LUTs of all items AND their survivor regions)
  size_t n = ((size_t)ix->tune.lut_budget_mb << 20) / std::max<size_t>(per_query, 1);
  // the fused path's per-cell item buckets are [C][queries of the chunk]: keep them within 256 MiB
  if (surv_bytes) n = std::min<size_t>(n, ((size_t)256 << 20) / (sizeof(int32_t) * (size_t)std::max(ix->C, 1)));
  if (n < 1) n = 1;
  if (n > (1u << 20)) n = 1u << 20;
  return (int)n;
}

extern "C" int freddy_gpu_ivfadc_search_dev(freddy_gpu_index_t* ix, const float* d_queries, int32_t Q, int32_t k,
                                            int32_t W, float sentinel, int32_t found_rule, int32_t* d_out_ids,
                                            float* d_out_dist, int32_t* d_status, void* hip_stream) {
  if (int rc = check_ivfadc_args(ix, d_queries, Q, k, &W, found_rule, d_out_ids, d_out_dist)) return rc;
  HIP_TRY(hipSetDevice(ix->device));
  hipStream_t s = hip_stream ? (hipStream_t)hip_stream : ix->stream;
  return for_chunks(Q, max_queries_per_chunk(ix, W, k), [&](int q0, int n) {
    IvfRun r;
    return ivfadc_begin(ix, s, scan_share_now(ix->tune.scan_share, false, ix->device), d_queries + (size_t)q0 * ix->d, n, k, W, sentinel, found_rule,
                        d_out_ids + (size_t)q0 * k, d_out_dist + (size_t)q0 * k, d_status, r);
  });
}
