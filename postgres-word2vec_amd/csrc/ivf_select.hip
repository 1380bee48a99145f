// ivf_select.hip -- cell selection of the IVFADC search (freddy.c:266-283, :853-866): the coarse distances of a chunk (with the
// filter + refine scan's query x codebook table beside them) and the probe plan of a round.
#include "internal.h"

#include "kernels.h"
#include "coarse.h"
#include "fused5.h"   // coarse_table5_kernel, query_codebook5_kernel
#include "ivf_host.h"

// coarse distances (a6/a7) of every query of the chunk, and -- for the filter + refine scan -- the
// per-batch query x codebook table beside them on the side stream
// (q_lo, q_n): the combined MFMA cell-selection + table launch for the queries [q_lo, q_lo + q_n) of the chunk only -- the host-buffer
// pipeline launches it piece by piece behind the pieces of the staged queries (q_lo a multiple of 32); q_n < 0: the whole chunk
bool ivf_coarse_by_pieces(const IvfRun& r) { return r.approx && r.fused && r.scan_kernel == 5; }
int ivf_coarse(IvfRun& r, int q_lo, int q_n) {
  Workspace* ws = r.ws;
  freddy_gpu_index* ix = r.ix;
  hipStream_t s = r.s;
  const int Q = r.Q, d = ix->d, C = ix->C, m = ix->m, K = ix->K, Cpad = ix->Cpad;
  if (q_n < 0) { q_lo = 0; q_n = Q; }
  if ((q_lo != 0 || q_n != Q) && !ivf_coarse_by_pieces(r)) return fail(FREDDY_E_ARG, "internal: this path launches its coarse kernel once");
  const int used_words = (C + 31) / 32;
  // round-one scratch that must start at zero: the probe bitmaps, the counters (n_next, n_groups, work
  // counter), the per-cell item counts and the accepted-candidate counts: every coarse kernel clears them itself
  // (ZeroArgs) -- except the small-batch kernel for vectors of more than 1024 dimensions, which gets memsets.
  const bool small_zero = !r.tiled && d <= 1024;
  if (!r.tiled && !small_zero) {
    HIP_TRY(hipMemsetAsync(ws->w_used.p, 0, sizeof(uint32_t) * (size_t)Q * used_words, s));
    HIP_TRY(hipMemsetAsync(ws->w_cnt.p, 0, sizeof(int32_t) * 8, s));
  }
  ZeroArgs za;
  za.p[0] = ws->w_used.as<uint32_t>(); za.n[0] = Q * used_words;
  za.p[1] = ws->w_cnt.as<uint32_t>(); za.n[1] = 8;
  za.p[2] = r.fused ? ws->w_cellcnt.as<uint32_t>() : nullptr; za.n[2] = r.fused ? C * 2 : 0;
  za.p[3] = ws->w_cand.as<uint32_t>(); za.n[3] = 2 * Q;   // accepted-row counts, then the queries' running bounds (FilterArgs::tau_run)
  // survivor counts: regions of chunks a list does not have, or of items without a cell, stay at zero
  za.p[4] = r.fused ? ws->w_surv_cnt.as<uint32_t>() : nullptr; za.n[4] = r.fused ? (int)surv_regions(r, (size_t)Q * r.W) : 0;

  // more than 1024 cells: the (query, 128-cell tile) minima for the plan's two-level selection (round one: no cell is used yet)
  float* tile_min = nullptr;
  if (r.approx && Cpad > COARSE_MAX_CPAD) {
    if (ws->w_tmin.ensure(sizeof(float) * (size_t)Q * (Cpad / 128))) return fail(FREDDY_E_NOMEM, "workspace allocation failed");
    tile_min = ws->w_tmin.as<float>();
  }
  // The query x codebook table is independent of the coarse distances: with the MFMA cell selection the coarse tiles and
  // the table units are the workgroups of ONE launch (fused5.h coarse_table5_kernel); otherwise the table kernel runs in
  // line before the coarse kernel.
  if (ivf_coarse_by_pieces(r)) {
    CoarseTableArgs ct;   // (every array is query-major: a piece is the same launch on offset pointers)
    ct.queries = r.d_q + (size_t)q_lo * d; ct.coarseF = ix->coarseP; ct.cn2 = ix->cn2; ct.dist = ws->w_distT.as<float>() + (size_t)q_lo * Cpad;
    ct.qn2 = ws->w_qn2.as<float>() + q_lo;
    ct.Q = q_n; ct.Cpad = Cpad; ct.d = d; ct.dp = ix->dp; ct.z = za; ct.coarse_gx = Cpad / 128; ct.coarse_gy = (q_n + COARSE_TQ - 1) / COARSE_TQ;
    const QueryTable qt = query_table_piece(query_table(ws, ix, Q), ix, q_lo);
    ct.cbT = ix->cbF; ct.cmax = ix->cmaxp; ct.qn = qt.qn; ct.qscale = qt.qscale; ct.qc = qt.qc; ct.qc8 = qt.qc8;
    ct.m = m; ct.K = K; ct.tmin = tile_min ? tile_min + (size_t)q_lo * (Cpad / 128) : nullptr; ct.C = C;
    ct.coarseH = (const ch8v*)ix->coarseH; ct.ec = ix->coarse_ec;
    const size_t lds = std::max<size_t>(ix->coarseH ? coarse_approx16_lds(d) : (size_t)(COARSE_TQ * (ix->dp + 4) + 128) * sizeof(float), (size_t)query_codebook5_lds<25, 16>());
    const unsigned grid = (unsigned)(ct.coarse_gx * ct.coarse_gy + m * ((q_n + 15) / 16));
    timed_launch(ix, s, "coarse_table", [&] {
      if (ix->coarseH) hipLaunchKernelGGL((coarse_table5_kernel<25, 16, true>), dim3(grid), dim3(256), lds, s, ct);
      else hipLaunchKernelGGL((coarse_table5_kernel<25, 16>), dim3(grid), dim3(256), lds, s, ct);
    });
    HIP_TRY(hipGetLastError());
    return 0;
  }
  if (r.fused && r.scan_kernel == 5) {
    const QueryTable qt = query_table(ws, ix, Q);
    timed_launch(ix, s, "query_codebook", [&] {
      hipLaunchKernelGGL((query_codebook5_kernel<25, 16>), dim3(m, (Q + 15) / 16), dim3(256), 0, s, r.d_q, ix->cbF, ix->cmaxp,
                         qt.qn, qt.qscale, qt.qc, Q, d, m, K, qt.qc8);
    });
    HIP_TRY(hipGetLastError());
  }
  timed_launch(ix, s, "coarse_dist", [&] {
    if (r.approx && ix->coarseH)
      hipLaunchKernelGGL(coarse_approx16_kernel, dim3(Cpad / 128, (Q + COARSE_TQ - 1) / COARSE_TQ), dim3(256), coarse_approx16_lds(d), s, r.d_q,
                         (const ch8v*)ix->coarseH, ix->coarse_ec, ix->cn2, ws->w_distT.as<float>(), ws->w_qn2.as<float>(), Q, Cpad, d, za, tile_min, C);
    else if (r.approx)
      hipLaunchKernelGGL(coarse_approx_kernel, dim3(Cpad / 128, (Q + COARSE_TQ - 1) / COARSE_TQ), dim3(256),
                         (size_t)(COARSE_TQ * (ix->dp + 4) + 128) * sizeof(float), s, r.d_q, ix->coarseP, ix->cn2,
                         ws->w_distT.as<float>(), ws->w_qn2.as<float>(), Q, Cpad, d, ix->dp, za, tile_min, C);
    else if (r.tiled)
      hipLaunchKernelGGL((coarse_tile_kernel<2, 16>), dim3(Cpad / 32, (Q + 63) / 64), dim3(256), 0, s, r.d_q, ix->coarseT,
                         ws->w_distT.as<float>(), Q, Cpad, d, za);
    else if (small_zero)
      hipLaunchKernelGGL((coarse_small_kernel<50>), dim3(Cpad / 64, Q), dim3(64), 0, s, r.d_q, ix->coarseT, ws->w_distT.as<float>(), Q, Cpad, d, za);
    else
      hipLaunchKernelGGL((coarse_dist_kernel<16>), dim3(Cpad / WG, (Q + 15) / 16), dim3(WG), (size_t)d * 16 * sizeof(float), s, r.d_q,
                         ix->coarseT, ws->w_distT.as<float>(), Q, Cpad, d);
  });
  HIP_TRY(hipGetLastError());
  return 0;
}

// a7: the W nearest not-yet-used cells of every active query (+ their items appended to the cells' buckets)
int ivf_plan(IvfRun& r, PlanArgs& pa) {
  Workspace* ws = r.ws;
  freddy_gpu_index* ix = r.ix;
  hipStream_t s = r.s;
  const int C = ix->C, W = r.W;
  pa = plan_items(r, C);
  pa.dist = ws->w_distT.as<float>(); pa.active = r.active; pa.list_off = ix->list_off;
  pa.used = ws->w_used.as<uint32_t>(); pa.Cpad = ix->Cpad; pa.used_words = (C + 31) / 32;
  pa.cell_count = r.fused ? ws->w_cellcnt.as<int32_t>() : nullptr;
  pa.cell_items = r.fused ? ws->w_sorted.as<int32_t>() : nullptr; pa.cell_cap = r.n_active;
  pa.cell_limit = r.cell_limit;
  const int n_items = r.n_active * W;
  if (r.fused && !(r.zeroed && r.first())) {
    HIP_TRY(hipMemsetAsync(ws->w_cellcnt.p, 0, sizeof(int32_t) * (size_t)C * 2, s));   // counts + fill cursors
    HIP_TRY(hipMemsetAsync(ws->w_surv_cnt.p, 0, sizeof(int32_t) * surv_regions(r, (size_t)n_items), s));
  }
  const int PV = pick_V(2 * W);
  const size_t plan_lds = (size_t)(64 + 64 * PV) * sizeof(u64) + (size_t)W * 8;
  if (r.approx) {
    Plan2Args g;
    g.p = pa; g.queries = r.d_q; g.coarse = ix->coarse; g.qn2 = ws->w_qn2.as<float>(); g.item_dist = pa.item_dist;
    g.violations = ix->viol; g.cmax = ix->cmax; g.d = ix->d; g.refine_all = (ix->tune.check_brackets & 2) ? 1 : 0; g.prof = nullptr;
    g.tmin = (r.first() && ix->Cpad > COARSE_MAX_CPAD && ws->w_tmin.p) ? ws->w_tmin.as<float>() : nullptr;
    timed_launch(ix, s, "probe_plan", [&] {
      // (one batch at a time: four waves per query, the shortest latency; batches in flight: one wave per query, the smallest footprint)
      if (ix->Cpad <= COARSE_MAX_CPAD && r.share > 1) hipLaunchKernelGGL((probe_plan2_kernel<0, false, 1>), dim3(r.n_active), dim3(64), 0, s, g);
      else if (ix->Cpad <= COARSE_MAX_CPAD) hipLaunchKernelGGL((probe_plan2_kernel<0, false>), dim3(r.n_active), dim3(64 * PLAN2_NW), 0, s, g);
      else hipLaunchKernelGGL((probe_plan2_kernel<0, true>), dim3(r.n_active), dim3(64 * PLAN2_NW), 0, s, g);   // (more than 1024 cells: streamed)
    });
  } else
  timed_launch(ix, s, "probe_plan", [&] {   // (2W <= 1024: ivfadc_begin)
    with_V(PV, [&](auto v) { hipLaunchKernelGGL((probe_plan_kernel<decltype(v)::value>), dim3(r.n_active), dim3(64), plan_lds, s, pa); });
  });
  HIP_TRY(hipGetLastError());
  if (!(r.zeroed && r.first())) HIP_TRY(hipMemsetAsync(ws->w_cand.p, 0, sizeof(int32_t) * 2 * r.Q, s));   // (every round starts without bounds)
  return 0;
}

// The kernels of this unit that want more than the default 64 KiB of dynamic LDS.
std::vector<LdsLimit> lds_limits_ivf_select() {
  return {&coarse_approx_kernel, &coarse_approx16_kernel,
          &coarse_dist_kernel<16>};   // (small batches over vectors of more than 1024 dimensions: 64 bytes per dimension)
}
