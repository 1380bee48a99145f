// ivf_scan.hip -- the cell-grouped scans of an IVFADC round and their merges: the work table, filter + refine (fused5.h / fused8.h,
// sparse5.h, refine.h), the reference's arithmetic for every row (fused3.h), every other index shape (multi.h).  pq.hip sends its
// batches over the flat table through ivf_scan_filter.
#include "internal.h"

#include "kernels.h"
#include "scan_common.h"
#include "fused3.h"
#include "fused5.h"
#include "fused8.h"
#include "sparse5.h"
#include "multi.h"
#include "ivf_host.h"
#include "scan_prof.h"

// kernel choosers (generic.hip says what one is)
// ivf_filter8_kernel (whole: the entry's slab stays in LDS, one-byte codes) / ivf_filter5_kernel<12, FULLK, CAND, PROF, U8>.  CAND: the
// accepted-rows rule doubles the selection code of a kernel larger than the instruction cache; prof (lab): one instantiation per kernel;
// elastic: ivf_filter5_elastic_kernel, the scan that brings extra workgroups (FilterArgs::elastic)
static void (*filter_kernel(bool whole, bool u8, bool k1024, bool counts_rows, bool prof, bool elastic = false))(FilterArgs) {
  if ((u8 && k1024) || (whole && !u8) || (elastic && (whole || prof))) return nullptr;   // (one byte per code: K <= 256)
  if (elastic && u8) return counts_rows ? &ivf_filter5_elastic_kernel<12, false, true, true> : &ivf_filter5_elastic_kernel<12, false, false, true>;
  if (elastic && k1024) return counts_rows ? &ivf_filter5_elastic_kernel<12, true, true> : &ivf_filter5_elastic_kernel<12, true, false>;
  if (elastic) return counts_rows ? &ivf_filter5_elastic_kernel<12, false, true> : &ivf_filter5_elastic_kernel<12, false, false>;
#ifdef FREDDY_LAB
  if (prof && !counts_rows && whole) return &ivf_filter8_kernel<12, false, true>;
  if (prof && !counts_rows && k1024) return &ivf_filter5_kernel<12, true, false, true>;
#endif
  (void)prof;
  if (whole) return counts_rows ? &ivf_filter8_kernel<12, true> : &ivf_filter8_kernel<12, false>;
  if (u8) return counts_rows ? &ivf_filter5_kernel<12, false, true, false, true> : &ivf_filter5_kernel<12, false, false, false, true>;
  if (k1024) return counts_rows ? &ivf_filter5_kernel<12, true, true> : &ivf_filter5_kernel<12, true, false>;
  return counts_rows ? &ivf_filter5_kernel<12, false, true> : &ivf_filter5_kernel<12, false, false>;
}
// (cell, chunk) units of one or two items (pairs: the rows of a two-item cell are read once) / of one item (sparse5.h)
static void (*sparse_kernel(bool pairs, bool u8, bool counts_rows))(SparseArgs) {
  if (pairs) return u8 ? (counts_rows ? &sparse_pair5_kernel<12, true, true> : &sparse_pair5_kernel<12, false, true>)
                       : (counts_rows ? &sparse_pair5_kernel<12, true, false> : &sparse_pair5_kernel<12, false, false>);
  return u8 ? (counts_rows ? &sparse_item5_kernel<12, true, true> : &sparse_item5_kernel<12, false, true>)
            : (counts_rows ? &sparse_item5_kernel<12, true> : &sparse_item5_kernel<12, false>);
}
static void (*spec2_kernel(bool k1024))(FusedArgs) { return k1024 ? &ivf_spec2_kernel<25, 12, true> : &ivf_spec2_kernel<25, 12, false>; }

int ivf_work_table(IvfRun& r, WorkTable& wt) {
  Workspace* ws = r.ws;
  freddy_gpu_index* ix = r.ix;
  hipStream_t s = r.s;
  const int n_items = r.n_active * r.W;
  wt = work_counters(ws, ((size_t)n_items / MULTI_G + (size_t)ix->C + 1) * r.upi);   // (group, chunk) work entries (the smallest group size: a bound for every scan)
  int32_t* base = ws->w_groups.as<int32_t>();
  wt.group_cell = base; wt.group_first = base + wt.max_groups; wt.group_cnt = base + 2 * wt.max_groups;
  // cells that one or two queries probe are scanned item by item -- where such cells are the rule (fewer than four items per
  // cell on average: a corpus with more cells than the batch has probes) and there are enough of them to fill the chip's
  // workgroup slots several times (the item-wise scan is built for throughput: a 256-query batch on 1000 cells took 0.187
  // instead of 0.155 ms with it); a dense batch does not pay the extra launch for its handful of thin cells
  // (a negative option value forces the item-wise scan for cells of up to that many items whatever the batch: tests)
  const int sparse_max = r.scan_kernel != 5 ? 0
                         : ix->tune.sparse_items < 0 ? -ix->tune.sparse_items
                         : sparse_by_itself(ix->n_cus, n_items, ix->C) ? ix->tune.sparse_items : 0;
  wt.sp_cap = sparse_max > 0 ? (size_t)n_items * r.upi : 0;
  wt.sp_cell = base + 3 * wt.max_groups; wt.sp_first = wt.sp_cell + wt.sp_cap; wt.sp_chunk = wt.sp_first + wt.sp_cap;
  timed_launch(ix, s, "work_table", [&] {
    hipLaunchKernelGGL(work_table_kernel, dim3(1), dim3(1024), 0, s, ws->w_cellcnt.as<int32_t>(), ix->C, r.n_active, r.scan_kernel == 5 ? SCAN5_G : r.scan_kernel == 2 ? MULTI_G : SPEC2_G, ix->blk_off,
                       wt.group_cell, wt.group_first, wt.group_cnt, wt.n_groups, r.scan_kernel == 5 ? 2 : 0,
                       sparse_max, wt.sp_cell, wt.sp_first, wt.sp_chunk, wt.n_sparse, sparse_max >= 2 ? 1 : 0);
  });
  wt.sp_pairs = sparse_max >= 2;
  HIP_TRY(hipGetLastError());
  if (!(r.zeroed && r.first())) HIP_TRY(hipMemsetAsync(wt.work_counter, 0, 2 * sizeof(int32_t), s));   // (both work counters)
  return 0;
}

// Default scan: filter + refine.  entry records -> ivf_filter5_kernel (+ the item-wise scan of thin cells) -> merge_refine_kernel.
int ivf_scan_filter(IvfRun& r, const PlanArgs& pa, const WorkTable& wt) {
  Workspace* ws = r.ws;
  freddy_gpu_index* ix = r.ix;
  hipStream_t s = r.s;
  const int K = ix->K;
  const QueryTable qt = query_table(ws, ix, r.Q);
  // One persistent workgroup per CU (LDS admits exactly one), never more than there is work.  Batches in flight share the
  // chip: a persistent scan that took every CU would hold up the small kernels of the other batches until it drains, and
  // their scans behind them; with n_cus / share GUARANTEED workgroups each, the scans of `share` batches run side by side, the small
  // kernels fit in between, and a scan's workgroups pull more entries each (a shorter tail).
  const unsigned n_own = filter_scan_own(ix->n_cus, r.share, ix->tune.reserve_cus, wt.max_groups);   // (grid_plan.h)
  // K <= 256: one byte per code (packed8) unless option codes_u8 = 0 asks for the int16 layout
  const bool u8 = ix->packed8 && ix->tune.codes_u8 != 0 && ix->K <= 256;
  // ... and by default the kernel that keeps the WHOLE entry's slab in LDS (fused8.h; option codes_u8 = 2: fused5.h's one-byte instantiation)
  const bool whole = u8 && qt.qc8;
  // Option scan_elastic (an IVFADC batch through ivf_filter5_kernel that shares the chip): while the other batches walk through their
  // small kernels their quarter of the CUs holds nothing, so the grid also brings EXTRA workgroups -- up to `cap` scan workgroups
  // alive over all streams of the handle -- which take entries only while no other scan is announced (the record launch of a batch
  // announces its scan's guaranteed workgroups, one launch ahead) and leave when one is (FilterArgs::elastic).  ivf_filter8_kernel
  // keeps its fixed grid.
  bool elastic = ix->tune.scan_elastic > 0 && r.share > 1 && !r.records_ready && !whole && ix->elastic != nullptr;
#ifdef FREDDY_LAB
  if (ix->tune.scan_prof) elastic = false;   // (the profiling instantiations have no extras)
#endif
  const int cap = filter_scan_cap(ix->n_cus, ix->tune.scan_elastic_reserve, ix->tune.reserve_cus, r.share);
  const unsigned n_persist = filter_scan_persist(elastic, n_own, cap, wt.max_groups);
  if (!r.records_ready) {   // (a batch over the flat PQ table: pq_front_kernel has written them)
    if (ws->w_records.ensure(sizeof(int32_t) * REC_DW * wt.max_groups)) return fail(FREDDY_E_NOMEM, "workspace allocation failed");
    RecordArgs ra;
    ra.group_cell = wt.group_cell; ra.group_first = wt.group_first; ra.group_cnt = wt.group_cnt; ra.n_groups = wt.n_groups;
    ra.sorted_item = ws->w_sorted.as<int32_t>(); ra.item_query = pa.item_query; ra.blk_off = ix->blk_off; ra.list_off = ix->list_off;
    ra.item_dist = pa.item_dist; ra.qn = qt.qn; ra.qscale = qt.qscale; ra.pmax = ix->pmax;
    ra.records = ws->w_records.as<int32_t>(); ra.sentinel = r.sentinel;
    ra.elastic = elastic ? ix->elastic : nullptr; ra.n_announce = (int)n_own;
    timed_launch(ix, s, "entry_records", [&] {
      hipLaunchKernelGGL((entry_record5_kernel<12>), dim3((unsigned)((wt.max_groups + 3) / 4)), dim3(256), 0, s, ra);
    });
    HIP_TRY(hipGetLastError());
  }
  FilterArgs fl;
  fl.qc = qt.qc; fl.qc8 = qt.qc8; fl.rterm = ix->rterm; fl.records = ws->w_records.as<int32_t>(); fl.n_groups = wt.n_groups;
  fl.work_counter = wt.work_counter; fl.packed = ix->packed; fl.surv = ws->w_surv.as<u64>(); fl.surv_count = ws->w_surv_cnt.as<int32_t>();
  fl.cand_count = rows_counter(r);
  fl.K = K; fl.L = r.L; fl.Lt = r.Lt; fl.upi = r.upi; fl.sentinel = r.sentinel; fl.keep_all = (ix->tune.check_brackets & 1) ? 1 : 0; fl.fence = 0;
  // (not for a batch over the flat PQ table: a few dozen queries x a thousand entries read and update the same two cache lines --
  // 96 -> 128 us -- and its merge gains nothing; an IVFADC batch: +2.6 % queries/s with four batches in flight)
  fl.tau_run = r.running_bound ? ws->w_cand.as<uint32_t>() + r.Q : nullptr;
  if (int rc = scan_prof_buffer(ix, ws, &fl.prof, &fl.fence)) return rc;
  if (n_persist > (unsigned)SCAN5_PROF_WGS) fl.prof = nullptr;   // (a grid the counters' buffer does not hold: no counters)
  fl.elastic = elastic ? ix->elastic : nullptr; fl.n_own = (int)n_own; fl.cap = cap; fl.elastic_yield = ix->tune.scan_elastic;
  // LDS: slabs [2 buffers][2 positions][K][16 items] int16 (whole: [12 positions][2 halves][256][8 items]), then column minima /
  // thresholds, two entry records, row terms
  const size_t desc_off = whole ? (size_t)scan8_slab_bytes(12) : (size_t)4 * SCAN5_G * 2 * K;
  const size_t flds = desc_off + 4096 + 64 + (2 * REC_DW + 4) * sizeof(int32_t) + 4096 * sizeof(float);
  fl.desc_offset = (uint32_t)desc_off;
  fl.packed8 = u8 ? ix->packed8 : nullptr;
  const auto filter = filter_kernel(whole, u8, K == 1024, fl.cand_count != nullptr, fl.prof != nullptr, elastic);
  if (!filter) return fail(FREDDY_E_ARG, "internal: no filter scan for this shape");
  timed_launch(ix, s, "ivf_filter", [&] { hipLaunchKernelGGL(filter, dim3(n_persist), dim3(SPEC2_T), flds, s, fl); });
  HIP_TRY(hipGetLastError());
  if (wt.sp_cap > 0) {
    // cells that one or two queries of the batch probe: item by item (sparse5.h), six workgroups of four waves per CU
    SparseArgs sp;
    sp.qc = qt.qc; sp.qscale = qt.qscale; sp.qn = qt.qn; sp.pmax = ix->pmax; sp.rterm = ix->rterm; sp.packed = ix->packed;
    sp.blk_off = ix->blk_off; sp.list_off = ix->list_off; sp.sorted_item = ws->w_sorted.as<int32_t>(); sp.item_query = pa.item_query;
    sp.item_dist = pa.item_dist; sp.sp_cell = wt.sp_cell; sp.sp_first = wt.sp_first; sp.sp_chunk = wt.sp_chunk;
    sp.n_units = wt.n_sparse; sp.work_counter = wt.sp_counter; sp.surv = fl.surv; sp.surv_count = fl.surv_count; sp.packed8 = fl.packed8;
    sp.cand_count = fl.cand_count; sp.K = K; sp.L = r.L; sp.Lt = r.Lt; sp.upi = r.upi; sp.sentinel = r.sentinel; sp.keep_all = fl.keep_all; sp.tau_run = fl.tau_run;
    const unsigned sp_grid = sparse_grid(ix->n_cus, r.share, ix->tune.reserve_cus, wt.sp_cap, wt.sp_pairs);
    const auto sparse = sparse_kernel(wt.sp_pairs, u8, fl.cand_count != nullptr);
    timed_launch(ix, s, "sparse_items", [&] { hipLaunchKernelGGL(sparse, dim3(sp_grid), dim3(256), 0, s, sp); });
    HIP_TRY(hipGetLastError());
  }
#ifdef FREDDY_LAB
  if (int rc = filter_prof_print(ix, s, fl, whole, n_persist)) return rc;
#endif

  MergeRefineArgs mr;
  mr.surv = fl.surv; mr.surv_count = fl.surv_count; mr.active = r.active; mr.round_rows = pa.round_rows;
  mr.item_cell = pa.item_cell; mr.queries = r.d_q; mr.coarse = ix->coarse; mr.cbR = ix->cbR;
  mr.qn = qt.qn; mr.pmax = ix->pmax; mr.qscale5 = qt.qscale; mr.packed = ix->packed; mr.pos = ix->pos; mr.blk_cell = ix->blk_cell;
  mr.cand_count = fl.cand_count; mr.violations = ix->viol; mr.out_ids = r.d_out_ids; mr.out_dist = r.d_out_dist;
  mr.found = ws->w_found.as<int32_t>(); mr.next_active = r.next; mr.n_next = ws->w_cnt.as<int32_t>();
  mr.status = r.d_status;
  mr.n_active = r.n_active; mr.W = r.W; mr.upi = r.upi; mr.L = r.L; mr.k = r.k; mr.found_rule = r.found_rule;
  mr.first_round = r.first() ? 1 : 0; mr.K = K; mr.d = ix->d; mr.sentinel = r.sentinel;
  mr.refine_all = (ix->tune.check_brackets & 1) ? 1 : 0; mr.fence = 0;
  mr.slices = 0; mr.part = nullptr;
  if (r.merge_slices > 0) {
    // a batch over the flat PQ table: `merge_slices` workgroups per query, each over its share of the pseudo-lists (r.W is the
    // padded item count per query, a multiple of the slices), then merge_replay_kernel over the slices' keys
    const int SL = r.merge_slices;
    if (ws->w_part.ensure(sizeof(u64) * (size_t)r.n_active * SL * r.L)) return fail(FREDDY_E_NOMEM, "workspace allocation failed");
    mr.slices = SL; mr.part = ws->w_part.as<u64>(); mr.W = r.W / SL; mr.n_active = r.n_active * SL;
    timed_launch(ix, s, "merge_refine", [&] {
      hipLaunchKernelGGL((merge_refine_kernel<25, 12, 12, true, true>), dim3(r.n_active * SL), dim3(768), 0, s, mr);
    });
    HIP_TRY(hipGetLastError());
    return launch_merge(ix, s, merge_args_flat(mr.part, r.n_active, SL, r.L, r.k, r.sentinel, nullptr, r.d_out_ids, r.d_out_dist));
  }
  timed_launch(ix, s, "merge_refine", [&] {
    // (one batch at a time: four waves per query, the shortest latency; batches in flight: one wave per query, the smallest footprint)
    // (hundreds of survivor regions per query -- a batch over the flat PQ table: four waves, which split the selection)
    const bool many_regions = (size_t)r.W * r.upi * FUSED_NW > 256;
    if (!many_regions && r.share > 1)
      hipLaunchKernelGGL((merge_refine_kernel<25, 12, 1>), dim3(r.n_active), dim3(64), 0, s, mr);
    else if (many_regions && r.n_active <= 256)   // (a few queries with many qualifying rows each: twelve waves, 64 rows per round of the exact stage)
      hipLaunchKernelGGL((merge_refine_kernel<25, 12, 12, true>), dim3(r.n_active), dim3(768), 0, s, mr);
    else if (many_regions)                         // (a large batch: the workgroups' footprint decides, 95 against 52 us at 1024 queries)
      hipLaunchKernelGGL((merge_refine_kernel<25, 12, 4, true>), dim3(r.n_active), dim3(256), 0, s, mr);
    else
      hipLaunchKernelGGL((merge_refine_kernel<25, 12, 4>), dim3(r.n_active), dim3(256), 0, s, mr);
  });
  HIP_TRY(hipGetLastError());
  return 0;
}

// merge_surv_kernel for a round whose scan (exact or multi) left its survivors in (surv, surv_count)
static int launch_merge_surv(const IvfRun& r, const PlanArgs& pa, const u64* surv, const int32_t* surv_count, const int32_t* cand_count) {
  MergeSurvArgs ms;
  ms.surv = surv; ms.surv_count = surv_count; ms.active = r.active; ms.round_rows = pa.round_rows;
  ms.cand_count = cand_count; ms.out_ids = r.d_out_ids; ms.out_dist = r.d_out_dist;
  ms.found = r.ws->w_found.as<int32_t>(); ms.next_active = r.next; ms.n_next = r.ws->w_cnt.as<int32_t>();
  ms.status = r.d_status;
  ms.n_active = r.n_active; ms.W = r.W; ms.upi = r.upi; ms.L = r.L; ms.k = r.k; ms.found_rule = r.found_rule;
  ms.first_round = r.first() ? 1 : 0; ms.sentinel = r.sentinel;
  timed_launch(r.ix, r.s, "merge_surv", [&] { hipLaunchKernelGGL(merge_surv_kernel, dim3(r.n_active), dim3(64), 0, r.s, ms); });
  HIP_TRY(hipGetLastError());
  return 0;
}

// The yardstick: the reference's arithmetic for every probed row (fused3.h).  ivf_spec2_kernel -> merge_surv_kernel.
int ivf_scan_exact(IvfRun& r, const PlanArgs& pa, const WorkTable& wt) {
  Workspace* ws = r.ws;
  freddy_gpu_index* ix = r.ix;
  hipStream_t s = r.s;
  const int K = ix->K;
  FusedArgs fa;
  fa.resid = nullptr; fa.item_query = pa.item_query; fa.queries = r.d_q; fa.coarse = ix->coarse;
  fa.sorted_item = ws->w_sorted.as<int32_t>(); fa.group_cell = wt.group_cell; fa.group_first = wt.group_first;
  fa.group_cnt = wt.group_cnt; fa.n_groups = wt.n_groups; fa.work_counter = wt.work_counter;
  fa.cbP = ix->cbP; fa.blk_off = ix->blk_off; fa.packed = ix->packed; fa.pos = ix->pos;
  fa.surv = ws->w_surv.as<u64>(); fa.surv_count = ws->w_surv_cnt.as<int32_t>();
  fa.cand_count = rows_counter(r);
  fa.d = ix->d; fa.K = K; fa.L = r.L; fa.upi = r.upi;
  memcpy(&fa.sentinel_bits, &r.sentinel, 4);
  if (int rc = scan_prof_buffer(ix, ws, &fa.prof)) return rc;
  const size_t desc_off = ((size_t)2 * SPEC2_G * K * sizeof(float) + 15) & ~(size_t)15;
  const size_t flds = desc_off + 4096 + 64 + 512 + (size_t)SPEC2_G * 12 * 28 * sizeof(float);
  fa.desc_offset = (uint32_t)desc_off;
  const unsigned n_persist = spec2_grid(ix->n_cus, wt.max_groups);
  timed_launch(ix, s, "ivf_exact_scan", [&] { hipLaunchKernelGGL(spec2_kernel(K == 1024), dim3(n_persist), dim3(SPEC2_T), flds, s, fa); });
  HIP_TRY(hipGetLastError());
#ifdef FREDDY_LAB
  if (fa.prof) if (int rc = scan_prof_print(ix, s, fa.prof, n_persist)) return rc;
#endif
  return launch_merge_surv(r, pa, fa.surv, fa.surv_count, fa.cand_count);
}

// Every other index shape (multi.h): exact LUTs of all items -> ivf_multi_kernel -> merge_surv_kernel.
int ivf_scan_multi(IvfRun& r, const PlanArgs& pa, const WorkTable& wt) {
  Workspace* ws = r.ws;
  freddy_gpu_index* ix = r.ix;
  hipStream_t s = r.s;
  const int n_items = r.n_active * r.W;
  if (int rc = launch_lut(ix, s, r.d_q, pa.item_cell, ws->w_lut.as<float>(), n_items, ix->coarse, pa.item_query)) return rc;
  MultiArgs ma;
  ma.lut = ws->w_lut.as<float>(); ma.item_query = pa.item_query; ma.sorted_item = ws->w_sorted.as<int32_t>();
  ma.group_cell = wt.group_cell; ma.group_first = wt.group_first; ma.group_cnt = wt.group_cnt; ma.n_groups = wt.n_groups;
  ma.work_counter = wt.work_counter; ma.blk_off = ix->blk_off; ma.packed = ix->packed; ma.pos = ix->pos;
  ma.surv = ws->w_surv.as<u64>(); ma.surv_count = ws->w_surv_cnt.as<int32_t>();
  ma.cand_count = rows_counter(r);
  ma.m = ix->m; ma.M2 = ix->M2; ma.K = ix->K; ma.L = r.L; ma.upi = r.upi;
  memcpy(&ma.sentinel_bits, &r.sentinel, 4);
  const size_t lds = multi_lds_bytes(ix->m, ix->K);
  // persistent workgroups: as many as fit (LDS, 8 waves of ~100 registers), never more than there is work
  const unsigned grid = multi_grid(ix->n_cus, wt.max_groups, lds);
  timed_launch(ix, s, "ivf_multi_scan", [&] { hipLaunchKernelGGL(ivf_multi_kernel, dim3(grid), dim3(MULTI_T), lds, s, ma); });
  HIP_TRY(hipGetLastError());
  return launch_merge_surv(r, pa, ma.surv, ma.surv_count, ma.cand_count);
}

// The kernels of this unit that want more than the default 64 KiB of dynamic LDS.
std::vector<LdsLimit> lds_limits_ivf_scan() {
  std::vector<LdsLimit> l = {&ivf_spec2_kernel<25, 12, true>, &ivf_spec2_kernel<25, 12, false>, &ivf_multi_kernel};
  for (int i = 0; i < 32; ++i) {   // every kernel the chooser returns (one that comes up twice gets its limit twice)
    if (const auto k = filter_kernel(i & 1, i & 2, i & 4, i & 8, i & 16)) l.emplace_back(k);
    if (const auto k = filter_kernel(i & 1, i & 2, i & 4, i & 8, i & 16, true)) l.emplace_back(k);
  }
  return l;
}
