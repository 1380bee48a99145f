// generic.hip -- the launches every index shape can take, which pq.hip calls as well (the flat PQ table, grouping_pq, the assignment
// step): LUTs -> adc_scan_kernel -> merge_replay_kernel, the selection passes of k > 512 (bigk.h), and the IVFADC round built of them.
#include "internal.h"

#include "kernels.h"
#include "bigk.h"
#include "ivf_host.h"

// ---------------------------------------------------------------------------------------
// kernel dispatch helpers.  A chooser maps the run-time facts to the instantiation (NULL: there is none); the launch site launches
// the pointer and the unit's lds_limits_*() walks the same function over its domain: nothing is launched without its LDS limit.
// ---------------------------------------------------------------------------------------
// adc_scan_kernel<M, V, FLOOR>: m = 12 or any m; V = pick_V(L); FLOOR: a later selection pass of a long list (bigk.h), 1024 keys wide
static void (*scan_kernel(bool m12, int V, bool floor))(ScanArgs) {
  void (*k)(ScanArgs) = nullptr;
  if (floor) return V != 16 ? nullptr : m12 ? &adc_scan_kernel<12, 16, true> : &adc_scan_kernel<0, 16, true>;
  with_V(V, [&](auto v) { k = m12 ? &adc_scan_kernel<12, decltype(v)::value> : &adc_scan_kernel<0, decltype(v)::value>; });
  return k;
}

int pick_V(int L) {
  if (L <= 64) return 1;
  if (L <= 128) return 2;
  if (L <= 256) return 4;
  if (L <= 512) return 8;
  if (L <= 1024) return 16;
  return 0;
}

int launch_scan(freddy_gpu_index* ix, hipStream_t s, const ScanArgs& a, int n_items) {
  if (n_items <= 0 || a.nchunk <= 0) return 0;
  const int V = pick_V(a.L);
  const size_t lds = std::max((((size_t)a.m * a.K * 4 + 15) & ~(size_t)15) + (size_t)SCAN_WAVES * 64 * sizeof(u64),
                              (size_t)SCAN_WAVES * 64 * V * sizeof(u64));
  dim3 grid((unsigned)a.nchunk, (unsigned)n_items);
  if (a.floor && V != 16) return fail(FREDDY_E_ARG, "selection passes are 1024 keys wide");   // (a later pass of a list of more than 512 entries, bigk.h)
  const auto kernel = scan_kernel(a.m == 12, V, a.floor != nullptr);
  if (!kernel) return fail(FREDDY_E_LIMIT, "unsupported selection width");
  timed_launch(ix, s, "adc_scan", [&] { hipLaunchKernelGGL(kernel, grid, dim3(SCAN_WG), lds, s, a); });
  HIP_TRY(hipGetLastError());
  return 0;
}

int launch_merge(freddy_gpu_index* ix, hipStream_t s, const MergeArgs& a) {
  if (a.n_active <= 0) return 0;
  const int V = pick_V(a.L);
  dim3 grid((unsigned)a.n_active), block(64);
  timed_launch(ix, s, "merge_replay", [&] {
    with_V(V, [&](auto v) { hipLaunchKernelGGL((merge_replay_kernel<decltype(v)::value>), grid, block, 0, s, a); });
  });
  HIP_TRY(hipGetLastError());
  return 0;
}

// k > 512 (bigk.h): the 2k smallest keys of every active query, 1024 per pass over the same rows, then the list in closed form.
// sa: the generic scan's arguments with L = 1024; ma: what merge_replay_kernel would get (its L is not used); Q: queries of the chunk.
int bigk_select_replay(freddy_gpu_index* ix, hipStream_t s, Workspace* ws, ScanArgs sa, int n_items, const MergeArgs& ma, int Q) {
  if (ma.n_active <= 0) return 0;
  const int k = ma.k;
  if (k > BIGK_KMAX) return fail(FREDDY_E_LIMIT, "k=%d exceeds this build's limit of %d", k, BIGK_KMAX);
  if (sa.L != BIGK_PASS) return fail(FREDDY_E_ARG, "selection passes are %d keys wide (got L=%d)", BIGK_PASS, sa.L);
  const int passes = (2 * k + BIGK_PASS - 1) / BIGK_PASS;
  const int nsel = passes * BIGK_PASS;
  int npad = 2048;
  while (npad < k + nsel) npad *= 2;
  if (ws->w_bigsel.ensure(sizeof(u64) * (size_t)ma.n_active * nsel) || ws->w_floor.ensure(sizeof(u64) * (size_t)std::max(Q, 1)))
    return fail(FREDDY_E_NOMEM, "workspace allocation failed (k=%d)", k);
  SelectArgs se;
  se.part = sa.part; se.active = ma.active; se.sel = ws->w_bigsel.as<u64>(); se.floor = ws->w_floor.as<u64>();
  se.parts_per_query = ma.parts_per_query; se.nsel = nsel;
  int32_t* const cand_count = sa.cand_count;
  for (int p = 0; p < passes; ++p) {
    sa.floor = p ? ws->w_floor.as<u64>() : nullptr;
    sa.cand_count = p ? nullptr : cand_count;   // (the accepted-rows rule counts every row once)
    if (int rc = launch_scan(ix, s, sa, n_items)) return rc;
    se.pass = p;
    timed_launch(ix, s, "merge_select", [&] { hipLaunchKernelGGL(merge_select_kernel, dim3(ma.n_active), dim3(64), 0, s, se); });
    HIP_TRY(hipGetLastError());
  }
  BigkArgs b;
  b.sel = se.sel; b.active = ma.active; b.pos_to_id = ma.pos_to_id; b.round_rows = ma.round_rows; b.cand_count = ma.cand_count;
  b.out_ids = ma.out_ids; b.out_dist = ma.out_dist; b.found = ma.found; b.next_active = ma.next_active; b.n_next = ma.n_next;
  b.status = ma.status; b.n_active = ma.n_active; b.nsel = nsel; b.npad = npad; b.k = k; b.found_rule = ma.found_rule;
  b.first_round = ma.first_round; b.sentinel = ma.sentinel;
  timed_launch(ix, s, "bigk_replay", [&] {
    hipLaunchKernelGGL(bigk_replay_kernel, dim3(ma.n_active), dim3(BIGK_T), bigk_lds_bytes(npad, k), s, b);
  });
  HIP_TRY(hipGetLastError());
  return 0;
}

// coarse != NULL: `vecs` are the queries and the kernel forms the residual q - coarse[cell] itself (no residual_kernel launch)
int launch_lut(freddy_gpu_index* ix, hipStream_t s, const float* vecs, const int32_t* item_cell,
                      float* lut, int n_items, const float* coarse, const int32_t* item_query) {
  if (n_items <= 0) return 0;
  // enough workgroups to fill 256 CUs several times over, while amortising the register
  // fill of the codebook slice over as many items as possible
  int ipw = (int)std::max<int64_t>(1, ((int64_t)ix->m * n_items + 4095) / 4096);
  ipw = std::min(ipw, 64);
  dim3 grid((unsigned)ix->m, (unsigned)((n_items + ipw - 1) / ipw));
  const int m = ix->m, K = ix->K, d = ix->d, S = ix->S;
  timed_launch(ix, s, "lut_build", [&] {
    if (S == 25) hipLaunchKernelGGL((lut_build_kernel<25, 4>), grid, dim3(WG), 0, s, vecs, item_cell, ix->cbT, lut, n_items, ipw, m, K, d, coarse, item_query);
    else if (S == 10) hipLaunchKernelGGL((lut_build_kernel<10, 4>), grid, dim3(WG), 0, s, vecs, item_cell, ix->cbT, lut, n_items, ipw, m, K, d, coarse, item_query);
    else if (S == 20) hipLaunchKernelGGL((lut_build_kernel<20, 4>), grid, dim3(WG), 0, s, vecs, item_cell, ix->cbT, lut, n_items, ipw, m, K, d, coarse, item_query);
    else hipLaunchKernelGGL(lut_build_generic_kernel, grid, dim3(WG), 0, s, vecs, item_cell, ix->cbT, lut, n_items, ipw, m, K, d, S, coarse, item_query);
  });
  HIP_TRY(hipGetLastError());
  return 0;
}

// Generic path (small batches, other m / S / K, k > 32): lut_build (residual inline) -> adc_scan -> merge_replay;
// the LUTs round-trip through memory.
int ivf_scan_generic(IvfRun& r, const PlanArgs& pa) {
  Workspace* ws = r.ws;
  freddy_gpu_index* ix = r.ix;
  hipStream_t s = r.s;
  const int n_items = r.n_active * r.W;
  const Chunks ch = generic_chunks(ix, (size_t)n_items);
  // (the residual r = q - coarse[cell] is formed by the LUT kernel: one launch less in a single query's chain)
  if (int rc = launch_lut(ix, s, r.d_q, pa.item_cell, ws->w_lut.as<float>(), n_items, ix->coarse, pa.item_query)) return rc;
  ScanArgs sa;
  sa.lut = ws->w_lut.as<float>(); sa.item_list = pa.item_cell; sa.item_query = pa.item_query;
  sa.blk_off = ix->blk_off; sa.packed = ix->packed; sa.pos = ix->pos; sa.part = ws->w_part.as<u64>();
  sa.cand_count = ws->w_cand.as<int32_t>();
  sa.m = ix->m; sa.K = ix->K; sa.chunk_blocks = ch.blocks; sa.nchunk = ch.n; sa.L = r.L;
  memcpy(&sa.sentinel_bits, &r.sentinel, 4);
  const MergeArgs ma = merge_args_round(r, pa, sa.part, r.W * ch.n, sa.cand_count);
  if (2 * r.k > 1024) return bigk_select_replay(ix, s, ws, sa, n_items, ma, r.Q);
  if (int rc = launch_scan(ix, s, sa, n_items)) return rc;
  return launch_merge(ix, s, ma);
}

// The kernels of this unit that want more than the default 64 KiB of dynamic LDS.
std::vector<LdsLimit> lds_limits_generic() {
  // (static LDS beside the dynamic: 16384 keys + 4096 carried ids = 144 KB)
  std::vector<LdsLimit> l = {{&bigk_replay_kernel, (int)bigk_lds_bytes(16384, BIGK_KMAX)}};
  for (int i = 0; i < 32; ++i)   // every kernel the chooser returns (one that comes up twice gets its limit twice)
    if (const auto k = scan_kernel(i & 1, 1 << (i >> 2), i & 2)) l.emplace_back(k);   // (V = 1 .. 128: none beyond 16)
  return l;
}
