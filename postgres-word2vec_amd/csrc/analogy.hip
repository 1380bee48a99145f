// analogy.hip -- the exact analogies on a raw-vector handle (freddy--0.0.1.sql:1231-1315; analogy.h): 3CosAdd, 3CosMul and pair
// direction, all-exact or as filter + refine (exact_host.h: what the filter shares with exact kNN); the rows of an id set are
// exact.hip's (resolve_row_set, vec_subset).  resolve_triples, the INNER JOIN of analogy triples, serves rerank.hip too.
#include "internal.h"

#include "analogy.h"
#include "exact_host.h"

// ---- analogy triples -> table rows -----------------------------------------------------------------------------------------------
// The INNER JOINs of the analogy entry points: a triple with an unknown id has no rows at all; the others, compacted -- live: their
// positions in the call, rows3 / ids3 (optional): their three table rows / ids.  h_ids is strictly ascending (pin_vectors); serial ids
// (last - first + 1 of them) make the row a subtraction: 3 Q binary searches over millions of ids cost more than a batch's device work.
void resolve_triples(const std::vector<int32_t>& h_ids, const int32_t* triples, int32_t Q, std::vector<int32_t>& live, std::vector<int32_t>& rows3,
                     std::vector<int32_t>* ids3) {
  const bool serial = !h_ids.empty() && (int64_t)h_ids.back() - h_ids.front() + 1 == (int64_t)h_ids.size();
  auto row = [&](int32_t id) -> int32_t {
    if (serial) return id >= h_ids.front() && id <= h_ids.back() ? id - h_ids.front() : -1;
    return row_of(h_ids, id);
  };
  live.reserve((size_t)Q); rows3.reserve((size_t)Q * 3);
  if (ids3) ids3->reserve((size_t)Q * 3);
  for (int32_t q = 0; q < Q; ++q) {
    const int32_t* t = triples + (size_t)q * 3;
    int32_t r[3];
    bool ok = true;
    for (int m = 0; m < 3 && ok; ++m) ok = (r[m] = row(t[m])) >= 0;
    if (!ok) continue;
    live.push_back(q);
    rows3.insert(rows3.end(), r, r + 3);
    if (ids3) ids3->insert(ids3->end(), t, t + 3);
  }
}

// ---- exact analogies (analogy.h) ----------------------------------------------------------------------------------------
// Analogies per workgroup of the pair-direction scan: the smallest tile of 1, 2, 4, 8 that holds the call (a tile's spare columns
// repeat the last analogy: their divisions are done and thrown away), 8 beyond -- per (row, analogy) the kernel keeps a sum, a
// length and three excluded rows in registers and 8 d bytes + 4.5 KiB of lists in LDS, so 8 analogies stay far from either budget
// up to d = 1983; wider tables halve the tile until its columns fit (4 fits every d the entry point accepts).
static int an_pair_tile(int na, int d) {
  int at = na >= 8 ? 8 : na > 2 ? 4 : na;
  while (at > 1 && (at == 8 ? an_pair_lds<8>(d) : at == 4 ? an_pair_lds<4>(d) : an_pair_lds<2>(d)) > AN_MAX_LDS) at /= 2;
  return at;
}

// The all-exact path for the na analogies at d_in_rows (device [na][3] table rows): their columns, scores of every eligible row and
// per-wave lists, one merge per analogy into d_ids / d_score ([na][k]).  Enqueued only.  M = 1 (3CosAdd: one column, 8 analogies per
// workgroup), 3 (3CosMul: 4 analogies) or 0: FREDDY_ANALOGY_PAIR_DIRECTION, the columns (A, v3) per analogy and the two-sweep scan.
static int analogy_scan(freddy_gpu_index* ix, Workspace* ws, hipStream_t s, int M, const int32_t* d_in_rows, int na, int k, const float* xb,
                        const int32_t* pos, int64_t n_rows, int64_t n_blocks, int32_t* d_ids, double* d_score) {
  const int d = ix->d;
  const int AT = M == 0 ? an_pair_tile(na, d) : M == 1 ? 8 : 4, ncols = M == 0 ? 2 : M;
  const int groups = (na + AT - 1) / AT;
  int chunk_blocks;
  const int nchunk = scan_chunks(n_blocks, groups, &chunk_blocks);
  if (ws->w_qc.ensure(sizeof(float) * (size_t)na * ncols * d) || ws->w_part.ensure(sizeof(AnEnt) * (size_t)na * nchunk * AN_WAVES * k))
    return fail(FREDDY_E_NOMEM, "workspace allocation failed");
  float* cols = ws->w_qc.as<float>();
  if (M == 0) timed_launch(ix, s, "analogy_pair_columns", [&] { hipLaunchKernelGGL(an_pair_columns_kernel, dim3((unsigned)na), dim3(64), 0, s, ix->coarse, d, d_in_rows, cols); });
  else timed_launch(ix, s, "analogy_gather", [&] { hipLaunchKernelGGL(an_gather_kernel, dim3((unsigned)(na * M)), dim3(256), 0, s, ix->coarse, d, d_in_rows, na, M, 0, cols); });
  HIP_TRY(hipGetLastError());
  AnScanArgs sa;
  sa.xb = xb; sa.pos = pos; sa.n_rows = n_rows; sa.n_blocks = (int)n_blocks; sa.chunk_blocks = chunk_blocks; sa.nchunk = nchunk;
  sa.cols = cols; sa.in_rows = d_in_rows; sa.na = na; sa.d = d; sa.k = k; sa.part = ws->w_part.as<AnEnt>();
  const dim3 grid((unsigned)nchunk, (unsigned)groups);
  timed_launch(ix, s, M == 0 ? "analogy_pair_scan" : "analogy_scan", [&] {
    if (M == 1) hipLaunchKernelGGL((an_scan_kernel<1, 8>), grid, dim3(AN_WG), (an_scan_lds<1, 8>(d)), s, sa);
    else if (M == 3) hipLaunchKernelGGL((an_scan_kernel<3, 4>), grid, dim3(AN_WG), (an_scan_lds<3, 4>(d)), s, sa);
    else if (AT == 8) hipLaunchKernelGGL((an_pair_scan_kernel<8>), grid, dim3(AN_WG), an_pair_lds<8>(d), s, sa);
    else if (AT == 4) hipLaunchKernelGGL((an_pair_scan_kernel<4>), grid, dim3(AN_WG), an_pair_lds<4>(d), s, sa);
    else if (AT == 2) hipLaunchKernelGGL((an_pair_scan_kernel<2>), grid, dim3(AN_WG), an_pair_lds<2>(d), s, sa);
    else hipLaunchKernelGGL((an_pair_scan_kernel<1>), grid, dim3(AN_WG), an_pair_lds<1>(d), s, sa);
  });
  HIP_TRY(hipGetLastError());
  timed_launch(ix, s, "analogy_merge", [&] {
    hipLaunchKernelGGL(an_merge_kernel, dim3((unsigned)na), dim3(AN_WG), 0, s, (const AnEnt*)sa.part, nchunk * AN_WAVES, k, ix->ids, d_ids, d_score);
  });
  HIP_TRY(hipGetLastError());
  return 0;
}

// The filter + refine path over the whole table, passes of AN_PASS analogies.  flags[p] (device, zeroed here) != 0: pass p's
// results are not valid (its columns were not finite, or a candidate buffer overflowed) -- the caller redoes it; flags[passes + p]
// receives the number of candidates pass p refined.  Enqueued only.  Its filter, threshold and refine kernels and its double
// thresholds are its own; the plan, the prep kernel and the sample / filter launch pair are exact kNN's (exact_host.h).
static int analogy_filter(freddy_gpu_index* ix, Workspace* ws, hipStream_t s, int M, const int32_t* d_in_rows, int na, int k,
                          int32_t* d_ids, double* d_score, int32_t* flags) {
  const int d = ix->d, T = (d + 15) / 16;
  const int64_t N = ix->N;
  const FilterPlan fp = filter_plan(N, (ix->tune.check_brackets & 8) != 0);
  const int n_sample = fp.n_sample, cap = fp.cap, all = fp.refine_all ? 1 : 0;
  const int passes = (na + AN_PASS - 1) / AN_PASS;
  // per-pass state: [0, 256) tau (double [32]), [256, 640) eps, [640, 1024) unscale (float [96]), [1024, 1152) candidate counts
  if (ws->w_found.ensure(2048) || ix->exf_qfrag.ensure((size_t)M * T * 2 * 64 * 16) || ws->w_qc.ensure(sizeof(float) * (size_t)M * AN_PASS * d) ||
      ix->exf_sample.ensure(sizeof(double) * (size_t)AN_PASS * std::max(n_sample, 1)) || ix->exf_cand.ensure(sizeof(uint4) * (size_t)AN_PASS * cap))
    return fail(FREDDY_E_NOMEM, "workspace allocation failed");
  if (int rc = ensure_viol(ix)) return rc;
  char* sm = ws->w_found.as<char>();
  double* thr = reinterpret_cast<double*>(sm);
  float* qeps = reinterpret_cast<float*>(sm + 256);
  float* qunscale = reinterpret_cast<float*>(sm + 640);
  int32_t* cand_cnt = reinterpret_cast<int32_t*>(sm + 1024);
  float* cols = ws->w_qc.as<float>();
  double* sample = ix->exf_sample.as<double>();
  HIP_TRY(hipMemsetAsync(flags, 0, sizeof(int32_t) * 2 * passes, s));
  const size_t flds = an_filter_lds(M, d);
  for (int p = 0; p < passes; ++p) {
    const int a0 = p * AN_PASS, np = std::min(AN_PASS, na - a0);
    const int32_t* in_rows = d_in_rows + (size_t)a0 * 3;
    timed_launch(ix, s, "analogy_gather", [&] {
      hipLaunchKernelGGL(an_gather_kernel, dim3((unsigned)(M * AN_PASS)), dim3(256), 0, s, ix->coarse, d, in_rows, np, M, 1, cols);
    });
    HIP_TRY(hipGetLastError());
    const ExfPrepArgs pa = exf_prep_args(ix, cols, M * AN_PASS, qeps, qunscale, flags + p, nullptr);
    timed_launch(ix, s, "analogy_prep", [&] { hipLaunchKernelGGL(exf_prep_kernel, dim3((unsigned)(M * AN_PASS)), dim3(256), 0, s, pa); });
    HIP_TRY(hipGetLastError());
    AnFilterArgs fa;
    fa.xf = ix->exf_xf.as<h8v>(); fa.T = T; fa.qfrag = ix->exf_qfrag.as<h8v>(); fa.qunscale = qunscale; fa.qeps = qeps; fa.in_rows = in_rows; fa.na = np;
    fa.thr = thr; fa.cand_cnt = cand_cnt; fa.cand = ix->exf_cand.as<uint4>(); fa.cap = cap; fa.refine_all = all;
    auto filter = [&](auto smp, int64_t n_rows) {
      constexpr bool SAMPLE = decltype(smp)::value;
      filter_rows(fa, fp, SAMPLE, n_rows, sample);
      if (M == 1) hipLaunchKernelGGL((an_filter_kernel<1, SAMPLE>), dim3(filter_grid(ix, n_rows)), dim3(EXF_WG), flds, s, fa);
      else hipLaunchKernelGGL((an_filter_kernel<3, SAMPLE>), dim3(filter_grid(ix, n_rows)), dim3(EXF_WG), flds, s, fa);
    };
    if (n_sample > 0) {
      timed_launch(ix, s, "analogy_sample", [&] { filter(std::true_type(), n_sample); });
      HIP_TRY(hipGetLastError());
    }
    timed_launch(ix, s, "analogy_threshold", [&] {
      hipLaunchKernelGGL(an_threshold_kernel, dim3(AN_PASS), dim3(AN_WG), 0, s, (const double*)sample, n_sample, np, k, all, thr, cand_cnt);
    });
    HIP_TRY(hipGetLastError());
    timed_launch(ix, s, "analogy_filter", [&] { filter(std::false_type(), N); });
    HIP_TRY(hipGetLastError());
    AnRefineArgs ra;
    ra.rows = ix->coarse; ra.cols = cols; ra.cand = fa.cand; ra.cand_cnt = cand_cnt; ra.qeps = qeps; ra.in_rows = in_rows; ra.viol = ix->viol;
    ra.flag = flags + p; ra.cand_total = flags + passes + p; ra.cap = cap; ra.d = d; ra.k = k; ra.count_checked = all; ra.ids = ix->ids;
    ra.out_ids = d_ids + (size_t)a0 * k; ra.out_score = d_score + (size_t)a0 * k;
    timed_launch(ix, s, "analogy_refine", [&] {
      if (M == 1) hipLaunchKernelGGL((an_refine_kernel<1>), dim3((unsigned)np), dim3(64 * AN_RW), an_refine_lds(1, d), s, ra);
      else hipLaunchKernelGGL((an_refine_kernel<3>), dim3((unsigned)np), dim3(64 * AN_RW), an_refine_lds(3, d), s, ra);
    });
    HIP_TRY(hipGetLastError());
  }
  return 0;
}

extern "C" int freddy_gpu_exact_analogy(freddy_gpu_index_t* ix, int32_t method, const int32_t* triples, int32_t Q, int32_t k,
                                        const int32_t* subset_ids, int64_t n_subset, int32_t* out_ids, double* out_score) {
  // (the scalar arguments first: they are checked before the handle is looked at, so no device is needed to see these errors)
  if (method != FREDDY_ANALOGY_3COSADD && method != FREDDY_ANALOGY_3COSMUL && method != FREDDY_ANALOGY_PAIR_DIRECTION)
    return fail(FREDDY_E_ARG, "unknown analogy method %d", method);
  if (Q < 0 || k <= 0 || n_subset < 0 || (n_subset > 0 && !subset_ids)) return fail(FREDDY_E_ARG, "bad sizes");
  if (Q > 0 && (!triples || !out_ids || !out_score)) return fail(FREDDY_E_ARG, "NULL buffer");
  if (k > AN_MAXK) return fail(FREDDY_E_LIMIT, "k=%d exceeds the exact analogy's limit of %d", k, AN_MAXK);
  if (int rc = check_vec_handle(ix)) return rc;
  const int M = method == FREDDY_ANALOGY_3COSMUL ? 3 : 1;
  const int d = ix->d;
  ix->an_stats[0] = ix->an_stats[1] = ix->an_stats[2] = 0;
  if (std::max(an_scan_lds<1, 8>(d), an_scan_lds<3, 4>(d)) > AN_MAX_LDS) return fail(FREDDY_E_LIMIT, "d=%d too large for the exact analogy", d);
  for (size_t i = 0; i < (size_t)Q * k; ++i) { out_ids[i] = -1; out_score[i] = -HUGE_VAL; }
  if (Q == 0) return FREDDY_OK;
  std::vector<int32_t> live, rows3;
  resolve_triples(ix->h_ids, triples, Q, live, rows3);
  const int na = (int)live.size();
  if (na == 0) return FREDDY_OK;
  HIP_TRY(hipSetDevice(ix->device));
  Workspace* ws = workspace_for(ix, ix->stream);
  hipStream_t s = ix->stream;
  const float* xb = ix->xb;
  const int32_t* pos = nullptr;
  int64_t n_rows = ix->N, n_blocks = ix->n_blocks;
  if (subset_ids) {
    std::vector<int32_t> h_rows;
    RowSet rows;
    if (int rc = resolve_row_set(ix, ix->tune.exact_resolve != 0, subset_ids, n_subset, &h_rows, &rows)) return rc;
    if (rows.size() == 0) return FREDDY_OK;   // (a host set: before any launch; the lists stay empty)
    if (int rc = vec_subset(ix, ws, s, rows, &xb, &pos, &n_rows, &n_blocks)) return rc;
  }
  const int passes = (na + AN_PASS - 1) / AN_PASS;
  if (ws->w_rows.ensure(sizeof(int32_t) * rows3.size()) || ws->w_out_ids.ensure(sizeof(int32_t) * (size_t)na * k) ||
      ws->w_out_dist.ensure(sizeof(double) * (size_t)na * k) || ws->w_cnt.ensure(sizeof(int32_t) * 2 * (size_t)passes))
    return fail(FREDDY_E_NOMEM, "workspace allocation failed");
  int32_t* d_rows = ws->w_rows.as<int32_t>();
  int32_t* d_ids = ws->w_out_ids.as<int32_t>();
  double* d_score = ws->w_out_dist.as<double>();
  HIP_TRY(hipMemcpyAsync(d_rows, rows3.data(), sizeof(int32_t) * rows3.size(), hipMemcpyHostToDevice, s));
  // filter + refine: the whole table, k <= 32, finite rows of a supported shape (exact kNN's eligibility)
  // and the pass's query fragments must fit the LDS of a CU (an_filter_kernel holds all M tiles: 3CosMul with d > 416 does not)
  // pair direction has no filter: its score is no dot product against a fixed column (analogy.h)
  const bool pair = method == FREDDY_ANALOGY_PAIR_DIRECTION;
  const bool want_filter = !pair && !subset_ids && exf_wanted(ix, n_rows) && an_filter_lds(M, d) <= AN_MAX_LDS;
  std::vector<int32_t> redo;   // passes the all-exact path computes
  if (want_filter) {
    if (int rc = analogy_filter(ix, ws, s, M, d_rows, na, k, d_ids, d_score, ws->w_cnt.as<int32_t>())) return rc;
    std::vector<int32_t> flags(2 * (size_t)passes);
    HIP_TRY(hipMemcpyAsync(flags.data(), ws->w_cnt.p, sizeof(int32_t) * 2 * passes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int p = 0; p < passes; ++p) {
      if (flags[p]) redo.push_back(p);
      else ix->an_stats[1] += flags[passes + p];
    }
    ix->an_stats[0] = passes;
    ix->an_stats[2] = (int64_t)redo.size();
  }
  // the all-exact path: everything, or the passes the filter could not vouch for (in chunks that bound the partial lists)
  const int chunk = 1024;
  auto scan_range = [&](int a0, int n) -> int {
    for (int c0 = a0; c0 < a0 + n; c0 += chunk) {
      const int nc = std::min(chunk, a0 + n - c0);
      if (int rc = analogy_scan(ix, ws, s, pair ? 0 : M, d_rows + (size_t)c0 * 3, nc, k, xb, pos, n_rows, n_blocks, d_ids + (size_t)c0 * k, d_score + (size_t)c0 * k))
        return rc;
    }
    return 0;
  };
  if (!want_filter) {
    if (int rc = scan_range(0, na)) return rc;
  } else {
    for (int p : redo) if (int rc = scan_range(p * AN_PASS, std::min(AN_PASS, na - p * AN_PASS))) return rc;
  }
  std::vector<int32_t> h_ids((size_t)na * k);
  std::vector<double> h_score((size_t)na * k);
  HIP_TRY(hipMemcpyAsync(h_ids.data(), d_ids, sizeof(int32_t) * h_ids.size(), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(h_score.data(), d_score, sizeof(double) * h_score.size(), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  for (int a = 0; a < na; ++a) {
    memcpy(out_ids + (size_t)live[a] * k, h_ids.data() + (size_t)a * k, sizeof(int32_t) * k);
    memcpy(out_score + (size_t)live[a] * k, h_score.data() + (size_t)a * k, sizeof(double) * k);
  }
  return FREDDY_OK;
}

extern "C" int freddy_gpu_last_analogy_stats(const freddy_gpu_index_t* ix, int64_t* filter_passes, int64_t* candidates, int64_t* redone_passes) {
  if (!ix) return fail(FREDDY_E_ARG, "NULL index");
  if (ix->kind != KIND_VEC) return fail(FREDDY_E_KIND, "index handle has the wrong kind for this call");
  if (filter_passes) *filter_passes = ix->an_stats[0];
  if (candidates) *candidates = ix->an_stats[1];
  if (redone_passes) *redone_passes = ix->an_stats[2];
  return FREDDY_OK;
}

// The kernels of this unit that want more than the default 64 KiB of dynamic LDS.
std::vector<LdsLimit> lds_limits_analogy() {
  const int b = (int)AN_MAX_LDS;
  return {{&an_filter_kernel<1, false>, b},  {&an_filter_kernel<3, false>, b},  {&an_filter_kernel<1, true>, b},  {&an_filter_kernel<3, true>, b},
          {&an_scan_kernel<1, 8>, b},        {&an_scan_kernel<3, 4>, b},
          {&an_pair_scan_kernel<1>, b},      {&an_pair_scan_kernel<2>, b},      {&an_pair_scan_kernel<4>, b},     {&an_pair_scan_kernel<8>, b}};
}
