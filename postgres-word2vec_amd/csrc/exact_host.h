// exact_host.h -- the host-side sequences that exact.hip and analogy.hip share (included after their kernel headers): the filter +
// refine chain of exact kNN and the exact join with the handle's state it runs on, when a call takes it, and the chunking of the
// all-exact scans.
#pragma once

#include "internal.h"
#include "exact2.h"

// ---- filter + refine (exact2.h, exact_join.h, analogy.h) -----------------------------------------------------------------
// Under option exact_filter = -1 (auto) a whole table takes filter + refine from this many rows on.
static constexpr int64_t EXF_AUTO_ROWS = 8192;
// What exact kNN, the exact join and the exact analogies all ask before they take filter + refine: the handle has the filter's copy
// of its rows, the option does not forbid it, and it is forced or the set has `auto_rows` rows.  What else a call asks (k, no
// subset, the LDS its tiles take) stands at the call.
static bool exf_wanted(const freddy_gpu_index* ix, int64_t n_rows, int64_t auto_rows = EXF_AUTO_ROWS) {
  return ix->exf_ok && ix->tune.exact_filter != 0 && (ix->tune.exact_filter == 1 || n_rows >= auto_rows);
}

// What the filter passes over a set of rows share.  The threshold's sample: whole 32-row strips of REAL rows (a zero-padded row
// would be a similarity of 0 that no row has), spread evenly over the set; the candidate buffer: 8192 rows per query (every row
// under the self-check that refines every row).
struct FilterPlan { int n_sample; int64_t sample_stride; int cap; bool refine_all; };
static FilterPlan filter_plan(int64_t N, bool refine_all) {
  const int64_t full_strips = N / 32;
  const int n_sample = (int)(std::min<int64_t>(full_strips, EXF_SAMPLE / 32) * 32);
  return {n_sample, n_sample > 0 ? std::max<int64_t>(1, full_strips / (n_sample / 32)) : 1, (int)(refine_all ? N : std::min<int64_t>(N, 8192)), refine_all};
}
// workgroups of a filter kernel over `rows` rows of the whole table: one per 256 rows, at most two per CU
static unsigned filter_grid(const freddy_gpu_index* ix, int64_t rows) {
  return freddy::filter_grid(ix->n_cus, rows);
}
// A filter kernel runs twice per pass: over the sample's strips (it writes the similarities the threshold kernel selects from),
// then over all `n_rows` rows (it writes candidates).  What the two launches change in its arguments (ExfArgs, ExjArgs, AnFilterArgs).
template <class Args, class S>
static void filter_rows(Args& fa, const FilterPlan& fp, bool sample, int64_t n_rows, S* sample_buf) {
  fa.n_rows = n_rows; fa.strip_stride = sample ? fp.sample_stride : 1; fa.sample_out = sample ? sample_buf : nullptr;
}
// exf_prep_kernel's arguments for `nq` query rows at `queries` (every filter chain starts with it: the analogies' columns are its queries)
static ExfPrepArgs exf_prep_args(const freddy_gpu_index* ix, const float* queries, int nq, float* qeps, float* qunscale, int32_t* qbad, float* copy_out) {
  ExfPrepArgs pa;
  pa.queries = queries; pa.nq = nq; pa.d = ix->d; pa.T = (ix->d + 15) / 16; pa.xmax_norm = ix->exf_xnorm; pa.ex = ix->exf_ex;
  pa.eps_factor = exf_eps_factor(ix->d); pa.qfrag = ix->exf_qfrag.as<h8v>(); pa.qeps = qeps; pa.qunscale = qunscale; pa.qbad = qbad; pa.copy_out = copy_out;
  return pa;
}
// the self-check counters the refine kernels write (allocated by the handle's first filter + refine call)
static int ensure_viol(freddy_gpu_index* ix) {
  if (ix->viol) return 0;
  HIP_TRY(dev_malloc((void**)&ix->viol, 4 * sizeof(int32_t)));
  HIP_TRY(hipMemset(ix->viol, 0, 4 * sizeof(int32_t)));
  return 0;
}

// The words exf_refine_kernel keeps on the handle between the launches of a call -- exf_small [256] qbad, [257] arrived, viol[3] --
// are zero when a call starts: its last workgroup leaves them so.  exf_begin before a call's first launch (the handle's first call, or
// the one after a call that failed part-way: the words may be anything and are cleared), exf_complete once its verdict words arrived.
static int exf_begin(freddy_gpu_index* ix, hipStream_t s) {
  if (ix->exf_small.ensure(4096)) return fail(FREDDY_E_NOMEM, "workspace allocation failed");
  if (int rc = ensure_viol(ix)) return rc;
  if (ix->exf_dirty) {
    HIP_TRY(hipMemsetAsync(ix->exf_small.as<float>() + 256, 0, 8, s));
    HIP_TRY(hipMemsetAsync(ix->viol + 3, 0, 4, s));
  }
  ix->exf_dirty = true;
  return 0;
}
static void exf_complete(freddy_gpu_index* ix) { ix->exf_dirty = false; }
// after the synchronisation that ends a pass: its last refine workgroup has overwritten the two verdict words the caller set to -1
static int exf_verdict_arrived(const int32_t* flags, const char* call) {
  return flags[0] == -1 || flags[1] == -1 ? fail(FREDDY_E_HIP, "%s: the verdict words did not arrive", call) : 0;
}

struct ExfLabels { const char *prep, *sample, *threshold, *filter, *refine; };   // the chain's launches in a profile
static constexpr ExfLabels EXF_KNN_LABELS = {"exact_prep", "exact_sample", "exact_threshold", "exact_filter", "exact_refine"};
static constexpr ExfLabels EXF_JOIN_LABELS = {"exact_join_prep", "exact_join_sample", "exact_join_threshold", "exact_join_filter", "exact_join_refine"};

// One pass of the chain: `nq` queries against one set of rows.  Exact kNN keeps the small arrays in exf_small (a pass is one tile of
// EXF_QT queries) and its verdict words in mapped host memory, the join keeps all of them in its workspace (thousands of queries).
struct ExfPass {
  const ExfLabels* labels;
  FilterPlan fp;
  float *thr, *qeps, *qunscale;      // [grid_q] per query
  int32_t *cand_cnt, *flags;         // [grid_q]; the two verdict words the pass's (kNN: the call's) last refine workgroup writes
  const float* queries;              // [nq][d], device-visible
  float* copy_out;                   // NULL, or device memory the prep kernel copies the queries to (the refine kernel then reads them there)
  int nq, k;
  unsigned grid_q;                   // workgroups of the prep and threshold kernels: nq rounded up to whole query tiles
  int32_t* out_ids; float* out_sim;  // [nq][k]
  int total_wgs;                     // refine workgroups before the verdict words are written (kNN: the whole call's)
  bool sample_when_empty;            // exact kNN launches its sample kernel over a sample of no rows too; the join does not
};

// prep -> sample -> threshold -> filter -> refine, enqueued on s.  filter(std::true_type / std::false_type, n_rows) launches the
// caller's filter kernel over the sample / over all rows: its instantiation, grid and arguments are what kNN and the join do not share.
template <class FilterLaunch>
static int exf_chain(freddy_gpu_index* ix, hipStream_t s, const ExfPass& p, int64_t n_rows, FilterLaunch&& filter) {
  const int d = ix->d, V = pick_V(p.k);
  int32_t* const qbad = ix->exf_small.as<int32_t>() + 256;   // (and [257] arrived: the handle's words, exf_begin)
  const ExfPrepArgs pa = exf_prep_args(ix, p.queries, p.nq, p.qeps, p.qunscale, qbad, p.copy_out);
  timed_launch(ix, s, p.labels->prep, [&] { hipLaunchKernelGGL(exf_prep_kernel, dim3(p.grid_q), dim3(256), 0, s, pa); });
  HIP_TRY(hipGetLastError());
  if (p.fp.n_sample > 0 || p.sample_when_empty) {
    timed_launch(ix, s, p.labels->sample, [&] { filter(std::true_type(), (int64_t)p.fp.n_sample); });
    HIP_TRY(hipGetLastError());
  }
  ExfThrArgs ta;
  ta.sample = ix->exf_sample.as<float>(); ta.n_sample = p.fp.n_sample; ta.nq = p.nq; ta.k = p.k; ta.qeps = p.qeps; ta.qunscale = p.qunscale; ta.thr = p.thr;
  ta.refine_all = p.fp.refine_all ? 1 : 0; ta.cand_cnt = p.cand_cnt;
  timed_launch(ix, s, p.labels->threshold, [&] { hipLaunchKernelGGL(exf_threshold_kernel, dim3(p.grid_q), dim3(64 * EXF_TW), 0, s, ta); });
  HIP_TRY(hipGetLastError());
  timed_launch(ix, s, p.labels->filter, [&] { filter(std::false_type(), n_rows); });
  HIP_TRY(hipGetLastError());
  ExfRefineArgs ra;
  ra.rows = ix->coarse; ra.queries = p.copy_out ? p.copy_out : p.queries; ra.cand = ix->exf_cand.as<uint2>(); ra.cand_cnt = p.cand_cnt; ra.qeps = p.qeps;
  ra.viol = ix->viol; ra.cap = p.fp.cap; ra.d = d; ra.L = p.k; ra.count_checked = p.fp.refine_all ? 1 : 0;
  ra.ids = ix->ids; ra.out_ids = p.out_ids; ra.out_sim = p.out_sim; ra.k = p.k; ra.arrived = qbad + 1; ra.total_wgs = p.total_wgs;
  ra.qbad = qbad; ra.flags_out = p.flags;
  const size_t rlds = exf_refine_lds(d, V == 1 ? 1 : 2);
  timed_launch(ix, s, p.labels->refine, [&] {
    if (V == 1) hipLaunchKernelGGL((exf_refine_kernel<1>), dim3((unsigned)p.nq), dim3(64 * EXF_TW), rlds, s, ra);
    else hipLaunchKernelGGL((exf_refine_kernel<2>), dim3((unsigned)p.nq), dim3(64 * EXF_TW), rlds, s, ra);
  });
  HIP_TRY(hipGetLastError());
  return 0;
}

// ---- the all-exact scans (exact.h, analogy.h) ------------------------------------------------------------------------------
// Grid x of a (chunks of row blocks) x (groups of queries) scan: 512 rows per workgroup-chunk, longer chunks once the grid is large enough
static int scan_chunks(int64_t n_blocks, int groups, int* chunk_blocks) {
  int cb = 8;
  while ((n_blocks + cb - 1) / cb * (int64_t)groups > 8192 && cb < 1024) cb *= 2;
  *chunk_blocks = cb;
  return (int)std::max<int64_t>(1, (n_blocks + cb - 1) / cb);
}
