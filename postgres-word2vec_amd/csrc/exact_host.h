// exact_host.h -- the host-side sequences that the entry points of exact.hip share (included by exact.hip alone, after the kernel
// headers): the filter + refine chain of exact kNN and the exact join with the handle's state it runs on, the chunking of the
// all-exact scans, the re-rank stage of post verification and the approximate analogies, and the INNER JOIN of analogy triples.
#pragma once

#include "internal.h"
#include "exact2.h"
#include "pv.h"
#include "approx_analogy.h"

// ---- filter + refine (exact2.h, exact_join.h, analogy.h) -----------------------------------------------------------------
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

// ---- the re-rank stage of post verification and the approximate analogies (pv.h, approx_analogy.h) ----------------------------
// Queries (triples) per pass: stage one's lists of `n_cand` entries hold at most 8 M entries
static int rerank_pass(int64_t n, int n_cand) { return (int)std::min<int64_t>(n, std::max<int64_t>(1, ((int64_t)8 << 20) / n_cand)); }

// The pinned block of one pass of Qc queries: [stage one's lists][the result lists][per-query counts]; the approximate analogies put
// their unit rows (padded to 16 bytes) in front and the input rows and ids behind.
struct RerankBlock {
  float *unit, *l_dist, *o_sim;
  int32_t *l_ids, *o_ids, *o_cnt, *p_rows, *p_excl;
};
static int rerank_block(freddy_gpu_index* ann, int Qc, int n_cand, int k, bool analogy, const char* call, RerankBlock* b) {
  const int d = ann->d;
  const size_t n_unit = analogy ? ((size_t)Qc * d + 3) / 4 * 4 : 0, n_list = (size_t)Qc * n_cand, n_out = (size_t)Qc * k;
  if (ann->pv_io.ensure(4 * (n_unit + 2 * n_list + 2 * n_out + 2 * (size_t)Qc + (analogy ? 6 * (size_t)Qc : 0))) || ann->pv_q.ensure(sizeof(float) * (size_t)Qc * d))
    return fail(FREDDY_E_NOMEM, "%s: staging allocation failed", call);
  b->unit = ann->pv_io.as<float>();
  b->l_ids = reinterpret_cast<int32_t*>(b->unit + n_unit); b->l_dist = reinterpret_cast<float*>(b->l_ids + n_list);
  b->o_ids = b->l_ids + 2 * n_list; b->o_sim = reinterpret_cast<float*>(b->o_ids + n_out);
  b->o_cnt = b->o_ids + 2 * n_out;
  b->p_rows = b->o_cnt + 2 * (size_t)Qc; b->p_excl = b->p_rows + 3 * (size_t)Qc;
  return 0;
}
// The re-rank of `nq` lists of the block against the raw queries in pv_q, by pv_rerank_kernel<NW> or aa_rerank_kernel<NW> (which
// leaves out the ids at `exclude`): k1 = <1>, one wave per query, for lists of up to 64 entries, k4 = <4> beyond.
using RerankKernel = void (*)(PvArgs);
static int launch_rerank(freddy_gpu_index* ann, const freddy_gpu_index* vecs, hipStream_t s, const char* label, RerankKernel k1, RerankKernel k4,
                         const RerankBlock& b, const int32_t* exclude, int nq, int n_cand, int k) {
  const int d = ann->d, P = pv_pad(n_cand);
  PvArgs pa;
  pa.cand = b.l_ids; pa.vec_ids = vecs->ids; pa.rows = vecs->coarse; pa.queries = ann->pv_q.as<float>(); pa.exclude = exclude; pa.out_ids = b.o_ids;
  pa.out_sim = b.o_sim; pa.counts = b.o_cnt; pa.N = vecs->N; pa.n_cand = n_cand; pa.k = k; pa.d = d; pa.P = P;
  timed_launch(ann, s, label, [&] {
    if (P == 64) hipLaunchKernelGGL(k1, dim3((unsigned)nq), dim3(64), pv_lds_bytes(1, P, d), s, pa);
    else hipLaunchKernelGGL(k4, dim3((unsigned)nq), dim3(256), pv_lds_bytes(4, P, d), s, pa);
  });
  HIP_TRY(hipGetLastError());
  return 0;
}

// ---- analogy triples -> table rows -----------------------------------------------------------------------------------------------
// The INNER JOINs of the analogy entry points: a triple with an unknown id has no rows at all; the others, compacted -- live: their
// positions in the call, rows3 / ids3 (optional): their three table rows / ids.  h_ids is strictly ascending (pin_vectors); serial ids
// (last - first + 1 of them) make the row a subtraction: 3 Q binary searches over millions of ids cost more than a batch's device work.
static void resolve_triples(const std::vector<int32_t>& h_ids, const int32_t* triples, int32_t Q, std::vector<int32_t>& live, std::vector<int32_t>& rows3,
                            std::vector<int32_t>* ids3 = nullptr) {
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
