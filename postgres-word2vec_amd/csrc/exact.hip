// exact.hip -- pin_vectors, exact brute-force kNN (core_functions.c:67-81, freddy--0.0.1.sql:426-454), the
// exact analogies on the same handle (freddy--0.0.1.sql:1231-1315; analogy.h), the post verification of pq / ivf lists against it (pv.h)
// the approximate analogies over such lists (approx_analogy.h) and the assignment step of cluster_exact (assign.h), the whole k-means of cluster_exact / cluster_pq (cluster.h); exact_host.h: what they share.
// Exact kNN and the exact join by row id (freddy_gpu_exact_search_ids / _exact_join_ids): queries through a QuerySrc (query_ids.h), id sets resolved on the device (resolve.h).
#include "internal.h"

#include "kernels.h"
#include "exact.h"
#include "exact2.h"
#include "exact_join.h"
#include "analogy.h"
#include "pv.h"
#include "approx_analogy.h"
#include "assign.h"
#include "cluster.h"
#include "similarity.h"
#include "query_ids.h"
#include "resolve.h"
#include "tokenize.h"
#include "exact_host.h"

// ---- exact brute-force kNN as filter + refine (exact2.h) ----------------------------------------------------------------------
// The table's largest |element| / largest row norm over rows [r0, r0 + n) of the row-major copy, folded into the handle's.
// changed_strips (update_rows, r0 = 0): the 32-row strips that hold a rewritten row -- all that is laid out again when the state
// the statistics lead to is the one the fragment copy was built for.
int exf_table_stats(freddy_gpu_index* ix, int64_t r0, int64_t n, const std::vector<int32_t>* changed_strips) {
  const bool shape_ok = ix->d % 4 == 0 && ix->d <= 512 && ix->d >= 16;
  if (!shape_ok) { ix->exf_ok = false; return 0; }
  if (ix->tune.exact_filter == 0 || ix->exf_never) { ix->exf_never = true; ix->exf_ok = false; return 0; }   // (option exact_filter = 0 when the table is pinned: no third copy of it -- nor later, when remove_rows takes the statistics again from row 0)
  if (n <= 0) return 0;
  if (ix->exf_small.ensure(4096)) return fail(FREDDY_E_NOMEM, "device allocation failed");
  uint32_t* st = ix->exf_small.as<uint32_t>() + 512;   // (the upper part of the small buffer; the lower one is per-call state)
  HIP_TRY(hipMemsetAsync(st, 0, 16, ix->stream));
  const unsigned grid = table_stats_grid(ix->n_cus, n);
  hipLaunchKernelGGL(exf_table_stats_kernel, dim3(grid), dim3(256), 0, ix->stream, ix->coarse + (size_t)r0 * ix->d, n, ix->d, st);
  HIP_TRY(hipGetLastError());
  uint32_t h[4] = {0, 0, 0, 0};
  HIP_TRY(hipMemcpyAsync(h, st, 16, hipMemcpyDeviceToHost, ix->stream));
  HIP_TRY(hipStreamSynchronize(ix->stream));
  float amax, n2;
  memcpy(&amax, &h[0], 4); memcpy(&n2, &h[1], 4);
  const bool first = r0 == 0;
  const bool was_ok = ix->exf_ok;
  const int ex_before = ix->exf_ex;
  if (h[2] || !(n2 < 1e30f)) { ix->exf_ok = false; return 0; }
  float tiny_norm;   // rows whose sum of squares is below EXF_N2_FLOOR: their bound comes from their largest |element| (exact2.h)
  memcpy(&tiny_norm, &h[3], 4);
  const float xn = std::max(std::sqrt(n2) * (1.0f + 1e-5f), tiny_norm);
  int64_t relayout_from = r0;
  if (first) { ix->exf_ok = true; ix->exf_xnorm = xn; ix->exf_ex = exf_scale_exp(amax); }
  else if (ix->exf_ok) {
    ix->exf_xnorm = std::max(ix->exf_xnorm, xn);
    const int ex_new = std::min(ix->exf_ex, exf_scale_exp(amax));   // (a larger element: a smaller scale -> everything is laid out again)
    if (ex_new != ix->exf_ex) relayout_from = 0;
    ix->exf_ex = ex_new;
  } else return 0;
  // the fragment-order copy: rows [relayout_from, r0 + n) (whole strips; the strip the old last row sat in is rewritten)
  const int T = (ix->d + 15) / 16;
  const int64_t n_total = r0 + n, strips = (n_total + 31) / 32, strip0 = relayout_from / 32;
  const size_t need = (size_t)strips * T * 2 * 64 * 16;
  if (need > ix->exf_xf.cap) {
    DevBuf bigger;
    // (no room for the copy is the call's failure, as any other allocation's: a handle that silently kept the all-exact kernels
    // would differ from a fresh pin of its table.  The statistics above have moved already: a mutation that gets this answer
    // poisons the handle, a pin fails)
    if (bigger.ensure(need)) return fail(FREDDY_E_NOMEM, "device allocation of %zu bytes failed (the exact filter's copy of the rows)", need);
    if (ix->exf_xf.p && strip0 > 0) HIP_TRY(hipMemcpy(bigger.p, ix->exf_xf.p, (size_t)strip0 * T * 2 * 64 * 16, hipMemcpyDeviceToDevice));
    ix->bytes += (int64_t)bigger.cap - (int64_t)ix->exf_xf.cap;
    ix->exf_xf.release();
    ix->exf_xf = bigger;
  }
  // update_rows: the scale and the strip count are those of the copy that is there -> only the strips that hold a changed row
  // (exf_xf_strips already equals `strips` on this path, so it stays; a list that names a strip outside the copy is not used: every
  // strip is laid out below instead)
  bool listed = first && changed_strips && was_ok && ex_before == ix->exf_ex && ix->exf_xf_strips == strips && need <= ix->exf_xf.cap;
  if (listed)
    for (int32_t st : *changed_strips) listed = listed && st >= 0 && st < strips;
  if (listed) {
    if (changed_strips->empty()) return 0;
    DevBuf list;
    if (list.ensure(sizeof(int32_t) * changed_strips->size())) return fail(FREDDY_E_NOMEM, "device allocation failed");
    int rc = 0;
    if (hipMemcpyAsync(list.p, changed_strips->data(), sizeof(int32_t) * changed_strips->size(), hipMemcpyHostToDevice, ix->stream) != hipSuccess) rc = fail(FREDDY_E_HIP, "hipMemcpy failed");
    if (!rc) {
      const int64_t threads = (int64_t)changed_strips->size() * T * 64;
      hipLaunchKernelGGL(exf_layout_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, ix->stream, ix->coarse, n_total, ix->d, T, ix->exf_ex,
                         (int64_t)0, (int64_t)changed_strips->size(), list.as<int32_t>(), ix->exf_xf.as<h8v>());
      if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ix->stream) != hipSuccess) rc = fail(FREDDY_E_HIP, "laying out the changed strips failed");
    }
    list.release();
    return rc;
  }
  const int64_t threads = (strips - strip0) * T * 64;
  hipLaunchKernelGGL(exf_layout_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, ix->stream, ix->coarse, n_total, ix->d, T, ix->exf_ex,
                     strip0, strips - strip0, (const int32_t*)nullptr, ix->exf_xf.as<h8v>());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(ix->stream));
  ix->exf_xf_strips = strips;
  return 0;
}

// The filter + refine path for all rows of the table (exact_host.h: the chain).  *fell_back = 1: a candidate buffer overflowed or
// a query was not finite -- nothing was written, the caller runs the all-exact kernels.
// q_copy: NULL, or device memory for the queries when d_queries is mapped host memory (exf_prep_kernel copies them).
// h_out: mapped host memory [Q*k ids][Q*k similarities][2 verdict words], p_out the same block as the device sees it: the merge
// writes there, ONE synchronisation ends the call (four 12-us copies and a second synchronisation before).
static int exact_filter_search(freddy_gpu_index* ix, hipStream_t s, const float* d_queries, int Q, int k, int* fell_back, int32_t* h_out, int32_t* p_out,
                               float* q_copy) {
  *fell_back = 0;
  const int d = ix->d, T = (d + 15) / 16;
  const int64_t N = ix->N;
  const FilterPlan fp = filter_plan(N, (ix->tune.check_brackets & 4) != 0);
  const size_t tile_lds = (size_t)T * 2 * 64 * 16;
  if (ix->exf_qfrag.ensure(2 * tile_lds) || ix->exf_sample.ensure(sizeof(float) * (size_t)EXF_QT * fp.n_sample) ||
      ix->exf_cand.ensure(sizeof(uint2) * (size_t)EXF_QT * fp.cap))
    return fail(FREDDY_E_NOMEM, "workspace allocation failed");
  if (int rc = exf_begin(ix, s)) return rc;
  int32_t* const flags = h_out + 2 * (size_t)Q * k;
  flags[0] = flags[1] = -1;   // (before anything is enqueued: the call's last workgroup overwrites both)
  // small per-call state: [0..63] thr, [64..127] qeps, [128..191] qunscale, [192..255] cand_cnt, [256] qbad, [257] arrived
  float* sm = ix->exf_small.as<float>();
  ExfPass p;
  p.labels = &EXF_KNN_LABELS; p.fp = fp; p.thr = sm; p.qeps = sm + 64; p.qunscale = sm + 128; p.cand_cnt = reinterpret_cast<int32_t*>(sm + 192);
  p.flags = p_out + 2 * (size_t)Q * k; p.k = k; p.grid_q = EXF_QT; p.total_wgs = Q; p.sample_when_empty = true;
  ExfArgs fa;
  fa.xf = ix->exf_xf.as<h8v>(); fa.T = T; fa.qfrag = ix->exf_qfrag.as<h8v>(); fa.qunscale = p.qunscale; fa.thr = p.thr; fa.cand_cnt = p.cand_cnt;
  fa.cand = ix->exf_cand.as<uint2>(); fa.cap = fp.cap;
  for (int q0 = 0; q0 < Q; q0 += EXF_QT) {
    p.nq = std::min(EXF_QT, Q - q0);
    p.queries = d_queries + (size_t)q0 * d; p.copy_out = q_copy ? q_copy + (size_t)q0 * d : nullptr;
    p.out_ids = p_out + (size_t)q0 * k; p.out_sim = reinterpret_cast<float*>(p_out + (size_t)Q * k) + (size_t)q0 * k;
    if (int rc = exf_chain(ix, s, p, N, [&](auto sample, int64_t n_rows) {
      constexpr bool SAMPLE = decltype(sample)::value;
      filter_rows(fa, fp, SAMPLE, n_rows, ix->exf_sample.as<float>());
      const dim3 grid(filter_grid(ix, n_rows));
      if (p.nq <= 32) hipLaunchKernelGGL((exf_filter_kernel<1, SAMPLE>), grid, dim3(EXF_WG), tile_lds, s, fa);
      else hipLaunchKernelGGL((exf_filter_kernel<2, SAMPLE>), grid, dim3(EXF_WG), 2 * tile_lds, s, fa);
    })) return rc;
  }
  HIP_TRY(hipStreamSynchronize(s));
  if (int rc = exf_verdict_arrived(flags, "exact search")) return rc;
  exf_complete(ix);
  if (flags[0] || flags[1]) *fell_back = 1;
  return 0;
}

extern "C" int freddy_gpu_pin_vectors(const freddy_vec_desc* t, int device, freddy_gpu_index_t** out) {
  if (!t || !out || t->d <= 0 || t->N < 0 || (t->N && (!t->ids || !t->vectors))) return fail(FREDDY_E_ARG, "bad argument");
  if (t->N > (int64_t)INT32_MAX - 64) return fail(FREDDY_E_LIMIT, "N too large for 32-bit row positions");
  if (t->d > EX_MAX_D) return fail(FREDDY_E_LIMIT, "d=%d exceeds the exact search's limit of %d dimensions (a query tile must fit the LDS)", t->d, EX_MAX_D);
  for (int64_t r = 1; r < t->N; ++r)
    if (t->ids[r] <= t->ids[r - 1]) return fail(FREDDY_E_ARG, "ids must be strictly ascending (row %lld)", (long long)r);
  freddy_gpu_index* ix = new freddy_gpu_index();
  ix->kind = KIND_VEC;
  ix->d = t->d; ix->N = t->N;
  int rc = open_device(ix, device);
  if (!rc) {
    ix->n_blocks = (t->N + 63) / 64;
    const size_t xb_bytes = sizeof(float) * (size_t)std::max<int64_t>(ix->n_blocks, 1) * t->d * 64;
    if (dev_malloc((void**)&ix->xb, xb_bytes) != hipSuccess) rc = fail(FREDDY_E_NOMEM, "device allocation of %zu bytes failed", xb_bytes);
    else ix->bytes += (int64_t)xb_bytes;
    if (!rc && upload(&ix->ids, t->ids, (size_t)t->N, &ix->bytes)) rc = fail(FREDDY_E_NOMEM, "device allocation failed");
    // row-major rows go up in slices and are re-blocked on the device
    const int64_t slice = 1 << 16;
    DevBuf tmp;
    for (int64_t r0 = 0; !rc && r0 < t->N; r0 += slice) {
      const int64_t n = std::min(slice, t->N - r0);
      if (tmp.ensure(sizeof(float) * (size_t)n * t->d)) { rc = fail(FREDDY_E_NOMEM, "device allocation failed"); break; }
      if (hipMemcpy(tmp.p, t->vectors + (size_t)r0 * t->d, sizeof(float) * (size_t)n * t->d, hipMemcpyHostToDevice) != hipSuccess) {
        rc = fail(FREDDY_E_HIP, "hipMemcpy failed"); break;
      }
      hipLaunchKernelGGL(block_rows_kernel, dim3((unsigned)((n + 63) / 64)), dim3(256), 0, ix->stream, tmp.as<float>(), nullptr, n,
                         ix->xb + (size_t)(r0 / 64) * t->d * 64, nullptr, t->d);
      if (hipStreamSynchronize(ix->stream) != hipSuccess) { rc = fail(FREDDY_E_HIP, "re-blocking kernel failed"); break; }
    }
    tmp.release();
  }
  if (!rc) {
    ix->h_ids.assign(t->ids, t->ids + t->N);
    // the source rows are only needed again for "id = ANY(...)" subsets: keep them row-major too
    if (t->N && upload(&ix->coarse, t->vectors, (size_t)t->N * t->d, &ix->bytes)) rc = fail(FREDDY_E_NOMEM, "device allocation failed");
    if (!rc && t->N) rc = exf_table_stats(ix, 0, t->N);
  }
  if (rc) { free_index(ix); return rc; }
  *out = ix;
  return FREDDY_OK;
}

// ---- the rows of an id set (resolve.h) and the queries of a call, for either source ---------------------------------------------
// Where the table rows of "id = ANY(set)" are: the host vector rows_of_ids made (every function then does exactly what it did
// before), or already in ws->w_sub_rows, `resident` of them, put there by resolve_ids_device -- the copy to the device is skipped.
// The buffer was sized for min(n_ids, N) >= resident rows before the resolve was launched, and DevBuf::ensure leaves a buffer
// that is large enough where it is: the consumers' own ensure() calls for `resident` rows do not move it.
struct RowSet {
  const std::vector<int32_t>* host = nullptr;
  int64_t resident = 0;
  static RowSet of_host(const std::vector<int32_t>& rows) { RowSet r; r.host = &rows; return r; }
  static RowSet on_device(int64_t n) { RowSet r; r.resident = n; return r; }
  int64_t size() const { return host ? (int64_t)host->size() : resident; }
};

// ids[n] -> *n_rows ascending, distinct table rows in ws->w_sub_rows (resolve.h): a memset and four launches, recorded as
// resolve_mark / resolve_scan / resolve_place, ONE synchronisation (the host reads the count from mapped memory behind it) and no
// host work per id.  The other buffers (ids: w_item_cell, bitmap + chunk sums: w_used, counts: w_cnt, offsets: w_part) are free
// again when this returns.  n == 0 or an empty table: no rows, nothing launched.
static int resolve_ids_device(freddy_gpu_index* ix, Workspace* ws, hipStream_t s, const int32_t* ids, int64_t n, int64_t* n_rows) {
  *n_rows = 0;
  const int64_t N = ix->N;
  if (n <= 0 || N <= 0) return 0;
  const int B = ix->tune.resolve_block > 0 ? ix->tune.resolve_block : RESOLVE_BLOCK;
  const int64_t n_words = (N + 31) / 32, n_blocks = (n_words + B - 1) / B, chunks = (n_blocks + SIM_CHUNK - 1) / SIM_CHUNK;
  if (ws->w_sub_rows.ensure(sizeof(int32_t) * (size_t)std::min(n, N)) || ws->w_item_cell.ensure(sizeof(int32_t) * (size_t)n) ||
      ws->w_used.ensure(sizeof(uint32_t) * (size_t)(n_words + chunks)) || ws->w_cnt.ensure(sizeof(int32_t) * (size_t)n_blocks) ||
      ws->w_part.ensure(sizeof(int32_t) * (size_t)(n_blocks + 1)))
    return fail(FREDDY_E_NOMEM, "workspace allocation failed");
  if (ix->hio_in.ensure(sizeof(int32_t))) return fail(FREDDY_E_NOMEM, "pinned staging allocation failed");
  volatile int32_t* const h_total = ix->hio_in.as<int32_t>();
  *h_total = -1;
  uint32_t* const bitmap = ws->w_used.as<uint32_t>();
  int32_t* const part = reinterpret_cast<int32_t*>(bitmap + n_words);
  HIP_TRY(hipMemcpyAsync(ws->w_item_cell.p, ids, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, s));
  timed_launch(ix, s, "resolve_mark", [&] {
    (void)hipMemsetAsync(bitmap, 0, sizeof(uint32_t) * (size_t)(n_words + chunks), s);
    hipLaunchKernelGGL(resolve_mark_kernel, dim3(resolve_grid(ix->n_cus, (n + 255) / 256)), dim3(256), 0, s,
                       ws->w_item_cell.as<const int32_t>(), n, (const int32_t*)ix->ids, N, bitmap);
  });
  HIP_TRY(hipGetLastError());
  const dim3 bgrid(resolve_grid(ix->n_cus, (n_blocks + 3) / 4));   // (grid_plan.h: the kernels walk what a smaller grid leaves)
  timed_launch(ix, s, "resolve_scan", [&] {
    hipLaunchKernelGGL(resolve_count_kernel, bgrid, dim3(256), 0, s, (const uint32_t*)bitmap, n_words, B, n_blocks, ws->w_cnt.as<int32_t>(), part);
    hipLaunchKernelGGL(sim_scan_kernel, dim3((unsigned)chunks), dim3(256), 0, s, ws->w_cnt.as<const int32_t>(), (const int32_t*)part, n_blocks,
                       ws->w_part.as<int32_t>());
  });
  HIP_TRY(hipGetLastError());
  timed_launch(ix, s, "resolve_place", [&] {
    hipLaunchKernelGGL(resolve_place_kernel, bgrid, dim3(256), 0, s, (const uint32_t*)bitmap, n_words, B, n_blocks, ws->w_part.as<const int32_t>(),
                       ws->w_sub_rows.as<int32_t>(), ix->hio_in.as<int32_t>());
  });
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(s));
  const int64_t total = *h_total;
  if (total < 0 || total > std::min(n, N)) return fail(FREDDY_E_HIP, "the device resolve reported %lld rows of %lld ids", (long long)total, (long long)n);
  *n_rows = total;
  return 0;
}

// The queries of a call where the kernels read them: the caller's floats copied into ws->w_q, or rows of the table (query_ids.h) --
// one is read where it lies, more are gathered into ws->w_q by row numbers staged in the handle's pinned block (4 bytes per query).
// Enqueued only; w_q holds Q d floats already.
static int stage_queries(freddy_gpu_index* ix, Workspace* ws, hipStream_t s, const QuerySrc& qs, int Q, const float** d_q) {
  const int d = ix->d;
  *d_q = ws->w_q.as<float>();
  if (qs.host) {
    HIP_TRY(hipMemcpyAsync(ws->w_q.p, qs.host, sizeof(float) * (size_t)Q * d, hipMemcpyHostToDevice, s));
    return 0;
  }
  if (Q == 1) { *d_q = qs.row_ptr(0, d); return 0; }
  if (ix->hio_in.ensure(sizeof(int32_t) * (size_t)Q)) return fail(FREDDY_E_NOMEM, "pinned staging allocation failed");
  memcpy(ix->hio_in.p, qs.rows, sizeof(int32_t) * (size_t)Q);   // (every earlier reader of the block has been synchronised)
  return launch_query_gather(ix, s, qs, ix->hio_in.as<const int32_t>(), ws->w_q.as<float>(), Q, d);
}

// "id = ANY(subset)" on a vector handle: the subset's rows (rows_of_ids, or the device resolve's) re-blocked into w_resid, their
// positions in w_sub_pos, for the all-exact kernels.  An empty subset launches nothing (its buffers still exist).  Synchronises the stream.
static int vec_subset(freddy_gpu_index* ix, Workspace* ws, hipStream_t s, const RowSet& rows, const float** xb,
                      const int32_t** pos, int64_t* n_rows, int64_t* n_blocks) {
  *n_rows = rows.size();
  *n_blocks = (*n_rows + 63) / 64;
  if (ws->w_sub_rows.ensure(sizeof(int32_t) * (size_t)std::max<int64_t>(rows.size(), 1)) ||
      ws->w_sub_pos.ensure(sizeof(int32_t) * (size_t)std::max<int64_t>(*n_blocks, 1) * 64) ||
      ws->w_resid.ensure(sizeof(float) * (size_t)std::max<int64_t>(*n_blocks, 1) * ix->d * 64))
    return fail(FREDDY_E_NOMEM, "workspace allocation failed");
  if (*n_rows) {
    if (rows.host) HIP_TRY(hipMemcpyAsync(ws->w_sub_rows.p, rows.host->data(), sizeof(int32_t) * rows.host->size(), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(block_rows_kernel, dim3((unsigned)*n_blocks), dim3(256), 0, s, ix->coarse, ws->w_sub_rows.as<int32_t>(), *n_rows,
                       ws->w_resid.as<float>(), ws->w_sub_pos.as<int32_t>(), ix->d);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));   // `rows` is the caller's host memory
  }
  *xb = ws->w_resid.as<float>();
  *pos = ws->w_sub_pos.as<int32_t>();
  return 0;
}

// Exact kNN of checked arguments (Q > 0) over all rows (sub_rows == NULL) or over the table rows *sub_rows (rows_of_ids' result;
// the exact join hands over the rows it has resolved).
static int exact_search_rows(freddy_gpu_index* ix, const QuerySrc& queries, int32_t Q, int32_t k, const RowSet* sub_rows,
                             int32_t* out_ids, float* out_sim) {
  HIP_TRY(hipSetDevice(ix->device));
  Workspace* ws = workspace_for(ix, ix->stream);
  hipStream_t s = ix->stream;
  const int d = ix->d, L = std::min(k, 1024), V = pick_V(L);   // (k > 1024: passes of 1024 keys, below)
  const float* xb = ix->xb;
  const int32_t* pos = nullptr;
  int64_t n_rows = ix->N, n_blocks = ix->n_blocks;
  if (sub_rows)   // (an empty subset: the scan below finds nothing)
    if (int rc = vec_subset(ix, ws, s, *sub_rows, &xb, &pos, &n_rows, &n_blocks)) return rc;
  // Filter + refine (exact2.h): the whole table, k <= 32, finite rows of a supported shape; identical lists.
  const bool want_filter = !sub_rows && ix->exf_ok && k <= 32 && ix->tune.exact_filter != 0 &&
                           (ix->tune.exact_filter == 1 || n_rows >= 8192) && n_rows >= 1;
  if (want_filter) {
    // one block of mapped host memory: [lists][verdict words][the queries, when they are few]: the kernels read a handful of
    // queries where the host put them (1.2 KB each over PCIe) and write the lists where the host reads them
    const size_t n_out = (size_t)Q * k, q_bytes = sizeof(float) * (size_t)Q * d;
    const bool q_pinned = queries.host && q_bytes <= (256u << 10);   // (queries that are rows of the table are on the device already)
    const size_t out_bytes = (n_out * 8 + 8 + 255) & ~(size_t)255, need = out_bytes + (q_pinned ? q_bytes : 0);
    if (ix->hio_out.ensure(need)) return fail(FREDDY_E_NOMEM, "pinned staging allocation failed");
    void* dp = nullptr;
    HIP_TRY(hipHostGetDevicePointer(&dp, ix->hio_out.p, 0));
    int32_t* const h_out = ix->hio_out.as<int32_t>();
    const float* d_q = nullptr;
    if (ws->w_q.ensure(q_bytes)) return fail(FREDDY_E_NOMEM, "workspace allocation failed");
    if (q_pinned) {
      memcpy(ix->hio_out.as<char>() + out_bytes, queries.host, q_bytes);
      d_q = reinterpret_cast<const float*>(static_cast<char*>(dp) + out_bytes);
    } else if (int rc = stage_queries(ix, ws, s, queries, Q, &d_q)) return rc;
    int fell_back = 0;
    if (int rc = exact_filter_search(ix, s, d_q, Q, k, &fell_back, h_out, static_cast<int32_t*>(dp), q_pinned ? ws->w_q.as<float>() : nullptr)) return rc;
    if (!fell_back) {
      memcpy(out_ids, h_out, n_out * 4);
      memcpy(out_sim, h_out + n_out, n_out * 4);
      return FREDDY_OK;
    }
  }
  int EX_QT = ex_qt(V, Q);
  if (EX_QT == 16 && exact_scan_lds(d, 16) > EX_MAX_LDS) EX_QT = 8;   // (d > 2048: sixteen queries do not fit the LDS; d <= EX_MAX_D: eight do)
  const int qgroups = (Q + EX_QT - 1) / EX_QT;
  int chunk_blocks;
  const int nchunk = scan_chunks(n_blocks, qgroups, &chunk_blocks);
  if (ws->w_q.ensure(sizeof(float) * (size_t)Q * d) || ws->w_out_ids.ensure(sizeof(int32_t) * (size_t)Q * k) ||
      ws->w_out_dist.ensure(sizeof(float) * (size_t)Q * k) ||
      ws->w_part.ensure(sizeof(u64) * (size_t)Q * nchunk * EX_WAVES * L))
    return fail(FREDDY_E_NOMEM, "workspace allocation failed");
  const float* d_q = nullptr;
  if (int rc = stage_queries(ix, ws, s, queries, Q, &d_q)) return rc;
  ExactArgs ea;
  ea.xb = xb; ea.pos = pos; ea.queries = d_q; ea.part = ws->w_part.as<u64>();
  ea.n_rows = n_rows; ea.n_blocks = (int)n_blocks; ea.chunk_blocks = chunk_blocks; ea.nchunk = nchunk; ea.Q = Q; ea.d = d; ea.L = L; ea.floor = nullptr;
  const size_t lds = exact_scan_lds(d, EX_QT);
  dim3 grid((unsigned)nchunk, (unsigned)qgroups);
  const int ppq = nchunk * EX_WAVES;
  if (k > 1024) {
    // lists of 1025 .. 4096 entries: 1024 keys per pass over the same rows, each pass above the last key of the one before
    if (ws->w_floor.ensure(sizeof(u64) * (size_t)Q)) return fail(FREDDY_E_NOMEM, "workspace allocation failed");
    for (int p0 = 0; p0 < k; p0 += 1024) {
      const int Lp = std::min(1024, k - p0);
      ea.L = Lp; ea.floor = p0 ? ws->w_floor.as<u64>() : nullptr;
      timed_launch(ix, s, "exact_scan", [&] {
        if (p0) hipLaunchKernelGGL((exact_scan_kernel<16, 8, true>), grid, dim3(EX_WG), lds, s, ea);
        else hipLaunchKernelGGL((exact_scan_kernel<16, 8>), grid, dim3(EX_WG), lds, s, ea);
      });
      HIP_TRY(hipGetLastError());
      timed_launch(ix, s, "exact_merge", [&] {
        hipLaunchKernelGGL((exact_merge_kernel<16>), dim3(Q), dim3(4 * 64), (size_t)4 * 64 * (16 + 1) * sizeof(u64), s, ea.part, ppq, Lp, k, ix->ids,
                           ws->w_out_ids.as<int32_t>(), ws->w_out_dist.as<float>(), p0, Lp, ws->w_floor.as<u64>());
      });
      HIP_TRY(hipGetLastError());
    }
  } else {
    timed_launch(ix, s, "exact_scan", [&] {
      with_V(V, [&](auto v) {   // (query tiles of 16 only for V <= 4: ex_qt)
        constexpr int VV = decltype(v)::value;
        if constexpr (VV <= 4) {
          if (EX_QT == 16) { hipLaunchKernelGGL((exact_scan_kernel<VV, 16>), grid, dim3(EX_WG), lds, s, ea); return; }
        }
        hipLaunchKernelGGL((exact_scan_kernel<VV, 8>), grid, dim3(EX_WG), lds, s, ea);
      });
    });
    HIP_TRY(hipGetLastError());
    timed_launch(ix, s, "exact_merge", [&] {
      with_V(V, [&](auto v) {   // (16 waves per query up to V = 4, then 64 / V)
        constexpr int VV = decltype(v)::value, NW = VV <= 4 ? 16 : 64 / VV;
        hipLaunchKernelGGL((exact_merge_kernel<VV>), dim3(Q), dim3(NW * 64), (size_t)NW * 64 * (VV + 1) * sizeof(u64), s, ea.part, ppq, L, k, ix->ids,
                           ws->w_out_ids.as<int32_t>(), ws->w_out_dist.as<float>());
      });
    });
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipMemcpyAsync(out_ids, ws->w_out_ids.p, sizeof(int32_t) * (size_t)Q * k, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(out_sim, ws->w_out_dist.p, sizeof(float) * (size_t)Q * k, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return FREDDY_OK;
}

// The id set of a call as a RowSet: on the device (resolve.h) into the workspace of the handle's stream, or on the host into *h_rows.
static int resolve_row_set(freddy_gpu_index* ix, bool on_device, const int32_t* ids, int64_t n, std::vector<int32_t>* h_rows, RowSet* out) {
  if (!on_device) {
    *h_rows = rows_of_ids(ix->h_ids, ids, n);
    *out = RowSet::of_host(*h_rows);
    return 0;
  }
  HIP_TRY(hipSetDevice(ix->device));
  int64_t n_rows = 0;
  if (int rc = resolve_ids_device(ix, workspace_for(ix, ix->stream), ix->stream, ids, n, &n_rows)) return rc;
  *out = RowSet::on_device(n_rows);
  return 0;
}

// freddy_gpu_exact_search of checked arguments (Q > 0) for either source of the queries
static int exact_search_src(freddy_gpu_index* ix, const QuerySrc& queries, int32_t Q, int32_t k, const int32_t* subset_ids, int64_t n_subset,
                            bool resolve_on_device, int32_t* out_ids, float* out_sim) {
  if (!subset_ids) return exact_search_rows(ix, queries, Q, k, nullptr, out_ids, out_sim);
  std::vector<int32_t> h_rows;
  RowSet rows;
  if (int rc = resolve_row_set(ix, resolve_on_device, subset_ids, n_subset, &h_rows, &rows)) return rc;
  return exact_search_rows(ix, queries, Q, k, &rows, out_ids, out_sim);
}

extern "C" int freddy_gpu_exact_search(freddy_gpu_index_t* ix, const float* queries, int32_t Q, int32_t k,
                                       const int32_t* subset_ids, int64_t n_subset, int32_t* out_ids, float* out_sim) {
  if (!ix) return fail(FREDDY_E_ARG, "NULL index");
  if (ix->kind != KIND_VEC) return fail(FREDDY_E_KIND, "index handle has the wrong kind for this call");
  if (int rc = refuse_poisoned(ix)) return rc;
  if (Q < 0 || k <= 0 || n_subset < 0 || (n_subset > 0 && !subset_ids)) return fail(FREDDY_E_ARG, "bad sizes");
  if (Q > 0 && (!queries || !out_ids || !out_sim)) return fail(FREDDY_E_ARG, "NULL buffer");
  if (k > 4096) return fail(FREDDY_E_LIMIT, "k=%d exceeds this build's limit of 4096", k);
  if (Q == 0) return FREDDY_OK;
  return exact_search_src(ix, QuerySrc::of_host(queries), Q, k, subset_ids, n_subset, ix->tune.exact_resolve != 0, out_ids, out_sim);
}

// Exact kNN of rows named by id (query_ids.h) over the whole table (subset_ids == NULL) or over an id set, which is resolved on the device.
extern "C" int freddy_gpu_exact_search_ids(freddy_gpu_index_t* vecs, const int32_t* query_ids, int32_t n_ids, int32_t id_rule, int32_t k,
                                           const int32_t* subset_ids, int64_t n_subset, int32_t* out_query_ids, int32_t* n_queries,
                                           int32_t* out_ids, float* out_sim) {
  if (int rc = check_query_ids_front(vecs, vecs, query_ids, n_ids, id_rule, out_query_ids, n_queries, out_ids, out_sim)) return rc;
  if (k <= 0 || n_subset < 0 || (n_subset > 0 && !subset_ids)) return fail(FREDDY_E_ARG, "bad sizes");
  if (k > 4096) return fail(FREDDY_E_LIMIT, "k=%d exceeds this build's limit of 4096", k);
  if (vecs->kind != KIND_VEC) return fail(FREDDY_E_KIND, "index handle has the wrong kind for this call");
  if (int rc = refuse_poisoned(vecs)) return rc;
  return search_selected_ids(vecs, query_ids, n_ids, id_rule, k, -HUGE_VALF, out_query_ids, n_queries, out_ids, out_sim,
                             [&](const QuerySrc& qs, int n, int32_t* oi, float* os) {
    return exact_search_src(vecs, qs, n, k, subset_ids, n_subset, true, oi, os);
  });
}

// ---- the exact kNN-join (exact_join.h) ---------------------------------------------------------------------------------
// Target sets below this many rows take the all-exact subset path unless option exact_filter = 1 forces the filter: the smallest
// set size of tools/exact_join_timing.py's sweep (profiles/exact_join_timing.txt: n_targets x Q, filter forced, against the parent
// commit's subset path) at which filter + refine is not slower at any Q -- at 1 000 and 4 000 targets it loses at Q >= 1024.
static constexpr int64_t EXJ_MIN_TARGETS = 8000;

// Device memory the per-query buffers of one pass may take (the threshold sample and the candidate buffers): more queries than
// fit are answered in passes over the same gathered copy (10 880 queries per pass for sets of 32 768 rows or more).
// A pass is never smaller than 128 queries: under check_brackets bit 2 (tests), where a candidate buffer holds the whole set, a
// pass over a large set takes 128 n_targets 8 bytes however that compares with this budget.
static constexpr size_t EXJ_PASS_BYTES = (size_t)2 << 30;

// Filter + refine over the target rows `rows` (table order, distinct) for all Q queries: one gather, then five launches per pass
// of queries.  cnt_out[q] = candidates the filter found for query q (> cap: its list is not valid, the caller redoes it);
// *qbad_out: a query was not finite (no list is valid, the passes stop).
static int exact_join_filter(freddy_gpu_index* ix, Workspace* ws, hipStream_t s, const RowSet& rows, const QuerySrc& queries, int Q, int k,
                             int32_t* out_ids, float* out_sim, std::vector<int32_t>& cnt_out, int* cap_out, bool* qbad_out) {
  const int d = ix->d, T = (d + 15) / 16;
  const int64_t nT = rows.size(), strips = (nT + 31) / 32;
  const FilterPlan fp = filter_plan(nT, (ix->tune.check_brackets & 4) != 0);
  const int n_sample = fp.n_sample, cap = fp.cap;
  *cap_out = cap; *qbad_out = false;
  // the query tile: 128 queries (NT = 4) when more than one 64-tile is needed and four tiles' fragments fit the LDS
  int NT = Q <= 32 ? 1 : 2;
  const size_t tile_lds = (size_t)T * 2 * 64 * 16;
  if (Q > 64 && 4 * tile_lds <= AN_MAX_LDS && ix->tune.exact_join_tile != 64) NT = 4;
  const int QT = 32 * NT;
  const size_t per_query = sizeof(float) * (size_t)std::max(n_sample, 1) + sizeof(uint2) * (size_t)cap;
  const int Qc = (int)std::min<int64_t>(Q, std::max<int64_t>(128, (int64_t)(EXJ_PASS_BYTES / per_query) / 128 * 128));   // queries per pass
  const int QcPad = (Qc + QT - 1) / QT * QT;
  // per-pass state in w_found: [QcPad] thr, qeps, qunscale, cand_cnt, then the refine kernel's two verdict words
  if (ws->w_found.ensure(sizeof(float) * (4 * (size_t)QcPad + 2)) || ws->w_sub_rows.ensure(sizeof(int32_t) * (size_t)nT) ||
      ws->w_resid.ensure((size_t)strips * T * 2 * 64 * 16) || ix->exf_qfrag.ensure((size_t)(QcPad / 32) * tile_lds) || ws->w_q.ensure(sizeof(float) * (size_t)Q * d) ||
      ix->exf_sample.ensure(sizeof(float) * (size_t)QcPad * std::max(n_sample, 1)) || ix->exf_cand.ensure(sizeof(uint2) * (size_t)Qc * cap) ||
      ws->w_out_ids.ensure(sizeof(int32_t) * (size_t)Qc * k) || ws->w_out_dist.ensure(sizeof(float) * (size_t)Qc * k))
    return fail(FREDDY_E_NOMEM, "workspace allocation failed");
  if (int rc = exf_begin(ix, s)) return rc;
  ExfPass p;
  p.labels = &EXF_JOIN_LABELS; p.fp = fp; p.thr = ws->w_found.as<float>(); p.qeps = p.thr + QcPad; p.qunscale = p.qeps + QcPad;
  p.cand_cnt = reinterpret_cast<int32_t*>(p.qunscale + QcPad); p.flags = p.cand_cnt + QcPad;
  p.copy_out = nullptr; p.k = k; p.out_ids = ws->w_out_ids.as<int32_t>(); p.out_sim = ws->w_out_dist.as<float>(); p.sample_when_empty = false;
  const int32_t* map = ws->w_sub_rows.as<int32_t>();
  h8v* xf = ws->w_resid.as<h8v>();
  if (rows.host) HIP_TRY(hipMemcpyAsync(ws->w_sub_rows.p, rows.host->data(), sizeof(int32_t) * (size_t)nT, hipMemcpyHostToDevice, s));
  const float* d_q = nullptr;
  if (int rc = stage_queries(ix, ws, s, queries, Q, &d_q)) return rc;
  const int64_t gthreads = strips * T * 64;
  timed_launch(ix, s, "exact_join_gather", [&] {
    hipLaunchKernelGGL(exj_gather_kernel, dim3((unsigned)((gthreads + 255) / 256)), dim3(256), 0, s, ix->coarse, map, nT, d, T, ix->exf_ex, xf);
  });
  HIP_TRY(hipGetLastError());
  cnt_out.assign((size_t)Q, 0);
  ExjArgs fa;
  fa.xf = xf; fa.map = map; fa.T = T; fa.qfrag = ix->exf_qfrag.as<h8v>(); fa.qunscale = p.qunscale; fa.thr = p.thr; fa.cand_cnt = p.cand_cnt;
  fa.cand = ix->exf_cand.as<uint2>(); fa.cap = cap;
  for (int q0 = 0; q0 < Q; q0 += Qc) {
    const int nq = std::min(Qc, Q - q0), qtiles = (nq + QT - 1) / QT;
    p.nq = fa.nq = nq; p.grid_q = (unsigned)(qtiles * QT); p.total_wgs = nq; p.queries = d_q + (size_t)q0 * d;
    HIP_TRY(hipMemsetAsync(p.flags, 0xFF, 8, s));   // (-1, -1: the pass's last refine workgroup overwrites both)
    // strip chunks: a workgroup's 8 waves take 8 strips per step; with many query tiles every workgroup stays long enough (>= 64
    // strips) to pay for its LDS image of the tile
    if (int rc = exf_chain(ix, s, p, nT, [&](auto sample, int64_t n_rows) {
      constexpr bool SAMPLE = decltype(sample)::value;
      filter_rows(fa, fp, SAMPLE, n_rows, ix->exf_sample.as<float>());
      const int64_t gx = exact_join_gx(ix->n_cus, n_rows, qtiles);
      const dim3 grid((unsigned)gx, (unsigned)qtiles);
      switch (NT) {
        case 1: hipLaunchKernelGGL((exj_filter_kernel<1, SAMPLE>), grid, dim3(EXF_WG), tile_lds, s, fa); break;
        case 2: hipLaunchKernelGGL((exj_filter_kernel<2, SAMPLE>), grid, dim3(EXF_WG), 2 * tile_lds, s, fa); break;
        default: hipLaunchKernelGGL((exj_filter_kernel<4, SAMPLE>), grid, dim3(EXF_WG), 4 * tile_lds, s, fa); break;
      }
    })) return rc;
    int32_t h_flags[2] = {-1, -1};
    const size_t n_out = (size_t)nq * k;
    HIP_TRY(hipMemcpyAsync(h_flags, p.flags, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(cnt_out.data() + q0, p.cand_cnt, sizeof(int32_t) * (size_t)nq, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(out_ids + (size_t)q0 * k, ws->w_out_ids.p, sizeof(int32_t) * n_out, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(out_sim + (size_t)q0 * k, ws->w_out_dist.p, sizeof(float) * n_out, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (int rc = exf_verdict_arrived(h_flags, "exact join")) return rc;
    if (h_flags[1]) { *qbad_out = true; break; }   // (the refine kernel has cleared its device-side words)
  }
  exf_complete(ix);
  return 0;
}

// freddy_gpu_exact_join of checked arguments (Q > 0, the stats cleared) for either source of the queries and either place of the resolve
static int exact_join_src(freddy_gpu_index* ix, const QuerySrc& queries, int32_t Q, int32_t k, const int32_t* target_ids, int64_t n_targets,
                          bool resolve_on_device, int32_t* out_ids, float* out_sim) {
  // the target ids resolved once: the filter and every all-exact answer (fall-back, redo) share the rows -- a resident set stays in
  // w_sub_rows through all of them (nothing below writes that buffer but the copy of a host set), while w_q is written again by
  // every stage: the redo and the fall-back take their queries from the source again, never from the filter's copy
  std::vector<int32_t> h_rows;
  RowSet rows;
  if (int rc = resolve_row_set(ix, resolve_on_device, target_ids, n_targets, &h_rows, &rows)) return rc;
  const int64_t nT = rows.size();
  const bool want_filter = ix->exf_ok && k <= 32 && ix->tune.exact_filter != 0 && (ix->tune.exact_filter == 1 || nT >= EXJ_MIN_TARGETS) && nT >= 1;
  if (!want_filter) return exact_search_rows(ix, queries, Q, k, &rows, out_ids, out_sim);
  HIP_TRY(hipSetDevice(ix->device));
  Workspace* ws = workspace_for(ix, ix->stream);
  std::vector<int32_t> cnt;
  int cap = 0;
  bool qbad = false;
  if (int rc = exact_join_filter(ix, ws, ix->stream, rows, queries, Q, k, out_ids, out_sim, cnt, &cap, &qbad)) return rc;
  // a query is not finite: every list all-exact.  (Found by the prep kernel, which reads every query anyway; a host-side scan
  // would put Q d comparisons in front of every call for the sake of this one.)
  if (qbad) return exact_search_rows(ix, queries, Q, k, &rows, out_ids, out_sim);
  // the queries whose candidate buffer overflowed: answered again, all-exact, in one call
  std::vector<int32_t> redo;
  int64_t cands = 0;
  for (int q = 0; q < Q; ++q) {
    if (cnt[(size_t)q] > cap) redo.push_back(q);
    else cands += cnt[(size_t)q];
  }
  ix->exj_stats[0] = Q; ix->exj_stats[1] = cands; ix->exj_stats[2] = (int64_t)redo.size();
  if (!redo.empty()) {
    const int d = ix->d, nr = (int)redo.size();
    std::vector<float> rq, rs((size_t)nr * k);
    std::vector<int32_t> ri((size_t)nr * k), rrows;
    QuerySrc rsrc = queries;
    if (queries.host) {
      rq.resize((size_t)nr * d);
      for (int i = 0; i < nr; ++i) memcpy(&rq[(size_t)i * d], queries.host + (size_t)redo[(size_t)i] * d, sizeof(float) * d);
      rsrc.host = rq.data();
    } else {   // (their row numbers: the rows are gathered again from the table)
      rrows.resize((size_t)nr);
      for (int i = 0; i < nr; ++i) rrows[(size_t)i] = queries.rows[redo[(size_t)i]];
      rsrc.rows = rrows.data();
    }
    if (int rc = exact_search_rows(ix, rsrc, nr, k, &rows, ri.data(), rs.data())) return rc;
    for (int i = 0; i < nr; ++i) {
      memcpy(out_ids + (size_t)redo[(size_t)i] * k, &ri[(size_t)i * k], sizeof(int32_t) * k);
      memcpy(out_sim + (size_t)redo[(size_t)i] * k, &rs[(size_t)i * k], sizeof(float) * k);
    }
  }
  return FREDDY_OK;
}

extern "C" int freddy_gpu_exact_join(freddy_gpu_index_t* ix, const float* queries, int32_t Q, int32_t k, const int32_t* target_ids,
                                     int64_t n_targets, int32_t* out_ids, float* out_sim) {
  // (the scalar arguments first: they are checked before the handle is looked at, so no device is needed to see these errors)
  if (Q < 0 || k <= 0 || n_targets < 0) return fail(FREDDY_E_ARG, "bad sizes (Q=%d, k=%d, n_targets=%lld)", Q, k, (long long)n_targets);
  if (n_targets > 0 && !target_ids) return fail(FREDDY_E_ARG, "NULL target_ids with n_targets=%lld", (long long)n_targets);
  if (Q > 0 && (!queries || !out_ids || !out_sim)) return fail(FREDDY_E_ARG, "NULL buffer");
  if (k > 4096) return fail(FREDDY_E_LIMIT, "k=%d exceeds this build's limit of 4096", k);
  if (!ix) return fail(FREDDY_E_ARG, "NULL index");
  if (ix->kind != KIND_VEC) return fail(FREDDY_E_KIND, "index handle has the wrong kind for this call");
  if (int rc = refuse_poisoned(ix)) return rc;
  ix->exj_stats[0] = ix->exj_stats[1] = ix->exj_stats[2] = 0;
  if (Q == 0) return FREDDY_OK;
  return exact_join_src(ix, QuerySrc::of_host(queries), Q, k, target_ids, n_targets, ix->tune.exact_resolve != 0, out_ids, out_sim);
}

// The exact kNN-join of rows named by id (query_ids.h): the queries are gathered from the table, the target set is resolved on the
// device (resolve.h); no vector and no row number of the set crosses PCIe.
extern "C" int freddy_gpu_exact_join_ids(freddy_gpu_index_t* vecs, const int32_t* query_ids, int32_t n_ids, int32_t id_rule, int32_t k,
                                         const int32_t* target_ids, int64_t n_targets, int32_t* out_query_ids, int32_t* n_queries,
                                         int32_t* out_ids, float* out_sim) {
  if (int rc = check_query_ids_front(vecs, vecs, query_ids, n_ids, id_rule, out_query_ids, n_queries, out_ids, out_sim)) return rc;
  if (k <= 0 || n_targets < 0) return fail(FREDDY_E_ARG, "bad sizes (Q=%d, k=%d, n_targets=%lld)", n_ids, k, (long long)n_targets);
  if (n_targets > 0 && !target_ids) return fail(FREDDY_E_ARG, "NULL target_ids with n_targets=%lld", (long long)n_targets);
  if (k > 4096) return fail(FREDDY_E_LIMIT, "k=%d exceeds this build's limit of 4096", k);
  if (vecs->kind != KIND_VEC) return fail(FREDDY_E_KIND, "index handle has the wrong kind for this call");
  if (int rc = refuse_poisoned(vecs)) return rc;
  vecs->exj_stats[0] = vecs->exj_stats[1] = vecs->exj_stats[2] = 0;
  return search_selected_ids(vecs, query_ids, n_ids, id_rule, k, -HUGE_VALF, out_query_ids, n_queries, out_ids, out_sim,
                             [&](const QuerySrc& qs, int n, int32_t* oi, float* os) {
    return exact_join_src(vecs, qs, n, k, target_ids, n_targets, true, oi, os);
  });
}

// Test hook: the device resolve alone -- the rows of ids[n] in table order, distinct (what rows_of_ids gives), copied back.
extern "C" int freddy_gpu_debug_resolve_ids(freddy_gpu_index_t* vecs, const int32_t* ids, int64_t n, int32_t* out_rows, int64_t* n_rows) {
  if (!vecs) return fail(FREDDY_E_ARG, "NULL index");
  if (n < 0 || !n_rows || (n > 0 && (!ids || !out_rows))) return fail(FREDDY_E_ARG, "bad argument (n=%lld)", (long long)n);
  if (vecs->kind != KIND_VEC) return fail(FREDDY_E_KIND, "index handle has the wrong kind for this call");
  if (int rc = refuse_poisoned(vecs)) return rc;
  *n_rows = 0;
  HIP_TRY(hipSetDevice(vecs->device));
  Workspace* ws = workspace_for(vecs, vecs->stream);
  int64_t nT = 0;
  if (int rc = resolve_ids_device(vecs, ws, vecs->stream, ids, n, &nT)) return rc;
  if (nT) {
    HIP_TRY(hipMemcpyAsync(out_rows, ws->w_sub_rows.p, sizeof(int32_t) * (size_t)nT, hipMemcpyDeviceToHost, vecs->stream));
    HIP_TRY(hipStreamSynchronize(vecs->stream));
  }
  *n_rows = nT;
  return FREDDY_OK;
}

extern "C" int freddy_gpu_last_exact_join_stats(const freddy_gpu_index_t* ix, int64_t* filter_queries, int64_t* candidates, int64_t* redone_queries) {
  if (!ix) return fail(FREDDY_E_ARG, "NULL index");
  if (ix->kind != KIND_VEC) return fail(FREDDY_E_KIND, "index handle has the wrong kind for this call");
  if (filter_queries) *filter_queries = ix->exj_stats[0];
  if (candidates) *candidates = ix->exj_stats[1];
  if (redone_queries) *redone_queries = ix->exj_stats[2];
  return FREDDY_OK;
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
  if (!ix) return fail(FREDDY_E_ARG, "NULL index");
  if (ix->kind != KIND_VEC) return fail(FREDDY_E_KIND, "index handle has the wrong kind for this call");
  if (int rc = refuse_poisoned(ix)) return rc;
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
  const bool want_filter = !pair && !subset_ids && ix->exf_ok && ix->tune.exact_filter != 0 && (ix->tune.exact_filter == 1 || n_rows >= 8192) &&
                           an_filter_lds(M, d) <= AN_MAX_LDS;
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

// ---- post verification of pq / ivf result lists (pv.h) -------------------------------------------------------------------
// The handles of a call that takes a pq / ivf handle and the raw-vector handle it re-ranks against (post verification, approximate
// analogies): check_ann_vecs (query_ids.h, which the searches by id share); nothing there touches a device.
static int pv_check_handles(const freddy_gpu_index* ann, int kind, const freddy_gpu_index* vecs, const char* what) { return check_ann_vecs(ann, kind, vecs, what); }

// The scalar refusals of post verification, each with its one message (the host-vector entry points and the ones by row id)
static int pv_check_count(int32_t Q, int32_t k, int32_t pvf) { return (Q < 0 || k < 1 || pvf < 1) ? fail(FREDDY_E_ARG, "bad sizes (Q=%d, k=%d, pvf=%d)", Q, k, pvf) : 0; }
static int pv_check_limit(int32_t k, int32_t pvf) {
  return (int64_t)k * pvf > PV_MAX_CAND ? fail(FREDDY_E_LIMIT, "k * pvf = %lld exceeds this build's limit of %d candidates", (long long)k * pvf, PV_MAX_CAND) : 0;
}
static int pv_check_subset(const int32_t* subset_ids, int64_t n_subset) {
  return (n_subset < 0 || (n_subset > 0 && !subset_ids)) ? fail(FREDDY_E_ARG, "bad subset (n_subset=%lld)", (long long)n_subset) : 0;
}
// Everything both entry points refuse, in the order of the header's table; nothing here touches a device.
static int pv_check(const freddy_gpu_index* ann, int kind, const freddy_gpu_index* vecs, const float* queries, int32_t Q, int32_t k, int32_t pvf,
                    const int32_t* out_ids, const float* out_sim) {
  if (int rc = pv_check_count(Q, k, pvf)) return rc;
  if (Q > 0 && (!queries || !out_ids || !out_sim)) return fail(FREDDY_E_ARG, "NULL buffer");
  if (int rc = pv_check_limit(k, pvf)) return rc;
  return pv_check_handles(ann, kind, vecs, "post verification");
}

// Stage one (`search`: the public entry point at k * pvf, writing its lists into the pinned block) and stage two (pv_rerank) for
// passes of queries that bound the pinned block; the kernel reads the lists where stage one left them and writes the result lists
// and the counts beside them, one synchronisation per pass.
template <class F>
static int pv_search(freddy_gpu_index* ann, freddy_gpu_index* vecs, const QuerySrc& queries, int32_t Q, int32_t k, int32_t pvf, int32_t* out_ids,
                     float* out_sim, F&& search) {
  ann->pv_stats[0] = ann->pv_stats[1] = 0;
  if (Q == 0) return FREDDY_OK;
  const int kc = k * pvf, d = ann->d;
  const int Qc = rerank_pass(Q, kc);
  HIP_TRY(hipSetDevice(ann->device));
  RerankBlock b;
  if (int rc = rerank_block(ann, Qc, kc, k, false, "post verification", &b)) return rc;
  hipStream_t s = ann->stream;
  for (int q0 = 0; q0 < Q; q0 += Qc) {
    const int nq = std::min(Qc, Q - q0);
    const QuerySrc qp = queries.from((size_t)q0, d);
    if (int rc = search(qp, nq, kc, b.l_ids, b.l_dist)) return rc;
    HIP_TRY(hipSetDevice(ann->device));
    if (qp.host) {
      HIP_TRY(hipMemcpyAsync(ann->pv_q.p, qp.host, sizeof(float) * (size_t)nq * d, hipMemcpyHostToDevice, s));
    } else {
      // queries by row id (query_ids.h): the raw queries are rows of `vecs` -- gathered, by row numbers staged in the handle's pinned
      // block (stage one has returned: the block is free)
      if (ann->hio_in.ensure(sizeof(int32_t) * (size_t)nq)) return fail(FREDDY_E_NOMEM, "pinned staging allocation failed");
      memcpy(ann->hio_in.p, qp.rows, sizeof(int32_t) * (size_t)nq);
      if (int rc = launch_query_gather(ann, s, qp, ann->hio_in.as<const int32_t>(), ann->pv_q.as<float>(), nq, d)) return rc;
    }
    if (int rc = launch_rerank(ann, vecs, s, "pv_rerank", pv_rerank_kernel<1>, pv_rerank_kernel<4>, b, nullptr, nq, kc, k)) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    memcpy(out_ids + (size_t)q0 * k, b.o_ids, sizeof(int32_t) * (size_t)nq * k);
    memcpy(out_sim + (size_t)q0 * k, b.o_sim, sizeof(float) * (size_t)nq * k);
    for (int q = 0; q < nq; ++q) { ann->pv_stats[0] += b.o_cnt[2 * q]; ann->pv_stats[1] += b.o_cnt[2 * q + 1]; }
  }
  return FREDDY_OK;
}

extern "C" int freddy_gpu_ivfadc_search_pv(freddy_gpu_index_t* ivf, freddy_gpu_index_t* vecs, const float* queries, int32_t Q, int32_t k, int32_t pvf,
                                           int32_t W, float sentinel, int32_t found_rule, int32_t* out_ids, float* out_sim) {
  if (int rc = pv_check(ivf, KIND_IVF, vecs, queries, Q, k, pvf, out_ids, out_sim)) return rc;
  if (int rc = check_probe_args(W, found_rule)) return rc;
  return pv_search(ivf, vecs, QuerySrc::of_host(queries), Q, k, pvf, out_ids, out_sim, [&](const QuerySrc& qp, int nq, int kc, int32_t* l_ids, float* l_dist) {
    return freddy_gpu_ivfadc_search(ivf, qp.host, nq, kc, W, sentinel, found_rule, l_ids, l_dist);
  });
}

extern "C" int freddy_gpu_pq_search_pv(freddy_gpu_index_t* pq, freddy_gpu_index_t* vecs, const float* queries, int32_t Q, int32_t k, int32_t pvf,
                                       float sentinel, const int32_t* subset_ids, int64_t n_subset, int32_t* out_ids, float* out_sim) {
  if (int rc = pv_check_subset(subset_ids, n_subset)) return rc;
  if (int rc = pv_check(pq, KIND_PQ, vecs, queries, Q, k, pvf, out_ids, out_sim)) return rc;
  return pv_search(pq, vecs, QuerySrc::of_host(queries), Q, k, pvf, out_ids, out_sim, [&](const QuerySrc& qp, int nq, int kc, int32_t* l_ids, float* l_dist) {
    return freddy_gpu_pq_search(pq, qp.host, nq, kc, sentinel, subset_ids, n_subset, l_ids, l_dist);
  });
}

// Post verification of queries named by row id (query_ids.h): stage one is the search by id's body (ivfadc_search_src / pq_search_src
// at k * pvf), the raw queries of stage two are gathered from `vecs`.  The counts of freddy_gpu_last_pv_stats cover the searched slots.
extern "C" int freddy_gpu_ivfadc_search_pv_ids(freddy_gpu_index_t* ivf, freddy_gpu_index_t* vecs, const int32_t* query_ids, int32_t n_ids, int32_t id_rule,
                                               int32_t k, int32_t pvf, int32_t W, float sentinel, int32_t found_rule, int32_t* out_query_ids,
                                               int32_t* n_queries, int32_t* out_ids, float* out_sim) {
  if (int rc = check_query_ids_front(ivf, vecs, query_ids, n_ids, id_rule, out_query_ids, n_queries, out_ids, out_sim)) return rc;
  if (int rc = pv_check_count(n_ids, k, pvf)) return rc;
  if (int rc = pv_check_limit(k, pvf)) return rc;
  if (int rc = check_probe_args(W, found_rule)) return rc;
  if (int rc = check_ann_vecs(ivf, KIND_IVF, vecs, "a search by row id")) return rc;
  if (W > ivf->C) W = ivf->C;
  ivf->pv_stats[0] = ivf->pv_stats[1] = 0;
  return search_selected_ids(vecs, query_ids, n_ids, id_rule, k, -HUGE_VALF, out_query_ids, n_queries, out_ids, out_sim,
                             [&](const QuerySrc& qs, int n, int32_t* oi, float* os) {
    return pv_search(ivf, vecs, qs, n, k, pvf, oi, os, [&](const QuerySrc& qp, int nq, int kc, int32_t* l_ids, float* l_dist) {
      return ivfadc_search_src(ivf, qp, nq, kc, W, sentinel, found_rule, l_ids, l_dist);
    });
  });
}

extern "C" int freddy_gpu_pq_search_pv_ids(freddy_gpu_index_t* pq, freddy_gpu_index_t* vecs, const int32_t* query_ids, int32_t n_ids, int32_t id_rule,
                                           int32_t k, int32_t pvf, float sentinel, const int32_t* subset_ids, int64_t n_subset, int32_t* out_query_ids,
                                           int32_t* n_queries, int32_t* out_ids, float* out_sim) {
  if (int rc = check_query_ids_front(pq, vecs, query_ids, n_ids, id_rule, out_query_ids, n_queries, out_ids, out_sim)) return rc;
  if (int rc = pv_check_subset(subset_ids, n_subset)) return rc;
  if (int rc = pv_check_count(n_ids, k, pvf)) return rc;
  if (int rc = pv_check_limit(k, pvf)) return rc;
  if (int rc = check_ann_vecs(pq, KIND_PQ, vecs, "a search by row id")) return rc;
  pq->pv_stats[0] = pq->pv_stats[1] = 0;
  return search_selected_ids(vecs, query_ids, n_ids, id_rule, k, -HUGE_VALF, out_query_ids, n_queries, out_ids, out_sim,
                             [&](const QuerySrc& qs, int n, int32_t* oi, float* os) {
    return pv_search(pq, vecs, qs, n, k, pvf, oi, os, [&](const QuerySrc& qp, int nq, int kc, int32_t* l_ids, float* l_dist) {
      return pq_search_src(pq, qp, nq, kc, sentinel, subset_ids, n_subset, l_ids, l_dist);
    });
  });
}

extern "C" int freddy_gpu_last_pv_stats(const freddy_gpu_index_t* ann, int64_t* candidates, int64_t* scored) {
  if (!ann) return fail(FREDDY_E_ARG, "NULL index");
  if (ann->kind != KIND_PQ && ann->kind != KIND_IVF) return fail(FREDDY_E_KIND, "index handle has the wrong kind for this call");
  if (candidates) *candidates = ann->pv_stats[0];
  if (scored) *scored = ann->pv_stats[1];
  return FREDDY_OK;
}

// ---- approximate analogies: 3CosAdd over the candidates of pq / ivf lists (approx_analogy.h) ---------------------------------------
// Everything both entry points refuse, scalars before handles; nothing here touches a device.
static int aa_check_scalars(const int32_t* triples, int32_t Q, int32_t k, int32_t n_cand, const int32_t* out_ids, const float* out_sim) {
  if (Q < 0 || k < 1 || n_cand < k) return fail(FREDDY_E_ARG, "bad sizes (Q=%d, k=%d, n_cand=%d)", Q, k, n_cand);
  if (Q > 0 && (!triples || !out_ids || !out_sim)) return fail(FREDDY_E_ARG, "NULL buffer");
  if (n_cand > PV_MAX_CAND) return fail(FREDDY_E_LIMIT, "n_cand = %d exceeds this build's limit of %d candidates", n_cand, PV_MAX_CAND);
  return 0;
}
static int aa_check(const freddy_gpu_index* ann, int kind, const freddy_gpu_index* vecs, const int32_t* triples, int32_t Q, int32_t k, int32_t n_cand,
                    const int32_t* out_ids, const float* out_sim) {
  if (int rc = aa_check_scalars(triples, Q, k, n_cand, out_ids, out_sim)) return rc;
  return pv_check_handles(ann, kind, vecs, "the approximate analogy");
}

// The triples whose three ids have a row, compacted, in passes that bound the pinned block as pv_search's do: aa_query writes a
// pass's raw rows to device memory and its unit rows into the pinned block, stage one (`search`: the public entry point at n_cand,
// reading its queries from that block and writing its lists into it) runs once the kernel has finished, and the re-rank scores the
// lists against the raw rows without the inputs; the result rows are scattered back to their triples.
// unit_block (the ivpq form): `block(Qc, &p)` names device memory for a pass's unit rows instead of the pinned block -- the kNN-join's
// query block, which stage one reads in stream order: aa_query is not waited for, and the unit rows never reach the host.
static int aa_pinned_units(int, float** block) { *block = nullptr; return 0; }   // (the pq / ivf forms: the pinned block's unit rows)
template <class F, class B>
static int aa_search(freddy_gpu_index* ann, freddy_gpu_index* vecs, const int32_t* triples, int32_t Q, int32_t k, int32_t n_cand, int32_t* out_ids,
                     float* out_sim, F&& search, B&& unit_block) {
  ann->aa_stats[0] = ann->aa_stats[1] = ann->aa_stats[2] = 0;
  for (size_t i = 0; i < (size_t)Q * k; ++i) { out_ids[i] = -1; out_sim[i] = -HUGE_VALF; }
  std::vector<int32_t> live, rows3, ids3;
  resolve_triples(vecs->h_ids, triples, Q, live, rows3, &ids3);
  const int na = (int)live.size();
  if (na == 0) return FREDDY_OK;   // (before any launch)
  const int d = ann->d;
  int Qc = rerank_pass(na, n_cand);   // triples per pass
  if (ann->tune.analogy_pass > 0) Qc = std::min(Qc, ann->tune.analogy_pass);
  HIP_TRY(hipSetDevice(ann->device));
  RerankBlock b;
  if (int rc = rerank_block(ann, Qc, n_cand, k, true, "approximate analogy", &b)) return rc;
  float* d_unit = nullptr;
  if (int rc = unit_block(Qc, &d_unit)) return rc;
  hipStream_t s = ann->stream;
  for (int q0 = 0; q0 < na; q0 += Qc) {
    const int nq = std::min(Qc, na - q0);
    memcpy(b.p_rows, rows3.data() + (size_t)q0 * 3, sizeof(int32_t) * 3 * (size_t)nq);
    memcpy(b.p_excl, ids3.data() + (size_t)q0 * 3, sizeof(int32_t) * 3 * (size_t)nq);
    AaQueryArgs qa;
    qa.rows = vecs->coarse; qa.in_rows = b.p_rows; qa.raw = ann->pv_q.as<float>(); qa.unit = d_unit ? d_unit : b.unit; qa.d = d;
    timed_launch(ann, s, "aa_query", [&] { hipLaunchKernelGGL(aa_query_kernel, dim3((unsigned)nq), dim3(64), aa_query_lds(d), s, qa); });
    HIP_TRY(hipGetLastError());
    if (!d_unit) HIP_TRY(hipStreamSynchronize(s));   // (stage one reads the unit rows on streams of its own)
    if (int rc = search(qa.unit, nq, b.l_ids, b.l_dist)) return rc;
    HIP_TRY(hipSetDevice(ann->device));
    if (int rc = launch_rerank(ann, vecs, s, "aa_rerank", aa_rerank_kernel<1>, aa_rerank_kernel<4>, b, b.p_excl, nq, n_cand, k)) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    for (int q = 0; q < nq; ++q) {
      memcpy(out_ids + (size_t)live[(size_t)q0 + q] * k, b.o_ids + (size_t)q * k, sizeof(int32_t) * k);
      memcpy(out_sim + (size_t)live[(size_t)q0 + q] * k, b.o_sim + (size_t)q * k, sizeof(float) * k);
      ann->aa_stats[1] += b.o_cnt[2 * q]; ann->aa_stats[2] += b.o_cnt[2 * q + 1];
    }
    ann->aa_stats[0] += nq;
  }
  return FREDDY_OK;
}

extern "C" int freddy_gpu_ivfadc_analogy(freddy_gpu_index_t* ivf, freddy_gpu_index_t* vecs, const int32_t* triples, int32_t Q, int32_t k, int32_t n_cand,
                                         int32_t W, float sentinel, int32_t found_rule, int32_t* out_ids, float* out_sim) {
  if (int rc = check_probe_args(W, found_rule)) return rc;
  if (int rc = aa_check(ivf, KIND_IVF, vecs, triples, Q, k, n_cand, out_ids, out_sim)) return rc;
  return aa_search(ivf, vecs, triples, Q, k, n_cand, out_ids, out_sim, [&](const float* qp, int nq, int32_t* l_ids, float* l_dist) {
    return freddy_gpu_ivfadc_search(ivf, qp, nq, n_cand, W, sentinel, found_rule, l_ids, l_dist);
  }, aa_pinned_units);
}

extern "C" int freddy_gpu_pq_analogy(freddy_gpu_index_t* pq, freddy_gpu_index_t* vecs, const int32_t* triples, int32_t Q, int32_t k, int32_t n_cand,
                                     float sentinel, const int32_t* subset_ids, int64_t n_subset, int32_t* out_ids, float* out_sim) {
  if (int rc = pv_check_subset(subset_ids, n_subset)) return rc;
  if (int rc = aa_check(pq, KIND_PQ, vecs, triples, Q, k, n_cand, out_ids, out_sim)) return rc;
  return aa_search(pq, vecs, triples, Q, k, n_cand, out_ids, out_sim, [&](const float* qp, int nq, int32_t* l_ids, float* l_dist) {
    return freddy_gpu_pq_search(pq, qp, nq, n_cand, sentinel, subset_ids, n_subset, l_ids, l_dist);
  }, aa_pinned_units);
}

// analogy_3cosadd_in_ivpq (freddy--0.0.1.sql:1383-1425) for a batch of triples: stage one is ONE kNN-join per pass at k = n_cand (the
// reference's literal 4) over the unit rows of the pass's live triples, which aa_query writes straight into the join's query block; the
// join's fillers (-1, 1000.0) are no candidates.
extern "C" int freddy_gpu_ivpq_analogy(freddy_gpu_index_t* ivpq, freddy_gpu_index_t* vecs, const int32_t* triples, int32_t Q, int32_t k, int32_t n_cand,
                                       const int32_t* target_ids, int64_t n_targets, int32_t alpha, int32_t pvf, int32_t method, int32_t use_target_lists,
                                       float confidence, int32_t double_threshold, int32_t* out_ids, float* out_sim) {
  if (int rc = aa_check_scalars(triples, Q, k, n_cand, out_ids, out_sim)) return rc;
  if (!ivpq || !vecs) return fail(FREDDY_E_ARG, "NULL index");
  if (int rc = knn_join_check(ivpq, n_cand, target_ids, n_targets, alpha, pvf, method, double_threshold)) return rc;
  if (int rc = check_ann_vecs(ivpq, KIND_IVPQ, vecs, "the approximate analogy")) return rc;
  return aa_search(ivpq, vecs, triples, Q, k, n_cand, out_ids, out_sim, [&](const float*, int nq, int32_t* l_ids, float* l_dist) {
    return knn_join_block(ivpq, nq, n_cand, target_ids, n_targets, alpha, pvf, method, use_target_lists, confidence, double_threshold, l_ids, l_dist, nullptr);
  }, [&](int Qc, float** block) { return join_query_block_for(ivpq, Qc, block); });
}

extern "C" int freddy_gpu_last_approx_analogy_stats(const freddy_gpu_index_t* ann, int64_t* searched, int64_t* candidates, int64_t* scored) {
  if (!ann) return fail(FREDDY_E_ARG, "NULL index");
  if (ann->kind != KIND_PQ && ann->kind != KIND_IVF && ann->kind != KIND_IVPQ) return fail(FREDDY_E_KIND, "index handle has the wrong kind for this call");
  if (searched) *searched = ann->aa_stats[0];
  if (candidates) *candidates = ann->aa_stats[1];
  if (scored) *scored = ann->aa_stats[2];
  return FREDDY_OK;
}

// ---- the assignment step of cluster_exact (assign.h) ----------------------------------------------------------------------
// Targets per pass: the ids go up and the two result arrays come back through workspace buffers of this many entries.
static constexpr int64_t AS_PASS = (int64_t)1 << 22;

// One pass of n targets with everything on the device, enqueued on s (freddy_gpu_exact_assign and freddy_gpu_cluster share it).
static int exact_assign_pass(freddy_gpu_index* ix, hipStream_t s, const float* d_queries, int Q, const int32_t* d_targets, int n, int32_t* d_best,
                             float* d_sim) {
  AssignExactArgs aa;
  aa.targets = d_targets; aa.vec_ids = ix->ids; aa.rows = ix->coarse; aa.queries = d_queries;
  aa.out_query = d_best; aa.out_sim = d_sim; aa.N = ix->N; aa.n_targets = n; aa.Q = Q; aa.d = ix->d;
  timed_launch(ix, s, "assign_exact_kernel", [&] { hipLaunchKernelGGL(assign_exact_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, aa); });
  HIP_TRY(hipGetLastError());
  return FREDDY_OK;
}

extern "C" int freddy_gpu_exact_assign(freddy_gpu_index_t* ix, const float* queries, int32_t Q, const int32_t* target_ids, int64_t n_targets,
                                       int32_t* out_query, float* out_sim) {
  // (the scalar arguments first: they are checked before the handle is looked at, so no device is needed to see these errors)
  if (Q < 0 || n_targets < 0) return fail(FREDDY_E_ARG, "bad sizes (Q=%d, n_targets=%lld)", Q, (long long)n_targets);
  if (Q > 0 && n_targets > 0 && (!queries || !target_ids || !out_query || !out_sim)) return fail(FREDDY_E_ARG, "NULL buffer");
  if (Q > AS_MAX_Q) return fail(FREDDY_E_LIMIT, "Q=%d exceeds this build's limit of %d queries per assign call", Q, AS_MAX_Q);
  if (!ix) return fail(FREDDY_E_ARG, "NULL index");
  if (ix->kind != KIND_VEC) return fail(FREDDY_E_KIND, "index handle has the wrong kind for this call");
  if (int rc = refuse_poisoned(ix)) return rc;
  if (Q == 0 || n_targets == 0) return FREDDY_OK;
  HIP_TRY(hipSetDevice(ix->device));
  Workspace* ws = workspace_for(ix, ix->stream);
  hipStream_t s = ix->stream;
  const int d = ix->d;
  const int64_t pass = std::min(AS_PASS, n_targets);
  if (ws->w_q.ensure(sizeof(float) * (size_t)Q * d) || ws->w_sub_rows.ensure(sizeof(int32_t) * (size_t)pass) ||
      ws->w_out_ids.ensure(sizeof(int32_t) * (size_t)pass) || ws->w_out_dist.ensure(sizeof(float) * (size_t)pass))
    return fail(FREDDY_E_NOMEM, "workspace allocation failed");
  HIP_TRY(hipMemcpyAsync(ws->w_q.p, queries, sizeof(float) * (size_t)Q * d, hipMemcpyHostToDevice, s));
  for (int64_t t0 = 0; t0 < n_targets; t0 += pass) {
    const int n = (int)std::min(pass, n_targets - t0);
    HIP_TRY(hipMemcpyAsync(ws->w_sub_rows.p, target_ids + t0, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, s));
    if (int rc = exact_assign_pass(ix, s, ws->w_q.as<float>(), Q, ws->w_sub_rows.as<int32_t>(), n, ws->w_out_ids.as<int32_t>(), ws->w_out_dist.as<float>())) return rc;
    HIP_TRY(hipMemcpyAsync(out_query + t0, ws->w_out_ids.p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(out_sim + t0, ws->w_out_dist.p, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));   // (the next pass overwrites the three buffers)
  }
  return FREDDY_OK;
}

// ---- the whole k-means of cluster_exact / cluster_pq (cluster.h) ---------------------------------------------------------------
// Everything is enqueued on the vector handle's stream and nothing waits for the device between the rounds: ids and draws go up,
// the kernels of all rounds follow, the unknown-id word comes down behind them, and only a call that word clears copies its outputs.
static constexpr int64_t CL_PASS = (int64_t)1 << 22;   // targets per assignment pass (option cluster_pass)

extern "C" int freddy_gpu_cluster(freddy_gpu_index_t* vecs, freddy_gpu_index_t* pq, float sentinel, const int32_t* token_ids, int64_t n, int32_t kc,
                                  int32_t rounds, const double* draws, int64_t n_draws, int32_t* out_cluster, float* out_sim, float* out_centroids) {
  // (the scalar arguments first: they are checked before a handle is looked at, so no device is needed to see these errors)
  if (n <= 0 || kc <= 0 || rounds <= 0) return fail(FREDDY_E_ARG, "bad sizes (n=%lld, kc=%d, rounds=%d)", (long long)n, kc, rounds);
  if (!token_ids || !draws || !out_cluster) return fail(FREDDY_E_ARG, "NULL buffer");
  if (kc > AS_MAX_Q) return fail(FREDDY_E_LIMIT, "kc=%d exceeds this build's limit of %d clusters", kc, AS_MAX_Q);
  if (n > (int64_t)INT32_MAX) return fail(FREDDY_E_LIMIT, "n=%lld exceeds this build's limit of %d tokens per cluster call", (long long)n, INT32_MAX);
  const int64_t need = (int64_t)kc + (int64_t)CL_SAMPLES * kc * ((int64_t)rounds - 1);
  if (n_draws < need) return fail(FREDDY_E_ARG, "n_draws=%lld, but kc=%d clusters over %d rounds take %lld draws", (long long)n_draws, kc, rounds, (long long)need);
  for (int64_t i = 0; i < need; ++i)
    if (draws[i] != draws[i]) return fail(FREDDY_E_ARG, "draw %lld is not a number", (long long)i);
  if (pq && !(sentinel <= 16777216.0f)) return fail(FREDDY_E_ARG, "sentinel=%g is not a number or above 2^24, the range the similarity of a distance is defined for", (double)sentinel);
  if (!vecs) return fail(FREDDY_E_ARG, "NULL index");
  if (vecs->kind != KIND_VEC || (pq && pq->kind != KIND_PQ)) return fail(FREDDY_E_KIND, "index handle has the wrong kind for this call");
  if (int rc = refuse_poisoned(vecs)) return rc;
  if (pq) {
    if (int rc = refuse_poisoned(pq)) return rc;
    if (pq->device != vecs->device) return fail(FREDDY_E_ARG, "the two handles are pinned on different devices (%d and %d)", vecs->device, pq->device);
    if (pq->d != vecs->d) return fail(FREDDY_E_ARG, "the two tables have different dimensions (%d and %d)", vecs->d, pq->d);
  }
  HIP_TRY(hipSetDevice(vecs->device));
  hipStream_t s = vecs->stream;
  Workspace* ws = workspace_for(vecs, s);
  Workspace* wpq = pq ? workspace_for(pq, s) : nullptr;
  const int d = vecs->d, nn = (int)n;
  const int64_t pass = std::min<int64_t>(vecs->tune.cluster_pass > 0 ? vecs->tune.cluster_pass : CL_PASS, n);
  const int Qc = pq ? pq_assign_lut_queries(pq, kc) : 0;
  const size_t head = 64;   // bytes in front of lens[]: the unknown-id word
  const int n_blk = (int)((n + CL_STEP - 1) / CL_STEP);
  // the sample kernel walks only the steps its ranks fall into: from 16 steps on (below, the sum over the block counts costs what it saves)
  const bool two_level = kc <= CL_HIST && rounds > 1 && (vecs->tune.cluster_walk == 2 || (vecs->tune.cluster_walk == 0 && n_blk > 16));
  if (ws->w_sub_rows.ensure(sizeof(int32_t) * (size_t)n) || ws->w_rows.ensure(sizeof(int32_t) * (size_t)n) || ws->w_cand.ensure(sizeof(int32_t) * (size_t)n) ||
      ws->w_out_ids.ensure(sizeof(int32_t) * (size_t)n) || ws->w_out_dist.ensure(sizeof(float) * (size_t)n) ||
      ws->w_q.ensure(sizeof(float) * (size_t)kc * d) || ws->w_cnt.ensure(head + sizeof(int32_t) * (size_t)kc) || ws->w_qc.ensure(sizeof(double) * (size_t)need) ||
      (two_level && ws->w_cellcnt.ensure(sizeof(int32_t) * (size_t)kc * n_blk)) ||
      (pq && (ws->w_found.ensure(sizeof(float) * (size_t)n) || wpq->w_lut.ensure((size_t)pq->m * pq->K * sizeof(float) * (size_t)Qc))))
    return fail(FREDDY_E_NOMEM, "workspace allocation failed");
  int32_t* d_ids = ws->w_sub_rows.as<int32_t>();
  int32_t* d_row = ws->w_rows.as<int32_t>();
  int32_t* d_clusters = ws->w_cand.as<int32_t>();
  int32_t* d_best = ws->w_out_ids.as<int32_t>();
  float* d_sim = ws->w_out_dist.as<float>();
  float* d_cent = ws->w_q.as<float>();
  uint32_t* d_flag = ws->w_cnt.as<uint32_t>();
  int32_t* d_lens = reinterpret_cast<int32_t*>(ws->w_cnt.as<char>() + head);
  double* d_draws = ws->w_qc.as<double>();
  HIP_TRY(hipMemcpyAsync(d_ids, token_ids, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(d_draws, draws, sizeof(double) * (size_t)need, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemsetAsync(d_flag, 0xff, sizeof(uint32_t), s));   // CL_NO_FLAG
  {
    ClusterInitArgs ia;
    ia.token_ids = d_ids; ia.vec_ids = vecs->ids; ia.rows = vecs->coarse; ia.draws = d_draws; ia.row_of = d_row; ia.clusters = d_clusters; ia.lens = d_lens;
    ia.centroids = d_cent; ia.flag = d_flag; ia.N = vecs->N; ia.n = nn; ia.kc = kc; ia.d = d; ia.pos_blocks = (unsigned)((n + CL_WG - 1) / CL_WG);
    timed_launch(vecs, s, "cluster_init_kernel", [&] { hipLaunchKernelGGL(cluster_init_kernel, dim3(ia.pos_blocks + (unsigned)kc), dim3(CL_WG), 0, s, ia); });
    HIP_TRY(hipGetLastError());
  }
  for (int J = 1; J <= rounds; ++J) {
    int lut_q0 = -1;   // (new centroids: no LUT of the round before is theirs)
    for (int64_t t0 = 0; t0 < n; t0 += pass) {
      const int np = (int)std::min(pass, n - t0);
      if (pq) {
        if (int rc = pq_assign_pass(pq, s, wpq->w_lut.as<float>(), Qc, &lut_q0, d_cent, kc, sentinel, d_ids + t0, np, d_best + t0, d_sim + t0, ws->w_found.as<float>() + t0)) return rc;
      } else {
        if (int rc = exact_assign_pass(vecs, s, d_cent, kc, d_ids + t0, np, d_best + t0, d_sim + t0)) return rc;
      }
    }
    ClusterApplyArgs pa;
    pa.best = d_best; pa.clusters = d_clusters; pa.lens = d_lens; pa.n = nn; pa.kc = kc; pa.n_blk = n_blk;
    pa.blk_members = two_level && J < rounds ? ws->w_cellcnt.as<int32_t>() : nullptr;
    timed_launch(vecs, s, "cluster_apply_kernel", [&] { hipLaunchKernelGGL(cluster_apply_kernel, dim3((unsigned)n_blk), dim3(CL_WG), 0, s, pa); });
    HIP_TRY(hipGetLastError());
    if (J == rounds) break;
    ClusterSampleArgs sa;
    sa.clusters = d_clusters; sa.row_of = d_row; sa.rows = vecs->coarse; sa.draws = d_draws + kc + (size_t)(J - 1) * kc * CL_SAMPLES; sa.lens = d_lens;
    sa.centroids = d_cent; sa.n = nn; sa.d = d; sa.n_blk = n_blk; sa.blk_members = pa.blk_members;
    timed_launch(vecs, s, "cluster_sample_kernel", [&] { hipLaunchKernelGGL(cluster_sample_kernel, dim3((unsigned)kc), dim3(CL_WG), 0, s, sa); });
    HIP_TRY(hipGetLastError());
  }
  uint32_t unknown = CL_NO_FLAG;
  HIP_TRY(hipMemcpyAsync(&unknown, d_flag, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (unknown != CL_NO_FLAG) return fail(FREDDY_E_ARG, "token id %d has no vector", token_ids[unknown]);   // (the first such position; nothing was written)
  HIP_TRY(hipMemcpyAsync(out_cluster, d_clusters, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, s));
  if (out_sim) HIP_TRY(hipMemcpyAsync(out_sim, d_sim, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, s));
  if (out_centroids) HIP_TRY(hipMemcpyAsync(out_centroids, d_cent, sizeof(float) * (size_t)kc * d, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return FREDDY_OK;
}

// ---- similarities by row id: pairs, matrices, joins (similarity.h) ----------------------------------------------------------
static constexpr int64_t SIM_PAIR_PASS = (int64_t)1 << 22;        // pairs per pass: the ids go up and the values come back through buffers of this many entries
static constexpr size_t SIM_PASS_BYTES = (size_t)256 << 20;       // the device result block of a pass of A rows (option similarity_pass_bytes)
static constexpr int SIM_PASS_ROWS = 65536;                       // and its A rows at most (their staged copy: 4 d bytes each)

static int sim_check_handle(const freddy_gpu_index* ix) {
  if (!ix) return fail(FREDDY_E_ARG, "NULL index");
  if (ix->kind != KIND_VEC) return fail(FREDDY_E_KIND, "index handle has the wrong kind for this call");
  return refuse_poisoned(ix);
}

extern "C" int freddy_gpu_similarity_pairs(freddy_gpu_index_t* ix, const int32_t* ids_a, const int32_t* ids_b, int64_t n, float* out_sim,
                                           uint8_t* out_known) {
  if (n < 0) return fail(FREDDY_E_ARG, "bad sizes (n=%lld)", (long long)n);
  if (n > 0 && (!ids_a || !ids_b || !out_sim || !out_known)) return fail(FREDDY_E_ARG, "NULL buffer");
  if (int rc = sim_check_handle(ix)) return rc;
  if (n == 0) return FREDDY_OK;
  // a call in which no pair has both rows launches nothing (the usual call ends this loop at its first pair)
  int64_t first = 0;
  while (first < n && (row_of_near(ix->h_ids, ids_a[first]) < 0 || row_of_near(ix->h_ids, ids_b[first]) < 0)) ++first;
  if (first == n) {
    memset(out_sim, 0, sizeof(float) * (size_t)n);
    memset(out_known, 0, (size_t)n);
    return FREDDY_OK;
  }
  HIP_TRY(hipSetDevice(ix->device));
  Workspace* ws = workspace_for(ix, ix->stream);
  hipStream_t s = ix->stream;
  const int64_t pass = std::min(SIM_PAIR_PASS, n);
  if (ws->w_sub_rows.ensure(sizeof(int32_t) * (size_t)pass) || ws->w_out_ids.ensure(sizeof(int32_t) * (size_t)pass) ||
      ws->w_out_dist.ensure(sizeof(float) * (size_t)pass) || ws->w_found.ensure((size_t)pass))
    return fail(FREDDY_E_NOMEM, "workspace allocation failed");
  for (int64_t t0 = 0; t0 < n; t0 += pass) {
    const int np = (int)std::min(pass, n - t0);
    HIP_TRY(hipMemcpyAsync(ws->w_sub_rows.p, ids_a + t0, sizeof(int32_t) * (size_t)np, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(ws->w_out_ids.p, ids_b + t0, sizeof(int32_t) * (size_t)np, hipMemcpyHostToDevice, s));
    SimPairsArgs pa;
    pa.ids_a = ws->w_sub_rows.as<int32_t>(); pa.ids_b = ws->w_out_ids.as<int32_t>(); pa.vec_ids = ix->ids; pa.rows = ix->coarse;
    pa.out_sim = ws->w_out_dist.as<float>(); pa.out_known = ws->w_found.as<uint8_t>(); pa.N = ix->N; pa.n = np; pa.d = ix->d;
    timed_launch(ix, s, "sim_pairs_kernel", [&] { hipLaunchKernelGGL(sim_pairs_kernel, dim3((unsigned)((np + 63) / 64)), dim3(64), 0, s, pa); });
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out_sim + t0, ws->w_out_dist.p, sizeof(float) * (size_t)np, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(out_known + t0, ws->w_found.p, (size_t)np, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));   // (the next pass overwrites the four buffers)
  }
  return FREDDY_OK;
}

// What the matrix and the join refuse before they look at the handle.
static int sim_check_sides(const int32_t* a_ids, const float* a_vectors, int32_t na, const int32_t* b_ids, int64_t nb) {
  if (na < 0 || nb < 0) return fail(FREDDY_E_ARG, "bad sizes (na=%d, nb=%lld)", na, (long long)nb);
  if ((a_ids != nullptr) == (a_vectors != nullptr)) return fail(FREDDY_E_ARG, "exactly one of a_ids and a_vectors names the A side");
  if (nb > 0 && !b_ids) return fail(FREDDY_E_ARG, "NULL buffer");
  if (nb > SIM_MAX_NB) return fail(FREDDY_E_LIMIT, "nb=%lld exceeds this build's limit of %lld B ids per call", (long long)nb, (long long)SIM_MAX_NB);
  return 0;
}

// The A side in passes over the matrix (arguments checked, na > 0, nb > 0).  B's ids go up once and are resolved on the device;
// per pass the A rows are gathered by row number (ids: row_of_near on the host, POSITIONAL -- an id without a row keeps its slot,
// its gathered row is zeros and its known byte 0) or staged from the caller's floats, sim_matrix_kernel writes the block
// [rows of the pass][nb] into the workspace, and block(a0, n, d_block, d_known_a, d_known_b) takes it from there -- enqueued on the
// stream; it synchronises before it returns, so the passes are serial: the D2H of pass p does not overlap the kernel of pass p + 1
// (that would take a second block and a second stream; the copy is the larger part of either, see profiles/similarity_timing.txt).
// known_a / known_b: the caller's arrays, or NULL.  *launched = false: no A row or no B row is known; nothing was launched, the
// known arrays are filled and the block is all zeros / the join empty.
template <class F>
static int sim_matrix_passes(freddy_gpu_index* ix, const int32_t* a_ids, const float* a_vectors, int32_t na, const int32_t* b_ids, int nb,
                             uint8_t* known_a, uint8_t* known_b, bool* launched, F&& block) {
  const std::vector<int32_t>& h_ids = ix->h_ids;
  const int d = ix->d;
  int64_t fa = 0, fb = 0;
  if (a_ids) while (fa < na && row_of_near(h_ids, a_ids[fa]) < 0) ++fa;
  while (fb < nb && row_of_near(h_ids, b_ids[fb]) < 0) ++fb;
  *launched = fa < na && fb < nb;
  if (!*launched) {
    if (known_a) for (int32_t i = 0; i < na; ++i) known_a[i] = a_ids ? (row_of_near(h_ids, a_ids[i]) >= 0) : 1;
    if (known_b) for (int j = 0; j < nb; ++j) known_b[j] = row_of_near(h_ids, b_ids[j]) >= 0;
    return 0;
  }
  HIP_TRY(hipSetDevice(ix->device));
  Workspace* ws = workspace_for(ix, ix->stream);
  hipStream_t s = ix->stream;
  // rows of A per pass: the block within the budget, a multiple of 16 rows (16 at least, whatever the budget)
  const size_t budget = ix->tune.similarity_pass_bytes > 0 ? (size_t)ix->tune.similarity_pass_bytes : SIM_PASS_BYTES;
  int64_t rows = (int64_t)(budget / (sizeof(float) * (size_t)nb)) / TILE_QT * TILE_QT;
  rows = std::max<int64_t>(TILE_QT, std::min<int64_t>(rows, SIM_PASS_ROWS));
  if (rows > na) rows = na;
  if (ws->w_sub_rows.ensure(sizeof(int32_t) * (size_t)nb) || ws->w_sub_pos.ensure(sizeof(int32_t) * (size_t)nb) || ws->w_found.ensure((size_t)nb) ||
      ws->w_q.ensure(sizeof(float) * (size_t)rows * d) || ws->w_lut.ensure(sizeof(float) * (size_t)rows * nb))
    return fail(FREDDY_E_NOMEM, "workspace allocation failed");
  std::vector<uint8_t> ka;
  struct Drain { hipStream_t s; ~Drain() { (void)hipStreamSynchronize(s); } } drain{s};   // (a pass that fails half-way leaves copies from `ka` and the caller's arrays enqueued)
  if (a_ids) {
    if (ws->w_used.ensure((size_t)rows)) return fail(FREDDY_E_NOMEM, "workspace allocation failed");
    if (ix->hio_in.ensure(sizeof(int32_t) * (size_t)rows)) return fail(FREDDY_E_NOMEM, "pinned staging allocation failed");
    ka.resize((size_t)rows);
  } else if (known_a) {
    memset(known_a, 1, (size_t)na);
  }
  HIP_TRY(hipMemcpyAsync(ws->w_sub_rows.p, b_ids, sizeof(int32_t) * (size_t)nb, hipMemcpyHostToDevice, s));
  timed_launch(ix, s, "sim_rows_kernel", [&] {
    hipLaunchKernelGGL(sim_rows_kernel, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, s, ws->w_sub_rows.as<const int32_t>(), nb, ix->ids, ix->N,
                       ws->w_sub_pos.as<int32_t>(), ws->w_found.as<uint8_t>());
  });
  HIP_TRY(hipGetLastError());
  if (known_b) HIP_TRY(hipMemcpyAsync(known_b, ws->w_found.p, (size_t)nb, hipMemcpyDeviceToHost, s));
  const int nblk = (nb + 63) / 64;
  for (int64_t a0 = 0; a0 < na; a0 += rows) {
    const int n = (int)std::min<int64_t>(rows, na - a0);
    if (a_ids) {
      int32_t* h_rows = ix->hio_in.as<int32_t>();   // (the last pass has been synchronised: the block is free)
      for (int i = 0; i < n; ++i) {
        h_rows[i] = row_of_near(h_ids, a_ids[a0 + i]);
        ka[(size_t)i] = h_rows[i] >= 0;
      }
      if (known_a) memcpy(known_a + a0, ka.data(), (size_t)n);
      HIP_TRY(hipMemcpyAsync(ws->w_used.p, ka.data(), (size_t)n, hipMemcpyHostToDevice, s));
      if (int rc = launch_query_gather(ix, s, QuerySrc::of_rows(ix, h_rows), ix->hio_in.as<const int32_t>(), ws->w_q.as<float>(), n, d)) return rc;
    } else {
      HIP_TRY(hipMemcpyAsync(ws->w_q.p, a_vectors + (size_t)a0 * d, sizeof(float) * (size_t)n * d, hipMemcpyHostToDevice, s));
    }
    // workgroups: 64 B rows x a range of A tiles; A is split only until the chip has about sixteen waves per CU to place
    const int n_tiles = (n + TILE_QT - 1) / TILE_QT;
    SimMatrixArgs ma;
    ma.b_rows = ws->w_sub_pos.as<int32_t>(); ma.rows = ix->coarse; ma.a = ws->w_q.as<float>(); ma.known_a = a_ids ? ws->w_used.as<uint8_t>() : nullptr;
    ma.out = ws->w_lut.as<float>(); ma.na = n; ma.nb = nb; ma.d = d; ma.tiles_per_wg = sim_tiles_per_wg(ix->n_cus, n_tiles, nblk);
    const dim3 grid((unsigned)nblk, sim_grid_y(ix->n_cus, n_tiles, nblk));
    timed_launch(ix, s, "sim_matrix_kernel", [&] { hipLaunchKernelGGL(sim_matrix_kernel, grid, dim3(64), 0, s, ma); });
    HIP_TRY(hipGetLastError());
    if (int rc = block((int32_t)a0, n, ma.out, ma.known_a, ws->w_found.as<const uint8_t>(), ws, s)) return rc;
  }
  return 0;
}

extern "C" int freddy_gpu_similarity_matrix(freddy_gpu_index_t* ix, const int32_t* a_ids, const float* a_vectors, int32_t na, const int32_t* b_ids,
                                            int64_t nb, float* out, uint8_t* known_a, uint8_t* known_b) {
  if (int rc = sim_check_sides(a_ids, a_vectors, na, b_ids, nb)) return rc;
  if (na > 0 && nb > 0 && (!out || !known_a || !known_b)) return fail(FREDDY_E_ARG, "NULL buffer");
  if (int rc = sim_check_handle(ix)) return rc;
  if (na == 0 || nb == 0) return FREDDY_OK;
  bool launched = false;
  const int rc = sim_matrix_passes(ix, a_ids, a_vectors, na, b_ids, (int)nb, known_a, known_b, &launched,
                                   [&](int32_t a0, int n, const float* d_block, const uint8_t*, const uint8_t*, Workspace*, hipStream_t s) {
    HIP_TRY(hipMemcpyAsync(out + (size_t)a0 * (size_t)nb, d_block, sizeof(float) * (size_t)n * (size_t)nb, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
  });
  if (rc) return rc;
  if (!launched) memset(out, 0, sizeof(float) * (size_t)na * (size_t)nb);
  return FREDDY_OK;
}

extern "C" int freddy_gpu_similarity_join(freddy_gpu_index_t* ix, const int32_t* a_ids, const float* a_vectors, int32_t na, const int32_t* b_ids,
                                          int64_t nb, float threshold, int64_t max_pairs, int32_t* out_a, int32_t* out_b, float* out_sim,
                                          int64_t* n_pairs) {
  if (int rc = sim_check_sides(a_ids, a_vectors, na, b_ids, nb)) return rc;
  if (max_pairs < 0) return fail(FREDDY_E_ARG, "bad sizes (max_pairs=%lld)", (long long)max_pairs);
  if (!n_pairs) return fail(FREDDY_E_ARG, "NULL n_pairs");
  if (na > 0 && nb > 0 && max_pairs > 0 && (!out_a || !out_b || !out_sim)) return fail(FREDDY_E_ARG, "NULL buffer");
  if (int rc = sim_check_handle(ix)) return rc;
  if (na == 0 || nb == 0) { *n_pairs = 0; return FREDDY_OK; }
  int64_t total = 0;   // matches of the passes so far: the position of the next pass's first match
  bool launched = false;
  const int nblk = (int)((nb + 63) / 64);
  const int rc = sim_matrix_passes(ix, a_ids, a_vectors, na, b_ids, (int)nb, nullptr, nullptr, &launched,
                                   [&](int32_t a0, int n, const float* d_block, const uint8_t* d_known_a, const uint8_t* d_known_b, Workspace* ws, hipStream_t s) {
    const int64_t units = (int64_t)n * nblk, chunks = (units + SIM_CHUNK - 1) / SIM_CHUNK;
    // (w_part: the scanned offsets, the total behind them, then the chunks' sums)
    if (ws->w_cnt.ensure(sizeof(int32_t) * (size_t)units) || ws->w_part.ensure(sizeof(int32_t) * (size_t)(units + 1 + chunks)))
      return fail(FREDDY_E_NOMEM, "workspace allocation failed");
    SimJoinArgs ja;
    ja.blk = d_block; ja.known_a = d_known_a; ja.known_b = d_known_b; ja.cnt = ws->w_cnt.as<int32_t>(); ja.off = ws->w_part.as<int32_t>();
    ja.part = ws->w_part.as<int32_t>() + units + 1;
    ja.out_a = nullptr; ja.out_b = nullptr; ja.out_sim = nullptr; ja.units = units; ja.na = n; ja.nb = (int)nb; ja.nblk = nblk; ja.a0 = a0; ja.cap = 0;
    ja.threshold = threshold;
    timed_launch(ix, s, "sim_count_kernel", [&] { hipLaunchKernelGGL(sim_count_kernel, dim3((unsigned)chunks), dim3(SIM_COUNT_WAVES * 64), 0, s, ja); });
    HIP_TRY(hipGetLastError());
    timed_launch(ix, s, "sim_scan_kernel", [&] {
      hipLaunchKernelGGL(sim_scan_kernel, dim3((unsigned)chunks), dim3(256), 0, s, ws->w_cnt.as<const int32_t>(), (const int32_t*)ja.part, units,
                         ws->w_part.as<int32_t>());
    });
    HIP_TRY(hipGetLastError());
    int32_t found = 0;   // (a block holds at most 2^30 values: option similarity_pass_bytes)
    HIP_TRY(hipMemcpyAsync(&found, ws->w_part.as<int32_t>() + units, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const int64_t cap = std::min<int64_t>(found, std::max<int64_t>(0, max_pairs - total));
    if (cap > 0) {   // only the matches that are asked for cross the bus
      if (ws->w_out_ids.ensure(sizeof(int32_t) * (size_t)cap) || ws->w_item_cell.ensure(sizeof(int32_t) * (size_t)cap) ||
          ws->w_out_dist.ensure(sizeof(float) * (size_t)cap))
        return fail(FREDDY_E_NOMEM, "workspace allocation failed");
      ja.out_a = ws->w_out_ids.as<int32_t>(); ja.out_b = ws->w_item_cell.as<int32_t>(); ja.out_sim = ws->w_out_dist.as<float>(); ja.cap = (int32_t)cap;
      const dim3 grid((unsigned)std::min<int64_t>((units + 3) / 4, 8192));
      timed_launch(ix, s, "sim_fill_kernel", [&] { hipLaunchKernelGGL(sim_fill_kernel, grid, dim3(256), 0, s, ja); });
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpyAsync(out_a + total, ja.out_a, sizeof(int32_t) * (size_t)cap, hipMemcpyDeviceToHost, s));
      HIP_TRY(hipMemcpyAsync(out_b + total, ja.out_b, sizeof(int32_t) * (size_t)cap, hipMemcpyDeviceToHost, s));
      HIP_TRY(hipMemcpyAsync(out_sim + total, ja.out_sim, sizeof(float) * (size_t)cap, hipMemcpyDeviceToHost, s));
      HIP_TRY(hipStreamSynchronize(s));
    }
    total += found;
    return 0;
  });
  if (rc) return rc;
  *n_pairs = total;
  return FREDDY_OK;
}

// The kernels of this unit that want more than the default 64 KiB of dynamic LDS.
std::vector<LdsLimit> lds_limits_exact() {
  const int b = (int)AN_MAX_LDS;
  return {{&exf_filter_kernel<1, false>, b}, {&exf_filter_kernel<2, false>, b}, {&exf_filter_kernel<1, true>, b}, {&exf_filter_kernel<2, true>, b},
          {&exj_filter_kernel<1, false>, b}, {&exj_filter_kernel<2, false>, b}, {&exj_filter_kernel<4, false>, b},
          {&exj_filter_kernel<1, true>, b},  {&exj_filter_kernel<2, true>, b},  {&exj_filter_kernel<4, true>, b},
          {&an_filter_kernel<1, false>, b},  {&an_filter_kernel<3, false>, b},  {&an_filter_kernel<1, true>, b},  {&an_filter_kernel<3, true>, b},
          {&an_scan_kernel<1, 8>, b},        {&an_scan_kernel<3, 4>, b},
          {&an_pair_scan_kernel<1>, b},      {&an_pair_scan_kernel<2>, b},      {&an_pair_scan_kernel<4>, b},     {&an_pair_scan_kernel<8>, b},
          // (the all-exact scan: more than 64 KiB from d = 513 on with tiles of 16 queries, from d = 1537 on with tiles of 8)
          &exact_scan_kernel<1, 16>, &exact_scan_kernel<2, 16>, &exact_scan_kernel<4, 16>,
          &exact_scan_kernel<1, 8>, &exact_scan_kernel<2, 8>, &exact_scan_kernel<4, 8>, &exact_scan_kernel<8, 8>, &exact_scan_kernel<16, 8>,
          &exact_scan_kernel<16, 8, true>,
          // (4096 keys + four tiles + the query: 66 KiB at d = 300, 83 KiB at EX_MAX_D; the kernel has static LDS beside the dynamic)
          {&pv_rerank_kernel<4>, (int)pv_lds_bytes(4, PV_MAX_CAND, EX_MAX_D)}, {&aa_rerank_kernel<4>, (int)pv_lds_bytes(4, PV_MAX_CAND, EX_MAX_D)}};
}

// ---- text vectors from token ids (tokenize.h) ---------------------------------------------------------------------------------------
// The texts of a call, checked: scalars, then buffers, then the length limit; nothing here touches a device or a handle.
struct TokTexts {
  const int32_t* ids = nullptr;
  const int64_t* off = nullptr;
  int32_t n = 0;
  int id_rule = 0;
  int64_t total = 0;   // offsets[n]
  int max_len = 0;     // the longest text
};
static int tok_check_texts(const int32_t* token_ids, const int64_t* offsets, int32_t n_texts, int32_t id_rule, const int32_t* out_count, TokTexts* tx) {
  if (n_texts < 0) return fail(FREDDY_E_ARG, "bad sizes (n_texts=%d)", n_texts);
  if (id_rule != FREDDY_QIDS_TABLE_ORDER && id_rule != FREDDY_QIDS_POSITIONAL) return fail(FREDDY_E_ARG, "bad id_rule %d", id_rule);
  tx->ids = token_ids; tx->off = offsets; tx->n = n_texts; tx->id_rule = id_rule;
  if (n_texts == 0) return 0;
  if (!offsets || !out_count) return fail(FREDDY_E_ARG, "NULL buffer");
  if (offsets[0] != 0) return fail(FREDDY_E_ARG, "offsets[0] is %lld, not 0", (long long)offsets[0]);
  int32_t longest = -1;
  int64_t longest_len = 0;
  for (int32_t t = 0; t < n_texts; ++t) {
    const int64_t len = offsets[t + 1] - offsets[t];
    if (len < 0) return fail(FREDDY_E_ARG, "offsets decrease at text %d (%lld after %lld)", t, (long long)offsets[t + 1], (long long)offsets[t]);
    if (len > longest_len) { longest_len = len; longest = t; }
  }
  tx->total = offsets[n_texts];
  if (tx->total > 0 && !token_ids) return fail(FREDDY_E_ARG, "NULL buffer");
  if (longest_len > TOK_MAX_LEN)
    return fail(FREDDY_E_LIMIT, "text %d has %lld ids: this build's limit is %d ids per text", longest, (long long)longest_len, TOK_MAX_LEN);
  tx->max_len = (int)longest_len;
  return 0;
}

// The texts on the device: [offsets][ids][rows][counts] in vecs->tok_dev.
struct TokDev {
  int64_t* off;
  int32_t *ids, *rows, *counts;
};
// Every id's row and every text's row list (tok_resolve, tok_rows); the lists' lengths come back into out_count[n_texts], which is
// all the host learns of them.  One synchronisation.
static int tok_row_lists(freddy_gpu_index* vecs, hipStream_t s, const TokTexts& tx, int32_t* out_count, TokDev* dv) {
  const size_t n_off = (size_t)tx.n + 1, total = (size_t)tx.total;
  if (vecs->tok_dev.ensure(sizeof(int64_t) * n_off + sizeof(int32_t) * (2 * total + (size_t)tx.n)))
    return fail(FREDDY_E_NOMEM, "tokenize: device allocation failed");
  dv->off = vecs->tok_dev.as<int64_t>();
  dv->ids = reinterpret_cast<int32_t*>(dv->off + n_off); dv->rows = dv->ids + total; dv->counts = dv->rows + total;
  HIP_TRY(hipMemcpyAsync(dv->off, tx.off, sizeof(int64_t) * n_off, hipMemcpyHostToDevice, s));
  if (total) {
    HIP_TRY(hipMemcpyAsync(dv->ids, tx.ids, sizeof(int32_t) * total, hipMemcpyHostToDevice, s));
    timed_launch(vecs, s, "tok_resolve", [&] {
      hipLaunchKernelGGL(tok_resolve_kernel, dim3(resolve_grid(vecs->n_cus, ((int64_t)total + 255) / 256)), dim3(256), 0, s, (const int32_t*)dv->ids,
                         (int64_t)total, (const int32_t*)vecs->ids, vecs->N, dv->rows);
    });
    HIP_TRY(hipGetLastError());
  }
  timed_launch(vecs, s, "tok_rows", [&] {   // (a wave per text; a smaller grid walks the rest)
    hipLaunchKernelGGL(tok_rows_kernel, dim3(resolve_grid(vecs->n_cus, tx.n)), dim3(64), tok_rows_lds(tx.max_len), s, dv->rows, (const int64_t*)dv->off,
                       (int)tx.n, tx.id_rule == FREDDY_QIDS_TABLE_ORDER ? 1 : 0, dv->counts);
  });
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out_count, dv->counts, sizeof(int32_t) * (size_t)tx.n, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return 0;
}

// The vectors of n_out texts (sel[q], or text q where sel == NULL) into dst[n_out][d] (device or mapped host memory): the centroids
// (tok_centroid), through `raw` (device memory, n_out d floats) and tok_unit when they are normalised.  Enqueued only.
static int tok_vectors(freddy_gpu_index* vecs, hipStream_t s, const TokDev& dv, const int32_t* sel, int64_t n_out, bool normalize, float* raw, float* dst) {
  const int d = vecs->d;
  auto aligned = [](const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; };
  const bool wide = d % 4 == 0 && aligned(vecs->coarse) && aligned(dst) && (!normalize || aligned(raw));
  const uint32_t U = wide ? (uint32_t)d / 4 : (uint32_t)d;
  TokArgs a;
  a.table = vecs->coarse; a.rows = dv.rows; a.offsets = dv.off; a.counts = dv.counts; a.sel = sel; a.raw = raw; a.out = normalize ? raw : dst;
  a.n_out = n_out; a.d = d;
  const dim3 cgrid(resolve_grid(vecs->n_cus, (n_out + 3) / 4));
  timed_launch(vecs, s, "tok_centroid", [&] {
    if (wide) hipLaunchKernelGGL(tok_centroid_kernel<float4>, cgrid, dim3(256), 0, s, a, U);
    else hipLaunchKernelGGL(tok_centroid_kernel<float>, cgrid, dim3(256), 0, s, a, U);
  });
  HIP_TRY(hipGetLastError());
  if (!normalize) return 0;
  a.out = dst;
  // a wave per text while the texts do not fill the chip's lanes, a chain per lane from TOK_UNIT_LANES texts on (tokenize.h has the figures)
  const int mode = vecs->tune.tokenize_unit;
  const bool by_wave = (mode == 1 || (mode == 0 && n_out < TOK_UNIT_LANES)) && tok_unit_wave_lds(d) <= (size_t)(48 << 10);
  timed_launch(vecs, s, "tok_unit", [&] {
    if (by_wave) hipLaunchKernelGGL(tok_unit_wave_kernel, dim3(resolve_grid(vecs->n_cus, n_out)), dim3(64), tok_unit_wave_lds(d), s, a);
    else if (wide) hipLaunchKernelGGL(tok_unit_kernel<float4>, dim3(resolve_grid(vecs->n_cus, (n_out + 63) / 64)), dim3(64), 0, s, a, U);
    else hipLaunchKernelGGL(tok_unit_kernel<float>, dim3(resolve_grid(vecs->n_cus, (n_out + 63) / 64)), dim3(64), 0, s, a, U);
  });
  HIP_TRY(hipGetLastError());
  return 0;
}

static int tok_check_vecs(const freddy_gpu_index* vecs) {
  if (!vecs) return fail(FREDDY_E_ARG, "NULL index");
  if (vecs->kind != KIND_VEC) return fail(FREDDY_E_KIND, "index handle has the wrong kind for this call");
  return refuse_poisoned(vecs);
}

extern "C" int freddy_gpu_tokenize(freddy_gpu_index_t* vecs, const int32_t* token_ids, const int64_t* offsets, int32_t n_texts, int32_t id_rule,
                                   int32_t normalize, float* out_vectors, int32_t* out_count) {
  TokTexts tx;
  if (n_texts > 0 && !out_vectors) return fail(FREDDY_E_ARG, "NULL buffer");
  if (int rc = tok_check_texts(token_ids, offsets, n_texts, id_rule, out_count, &tx)) return rc;
  if (int rc = tok_check_vecs(vecs)) return rc;
  if (n_texts == 0) return FREDDY_OK;
  HIP_TRY(hipSetDevice(vecs->device));
  hipStream_t s = vecs->stream;
  const size_t bytes = sizeof(float) * (size_t)n_texts * vecs->d;
  if (vecs->tok_vec.ensure(bytes) || (normalize && vecs->tok_raw.ensure(bytes))) return fail(FREDDY_E_NOMEM, "tokenize: device allocation failed");
  TokDev dv;
  if (int rc = tok_row_lists(vecs, s, tx, out_count, &dv)) return rc;
  if (int rc = tok_vectors(vecs, s, dv, nullptr, n_texts, normalize != 0, vecs->tok_raw.as<float>(), vecs->tok_vec.as<float>())) return rc;
  HIP_TRY(hipMemcpyAsync(out_vectors, vecs->tok_vec.p, bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return FREDDY_OK;
}

// The pinned block of a pass of the *_search_texts calls holds at most this many bytes of vectors (option tokenize_pass: fewer texts).
static constexpr size_t TOK_PASS_BYTES = (size_t)256 << 20;

// The frame of the three *_search_texts entry points once nothing is refused: fillers everywhere, the row lists of every text, then the
// texts with a non-empty list, compacted, in passes: their vectors go straight into the pinned block (tok_centroid / tok_unit read the
// pass's text numbers from the same block), `search(block, nq, ids, values)` -- the public float entry point -- runs over it once the
// kernels have finished, and the lists are put in their texts' slots.  The vectors never reach the caller's memory, the table's rows
// never reach the host; a call without a live text launches nothing after the row lists.
template <class F>
static int tok_search(freddy_gpu_index* vecs, const TokTexts& tx, bool normalize, int32_t k, float filler, int32_t* out_count, int32_t* out_ids,
                      float* out_val, F&& search) {
  for (size_t i = 0; i < (size_t)tx.n * k; ++i) { out_ids[i] = -1; out_val[i] = filler; }
  HIP_TRY(hipSetDevice(vecs->device));
  hipStream_t s = vecs->stream;
  TokDev dv;
  if (int rc = tok_row_lists(vecs, s, tx, out_count, &dv)) return rc;
  std::vector<int32_t> live;
  for (int32_t t = 0; t < tx.n; ++t)
    if (out_count[t] > 0) live.push_back(t);
  const int na = (int)live.size(), d = vecs->d;
  if (na == 0) return FREDDY_OK;
  int Qc = (int)std::min<size_t>((size_t)na, std::max<size_t>(1, TOK_PASS_BYTES / (sizeof(float) * (size_t)d)));
  if (vecs->tune.tokenize_pass > 0) Qc = std::min(Qc, vecs->tune.tokenize_pass);
  const size_t n_unit = ((size_t)Qc * d + 3) / 4 * 4;   // (the text numbers behind the vectors, 16-byte aligned)
  if (vecs->tok_io.ensure(sizeof(float) * n_unit + sizeof(int32_t) * (size_t)Qc)) return fail(FREDDY_E_NOMEM, "tokenize: pinned staging allocation failed");
  if (normalize && vecs->tok_raw.ensure(sizeof(float) * (size_t)Qc * d)) return fail(FREDDY_E_NOMEM, "tokenize: device allocation failed");
  float* const block = vecs->tok_io.as<float>();
  int32_t* const sel = reinterpret_cast<int32_t*>(block + n_unit);
  const bool direct = na == tx.n && Qc == na;   // (every text is live and one pass takes them: the lists are written where they belong)
  std::vector<int32_t> ti(direct ? 0 : (size_t)Qc * k);
  std::vector<float> tv(direct ? 0 : (size_t)Qc * k);
  for (int q0 = 0; q0 < na; q0 += Qc) {
    const int nq = std::min(Qc, na - q0);
    memcpy(sel, live.data() + q0, sizeof(int32_t) * (size_t)nq);
    if (int rc = tok_vectors(vecs, s, dv, sel, nq, normalize, vecs->tok_raw.as<float>(), block)) return rc;
    HIP_TRY(hipStreamSynchronize(s));   // (the search reads the block on streams of its own)
    if (direct) return search(block, nq, out_ids, out_val);
    if (int rc = search(block, nq, ti.data(), tv.data())) return rc;
    HIP_TRY(hipSetDevice(vecs->device));
    for (int q = 0; q < nq; ++q) {
      memcpy(out_ids + (size_t)live[(size_t)q0 + q] * k, ti.data() + (size_t)q * k, sizeof(int32_t) * (size_t)k);
      memcpy(out_val + (size_t)live[(size_t)q0 + q] * k, tv.data() + (size_t)q * k, sizeof(float) * (size_t)k);
    }
  }
  return FREDDY_OK;
}

static int tok_check_lists(int32_t n_texts, int32_t k, const int32_t* out_ids, const float* out_val) {
  if (k <= 0) return fail(FREDDY_E_ARG, "k must be > 0");
  if (n_texts > 0 && (!out_ids || !out_val)) return fail(FREDDY_E_ARG, "NULL buffer");
  return 0;
}

extern "C" int freddy_gpu_ivfadc_search_texts(freddy_gpu_index_t* ivf, freddy_gpu_index_t* vecs, const int32_t* token_ids, const int64_t* offsets,
                                              int32_t n_texts, int32_t id_rule, int32_t k, int32_t W, float sentinel, int32_t found_rule,
                                              int32_t* out_count, int32_t* out_ids, float* out_dist) {
  TokTexts tx;
  if (int rc = tok_check_lists(n_texts, k, out_ids, out_dist)) return rc;
  if (int rc = check_probe_args(W, found_rule)) return rc;
  if (int rc = tok_check_texts(token_ids, offsets, n_texts, id_rule, out_count, &tx)) return rc;
  if (int rc = check_list_limit(k)) return rc;
  if (int rc = check_ann_vecs(ivf, KIND_IVF, vecs, "a search by texts")) return rc;
  if (n_texts == 0) return FREDDY_OK;
  return tok_search(vecs, tx, true, k, sentinel, out_count, out_ids, out_dist, [&](const float* q, int nq, int32_t* oi, float* od) {
    return freddy_gpu_ivfadc_search(ivf, q, nq, k, W, sentinel, found_rule, oi, od);
  });
}

extern "C" int freddy_gpu_pq_search_texts(freddy_gpu_index_t* pq, freddy_gpu_index_t* vecs, const int32_t* token_ids, const int64_t* offsets,
                                          int32_t n_texts, int32_t id_rule, int32_t k, float sentinel, const int32_t* subset_ids, int64_t n_subset,
                                          int32_t* out_count, int32_t* out_ids, float* out_dist) {
  TokTexts tx;
  if (int rc = tok_check_lists(n_texts, k, out_ids, out_dist)) return rc;
  if (int rc = pv_check_subset(subset_ids, n_subset)) return rc;
  if (int rc = tok_check_texts(token_ids, offsets, n_texts, id_rule, out_count, &tx)) return rc;
  if (int rc = check_list_limit(k)) return rc;
  if (int rc = check_ann_vecs(pq, KIND_PQ, vecs, "a search by texts")) return rc;
  if (n_texts == 0) return FREDDY_OK;
  return tok_search(vecs, tx, true, k, sentinel, out_count, out_ids, out_dist, [&](const float* q, int nq, int32_t* oi, float* od) {
    return freddy_gpu_pq_search(pq, q, nq, k, sentinel, subset_ids, n_subset, oi, od);
  });
}

extern "C" int freddy_gpu_exact_search_texts(freddy_gpu_index_t* vecs, const int32_t* token_ids, const int64_t* offsets, int32_t n_texts,
                                             int32_t id_rule, int32_t normalize, int32_t k, const int32_t* subset_ids, int64_t n_subset,
                                             int32_t* out_count, int32_t* out_ids, float* out_sim) {
  TokTexts tx;
  if (int rc = tok_check_lists(n_texts, k, out_ids, out_sim)) return rc;
  if (int rc = pv_check_subset(subset_ids, n_subset)) return rc;
  if (int rc = tok_check_texts(token_ids, offsets, n_texts, id_rule, out_count, &tx)) return rc;
  if (int rc = check_list_limit(k)) return rc;
  if (int rc = tok_check_vecs(vecs)) return rc;
  if (n_texts == 0) return FREDDY_OK;
  return tok_search(vecs, tx, normalize != 0, k, -HUGE_VALF, out_count, out_ids, out_sim, [&](const float* q, int nq, int32_t* oi, float* os) {
    return freddy_gpu_exact_search(vecs, q, nq, k, subset_ids, n_subset, oi, os);
  });
}
