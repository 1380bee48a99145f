// exact.hip -- pin_vectors, exact brute-force kNN (core_functions.c:67-81, freddy--0.0.1.sql:426-454) and the exact
// kNN-join (exact_join.h) on the same handle; exact_host.h: the filter + refine chain they share with the exact analogies (analogy.hip).
// Exact kNN and the exact join by row id (freddy_gpu_exact_search_ids / _exact_join_ids): queries through a QuerySrc (query_ids.h), id sets resolved on the device (resolve.h).
// The rows of an id set (resolve_row_set, vec_subset) are what analogy.hip calls here.
#include "internal.h"

#include "exact.h"
#include "exact2.h"
#include "exact_join.h"
#include "query_ids.h"
#include "resolve.h"
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

// ---- the rows of an id set (resolve.h; RowSet: internal.h) and the queries of a call, for either source ---------------------------
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
int vec_subset(freddy_gpu_index* ix, Workspace* ws, hipStream_t s, const RowSet& rows, const float** xb,
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
  const bool want_filter = !sub_rows && exf_wanted(ix, n_rows) && k <= 32 && n_rows >= 1;
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
int resolve_row_set(freddy_gpu_index* ix, bool on_device, const int32_t* ids, int64_t n, std::vector<int32_t>* h_rows, RowSet* out) {
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
  if (int rc = check_vec_handle(ix)) return rc;
  if (Q < 0 || k <= 0 || n_subset < 0 || (n_subset > 0 && !subset_ids)) return fail(FREDDY_E_ARG, "bad sizes");
  if (Q > 0 && (!queries || !out_ids || !out_sim)) return fail(FREDDY_E_ARG, "NULL buffer");
  if (int rc = check_list_limit(k)) return rc;
  if (Q == 0) return FREDDY_OK;
  return exact_search_src(ix, QuerySrc::of_host(queries), Q, k, subset_ids, n_subset, ix->tune.exact_resolve != 0, out_ids, out_sim);
}

// Exact kNN of rows named by id (query_ids.h) over the whole table (subset_ids == NULL) or over an id set, which is resolved on the device.
extern "C" int freddy_gpu_exact_search_ids(freddy_gpu_index_t* vecs, const int32_t* query_ids, int32_t n_ids, int32_t id_rule, int32_t k,
                                           const int32_t* subset_ids, int64_t n_subset, int32_t* out_query_ids, int32_t* n_queries,
                                           int32_t* out_ids, float* out_sim) {
  if (int rc = check_query_ids_front(vecs, vecs, query_ids, n_ids, id_rule, out_query_ids, n_queries, out_ids, out_sim)) return rc;
  if (k <= 0 || n_subset < 0 || (n_subset > 0 && !subset_ids)) return fail(FREDDY_E_ARG, "bad sizes");
  if (int rc = check_list_limit(k)) return rc;
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
  if (Q > 64 && 4 * tile_lds <= EX_MAX_LDS && ix->tune.exact_join_tile != 64) NT = 4;
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
  const bool want_filter = exf_wanted(ix, nT, EXJ_MIN_TARGETS) && k <= 32 && nT >= 1;
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
  if (int rc = check_list_limit(k)) return rc;
  if (int rc = check_vec_handle(ix)) return rc;
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
  if (int rc = check_list_limit(k)) return rc;
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

// The kernels of this unit that want more than the default 64 KiB of dynamic LDS.
std::vector<LdsLimit> lds_limits_exact() {
  const int b = (int)EX_MAX_LDS;
  return {{&exf_filter_kernel<1, false>, b}, {&exf_filter_kernel<2, false>, b}, {&exf_filter_kernel<1, true>, b}, {&exf_filter_kernel<2, true>, b},
          {&exj_filter_kernel<1, false>, b}, {&exj_filter_kernel<2, false>, b}, {&exj_filter_kernel<4, false>, b},
          {&exj_filter_kernel<1, true>, b},  {&exj_filter_kernel<2, true>, b},  {&exj_filter_kernel<4, true>, b},
          // (the all-exact scan: more than 64 KiB from d = 513 on with tiles of 16 queries, from d = 1537 on with tiles of 8)
          &exact_scan_kernel<1, 16>, &exact_scan_kernel<2, 16>, &exact_scan_kernel<4, 16>,
          &exact_scan_kernel<1, 8>, &exact_scan_kernel<2, 8>, &exact_scan_kernel<4, 8>, &exact_scan_kernel<8, 8>, &exact_scan_kernel<16, 8>,
          &exact_scan_kernel<16, 8, true>};
}
