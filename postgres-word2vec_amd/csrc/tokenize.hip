// tokenize.hip -- text vectors from token ids on a raw-vector handle (tokenize.h): freddy_gpu_tokenize, and the three *_search_texts
// calls, which search over such vectors through the public float entry points of pipeline.hip, pq.hip and exact.hip.
#include "internal.h"

#include "tokenize.h"
#include "query_ids.h"

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

extern "C" int freddy_gpu_tokenize(freddy_gpu_index_t* vecs, const int32_t* token_ids, const int64_t* offsets, int32_t n_texts, int32_t id_rule,
                                   int32_t normalize, float* out_vectors, int32_t* out_count) {
  TokTexts tx;
  if (n_texts > 0 && !out_vectors) return fail(FREDDY_E_ARG, "NULL buffer");
  if (int rc = tok_check_texts(token_ids, offsets, n_texts, id_rule, out_count, &tx)) return rc;
  if (int rc = check_vec_handle(vecs)) return rc;
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
  if (int rc = check_vec_handle(vecs)) return rc;
  if (n_texts == 0) return FREDDY_OK;
  return tok_search(vecs, tx, normalize != 0, k, -HUGE_VALF, out_count, out_ids, out_sim, [&](const float* q, int nq, int32_t* oi, float* os) {
    return freddy_gpu_exact_search(vecs, q, nq, k, subset_ids, n_subset, oi, os);
  });
}
