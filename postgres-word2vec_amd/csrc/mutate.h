// mutate.h -- freddy_gpu_append_rows / freddy_gpu_remove_rows / freddy_gpu_update_rows, included by pin.hip.
// An entry point checks its arguments, fans out over the replicas (on_every_device) and dispatches on the handle's kind.
// Every append_<kind> / remove_<kind> reads top to bottom as
//   stage     everything that can fail, into the call's Staged (mutate_host.h): the handle is not touched
//   reserve   the host vectors' capacity (may throw: still before anything has changed)
//   commit    assignments, frees of the old arrays and host-vector edits that cannot fail
// so a failed call leaves the handle as it was.  The one exception is a vector handle, whose filter statistics are rewritten in
// place behind the commit (exf_table_stats): a failure there poisons the handle.  update_<kind> writes in place by design; it
// raises *wrote before its first write, and a failure after that poisons the handle.
#pragma once
#include "mutate_host.h"

// views of the flat table are rebuilt on next use (the subset view is refreshed by every subset call anyway: an append leaves it)
static void drop_pq_views(freddy_gpu_index* ix, bool sub_view = true) {
  if (ix->pq_shadow) { free_index(ix->pq_shadow); ix->pq_shadow = nullptr; }
  if (sub_view && ix->pq_sub_view) { free_index(ix->pq_sub_view); ix->pq_sub_view = nullptr; }
}

// ---- append_rows
static int append_pq(freddy_gpu_index* ix, int64_t n, const int32_t* ids, const int16_t* codes) {
  if (!codes) return fail(FREDDY_E_ARG, "codes are required");
  if (int rc = check_payload(NEW_PACKED_ROW, n, nullptr, 1, codes, ix->m, ix->K)) return rc;
  const size_t old_n = (size_t)ix->N;
  std::vector<int32_t> row_pos((size_t)n);
  for (int64_t i = 0; i < n; ++i) row_pos[(size_t)i] = (int32_t)(ix->N + i);   // flat table: position = row index
  // stage
  Staged st(ix->stream);
  FreshLayout L;
  if (int rc = append_packed_rows(ix, st, 1, n, nullptr, row_pos.data(), codes, L)) return rc;
  int32_t* new_ids = st.grown(ix->ids, old_n, ids, (size_t)n);
  if (!new_ids) return grow_failed(st);
  // reserve
  ix->h_ids.reserve(ix->h_ids.size() + (size_t)n);
  // commit
  install_layout(ix, st, L);
  st.install(ix->ids, new_ids, old_n, old_n + (size_t)n, &ix->bytes);
  ix->h_ids.insert(ix->h_ids.end(), ids, ids + n);
  ix->max_id = ids[n - 1];
  drop_pq_views(ix, false);
  return FREDDY_OK;
}

static int append_ivf(freddy_gpu_index* ix, int64_t n, const int32_t* ids, const int32_t* coarse_id, const int16_t* codes) {
  if (!codes || !coarse_id) return fail(FREDDY_E_ARG, "coarse_id and codes are required");
  if (int rc = check_payload(NEW_PACKED_ROW, n, coarse_id, ix->C, codes, ix->m, ix->K)) return rc;
  // stage (the block layout, the one-byte codes and the row terms)
  Staged st(ix->stream);
  FreshLayout L;
  if (int rc = append_packed_rows(ix, st, ix->C, n, coarse_id, ids, codes, L)) return rc;
  // commit
  install_layout(ix, st, L);
  ix->max_id = ids[n - 1];
  return FREDDY_OK;
}

// the commit of an ivpq handle's row arrays, now nn rows long (vectors: NULL unless pinned), and of the joins' scratch bitmap, which
// like views and workspaces is outside the footprint
static void install_ivpq_arrays(freddy_gpu_index* ix, Staged& st, size_t nn, int32_t* ids, int32_t* cell, int16_t* codes, float* vectors, uint32_t* markbits) {
  JoinIndex& j = ix->join;
  const size_t o = (size_t)j.N;
  st.install(j.ids, ids, o, nn, &ix->bytes);
  st.install(j.cell, cell, o, nn, &ix->bytes);
  st.install(j.codes, codes, o * j.MP, nn * j.MP, &ix->bytes);
  if (j.has_vectors) st.install(j.vectors, vectors, o * j.d, nn * j.d, &ix->bytes);
  st.install(j.markbits, markbits);
  j.N = (int64_t)nn; ix->N = j.N;
}

static int append_ivpq(freddy_gpu_index* ix, int64_t n, const int32_t* ids, const int32_t* coarse_id, const int16_t* codes, const float* vectors) {
  JoinIndex& j = ix->join;
  if (!codes || !coarse_id || (j.has_vectors && !vectors)) return fail(FREDDY_E_ARG, "coarse_id, codes (and vectors, if pinned) are required");
  if (int rc = check_payload(NEW_IVPQ_ROW, n, coarse_id, j.cells, codes, j.m, j.K)) return rc;
  const size_t o = (size_t)j.N, nn = (size_t)(j.N + n);
  // stage: every longer array, and the longer scratch bitmap
  Staged st(ix->stream);
  int32_t *new_ids = nullptr, *new_cell = nullptr;
  int16_t* new_codes = nullptr;
  float* new_vec = nullptr;
  uint32_t* new_mark = nullptr;
  if (!(new_ids = st.grown(j.ids, o, ids, (size_t)n)) || !(new_cell = st.grown(j.cell, o, coarse_id, (size_t)n)) ||
      !(new_codes = st.grown(j.codes, o * j.MP, join_pad_codes(codes, n, j.m, j.MP).data(), (size_t)n * j.MP)) ||
      (j.has_vectors && !(new_vec = st.grown(j.vectors, o * j.d, vectors, (size_t)n * j.d))) || !(new_mark = st.empty<uint32_t>((nn + 31) / 32 + 1)))
    return grow_failed(st);
  // reserve
  j.h_ids.reserve(j.h_ids.size() + (size_t)n); j.h_cell.reserve(j.h_cell.size() + (size_t)n);
  // commit
  install_ivpq_arrays(ix, st, nn, new_ids, new_cell, new_codes, new_vec, new_mark);
  j.h_ids.insert(j.h_ids.end(), ids, ids + n);
  j.h_cell.insert(j.h_cell.end(), coarse_id, coarse_id + n);
  j.ids_affine = (int64_t)j.h_ids.back() - j.h_ids.front() == j.N - 1;
  return FREDDY_OK;
}

// the commit of a vector handle's three arrays, now nn rows long
static void install_vec_arrays(freddy_gpu_index* ix, Staged& st, size_t nn, int32_t* ids, float* rows, float* xb) {
  const size_t o = (size_t)ix->N, d = (size_t)ix->d;
  const int64_t new_blocks = (int64_t)((nn + 63) / 64);
  st.install(ix->ids, ids, o, nn, &ix->bytes);
  st.install(ix->coarse, nn ? rows : (float*)nullptr, o * d, nn * d, &ix->bytes);   // (pin_vectors keeps no row-major copy of an empty table)
  ix->bytes += xb_bytes(ix->d, new_blocks) - xb_bytes(ix->d, ix->n_blocks);
  st.install(ix->xb, xb);
  ix->n_blocks = new_blocks; ix->N = (int64_t)nn;
}

static int append_vec(freddy_gpu_index* ix, int64_t n, const int32_t* ids, const float* vectors) {
  if (!vectors) return fail(FREDDY_E_ARG, "vectors are required");
  const int d = ix->d;
  const size_t o = (size_t)ix->N, nn = (size_t)(ix->N + n);
  const int64_t new_blocks = (int64_t)((nn + 63) / 64);
  const size_t xb_size = sizeof(float) * (size_t)new_blocks * d * 64;
  // stage: the longer blocked copy, row-major copy and ids
  Staged st(ix->stream);
  float* xb = st.empty<float>((size_t)new_blocks * d * 64);
  if (!xb) return fail(FREDDY_E_NOMEM, "device allocation failed while appending rows");
  if (hipMemset(xb, 0, xb_size) != hipSuccess ||
      (ix->n_blocks && hipMemcpy(xb, ix->xb, sizeof(float) * (size_t)ix->n_blocks * d * 64, hipMemcpyDeviceToDevice) != hipSuccess))
    return fail(FREDDY_E_HIP, "copying the row blocks failed");
  float* new_rows = st.grown(ix->coarse, o * d, vectors, (size_t)n * d);
  if (!new_rows) return grow_failed(st);
  int32_t* new_ids = st.grown(ix->ids, o, ids, (size_t)n);
  if (!new_ids) return grow_failed(st);
  hipLaunchKernelGGL(place_vectors_kernel, dim3((unsigned)n), dim3(256), 0, ix->stream, new_rows + o * d, (int64_t)o, n, xb, d);
  st.in_flight = true;
  if (hipGetLastError() != hipSuccess || st.sync() != hipSuccess) return fail(FREDDY_E_HIP, "re-blocking the new rows failed");
  // reserve
  ix->h_ids.reserve(ix->h_ids.size() + (size_t)n);
  // commit
  install_vec_arrays(ix, st, nn, new_ids, new_rows, xb);
  ix->h_ids.insert(ix->h_ids.end(), ids, ids + n);
  // in place behind the commit: the filter's scale and norm bound cover the new rows.  A failure from here on leaves rows the
  // filter's state does not cover -> the handle is poisoned
  if (int rc = exf_table_stats(ix, (int64_t)o, n)) { ix->poisoned = true; return rc; }
  return FREDDY_OK;
}

static int append_on_device(freddy_gpu_index* ix, int64_t n, const int32_t* ids, const int32_t* coarse_id, const int16_t* codes, const float* vectors) {
  if (ix->kind == KIND_IVPQ) ix->join.tl_valid = false;   // (the cached "id IN (targets)" resolution refers to the rows as they were)
  const int32_t last_id = ix->kind == KIND_IVPQ ? (ix->join.h_ids.empty() ? -1 : ix->join.h_ids.back())
                          : ix->kind == KIND_IVF ? ix->max_id : (ix->h_ids.empty() ? -1 : ix->h_ids.back());
  for (int64_t i = 0; i < n; ++i)
    if (ids[i] <= (i ? ids[i - 1] : last_id))
      return fail(FREDDY_E_ARG, "appended ids must ascend beyond the largest pinned id %d (row %lld has %d)", last_id, (long long)i, ids[i]);
  if (ix->N + n > kMaxRows) return fail(FREDDY_E_LIMIT, "N too large for 32-bit row positions");
  switch (ix->kind) {
    case KIND_PQ: return append_pq(ix, n, ids, codes);
    case KIND_IVF: return append_ivf(ix, n, ids, coarse_id, codes);
    case KIND_IVPQ: return append_ivpq(ix, n, ids, coarse_id, codes, vectors);
    case KIND_VEC: return append_vec(ix, n, ids, vectors);
  }
  return fail(FREDDY_E_KIND, "index handle has the wrong kind for this call");
}

extern "C" int freddy_gpu_append_rows(freddy_gpu_index_t* ix, int64_t n, const int32_t* ids, const int32_t* coarse_id,
                                      const int16_t* codes, const float* vectors) {
  if (!ix) return fail(FREDDY_E_ARG, "NULL index");
  if (n < 0 || (n > 0 && !ids)) return fail(FREDDY_E_ARG, "bad argument");
  if (n == 0) return FREDDY_OK;
  return on_every_device(ix, [&](freddy_gpu_index* dev, bool) { return append_on_device(dev, n, ids, coarse_id, codes, vectors); });
}

// ---- remove_rows.  want: the ids to remove, ascending and distinct; *gone: the rows that left
static int remove_pq(freddy_gpu_index* ix, const std::vector<int32_t>& want, int64_t* gone) {
  const std::vector<int32_t> rows = rows_of_ids(ix->h_ids, want.data(), (int64_t)want.size());   // flat table: pos = row index
  if (rows.empty()) return FREDDY_OK;
  const size_t old_n = (size_t)ix->N, new_n = old_n - rows.size();
  // stage: the gathered ids, the compacted layout
  Staged st(ix->stream);
  int32_t* d_rm = st.put(rows.data(), rows.size());
  if (!d_rm) return fail(FREDDY_E_NOMEM, "device allocation failed while removing rows");
  int32_t* new_ids = nullptr;
  if (int rc = gather_rows(st, ix->ids, (int64_t)new_n, 1, d_rm, (int)rows.size(), &new_ids)) return rc;
  int32_t unused = -1;
  FreshLayout L;
  if (int rc = remove_packed_rows(ix, st, 1, rows, true, gone, &unused, L)) return rc;   // (synchronises the stream: new_ids is complete)
  if (!L.ready) return fail(FREDDY_E_HIP, "rows %d.. have no slot: the pinned layout is inconsistent", rows[0]);
  // commit
  install_layout(ix, st, L);
  drop_pq_views(ix);
  st.install(ix->ids, new_ids, old_n, new_n, &ix->bytes);
  erase_rows(ix->h_ids, rows);
  ix->max_id = ix->h_ids.empty() ? -1 : ix->h_ids.back();
  return FREDDY_OK;
}

static int remove_ivf(freddy_gpu_index* ix, const std::vector<int32_t>& want, int64_t* gone) {
  // stage (the compacted lists, their one-byte codes and row terms)
  Staged st(ix->stream);
  int32_t max_pos = -1;
  FreshLayout L;
  if (int rc = remove_packed_rows(ix, st, ix->C, want, false, gone, &max_pos, L)) return rc;   // (pos holds the ids)
  if (!L.ready) return FREDDY_OK;   // (no pinned row has one of the ids)
  // commit
  install_layout(ix, st, L);
  ix->max_id = max_pos;   // a later append may start above the largest id that is left, as on a fresh pin
  return FREDDY_OK;
}

static int remove_ivpq(freddy_gpu_index* ix, const std::vector<int32_t>& want, int64_t* gone) {
  JoinIndex& j = ix->join;
  const std::vector<int32_t> rows = rows_of_ids(j.h_ids, want.data(), (int64_t)want.size());
  if (rows.empty()) return FREDDY_OK;
  const size_t o = (size_t)j.N, nn = o - rows.size();
  const int n_rm = (int)rows.size();
  // stage: the shorter scratch bitmap, every gathered array
  Staged st(ix->stream);
  int32_t* d_rm = st.put(rows.data(), rows.size());
  uint32_t* markbits = st.empty<uint32_t>((nn + 31) / 32 + 1);
  if (!d_rm || !markbits) return fail(FREDDY_E_NOMEM, "device allocation failed while removing rows");
  int32_t *new_ids = nullptr, *new_cell = nullptr;
  int16_t* new_codes = nullptr;
  float* new_vec = nullptr;
  int rc = gather_rows(st, j.ids, (int64_t)nn, 1, d_rm, n_rm, &new_ids);
  if (!rc) rc = gather_rows(st, j.cell, (int64_t)nn, 1, d_rm, n_rm, &new_cell);
  if (!rc) rc = gather_rows(st, j.codes, (int64_t)nn, j.MP, d_rm, n_rm, &new_codes);
  if (!rc && j.has_vectors) rc = gather_rows(st, j.vectors, (int64_t)nn, j.d, d_rm, n_rm, &new_vec);
  if (!rc && st.sync() != hipSuccess) rc = fail(FREDDY_E_HIP, "compacting the ivpq rows failed");
  if (rc) return rc;
  // commit
  install_ivpq_arrays(ix, st, nn, new_ids, new_cell, new_codes, new_vec, markbits);
  erase_rows(j.h_ids, rows);
  erase_rows(j.h_cell, rows);
  j.ids_affine = j.N > 0 && (int64_t)j.h_ids.back() - j.h_ids.front() == j.N - 1;   // (a hole in the middle: binary search from now on)
  j.tl_valid = false;   // (the cached "id IN (targets)" resolution refers to the rows as they were)
  *gone = (int64_t)rows.size();
  return FREDDY_OK;
}

static int remove_vec(freddy_gpu_index* ix, const std::vector<int32_t>& want, int64_t* gone) {
  const std::vector<int32_t> rows = rows_of_ids(ix->h_ids, want.data(), (int64_t)want.size());
  if (rows.empty()) return FREDDY_OK;
  const int d = ix->d;
  const size_t o = (size_t)ix->N, nn = o - rows.size();
  const int64_t new_blocks = (int64_t)((nn + 63) / 64), xb_blocks = alloc_blocks(new_blocks);
  const int64_t same_blocks = std::min<int64_t>(rows[0] / 64, new_blocks);   // (the blocks before the first row that leaves stay as they are)
  const size_t blk = sizeof(float) * (size_t)d * 64;
  // stage: the gathered ids and rows, the blocked copy re-blocked from the first row that leaves
  Staged st(ix->stream);
  int32_t* d_rm = st.put(rows.data(), rows.size());
  if (!d_rm) return fail(FREDDY_E_NOMEM, "device allocation failed while removing rows");
  int32_t* new_ids = nullptr;
  float *new_rows = nullptr, *xb = nullptr;
  if (int rc = gather_rows(st, ix->ids, (int64_t)nn, 1, d_rm, (int)rows.size(), &new_ids)) return rc;
  if (int rc = gather_rows(st, ix->coarse, (int64_t)nn, d, d_rm, (int)rows.size(), &new_rows)) return rc;
  if (!(xb = st.empty<float>((size_t)xb_blocks * d * 64))) return fail(FREDDY_E_NOMEM, "device allocation failed while removing rows");
  st.in_flight = true;
  if (same_blocks > 0 && hipMemcpyAsync(xb, ix->xb, blk * (size_t)same_blocks, hipMemcpyDeviceToDevice, ix->stream) != hipSuccess)
    return fail(FREDDY_E_HIP, "copying the row blocks failed");
  if (xb_blocks > same_blocks && hipMemsetAsync(xb + (size_t)same_blocks * d * 64, 0, blk * (size_t)(xb_blocks - same_blocks), ix->stream) != hipSuccess)
    return fail(FREDDY_E_HIP, "clearing the row blocks failed");
  if ((int64_t)nn > same_blocks * 64) {
    const int64_t first = same_blocks * 64, cnt = (int64_t)nn - first;
    hipLaunchKernelGGL(place_vectors_kernel, dim3((unsigned)cnt), dim3(256), 0, ix->stream, new_rows + (size_t)first * d, first, cnt, xb, d);
    if (hipGetLastError() != hipSuccess) return fail(FREDDY_E_HIP, "re-blocking the rows failed");
  }
  if (st.sync() != hipSuccess) return fail(FREDDY_E_HIP, "compacting the vector rows failed");
  // commit
  install_vec_arrays(ix, st, nn, new_ids, new_rows, xb);
  erase_rows(ix->h_ids, rows);
  *gone = (int64_t)rows.size();
  // in place behind the commit: the exact filter's state over the rows that are left, as a fresh pin computes it -- a larger scale
  // once the row with the largest element has gone, the filter back on once the only non-finite row has (the fragment copy keeps
  // its capacity).  A failure there: the rows have gone, the filter's state has not followed -> the handle is poisoned
  if (nn == 0) ix->exf_ok = false;
  else if (int rc = exf_table_stats(ix, 0, (int64_t)nn)) { ix->poisoned = true; return rc; }
  return FREDDY_OK;
}

static int remove_on_device(freddy_gpu_index* ix, const std::vector<int32_t>& want, int64_t* removed) {
  int64_t gone = 0;
  int rc = 0;
  switch (ix->kind) {
    case KIND_PQ: rc = remove_pq(ix, want, &gone); break;
    case KIND_IVF: rc = remove_ivf(ix, want, &gone); break;
    case KIND_IVPQ: rc = remove_ivpq(ix, want, &gone); break;
    case KIND_VEC: rc = remove_vec(ix, want, &gone); break;
    default: return fail(FREDDY_E_KIND, "index handle has the wrong kind for this call");
  }
  if (!rc && removed) *removed = gone;
  return rc;
}

extern "C" int freddy_gpu_remove_rows(freddy_gpu_index_t* ix, int64_t n, const int32_t* ids, int64_t* removed) {
  if (n < 0 || (n > 0 && !ids)) return fail(FREDDY_E_ARG, "bad argument: n = %lld ids%s", (long long)n, ids ? "" : ", no ids");
  if (!ix) return fail(FREDDY_E_ARG, "NULL index");
  if (removed) *removed = 0;
  if (n == 0) return FREDDY_OK;
  for (int64_t i = 0; i < n; ++i)
    if (ids[i] < 0) return fail(FREDDY_E_ARG, "id %d at position %lld is negative (-1 is the filler of a result list)", ids[i], (long long)i);
  std::vector<int32_t> want(ids, ids + n);   // any order, an id listed twice counts once
  std::sort(want.begin(), want.end());
  want.erase(std::unique(want.begin(), want.end()), want.end());
  return on_every_device(ix, [&](freddy_gpu_index* dev, bool primary) { return remove_on_device(dev, want, primary ? removed : nullptr); });
}

// ---- update_rows.  Arrays are written in place: *wrote goes up before the first write, *changed counts the rows written
static int update_pq(freddy_gpu_index* ix, int64_t n, const int32_t* ids, const int16_t* codes, int64_t* changed, bool* wrote) {
  std::vector<int32_t> rows, cell;
  std::vector<int64_t> known, slot;
  known_rows(ix->h_ids, n, ids, rows, known);
  if (rows.empty()) return 0;
  if (int rc = locate_packed_rows(ix, 1, rows, slot, cell)) return rc;   // flat table: pos = row index
  for (size_t j = 0; j < rows.size(); ++j)
    if (slot[j] < 0) return fail(FREDDY_E_HIP, "row %d has no slot: the pinned layout is inconsistent", rows[j]);
  const std::vector<int16_t> new_codes = pick_rows(codes, known, (size_t)ix->m);
  drop_pq_views(ix);
  *wrote = true;
  if (int rc = rewrite_packed_rows(ix, slot, rows, new_codes)) return rc;
  *changed = (int64_t)rows.size();
  return build_packed8(ix);
}

static int update_ivf(freddy_gpu_index* ix, int64_t n, const int32_t* ids, const int32_t* coarse_id, const int16_t* codes, int64_t* changed, bool* wrote) {
  std::vector<std::pair<int32_t, int64_t>> by_id((size_t)n);
  for (int64_t i = 0; i < n; ++i) by_id[(size_t)i] = {ids[i], i};
  std::sort(by_id.begin(), by_id.end());
  std::vector<int32_t> want((size_t)n), cell;
  for (int64_t j = 0; j < n; ++j) want[(size_t)j] = by_id[(size_t)j].first;
  std::vector<int64_t> slot;
  if (int rc = locate_packed_rows(ix, ix->C, want, slot, cell)) return rc;   // (pos holds the ids; only the device knows an id's list)
  std::vector<int64_t> stay_slot;
  std::vector<int32_t> stay_id, move_id, move_cell;
  std::vector<int16_t> stay_codes, move_codes;
  for (int64_t j = 0; j < n; ++j) {
    if (slot[(size_t)j] < 0) continue;
    const int64_t i = by_id[(size_t)j].second;
    const int16_t* row = codes + (size_t)i * ix->m;
    if (coarse_id[i] == cell[(size_t)j]) {
      stay_slot.push_back(slot[(size_t)j]); stay_id.push_back(ids[i]); stay_codes.insert(stay_codes.end(), row, row + ix->m);
    } else {
      move_id.push_back(ids[i]); move_cell.push_back(coarse_id[i]); move_codes.insert(move_codes.end(), row, row + ix->m);
    }
  }
  if (stay_id.empty() && move_id.empty()) return 0;
  const int32_t max_id = ix->max_id;
  *wrote = true;
  if (int rc = rewrite_packed_rows(ix, stay_slot, stay_id, stay_codes)) return rc;
  *changed = (int64_t)stay_id.size();
  if (!move_id.empty()) {   // out of the old lists (a stable compaction), then to the end of the new ones
    int64_t gone = 0;
    int32_t unused = -1;
    Staged out_st(ix->stream), in_st(ix->stream);
    FreshLayout out, in;
    if (int rc = remove_packed_rows(ix, out_st, ix->C, move_id, false, &gone, &unused, out)) return rc;
    if (out.ready) install_layout(ix, out_st, out);
    *changed += gone;
    if (gone != (int64_t)move_id.size()) return fail(FREDDY_E_HIP, "%lld of %zu rows left their lists: the pinned layout is inconsistent", (long long)gone, move_id.size());
    if (int rc = append_packed_rows(ix, in_st, ix->C, (int64_t)move_id.size(), move_cell.data(), move_id.data(), move_codes.data(), in)) return rc;
    install_layout(ix, in_st, in);   // (with the one-byte codes and the row terms of the final layout)
    ix->max_id = max_id;             // no id has come or gone
    return 0;
  }
  if (int rc = build_packed8(ix)) return rc;
  ix->max_id = max_id;
  return refresh_row_terms(ix);
}

static int update_ivpq(freddy_gpu_index* ix, int64_t n, const int32_t* ids, const int32_t* coarse_id, const int16_t* codes, const float* vectors, int64_t* changed,
                       bool* wrote) {
  JoinIndex& j = ix->join;
  std::vector<int32_t> rows;
  std::vector<int64_t> known;
  known_rows(j.h_ids, n, ids, rows, known);
  if (rows.empty()) return 0;
  const size_t k = rows.size();
  const std::vector<int32_t> new_cell = pick_rows(coarse_id, known, 1);
  const std::vector<int16_t> new_codes = pick_rows(codes, known, (size_t)j.m);
  const std::vector<float> new_vec = j.has_vectors ? pick_rows(vectors, known, (size_t)j.d) : std::vector<float>();
  Staged tmp(ix->stream);
  int32_t* d_rows = tmp.put(rows.data(), k);
  if (!d_rows) return fail(FREDDY_E_NOMEM, "device allocation failed while updating rows");
  j.tl_valid = false;   // (the cached target lists are bucketed by cell)
  *wrote = true;
  int rc = scatter_rows(ix, tmp, new_cell.data(), (int64_t)k, 1, d_rows, j.cell);
  if (!rc) rc = scatter_rows(ix, tmp, join_pad_codes(new_codes.data(), (int64_t)k, j.m, j.MP).data(), (int64_t)k, j.MP, d_rows, j.codes);
  if (!rc && j.has_vectors) rc = scatter_rows(ix, tmp, new_vec.data(), (int64_t)k, j.d, d_rows, j.vectors);
  if (!rc) *changed = (int64_t)k;
  if (tmp.sync() != hipSuccess && !rc) rc = fail(FREDDY_E_HIP, "rewriting the ivpq rows failed");
  if (rc) return rc;
  for (size_t r = 0; r < k; ++r) j.h_cell[(size_t)rows[r]] = new_cell[r];
  return 0;
}

static int update_vec(freddy_gpu_index* ix, int64_t n, const int32_t* ids, const float* vectors, int64_t* changed, bool* wrote) {
  std::vector<int32_t> rows;
  std::vector<int64_t> known;
  known_rows(ix->h_ids, n, ids, rows, known);
  if (rows.empty()) return 0;
  const size_t k = rows.size();
  const int d = ix->d;
  const std::vector<float> new_vec = pick_rows(vectors, known, (size_t)d);
  {
    Staged tmp(ix->stream);
    int32_t* d_rows = tmp.put(rows.data(), k);
    float* d_src = tmp.put(new_vec.data(), new_vec.size());
    if (!d_rows || !d_src) return fail(FREDDY_E_NOMEM, "device allocation failed while updating rows");
    *wrote = true;
    hipLaunchKernelGGL(up_scatter_rows_kernel, dim3((unsigned)(((int64_t)k * d + 255) / 256)), dim3(256), 0, ix->stream, reinterpret_cast<const uint32_t*>(d_src),
                       reinterpret_cast<uint32_t*>(ix->coarse), d_rows, (int64_t)k, d);
    hipLaunchKernelGGL(up_place_vectors_kernel, dim3((unsigned)k), dim3(256), 0, ix->stream, d_src, d_rows, (int64_t)k, ix->xb, d);
    tmp.in_flight = true;
    *changed = (int64_t)k;
    if (hipGetLastError() != hipSuccess || tmp.sync() != hipSuccess) return fail(FREDDY_E_HIP, "rewriting the vector rows failed");
  }
  // the exact filter's state over all rows, as a fresh pin computes it (the old values have left the statistics); the fragment
  // copy: the strips of the updated rows, or every strip when the scale moved or the filter came back
  std::vector<int32_t> strips;
  for (int32_t r : rows)
    if (strips.empty() || strips.back() != r / 32) strips.push_back(r / 32);
  return exf_table_stats(ix, 0, ix->N, &strips);
}

static int update_on_device(freddy_gpu_index* ix, int64_t n, const int32_t* ids, const int32_t* coarse_id, const int16_t* codes, const float* vectors, int64_t* updated) {
  int64_t changed = 0;
  bool wrote = false;
  int rc = 0;
  switch (ix->kind) {
    case KIND_PQ: rc = update_pq(ix, n, ids, codes, &changed, &wrote); break;
    case KIND_IVF: rc = update_ivf(ix, n, ids, coarse_id, codes, &changed, &wrote); break;
    case KIND_IVPQ: rc = update_ivpq(ix, n, ids, coarse_id, codes, vectors, &changed, &wrote); break;
    case KIND_VEC: rc = update_vec(ix, n, ids, vectors, &changed, &wrote); break;
    default: return fail(FREDDY_E_KIND, "index handle has the wrong kind for this call");
  }
  if (rc) {
    if (wrote) ix->poisoned = true;   // a failure after the first write leaves a table that is neither the old nor the new one
    return rc;
  }
  if (updated) *updated = changed;
  return FREDDY_OK;
}

extern "C" int freddy_gpu_update_rows(freddy_gpu_index_t* ix, int64_t n, const int32_t* ids, const int32_t* coarse_id, const int16_t* codes,
                                      const float* vectors, int64_t* updated) {
  if (n < 0 || (n > 0 && !ids)) return fail(FREDDY_E_ARG, "bad argument: n = %lld ids%s", (long long)n, ids ? "" : ", no ids");
  if (!ix) return fail(FREDDY_E_ARG, "NULL index");
  if (updated) *updated = 0;
  if (n == 0) return FREDDY_OK;
  // everything that can be refused is refused here, before any device has changed
  if (n > (int64_t)INT32_MAX) return fail(FREDDY_E_LIMIT, "n = %lld: one call updates at most %d rows (there are no more distinct ids)", (long long)n, INT32_MAX);
  for (int64_t i = 0; i < n; ++i)
    if (ids[i] < 0) return fail(FREDDY_E_ARG, "id %d at position %lld is negative (-1 is the filler of a result list)", ids[i], (long long)i);
  {
    std::vector<std::pair<int32_t, int64_t>> by_id((size_t)n);
    for (int64_t i = 0; i < n; ++i) by_id[(size_t)i] = {ids[i], i};
    std::sort(by_id.begin(), by_id.end());
    for (int64_t i = 1; i < n; ++i)
      if (by_id[(size_t)i].first == by_id[(size_t)i - 1].first)
        return fail(FREDDY_E_ARG, "id %d is listed twice, at positions %lld and %lld: which payload would win is undefined", by_id[(size_t)i].first,
                    (long long)by_id[(size_t)i - 1].second, (long long)by_id[(size_t)i].second);
  }
  const bool flat = ix->kind == KIND_PQ, ivf = ix->kind == KIND_IVF, ivpq = ix->kind == KIND_IVPQ, vec = ix->kind == KIND_VEC;
  if (!flat && !ivf && !ivpq && !vec) return fail(FREDDY_E_KIND, "index handle has the wrong kind for this call");
  if (flat && !codes) return fail(FREDDY_E_ARG, "codes are required");
  if (ivf && (!codes || !coarse_id)) return fail(FREDDY_E_ARG, "coarse_id and codes are required");
  if (ivpq && (!codes || !coarse_id || (ix->join.has_vectors && !vectors))) return fail(FREDDY_E_ARG, "coarse_id, codes (and vectors, if pinned) are required");
  if (vec && !vectors) return fail(FREDDY_E_ARG, "vectors are required");
  if (!vec) {
    const int m = ivpq ? ix->join.m : ix->m, K = ivpq ? ix->join.K : ix->K, cells = ivpq ? ix->join.cells : ix->C;
    if (int rc = check_payload(UPDATE_ROW, n, flat ? nullptr : coarse_id, cells, codes, m, K)) return rc;
  }
  int64_t changed = 0;
  if (int rc = on_every_device(ix, [&](freddy_gpu_index* dev, bool primary) { return update_on_device(dev, n, ids, coarse_id, codes, vectors, primary ? &changed : nullptr); }))
    return rc;
  if (updated) *updated = changed;   // (only once every replica has followed)
  return FREDDY_OK;
}
