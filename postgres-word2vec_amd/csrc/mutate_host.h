// mutate_host.h -- what freddy_gpu_append_rows / remove_rows / update_rows (mutate.h) share on the host:
//   Staged          the one owner of every device array a call builds BESIDE the pinned ones, scratch included
//   FreshLayout     a block layout staged that way (plan_blocks, block_plan.h -> stage_plan -> finish_layout -> install_layout)
//   append_packed_rows / remove_packed_rows     a pq / ivf handle's lists extended / compacted into a FreshLayout
//   locate_packed_rows / rewrite_packed_rows / scatter_rows     the in-place writes of an update
//   check_payload, on_every_device              the one payload check and the one replica fan-out
// The rule they serve: a failed call leaves the handle as it was, or poisoned -- never in between.  So a call STAGES everything
// that can fail into a Staged, and COMMITS with steps that cannot: Staged::install, install_layout and host-vector edits.
#pragma once
#include "internal.h"
#include "block_plan.h"
#include "mutate_kernels.h"
#include "remove_kernels.h"
#include "update_kernels.h"

// ---- pin.hip: the arrays that follow a block layout, built beside the handle's ----
static int make_packed8(const freddy_gpu_index* ix, const uint32_t* packed, int64_t n_blocks, uint32_t** out, int64_t* out_bytes);
static void install_packed8(freddy_gpu_index* ix, uint32_t* p8, int64_t bytes);
static int make_row_terms(const freddy_gpu_index* ix, const uint32_t* packed, const int32_t* blk_cell, int64_t n_blocks, const float* cbR, float** out, int64_t* out_bytes);
static void install_row_terms(freddy_gpu_index* ix, float* rterm, int64_t bytes);
static int build_packed8(freddy_gpu_index* ix);       // ... and rebuilt from the handle's own arrays, once an update has rewritten them in place
static int refresh_row_terms(freddy_gpu_index* ix);

// Device arrays of one call.  Whatever has not been released to the handle (install / take) is freed when the record goes out of
// scope -- after the stream has drained, if work enqueued on it (a gather, a scatter) may still touch one of the arrays.  One
// dev_malloc per array; an array of no elements is one element long, as upload() sizes it.
struct Staged {
  hipStream_t stream;
  std::vector<void*> held;
  bool in_flight = false;     // set by whoever enqueues work on `stream` over a held array without waiting for it
  bool copy_failed = false;   // the NULL just returned came from a copy, not from the allocator
  explicit Staged(hipStream_t s) : stream(s) { held.reserve(16); }
  Staged(const Staged&) = delete;
  Staged& operator=(const Staged&) = delete;
  ~Staged() {
    if (in_flight) (void)hipStreamSynchronize(stream);
    for (void* p : held) if (p) (void)dev_free(p);
  }
  hipError_t sync() { in_flight = false; return hipStreamSynchronize(stream); }
  template <class T> T* adopt(T* p) { if (p) held.push_back(p); return p; }   // an array somebody else allocated (make_packed8, make_row_terms)
  template <class T> T* empty(size_t n) {
    void* p = nullptr;
    if (dev_malloc(&p, (size_t)counted_bytes<T>(n)) != hipSuccess) { copy_failed = false; return nullptr; }
    return adopt(static_cast<T*>(p));
  }
  template <class T> T* put(const T* src, size_t n) {   // n elements from the host
    T* p = empty<T>(n);
    if (p && n && hipMemcpy(p, src, sizeof(T) * n, hipMemcpyHostToDevice) != hipSuccess) { copy_failed = true; return nullptr; }
    return p;
  }
  template <class T> T* grown(const T* arr, size_t old_n, const T* tail, size_t tail_n) {   // the old_n elements of a device array, then tail_n from the host
    T* p = empty<T>(old_n + tail_n);
    if (p && ((old_n && hipMemcpy(p, arr, sizeof(T) * old_n, hipMemcpyDeviceToDevice) != hipSuccess) ||
              (tail_n && hipMemcpy(p + old_n, tail, sizeof(T) * tail_n, hipMemcpyHostToDevice) != hipSuccess))) { copy_failed = true; return nullptr; }
    return p;
  }
  template <class T> T* take(T* p) {   // p is the caller's from now on
    for (void*& h : held) if (h == p) h = nullptr;
    return p;
  }
  // The commit step: the handle's array gives way to a staged one (NULL: to none).  Cannot fail.
  template <class T> void install(T*& slot, T* fresh) {
    if (slot) (void)dev_free(slot);
    slot = take(fresh);
  }
  // ... of an array that upload() counted, going from old_n to new_n elements (an array the handle did not hold counted nothing)
  template <class T> void install(T*& slot, T* fresh, size_t old_n, size_t new_n, int64_t* bytes) {
    *bytes += (fresh ? counted_bytes<T>(new_n) : 0) - (slot ? counted_bytes<T>(old_n) : 0);
    install(slot, fresh);
  }
};
static int grow_failed(const Staged& st) { return st.copy_failed ? fail(FREDDY_E_HIP, "copying the rows failed") : fail(FREDDY_E_NOMEM, "device allocation failed while appending rows"); }

// the footprint of the three arrays of a block layout that follow the block count (blk_off and list_off follow the list count)
static int64_t layout_bytes(int M2, int64_t n_blocks) {
  const size_t nb = (size_t)alloc_blocks(n_blocks);
  return counted_bytes<uint32_t>(nb * M2 * 64) + counted_bytes<int32_t>(nb * 64) + counted_bytes<int32_t>(nb);
}
// ... and of a vector handle's blocked copy xb (pin_vectors counts one block at least)
static int64_t xb_bytes(int d, int64_t n_blocks) { return counted_bytes<float>((size_t)alloc_blocks(n_blocks) * d * 64); }

// The arrays of a pq / ivf handle that follow its rows -- the block layout, the one-byte codes and (ivf) the row terms -- as
// append_packed_rows / remove_packed_rows stage them: pointers into the call's Staged, and the layout's scalars.  install_layout
// swaps them in, and only then does the handle change.
struct FreshLayout {
  uint32_t *packed = nullptr, *packed8 = nullptr;
  int32_t *pos = nullptr, *blk_cell = nullptr, *blk_off = nullptr, *list_off = nullptr;
  float* rterm = nullptr;
  int64_t packed8_bytes = 0, rterm_bytes = 0, N = 0;
  BlockPlan plan;          // n_blocks, max_list_blocks, and list_off for the host
  bool ready = false;      // complete: install_layout may run (false after a call that found nothing to change)
};
// A plan's three index arrays and empty packed / pos of its size, staged; the layout's scalars.  `doing`: "appending" / "removing"
static int stage_plan(const freddy_gpu_index* ix, Staged& st, BlockPlan& plan, int64_t N, FreshLayout& L, const char* doing) {
  const size_t nb = (size_t)alloc_blocks(plan.n_blocks);
  if (!(L.packed = st.empty<uint32_t>(nb * ix->M2 * 64)) || !(L.pos = st.empty<int32_t>(nb * 64)) ||
      !(L.blk_cell = st.put(plan.blk_cell.data(), plan.blk_cell.size())) || !(L.blk_off = st.put(plan.blk_off.data(), plan.blk_off.size())) ||
      !(L.list_off = st.put(plan.list_off.data(), plan.list_off.size())))
    return fail(FREDDY_E_NOMEM, "device allocation failed while %s rows", doing);
  L.plan = std::move(plan);
  L.N = N;
  return 0;
}
// what follows from the fresh block arrays: the one-byte codes, and the row terms of an ivf handle
static int finish_layout(freddy_gpu_index* ix, Staged& st, FreshLayout& L) {
  int rc = 0;
  if (!ix->shadow_of) { rc = make_packed8(ix, L.packed, L.plan.n_blocks, &L.packed8, &L.packed8_bytes); st.adopt(L.packed8); }
  if (!rc && ix->kind == KIND_IVF) { rc = make_row_terms(ix, L.packed, L.blk_cell, L.plan.n_blocks, ix->cbR, &L.rterm, &L.rterm_bytes); st.adopt(L.rterm); }
  L.ready = !rc;
  return rc;
}
static void install_layout(freddy_gpu_index* ix, Staged& st, FreshLayout& L) {
  ix->bytes += layout_bytes(ix->M2, L.plan.n_blocks) - layout_bytes(ix->M2, ix->n_blocks);
  st.install(ix->packed, L.packed); st.install(ix->pos, L.pos); st.install(ix->blk_cell, L.blk_cell);
  st.install(ix->blk_off, L.blk_off); st.install(ix->list_off, L.list_off);
  ix->n_blocks = L.plan.n_blocks;
  ix->max_list_blocks = L.plan.max_list_blocks;
  ix->h_list_off.swap(L.plan.list_off);
  ix->N = L.N;
  if (!ix->shadow_of) install_packed8(ix, st.take(L.packed8), L.packed8_bytes);
  if (ix->kind == KIND_IVF) install_row_terms(ix, st.take(L.rterm), L.rterm_bytes);
  L.ready = false;
}

// ---- // insert_batch: HBM index mutation
// rows of a pq / ivf index (payload checked by the caller): each new row goes to the end of its list; the 64-row block layout is
// rebuilt on the device (old blocks copied to their new places, new rows written into the free slots behind them) into L; the
// handle is not touched
static int append_packed_rows(freddy_gpu_index* ix, Staged& st, int n_lists, int64_t n, const int32_t* cell /*NULL: list 0*/, const int32_t* row_pos,
                              const int16_t* codes, FreshLayout& L) {
  const int m = ix->m, M2 = ix->M2;
  const std::vector<int32_t>& old_off = ix->h_list_off;
  std::vector<int32_t> add((size_t)n_lists, 0);
  for (int64_t i = 0; i < n; ++i) add[(size_t)(cell ? cell[i] : 0)]++;
  BlockPlan plan;
  int bad = 0;
  if (plan_blocks(n_lists, [&](int c) { return (int64_t)old_off[(size_t)c + 1] - old_off[(size_t)c] + add[(size_t)c]; }, plan, &bad))
    return fail(FREDDY_E_LIMIT, "N too large for 32-bit row positions");
  std::vector<int64_t> slot((size_t)n);
  std::vector<int32_t> cursor((size_t)n_lists, 0);
  for (int64_t i = 0; i < n; ++i) {
    const int c = cell ? cell[i] : 0;
    const int64_t old_len = old_off[(size_t)c + 1] - old_off[(size_t)c];
    slot[(size_t)i] = (int64_t)plan.blk_off[(size_t)c] * 64 + old_len + cursor[(size_t)c]++;
  }
  if (int rc = stage_plan(ix, st, plan, ix->N + n, L, "appending")) return rc;
  int64_t* d_slot = nullptr;
  int32_t* d_row_pos = nullptr;
  int16_t* d_codes = nullptr;
  if (!(d_slot = st.put(slot.data(), slot.size())) || !(d_row_pos = st.put(row_pos, (size_t)n)) || !(d_codes = st.put(codes, (size_t)n * m)))
    return fail(FREDDY_E_NOMEM, "device allocation failed while appending rows");
  if (const int64_t nb = L.plan.n_blocks; nb > 0) {
    hipLaunchKernelGGL(repack_blocks_kernel, dim3((unsigned)((nb + 3) / 4)), dim3(256), 0, ix->stream, ix->packed, ix->pos, ix->blk_off, L.blk_off, L.blk_cell,
                       L.packed, L.pos, nb, M2);
    if (n > 0)
      hipLaunchKernelGGL(place_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ix->stream, d_slot, d_row_pos, d_codes, n, L.packed, L.pos, m, M2);
    st.in_flight = true;
    if (hipGetLastError() != hipSuccess || st.sync() != hipSuccess) return fail(FREDDY_E_HIP, "re-blocking the lists failed");
  }
  return finish_layout(ix, st, L);
}

// ---- // remove_rows: the DELETE beside insert_batch's INSERTs (kernels in remove_kernels.h)
// rows `rows` (ascending, distinct) out of a host array of `e` elements per row
template <class T>
static void erase_rows(std::vector<T>& a, const std::vector<int32_t>& rows, size_t e = 1) {
  size_t w = (size_t)rows[0], next = 0;
  const size_t n = a.size() / e;
  for (size_t r = (size_t)rows[0]; r < n; ++r) {
    if (next < rows.size() && (size_t)rows[next] == r) { ++next; continue; }
    if (w != r) std::copy(a.begin() + r * e, a.begin() + (r + 1) * e, a.begin() + w * e);
    ++w;
  }
  a.resize(w * e);
}

// A staged array of the rows that stay (n_new rows of e elements of T, a whole number of 4-byte words), the gather enqueued on
// st.stream and NOT waited for: st drains the stream before it frees anything.
template <class T>
static int gather_rows(Staged& st, const T* src, int64_t n_new, int e, const int32_t* d_rm, int n_rm, T** out) {
  if (!(*out = st.empty<T>((size_t)n_new * e))) return fail(FREDDY_E_NOMEM, "device allocation failed while removing rows");
  if (n_new > 0) {
    hipLaunchKernelGGL(rm_gather_rows_kernel, dim3((unsigned)((n_new + 63) / 64)), dim3(256), 0, st.stream, reinterpret_cast<const uint32_t*>(src),
                       reinterpret_cast<uint32_t*>(*out), d_rm, n_rm, n_new, (int)(sizeof(T) * e / 4));
    st.in_flight = true;
    HIP_TRY(hipGetLastError());
  }
  return 0;
}

// rows of a pq / ivf index: every slot whose pos is in `rm` (ascending, distinct: ids of an ivf handle, row indices of the flat
// table) leaves; the rows that stay keep their order inside their list.  The new block layout is built beside the old one on
// the device; nothing is built when no slot matches.  *removed: the rows that left; *max_pos: the largest pos
// that stays (-1: none).  The lists lose part of arrange_list_rows' bank-conflict arrangement (speed only).
// Everything is staged into st / L: the handle is not touched, and L.ready stays false when there is nothing to change.
static int remove_packed_rows(freddy_gpu_index* ix, Staged& st, int n_lists, const std::vector<int32_t>& rm, bool renumber, int64_t* removed, int32_t* max_pos,
                              FreshLayout& L) {
  const int M2 = ix->M2;
  const int64_t ob = ix->n_blocks;
  *removed = 0;
  if (ob <= 0 || rm.empty()) return 0;
  const int32_t minus_one = -1;
  int32_t* d_rm = st.put(rm.data(), rm.size());
  unsigned long long* keep_mask = st.empty<unsigned long long>((size_t)ob);
  int32_t *keep_cnt = st.empty<int32_t>((size_t)ob), *prefix = st.empty<int32_t>((size_t)ob), *list_keep = st.empty<int32_t>((size_t)n_lists);
  int32_t* d_max = st.put(&minus_one, 1);
  if (!d_rm || !keep_mask || !keep_cnt || !prefix || !list_keep || !d_max) return fail(FREDDY_E_NOMEM, "device allocation failed while removing rows");
  hipLaunchKernelGGL(rm_mark_kernel, dim3((unsigned)((ob + 3) / 4)), dim3(256), 0, ix->stream, ix->pos, ob, d_rm, (int)rm.size(), keep_mask, keep_cnt, d_max);
  hipLaunchKernelGGL(rm_list_scan_kernel, dim3((unsigned)n_lists), dim3(256), 0, ix->stream, ix->blk_off, keep_cnt, prefix, list_keep);
  HIP_TRY(hipGetLastError());
  std::vector<int32_t> keep((size_t)n_lists);
  HIP_TRY(hipMemcpyAsync(keep.data(), list_keep, sizeof(int32_t) * (size_t)n_lists, hipMemcpyDeviceToHost, ix->stream));
  HIP_TRY(hipMemcpyAsync(max_pos, d_max, sizeof(int32_t), hipMemcpyDeviceToHost, ix->stream));
  HIP_TRY(st.sync());
  for (int c = 0; c < n_lists; ++c)
    if (keep[(size_t)c] < 0 || keep[(size_t)c] > ix->h_list_off[(size_t)c + 1] - ix->h_list_off[(size_t)c])
      return fail(FREDDY_E_HIP, "list %d keeps %d of its %d rows: the pinned layout is inconsistent", c, keep[(size_t)c], ix->h_list_off[(size_t)c + 1] - ix->h_list_off[(size_t)c]);
  BlockPlan plan;
  int bad = 0;
  if (plan_blocks(n_lists, [&](int c) { return (int64_t)keep[(size_t)c]; }, plan, &bad)) return fail(FREDDY_E_LIMIT, "N too large for 32-bit row positions");
  const int64_t kept = plan.rows();
  if (kept == ix->N) return 0;   // (no pinned row has one of the ids)
  if (int rc = stage_plan(ix, st, plan, kept, L, "removing")) return rc;
  if (L.plan.n_blocks == 0) {   // (an empty table keeps one block of padding, as pack_lists leaves it)
    if (hipMemsetAsync(L.packed, 0, sizeof(uint32_t) * (size_t)M2 * 64, ix->stream) != hipSuccess || hipMemsetAsync(L.pos, 0xff, sizeof(int32_t) * 64, ix->stream) != hipSuccess)
      return fail(FREDDY_E_HIP, "clearing the empty table failed");
  } else {
    hipLaunchKernelGGL(rm_scatter_kernel, dim3((unsigned)((ob + 3) / 4)), dim3(256), 0, ix->stream, ix->packed, ix->pos, ix->blk_cell, L.blk_off, keep_mask,
                       prefix, ob, L.plan.n_blocks * 64, M2, renumber ? 1 : 0, L.packed, L.pos);
    hipLaunchKernelGGL(rm_fill_tail_kernel, dim3((unsigned)((n_lists + 3) / 4)), dim3(256), 0, ix->stream, L.list_off, L.blk_off, n_lists, M2, L.packed, L.pos);
  }
  st.in_flight = true;
  if (hipGetLastError() != hipSuccess || st.sync() != hipSuccess) return fail(FREDDY_E_HIP, "compacting the lists failed");
  if (int rc = finish_layout(ix, st, L)) return rc;
  *removed = ix->N - kept;
  return 0;
}

// ---- // update_rows: the UPDATE of a row -- the id stays, the payload changes (kernels in update_kernels.h)
// rows [known[0]], [known[1]], ... of a host array of e elements per row
template <class T>
static std::vector<T> pick_rows(const T* src, const std::vector<int64_t>& known, size_t e) {
  std::vector<T> out(known.size() * e);
  for (size_t r = 0; r < known.size(); ++r) std::copy(src + (size_t)known[r] * e, src + (size_t)(known[r] + 1) * e, out.begin() + r * e);
  return out;
}
// known[] = positions (in the caller's arrays) of the ids a row of the flat table h_ids has, rows[] = their row indices -- both in
// ascending row order
static void known_rows(const std::vector<int32_t>& h_ids, int64_t n, const int32_t* ids, std::vector<int32_t>& rows, std::vector<int64_t>& known) {
  std::vector<std::pair<int32_t, int64_t>> hit;
  for (int64_t i = 0; i < n; ++i)
    if (const int32_t r = row_of(h_ids, ids[i]); r >= 0) hit.emplace_back(r, i);
  std::sort(hit.begin(), hit.end());
  for (auto& h : hit) { rows.push_back(h.first); known.push_back(h.second); }
}

// The slots (block * 64 + lane) and lists of the rows whose pos is one of `upd` (ascending, distinct), -1 where no slot has it.
// Synchronises the stream.  Every pair is checked against the layout before the caller hands it to a kernel.
static int locate_packed_rows(freddy_gpu_index* ix, int n_lists, const std::vector<int32_t>& upd, std::vector<int64_t>& slot, std::vector<int32_t>& cell) {
  const size_t n = upd.size();
  slot.assign(n, -1);
  cell.assign(n, 0);
  if (ix->n_blocks <= 0 || n == 0) return 0;
  Staged tmp(ix->stream);
  int32_t* d_upd = tmp.put(upd.data(), n);
  int64_t* d_slot = tmp.empty<int64_t>(n);
  int32_t* d_cell = tmp.empty<int32_t>(n);
  if (!d_upd || !d_slot || !d_cell) return fail(FREDDY_E_NOMEM, "device allocation failed while updating rows");
  tmp.in_flight = true;
  HIP_TRY(hipMemsetAsync(d_slot, 0xff, sizeof(int64_t) * n, ix->stream));
  HIP_TRY(hipMemsetAsync(d_cell, 0, sizeof(int32_t) * n, ix->stream));
  hipLaunchKernelGGL(up_locate_kernel, dim3((unsigned)((ix->n_blocks + 3) / 4)), dim3(256), 0, ix->stream, ix->pos, ix->blk_cell, ix->n_blocks, d_upd, (int)n,
                     d_slot, d_cell);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(slot.data(), d_slot, sizeof(int64_t) * n, hipMemcpyDeviceToHost, ix->stream));
  HIP_TRY(hipMemcpyAsync(cell.data(), d_cell, sizeof(int32_t) * n, hipMemcpyDeviceToHost, ix->stream));
  HIP_TRY(tmp.sync());
  for (size_t j = 0; j < n; ++j)
    if (slot[j] < -1 || slot[j] >= ix->n_blocks * 64 || (slot[j] >= 0 && (cell[j] < 0 || cell[j] >= n_lists)))
      return fail(FREDDY_E_HIP, "row %d sits in slot %lld of list %d: the pinned layout is inconsistent", upd[j], (long long)slot[j], cell[j]);
  return 0;
}

// the code words of n rows rewritten in their slots (pos keeps its value: row_pos[i] is what the slot holds already)
static int rewrite_packed_rows(freddy_gpu_index* ix, const std::vector<int64_t>& slot, const std::vector<int32_t>& row_pos, const std::vector<int16_t>& codes) {
  const size_t n = slot.size();
  if (n == 0) return 0;
  Staged tmp(ix->stream);
  int64_t* d_slot = tmp.put(slot.data(), n);
  int32_t* d_pos = tmp.put(row_pos.data(), n);
  int16_t* d_codes = tmp.put(codes.data(), codes.size());
  if (!d_slot || !d_pos || !d_codes) return fail(FREDDY_E_NOMEM, "device allocation failed while updating rows");
  hipLaunchKernelGGL(place_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ix->stream, d_slot, d_pos, d_codes, (int64_t)n, ix->packed, ix->pos, ix->m, ix->M2);
  tmp.in_flight = true;
  if (hipGetLastError() != hipSuccess || tmp.sync() != hipSuccess) return fail(FREDDY_E_HIP, "rewriting the rows' codes failed");
  return 0;
}

// dst row rows[j] <- the j-th of n host rows of e elements of T (a whole number of 4-byte words), enqueued on the stream
template <class T>
static int scatter_rows(freddy_gpu_index* ix, Staged& tmp, const T* h_src, int64_t n, int e, const int32_t* d_rows, T* dst) {
  T* d_src = tmp.put(h_src, (size_t)n * e);
  if (!d_src) return fail(FREDDY_E_NOMEM, "device allocation failed while updating rows");
  const int wpr = (int)(sizeof(T) * e / 4);
  hipLaunchKernelGGL(up_scatter_rows_kernel, dim3((unsigned)((n * wpr + 255) / 256)), dim3(256), 0, ix->stream, reinterpret_cast<const uint32_t*>(d_src),
                     reinterpret_cast<uint32_t*>(dst), d_rows, n, wpr);
  tmp.in_flight = true;
  HIP_TRY(hipGetLastError());
  return 0;
}

// ---- // what the three entry points share
// The payload of n rows: coarse ids (NULL: the flat table has none) in [0, cells), every code in [0, K).  Worded as each of the
// three callers always has.
enum PayloadWording { NEW_PACKED_ROW, NEW_IVPQ_ROW, UPDATE_ROW };
static int check_payload(PayloadWording w, int64_t n, const int32_t* coarse_id, int cells, const int16_t* codes, int m, int K) {
  for (int64_t i = 0; i < n; ++i) {
    if (coarse_id && (coarse_id[i] < 0 || coarse_id[i] >= cells))
      return w == NEW_IVPQ_ROW ? fail(FREDDY_E_ARG, "coarse_id %d out of range", coarse_id[i])
                               : fail(FREDDY_E_ARG, "coarse_id %d of %s row %lld is outside [0, %d)", coarse_id[i], w == UPDATE_ROW ? "update" : "new", (long long)i, cells);
    for (int l = 0; l < m; ++l) {
      const int code = codes[(size_t)i * m + l];
      if (code >= 0 && code < K) continue;
      if (w == NEW_IVPQ_ROW) return fail(FREDDY_E_ARG, "code out of range at new row %lld", (long long)i);
      if (w == NEW_PACKED_ROW) return fail(FREDDY_E_ARG, "code %d of new row %lld is outside [0, %d)", code, (long long)i, K);
      return fail(FREDDY_E_ARG, "code %d of update row %lld position %d is outside [0, %d)", code, (long long)i, l, K);
    }
  }
  return 0;
}

// Every replica holds the same tables, so a mutation runs on every device: op(handle of one device, is it the primary).  The primary
// goes first (what it refuses is refused before anything has changed anywhere; if it fails it is as it was, or has poisoned
// itself); a failure after that leaves the devices with different tables -> the handle is poisoned and every search on it fails
// loudly until it is unpinned.  (freddy_gpu_update_codebook keeps an order of its own, pin.hip.)
template <class Op>
static int on_every_device(freddy_gpu_index* ix, Op op) {
  auto on = [&](freddy_gpu_index* dev) {   // the device's own searches have drained before its tables change
    HIP_TRY(hipSetDevice(dev->device));
    HIP_TRY(hipStreamSynchronize(dev->stream));
    return op(dev, dev == ix);
  };
  if (int rc = on(ix)) return rc;
  for (freddy_gpu_index* r : ix->replicas)
    if (int rc = on(r)) { ix->poisoned = true; return rc; }
  return FREDDY_OK;
}
