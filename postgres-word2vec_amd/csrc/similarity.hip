// similarity.hip -- cosine similarities of rows named by id on a raw-vector handle (similarity.h): pairs, matrices, joins.  The A side
// of a matrix is gathered by row number (query_ids.h) or staged from the caller's floats.
#include "internal.h"

#include "similarity.h"
#include "query_ids.h"

// ---- similarities by row id: pairs, matrices, joins (similarity.h) ----------------------------------------------------------
static constexpr int64_t SIM_PAIR_PASS = (int64_t)1 << 22;        // pairs per pass: the ids go up and the values come back through buffers of this many entries
static constexpr size_t SIM_PASS_BYTES = (size_t)256 << 20;       // the device result block of a pass of A rows (option similarity_pass_bytes)
static constexpr int SIM_PASS_ROWS = 65536;                       // and its A rows at most (their staged copy: 4 d bytes each)

extern "C" int freddy_gpu_similarity_pairs(freddy_gpu_index_t* ix, const int32_t* ids_a, const int32_t* ids_b, int64_t n, float* out_sim,
                                           uint8_t* out_known) {
  if (n < 0) return fail(FREDDY_E_ARG, "bad sizes (n=%lld)", (long long)n);
  if (n > 0 && (!ids_a || !ids_b || !out_sim || !out_known)) return fail(FREDDY_E_ARG, "NULL buffer");
  if (int rc = check_vec_handle(ix)) return rc;
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
  if (int rc = check_vec_handle(ix)) return rc;
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
  if (int rc = check_vec_handle(ix)) return rc;
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
