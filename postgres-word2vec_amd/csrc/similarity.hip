// similarity.hip -- cosine similarities of rows named by id on a raw-vector handle (similarity.h): pairs, matrices, joins.  The A side
// of a matrix is gathered by row number (query_ids.h) or staged from the caller's floats.
#include "internal.h"

#include "similarity.h"
#include "similarity_filter.h"
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
// The three steps are separate because the filter path of the join (option similarity_filter) stages passes of its own size and hands
// single ranges of A rows back to sim_matrix_range: sim_begin (B's ids, the buffers; stage_rows: the largest pass anyone will stage),
// sim_stage_a (the A rows [a0, a0 + n) into w_q, their known bytes into w_used), sim_matrix_range (today's sub-passes over a range).
struct SimRun {
  freddy_gpu_index* ix = nullptr;
  Workspace* ws = nullptr;
  hipStream_t s = nullptr;
  const int32_t* a_ids = nullptr;
  const float* a_vectors = nullptr;
  uint8_t* known_a = nullptr;
  int32_t na = 0;
  int nb = 0;
  int64_t rows = 0;            // A rows per pass of sim_matrix_range
  std::vector<uint8_t> ka;     // the staged pass's known bytes (a_ids)
  ~SimRun() { if (s) (void)hipStreamSynchronize(s); }
};

static int sim_begin(SimRun& r, freddy_gpu_index* ix, const int32_t* a_ids, const float* a_vectors, int32_t na, const int32_t* b_ids, int nb,
                     uint8_t* known_a, uint8_t* known_b, bool* launched, int64_t stage_rows) {
  const std::vector<int32_t>& h_ids = ix->h_ids;
  const int d = ix->d;
  r.ix = ix; r.a_ids = a_ids; r.a_vectors = a_vectors; r.known_a = known_a; r.na = na; r.nb = nb;
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
  r.ws = ws;
  // rows of A per pass: the block within the budget, a multiple of 16 rows (16 at least, whatever the budget)
  const size_t budget = ix->tune.similarity_pass_bytes > 0 ? (size_t)ix->tune.similarity_pass_bytes : SIM_PASS_BYTES;
  int64_t rows = (int64_t)(budget / (sizeof(float) * (size_t)nb)) / TILE_QT * TILE_QT;
  rows = std::max<int64_t>(TILE_QT, std::min<int64_t>(rows, SIM_PASS_ROWS));
  if (rows > na) rows = na;
  r.rows = rows;
  const int64_t staged = std::max(rows, std::min<int64_t>(stage_rows, na));
  if (ws->w_sub_rows.ensure(sizeof(int32_t) * (size_t)nb) || ws->w_sub_pos.ensure(sizeof(int32_t) * (size_t)nb) || ws->w_found.ensure((size_t)nb) ||
      ws->w_q.ensure(sizeof(float) * (size_t)staged * d) || ws->w_lut.ensure(sizeof(float) * (size_t)rows * nb))
    return fail(FREDDY_E_NOMEM, "workspace allocation failed");
  r.s = s;   // (from here on ~SimRun drains the stream: a pass that fails half-way leaves copies from `ka` and the caller's arrays enqueued)
  if (a_ids) {
    if (ws->w_used.ensure((size_t)staged)) return fail(FREDDY_E_NOMEM, "workspace allocation failed");
    if (ix->hio_in.ensure(sizeof(int32_t) * (size_t)staged)) return fail(FREDDY_E_NOMEM, "pinned staging allocation failed");
    r.ka.resize((size_t)staged);
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
  return 0;
}

// The A rows [a0, a0 + n) into w_q (the last pass has been synchronised: the pinned block is free); *n_known: how many have a row.
static int sim_stage_a(SimRun& r, int64_t a0, int n, int* n_known) {
  freddy_gpu_index* ix = r.ix;
  Workspace* ws = r.ws;
  const int d = ix->d;
  if (n_known) *n_known = n;
  if (r.a_ids) {
    int32_t* h_rows = ix->hio_in.as<int32_t>();
    int have = 0;
    for (int i = 0; i < n; ++i) {
      h_rows[i] = row_of_near(ix->h_ids, r.a_ids[a0 + i]);
      r.ka[(size_t)i] = h_rows[i] >= 0;
      have += h_rows[i] >= 0;
    }
    if (n_known) *n_known = have;
    if (r.known_a) memcpy(r.known_a + a0, r.ka.data(), (size_t)n);
    HIP_TRY(hipMemcpyAsync(ws->w_used.p, r.ka.data(), (size_t)n, hipMemcpyHostToDevice, r.s));
    if (int rc = launch_query_gather(ix, r.s, QuerySrc::of_rows(ix, h_rows), ix->hio_in.as<const int32_t>(), ws->w_q.as<float>(), n, d)) return rc;
  } else {
    HIP_TRY(hipMemcpyAsync(ws->w_q.p, r.a_vectors + (size_t)a0 * d, sizeof(float) * (size_t)n * d, hipMemcpyHostToDevice, r.s));
  }
  return 0;
}

// sim_matrix_kernel over the n staged A rows into w_lut
static int sim_launch_matrix(SimRun& r, int n, SimMatrixArgs& ma) {
  freddy_gpu_index* ix = r.ix;
  Workspace* ws = r.ws;
  const int nblk = (r.nb + 63) / 64;
  // workgroups: 64 B rows x a range of A tiles; A is split only until the chip has about sixteen waves per CU to place
  const int n_tiles = (n + TILE_QT - 1) / TILE_QT;
  ma.b_rows = ws->w_sub_pos.as<int32_t>(); ma.rows = ix->coarse; ma.a = ws->w_q.as<float>(); ma.known_a = r.a_ids ? ws->w_used.as<uint8_t>() : nullptr;
  ma.out = ws->w_lut.as<float>(); ma.na = n; ma.nb = r.nb; ma.d = ix->d; ma.tiles_per_wg = sim_tiles_per_wg(ix->n_cus, n_tiles, nblk);
  const dim3 grid((unsigned)nblk, sim_grid_y(ix->n_cus, n_tiles, nblk));
  timed_launch(ix, r.s, "sim_matrix_kernel", [&] { hipLaunchKernelGGL(sim_matrix_kernel, grid, dim3(64), 0, r.s, ma); });
  HIP_TRY(hipGetLastError());
  return 0;
}

template <class F>
static int sim_matrix_range(SimRun& r, int64_t a_begin, int64_t a_end, F&& block) {
  for (int64_t a0 = a_begin; a0 < a_end; a0 += r.rows) {
    const int n = (int)std::min<int64_t>(r.rows, a_end - a0);
    if (int rc = sim_stage_a(r, a0, n, nullptr)) return rc;
    SimMatrixArgs ma;
    if (int rc = sim_launch_matrix(r, n, ma)) return rc;
    if (int rc = block((int32_t)a0, n, ma.out, ma.known_a, r.ws->w_found.as<const uint8_t>(), r.ws, r.s)) return rc;
  }
  return 0;
}

template <class F>
static int sim_matrix_passes(freddy_gpu_index* ix, const int32_t* a_ids, const float* a_vectors, int32_t na, const int32_t* b_ids, int nb,
                             uint8_t* known_a, uint8_t* known_b, bool* launched, F&& block) {
  SimRun r;
  if (int rc = sim_begin(r, ix, a_ids, a_vectors, na, b_ids, nb, known_a, known_b, launched, 0)) return rc;
  if (!*launched) return 0;
  return sim_matrix_range(r, 0, na, block);
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

// ---- option similarity_filter: the join as MFMA filter + exact refine (similarity_filter.h) --------------------------------------
// cnt = popcount(words[0 .. n)) into w_cnt and its exclusive scan into w_part (the total behind it, then the chunks' sums): the
// join's own buffers, read by simf_list_kernel / simf_out_kernel
static int simf_scan(freddy_gpu_index* ix, Workspace* ws, hipStream_t s, const uint32_t* words, int64_t n) {
  const int64_t chunks = (n + SIM_CHUNK - 1) / SIM_CHUNK;
  if (ws->w_cnt.ensure(sizeof(int32_t) * (size_t)n) || ws->w_part.ensure(sizeof(int32_t) * (size_t)(n + 1 + chunks)))
    return fail(FREDDY_E_NOMEM, "workspace allocation failed");
  int32_t* off = ws->w_part.as<int32_t>();
  timed_launch(ix, s, "simf_count_kernel", [&] {
    hipLaunchKernelGGL(simf_count_kernel, dim3((unsigned)chunks), dim3(256), 0, s, words, n, ws->w_cnt.as<int32_t>(), off + n + 1);
  });
  timed_launch(ix, s, "sim_scan_kernel", [&] {
    hipLaunchKernelGGL(sim_scan_kernel, dim3((unsigned)chunks), dim3(256), 0, s, ws->w_cnt.as<const int32_t>(), (const int32_t*)(off + n + 1), n, off);
  });
  HIP_TRY(hipGetLastError());
  return 0;
}

static inline void (*simf_filter_of(int at, bool vec4))(SimfFilterArgs) {
  if (vec4) return at == 2 ? simf_filter_kernel<2, true> : simf_filter_kernel<1, true>;
  return at == 2 ? simf_filter_kernel<2, false> : simf_filter_kernel<1, false>;
}

// The join in filter passes: A rows per pass sized by the BITMAP (rows x nb pairs within min(8 x the byte budget, 2^30); under value 2
// also within 64 x the budget / SIMF_CAND_BYTES, so that a pass in which every pair is a candidate still has its lists), a multiple of
// 32 and 32 at least; under the self-check also by the float block.  Two synchronisations per pass: the candidate count (the lists'
// size, and under value 1 the density: a pass with more than known pairs / SIMF_DENSE_DIV candidates goes to `today` through
// sim_matrix_range, in today's sub-passes), then the match count.  *total carries through both paths, so the order is global.
template <class F>
static int simf_join_passes(freddy_gpu_index* ix, const int32_t* a_ids, const float* a_vectors, int32_t na, const int32_t* b_ids, int nb, float threshold,
                            int64_t max_pairs, int32_t* out_a, int32_t* out_b, float* out_sim, int64_t* total, F& today) {
  const int mode = ix->tune.similarity_filter, d = ix->d, T = (d + 15) / 16, W = (nb + 31) / 32;
  const bool check = (ix->tune.check_brackets & SIMF_CHECK) != 0;
  const int64_t budget = ix->tune.similarity_pass_bytes > 0 ? ix->tune.similarity_pass_bytes : (int64_t)SIM_PASS_BYTES;
  int64_t pairs = std::min<int64_t>(8 * budget, SIMF_PASS_PAIRS);
  if (mode == 2) pairs = std::min<int64_t>(pairs, 64 * budget / SIMF_CAND_BYTES);
  if (check) pairs = std::min<int64_t>(pairs, budget / (int64_t)sizeof(float));
  const int64_t rows_f = std::min<int64_t>(SIM_PASS_ROWS, std::max<int64_t>(32, pairs / nb / 32 * 32));
  SimRun r;
  bool launched = false;
  if (int rc = sim_begin(r, ix, a_ids, a_vectors, na, b_ids, nb, nullptr, nullptr, &launched, rows_f)) return rc;
  if (!launched) return 0;
  Workspace* ws = r.ws;
  hipStream_t s = r.s;
  const int64_t rows_max = std::min<int64_t>(rows_f, na);
  const int tiles_max = (int)((rows_max + 31) / 32);
  const size_t mask_bytes = (size_t)tiles_max * 8;
  if (ws->w_cellcnt.ensure(256 + mask_bytes + (size_t)tiles_max * 32) || ws->w_resid.ensure((size_t)tiles_max * T * 2048) ||
      ws->w_cand.ensure(sizeof(uint32_t) * (size_t)tiles_max * 32 * W) ||
      (check && (ws->w_lut.ensure(sizeof(float) * (size_t)rows_max * nb) || ws->w_distT.ensure(sizeof(float) * (size_t)tiles_max * 32 * nb) ||
                 ws->w_qn.ensure(sizeof(float) * (size_t)nb) || ws->w_qc.ensure((size_t)nb))))
    return fail(FREDDY_E_NOMEM, "workspace allocation failed");
  if (check)
    if (int rc = ensure_viol(ix)) return rc;
  SimfHead* head = ws->w_cellcnt.as<SimfHead>();
  uint32_t* amask = reinterpret_cast<uint32_t*>(ws->w_cellcnt.as<unsigned char>() + 256);
  uint8_t* row_flag = ws->w_cellcnt.as<unsigned char>() + 256 + mask_bytes;
  uint32_t* bitmap = ws->w_cand.as<uint32_t>();
  bool first = true;
  for (int64_t a0 = 0; a0 < na; a0 += rows_f) {
    const int n = (int)std::min<int64_t>(rows_f, na - a0);
    int n_known = 0;
    if (int rc = sim_stage_a(r, a0, n, &n_known)) return rc;
    if (n_known == 0) continue;   // (no pair of this pass is known)
    const int tiles = (n + 31) / 32;
    hipLaunchKernelGGL(simf_begin_kernel, dim3(1), dim3(64), 0, s, head, first ? 1 : 0);
    if (first) hipLaunchKernelGGL(simf_known_kernel, dim3((unsigned)std::min(1024, (nb + 255) / 256)), dim3(256), 0, s, ws->w_found.as<const uint8_t>(), nb, head);
    first = false;
    SimfImageArgs ia;
    ia.a = ws->w_q.as<float>(); ia.known_a = a_ids ? ws->w_used.as<uint8_t>() : nullptr; ia.head = head; ia.row_flag = row_flag; ia.amask = amask;
    ia.img = ws->w_resid.as<ench8>(); ia.n = n; ia.tiles = tiles; ia.d = d; ia.T = T;
    timed_launch(ix, s, "simf_image_kernel", [&] {
      ia.phase = 0; hipLaunchKernelGGL(simf_image_kernel, dim3((unsigned)std::min(tiles * 8, 4096)), dim3(256), 0, s, ia);
      ia.phase = 1; hipLaunchKernelGGL(simf_image_kernel, dim3((unsigned)(((int64_t)tiles * T * 64 + 255) / 256)), dim3(256), 0, s, ia);
    });
    SimfFilterArgs fa;
    fa.b_rows = ws->w_sub_pos.as<int32_t>(); fa.rows = ix->coarse; fa.img = ia.img; fa.head = head; fa.amask = amask; fa.bitmap = bitmap;
    fa.all_a = check ? ws->w_distT.as<float>() : nullptr; fa.b_eps = check ? ws->w_qn.as<float>() : nullptr; fa.b_fit = check ? ws->w_qc.as<uint8_t>() : nullptr;
    fa.n = n; fa.tiles = tiles; fa.nb = nb; fa.W = W; fa.d = d; fa.T = T; fa.eps_rel = asf_eps_rel(d); fa.threshold = threshold;
    // workgroups: y = groups of `at` A tiles (their image in LDS), x = as many as the CUs hold, each wave striding over the strips of 32 B rows
    const int at = simf_tiles_per_wg(T, tiles), gy = (tiles + at - 1) / at;
    const size_t lds = (size_t)at * T * 2048;
    void (*kernel)(SimfFilterArgs) = simf_filter_of(at, d % 4 == 0);
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)SIMF_LDS));
    const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(2, SIMF_LDS / lds));
    const dim3 grid((unsigned)std::max(1, std::min((W + SIMF_WAVES - 1) / SIMF_WAVES, ix->n_cus * per_cu / gy)), (unsigned)gy);
    timed_launch(ix, s, "simf_filter_kernel", [&] {
      hipLaunchKernelGGL(kernel, grid, dim3(SIMF_WAVES * 64), lds, s, fa);
    });
    HIP_TRY(hipGetLastError());
    if (check) {   // the chain of every pair of the pass beside every a
      SimMatrixArgs ma;
      if (int rc = sim_launch_matrix(r, n, ma)) return rc;
      const int64_t all = (int64_t)n * nb;
      timed_launch(ix, s, "simf_check_kernel", [&] {
        hipLaunchKernelGGL(simf_check_kernel, dim3((unsigned)std::min<int64_t>((all + 255) / 256, 8192)), dim3(256), 0, s, (const float*)fa.all_a, (const float*)ma.out,
                           (const float*)fa.b_eps, (const uint8_t*)fa.b_fit, ws->w_found.as<const uint8_t>(), (const uint32_t*)amask, n, nb, ix->viol);
      });
    }
    const int64_t units = (int64_t)n * W;
    if (int rc = simf_scan(ix, ws, s, bitmap, units)) return rc;
    int32_t cand = 0;
    SimfHead h_head;
    HIP_TRY(hipMemcpyAsync(&cand, ws->w_part.as<int32_t>() + units, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&h_head, head, sizeof(SimfHead), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (mode == 1 && (int64_t)cand * SIMF_DENSE_DIV > (int64_t)n_known * (int64_t)h_head.known_b) {   // dense: today's path for these rows
      if (int rc = sim_matrix_range(r, a0, a0 + n, today)) return rc;
      continue;
    }
    if (cand == 0) continue;
    if (ws->w_item_query.ensure(sizeof(int32_t) * (size_t)cand) || ws->w_rows.ensure(sizeof(int32_t) * (size_t)cand) ||
        ws->w_item_dist.ensure(sizeof(float) * (size_t)cand) || ws->w_surv.ensure(sizeof(uint32_t) * (size_t)cand))
      return fail(FREDDY_E_NOMEM, "workspace allocation failed");
    int32_t *ci = ws->w_item_query.as<int32_t>(), *cj = ws->w_rows.as<int32_t>();
    timed_launch(ix, s, "simf_list_kernel", [&] {
      hipLaunchKernelGGL(simf_list_kernel, dim3((unsigned)std::min<int64_t>((units + 255) / 256, 8192)), dim3(256), 0, s, (const uint32_t*)bitmap,
                         ws->w_part.as<const int32_t>(), units, W, ci, cj);
    });
    SimfRefineArgs ra;
    ra.ci = ci; ra.cj = cj; ra.b_rows = fa.b_rows; ra.a = ws->w_q.as<float>(); ra.rows = ix->coarse; ra.sim = ws->w_item_dist.as<float>();
    ra.flag = ws->w_surv.as<uint32_t>(); ra.n = cand; ra.d = d; ra.threshold = threshold;
    timed_launch(ix, s, "simf_refine_kernel", [&] { hipLaunchKernelGGL(simf_refine_kernel, dim3((unsigned)((cand + 63) / 64)), dim3(64), 0, s, ra); });
    HIP_TRY(hipGetLastError());
    if (int rc = simf_scan(ix, ws, s, ra.flag, cand)) return rc;
    int32_t found = 0;
    HIP_TRY(hipMemcpyAsync(&found, ws->w_part.as<int32_t>() + cand, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const int64_t cap = std::min<int64_t>(found, std::max<int64_t>(0, max_pairs - *total));
    if (cap > 0) {   // only the matches that are asked for cross the bus
      if (ws->w_out_ids.ensure(sizeof(int32_t) * (size_t)cap) || ws->w_item_cell.ensure(sizeof(int32_t) * (size_t)cap) ||
          ws->w_out_dist.ensure(sizeof(float) * (size_t)cap))
        return fail(FREDDY_E_NOMEM, "workspace allocation failed");
      timed_launch(ix, s, "simf_out_kernel", [&] {
        hipLaunchKernelGGL(simf_out_kernel, dim3((unsigned)((cand + 255) / 256)), dim3(256), 0, s, (const int32_t*)ci, (const int32_t*)cj, (const float*)ra.sim,
                           (const uint32_t*)ra.flag, ws->w_part.as<const int32_t>(), (int)cand, (int)a0, (int32_t)cap, ws->w_out_ids.as<int32_t>(),
                           ws->w_item_cell.as<int32_t>(), ws->w_out_dist.as<float>());
      });
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpyAsync(out_a + *total, ws->w_out_ids.p, sizeof(int32_t) * (size_t)cap, hipMemcpyDeviceToHost, s));
      HIP_TRY(hipMemcpyAsync(out_b + *total, ws->w_item_cell.p, sizeof(int32_t) * (size_t)cap, hipMemcpyDeviceToHost, s));
      HIP_TRY(hipMemcpyAsync(out_sim + *total, ws->w_out_dist.p, sizeof(float) * (size_t)cap, hipMemcpyDeviceToHost, s));
      HIP_TRY(hipStreamSynchronize(s));
    }
    *total += found;
  }
  return 0;
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
  // the matches of one block of the matrix: count, scan, fill (the filter path of option similarity_filter hands its dense passes here too)
  auto today = [&](int32_t a0, int n, const float* d_block, const uint8_t* d_known_a, const uint8_t* d_known_b, Workspace* ws, hipStream_t s) {
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
  };
  const bool filter = ix->tune.similarity_filter != 0 && ix->d >= SIMF_MIN_D && ix->d <= ENC_MAX_S;
  const int rc = filter ? simf_join_passes(ix, a_ids, a_vectors, na, b_ids, (int)nb, threshold, max_pairs, out_a, out_b, out_sim, &total, today)
                        : sim_matrix_passes(ix, a_ids, a_vectors, na, b_ids, (int)nb, nullptr, nullptr, &launched, today);
  if (rc) return rc;
  *n_pairs = total;
  return FREDDY_OK;
}
