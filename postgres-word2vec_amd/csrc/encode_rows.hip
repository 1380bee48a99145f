// encode_rows.hip -- freddy_gpu_encode_rows: the index build's encoding step for rows of a vector handle, as MFMA filter + exact
// refine (encode_filter.h), with freddy_gpu_encode's own kernels (kernels.h, launched here, not edited) for the redo and for the
// shapes the bracket does not cover.
#include "internal.h"

#include "kernels.h"
#include "encode_filter.h"

namespace {

inline size_t up256(size_t n) { return (n + 255) & ~(size_t)255; }

// One "position" set of the call's centroid image: K centroids of S dimensions at npos positions (the codebook: m positions; the
// coarse table: one position of C x d).  Offsets into the image buffer.
struct EncTable {
  int npos = 0, K = 0, S = 0, T = 0, Kpad = 0;
  bool coarse_table = false;   // the coarse quantizer: its transposed copy is assign_coarse_kernel's [d][Cpad], Cpad = C up to 64
  int tstride = 0;             // centroids per dimension row of the transposed copy: Cpad for the coarse table, K for a codebook (encode_pq_kernel reads [m][S][K])
  size_t img = 0, cn2 = 0, cmax = 0, ec = 0, rowmajor = 0, transposed = 0;   // byte offsets
  bool any_exact = false;   // some position has a non-finite centroid
};

// Lays one table out behind `buf`: [img][cn2][cmax][ec] (filter only) [row-major copy][transposed copy [npos][S][tstride]].
void enc_build_image(std::vector<unsigned char>& buf, EncTable& t, const float* cent, bool filter) {
  t.T = (t.S + 15) / 16;
  t.Kpad = (t.K + 127) / 128 * 128;
  const size_t nc = (size_t)t.npos * t.K * t.S;
  auto grow = [&](size_t bytes) { const size_t at = buf.size(); buf.resize(at + up256(bytes), 0); return at; };
  if (filter) {
    t.img = grow((size_t)t.npos * (t.Kpad / 32) * t.T * 128 * 16);
    t.cn2 = grow(sizeof(float) * (size_t)t.npos * t.Kpad);
    t.cmax = grow(sizeof(float) * (size_t)t.npos);
    t.ec = grow(sizeof(int32_t) * (size_t)t.npos);
    for (int p = 0; p < t.npos; ++p) {
      const float* cp = cent + (size_t)p * t.K * t.S;
      float amax = 0.0f;
      bool finite = true;
      for (size_t i = 0; i < (size_t)t.K * t.S; ++i) {
        if (!(std::fabs(cp[i]) < 3e38f)) finite = false;
        amax = std::max(amax, std::fabs(cp[i]));
      }
      int e = 0;
      if (amax > 0.0f && finite) { (void)frexpf(amax, &e); e = 14 - e; }
      if (e < -ENC_MAX_EXP || e > ENC_MAX_EXP) finite = false;   // (a scale the bracket does not cover: the position is searched all-exact)
      double cmax2 = 0.0;
      float* cn2 = reinterpret_cast<float*>(buf.data() + t.cn2) + (size_t)p * t.Kpad;
      _Float16* img = reinterpret_cast<_Float16*>(buf.data() + t.img) + (size_t)p * (t.Kpad / 32) * t.T * 128 * 8;
      for (int c = 0; c < t.K && finite; ++c) {
        double n2 = 0.0;
        for (int j = 0; j < t.S; ++j) {
          const float v0 = cp[(size_t)c * t.S + j];
          n2 += (double)v0 * v0;
          const float v = ldexpf(v0, e);
          const _Float16 hi = (_Float16)v;
          const _Float16 lo = (_Float16)(v - (float)hi);
          const int tt = j >> 4, g = (j >> 3) & 1, u = j & 7;
          const size_t base = (((size_t)(c >> 5) * t.T + tt) * 2) * 64;
          img[(base + (size_t)g * 32 + (c & 31)) * 8 + u] = hi;
          img[(base + 64 + (size_t)g * 32 + (c & 31)) * 8 + u] = lo;
        }
        cn2[c] = (float)n2;
        if (!(cn2[c] < 1e30f)) finite = false;
        cmax2 = std::max(cmax2, n2);
      }
      reinterpret_cast<float*>(buf.data() + t.cmax)[p] = (float)(std::sqrt(cmax2) * (1.0 + 1e-6));
      reinterpret_cast<int32_t*>(buf.data() + t.ec)[p] = finite ? e : ENC_POS_EXACT;
      if (!finite) t.any_exact = true;
    }
  }
  t.rowmajor = grow(sizeof(float) * nc);
  memcpy(buf.data() + t.rowmajor, cent, sizeof(float) * nc);
  t.tstride = t.coarse_table ? (t.K + 63) / 64 * 64 : t.K;   // (a codebook of m == 1 is one position too: the flag, not npos, tells them apart)
  t.transposed = grow(sizeof(float) * (size_t)t.npos * t.S * t.tstride);
  float* tr = reinterpret_cast<float*>(buf.data() + t.transposed);
  for (int p = 0; p < t.npos; ++p)
    for (int c = 0; c < t.K; ++c)
      for (int j = 0; j < t.S; ++j) tr[((size_t)p * t.S + j) * t.tstride + c] = cent[((size_t)p * t.K + c) * t.S + j];
}

// The chunk's workspace, carved from one allocation.
struct EncWork {
  int32_t* cell; int16_t* codes; int32_t* cand_cnt; int32_t* cand_idx; float* cand_a; float* item_eps;
  int32_t* redo_cnt; int32_t* redo_rows; unsigned long long* stats;
  static size_t bytes(int64_t n, int m) {
    const size_t items = (size_t)n * m;
    return up256(4 * (size_t)n) + up256(2 * items) + up256(4 * items) + 2 * up256(4 * items * ENC_KEEP) + up256(4 * items) +
           up256(4 * (size_t)(m + 1)) + up256(4 * (size_t)(m + 1) * n) + up256(3 * sizeof(unsigned long long));
  }
  void carve(unsigned char* p, int64_t n, int m) {
    const size_t items = (size_t)n * m;
    auto take = [&](size_t bytes) { unsigned char* at = p; p += up256(bytes); return at; };
    cell = (int32_t*)take(4 * (size_t)n);
    codes = (int16_t*)take(2 * items);
    cand_cnt = (int32_t*)take(4 * items);
    cand_idx = (int32_t*)take(4 * items * ENC_KEEP);
    cand_a = (float*)take(4 * items * ENC_KEEP);
    item_eps = (float*)take(4 * items);
    redo_cnt = (int32_t*)take(4 * (size_t)(m + 1));
    redo_rows = (int32_t*)take(4 * (size_t)(m + 1) * n);
    stats = (unsigned long long*)take(3 * sizeof(unsigned long long));
  }
};

void launch_encode_pq(hipStream_t s, const float* src, const float* cbT, int16_t* codes, int n, int m, int K, int d, int S) {
  const float inf = std::numeric_limits<float>::infinity();
  const int ipw = 64;
  const dim3 grid((unsigned)m, (unsigned)((n + ipw - 1) / ipw));
  if (S == 25) hipLaunchKernelGGL((encode_pq_kernel<25, 4>), grid, dim3(WG), 0, s, src, cbT, codes, n, ipw, m, K, d, S, inf, (int32_t*)nullptr, 1);
  else if (S == 10) hipLaunchKernelGGL((encode_pq_kernel<10, 4>), grid, dim3(WG), 0, s, src, cbT, codes, n, ipw, m, K, d, S, inf, (int32_t*)nullptr, 1);
  else hipLaunchKernelGGL((encode_pq_kernel<0, 4>), grid, dim3(WG), 0, s, src, cbT, codes, n, ipw, m, K, d, S, inf, (int32_t*)nullptr, 1);
}

}  // namespace

extern "C" int freddy_gpu_encode_rows(freddy_gpu_index_t* ix, const freddy_encode_desc* t, int64_t row0, int64_t n_rows, int32_t* out_cell,
                                      int16_t* out_codes) {
  // the refusals that need no handle first, then the handle, then what compares the two: all before any device work
  if (!t || !t->codebook || !out_codes) return fail(FREDDY_E_ARG, "NULL argument");
  if (t->d <= 0 || t->m <= 0 || t->K <= 0 || t->d % t->m) return fail(FREDDY_E_ARG, "bad shape d=%d m=%d K=%d", t->d, t->m, t->K);
  if (t->K > 32767) return fail(FREDDY_E_LIMIT, "K=%d does not fit an int16 code", t->K);
  if ((t->C > 0) != (t->coarse != nullptr)) return fail(FREDDY_E_ARG, "coarse and C must be given together");
  if (t->C > 0 && !out_cell) return fail(FREDDY_E_ARG, "out_cell is required with a coarse quantizer");
  if (int rc = check_vec_handle(ix)) return rc;
  if (t->d != ix->d) return fail(FREDDY_E_ARG, "desc->d=%d is not the handle's d=%d", t->d, ix->d);
  if (row0 < 0 || n_rows < 0 || row0 > ix->N || n_rows > ix->N - row0)
    return fail(FREDDY_E_ARG, "rows [%lld, %lld) are outside the table's [0, %lld)", (long long)row0, (long long)(row0 + n_rows), (long long)ix->N);
  if (n_rows == 0) return FREDDY_OK;
  HIP_TRY(hipSetDevice(ix->device));
  hipStream_t s = ix->stream;
  const int d = t->d, m = t->m, K = t->K, S = d / m, C = t->C;
  // The filter covers every search of up to ENC_MAX_S dimensions.  It does not ask for exf_ok or d % 4 == 0, as exact kNN's filter
  // does: its loads are scalar, and a row with a non-finite element has a non-finite |x|^2 and goes to the redo by itself.
  const bool filter = S <= ENC_MAX_S && (C == 0 || d <= ENC_MAX_S);
  const bool refine_all = filter && ix->tune.encode_refine_all != 0;

  // ---- the centroid image, once per call ----
  std::vector<unsigned char> h_img;
  EncTable pq, co;
  pq.npos = m; pq.K = K; pq.S = S;
  enc_build_image(h_img, pq, t->codebook, filter);
  if (C) { co.npos = 1; co.K = C; co.S = d; co.coarse_table = true; enc_build_image(h_img, co, t->coarse, filter); }
  const int64_t chunk = std::min<int64_t>(n_rows, enc_rows_per_chunk(m, pq.Kpad, co.Kpad, refine_all));
  const size_t all_bytes = refine_all ? sizeof(float) * (size_t)chunk * std::max((size_t)m * pq.Kpad, (size_t)co.Kpad) : 0;
  if (ix->enc_img.ensure(h_img.size()) || ix->enc_work.ensure(EncWork::bytes(chunk, m)) || (all_bytes && ix->enc_all.ensure(all_bytes)) ||
      (!filter && C && ix->enc_redo.ensure(sizeof(float) * (size_t)chunk * d)) || ix->enc_io.ensure(sizeof(int32_t) * (size_t)(m + 1) + 64))
    return fail(FREDDY_E_NOMEM, "encode_rows: workspace allocation failed");
  unsigned char* const dimg = ix->enc_img.as<unsigned char>();
  EncWork w;
  w.carve(ix->enc_work.as<unsigned char>(), chunk, m);
  int32_t* const h_redo = ix->enc_io.as<int32_t>();
  HIP_TRY(hipMemcpyAsync(dimg, h_img.data(), h_img.size(), hipMemcpyHostToDevice, s));
  HIP_TRY(hipStreamSynchronize(s));   // (h_img is pageable and leaves scope with the call)
  hipLaunchKernelGGL(encode_clear_kernel, dim3(1), dim3(64), 0, s, reinterpret_cast<int32_t*>(w.stats), 6);
  if (filter) HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&encode_filter_kernel<ENC_PF>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  const float* d_cbR = reinterpret_cast<const float*>(dimg + pq.rowmajor);
  const float* d_cbT = reinterpret_cast<const float*>(dimg + pq.transposed);
  const float* d_coarse = C ? reinterpret_cast<const float*>(dimg + co.rowmajor) : nullptr;
  const float* d_cT = C ? reinterpret_cast<const float*>(dimg + co.transposed) : nullptr;
  const float inf = std::numeric_limits<float>::infinity();
  int64_t redone = 0;
  for (int64_t& v : ix->enc_stats) v = 0;

  // one stage (the coarse search, or the m positions of the codes) of one chunk through filter + refine; leaves the redo counts in h_redo[slot0 ..]
  auto filter_stage = [&](const EncTable& tb, const float* rows, int n, bool residual, int slot0) -> int {
    EncFilterArgs fa;
    fa.rows = rows; fa.coarse = residual ? d_coarse : nullptr; fa.cell = residual ? w.cell : nullptr;
    fa.n = n; fa.d = d; fa.S = tb.S; fa.T = tb.T; fa.K = tb.K; fa.Kpad = tb.Kpad; fa.npos = tb.npos;
    fa.img = reinterpret_cast<const ench8*>(dimg + tb.img);
    fa.cn2 = reinterpret_cast<const float*>(dimg + tb.cn2);
    fa.cmax = reinterpret_cast<const float*>(dimg + tb.cmax);
    fa.ec = reinterpret_cast<const int32_t*>(dimg + tb.ec);
    fa.eps_rel = enc_eps_rel(tb.S);
    fa.cand_cnt = w.cand_cnt; fa.cand_idx = w.cand_idx; fa.cand_a = w.cand_a; fa.item_eps = w.item_eps;
    fa.redo_cnt = w.redo_cnt + slot0; fa.redo_rows = w.redo_rows + (size_t)slot0 * chunk; fa.redo_stride = (int)chunk;
    fa.all_a = refine_all ? ix->enc_all.as<float>() : nullptr;
    timed_launch(ix, s, "encode_filter_kernel", [&] {
      hipLaunchKernelGGL((encode_filter_kernel<ENC_PF>), dim3((unsigned)tb.npos, (unsigned)((n + ENC_TQ - 1) / ENC_TQ)), dim3(256), enc_filter_lds(tb.T), s, fa);
    });
    EncRefineArgs ra;
    ra.rows = rows; ra.coarse = fa.coarse; ra.cell = fa.cell; ra.cent = reinterpret_cast<const float*>(dimg + tb.rowmajor);
    ra.n = n; ra.d = d; ra.S = tb.S; ra.K = tb.K; ra.Kpad = tb.Kpad; ra.npos = tb.npos;
    ra.cand_cnt = w.cand_cnt; ra.cand_idx = w.cand_idx; ra.cand_a = w.cand_a; ra.item_eps = w.item_eps; ra.all_a = fa.all_a;
    ra.out_cell = slot0 == m ? w.cell : nullptr; ra.out_codes = w.codes; ra.stats = w.stats;
    timed_launch(ix, s, "encode_refine_kernel", [&] {
      hipLaunchKernelGGL(encode_refine_kernel, dim3((unsigned)(((size_t)n * tb.npos + 255) / 256)), dim3(256), 0, s, ra);
    });
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h_redo + slot0, w.redo_cnt + slot0, sizeof(int32_t) * (size_t)tb.npos, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return FREDDY_OK;
  };
  // the redo list of one position: compacted, through the all-exact kernel, scattered back
  auto redo_position = [&](const float* rows, int slot, int count, bool residual) -> int {
    const bool coarse_stage = slot == m;
    const int Sx = coarse_stage ? d : S;
    const size_t vec_bytes = up256(sizeof(float) * (size_t)count * Sx);
    if (ix->enc_redo.ensure(vec_bytes + up256(sizeof(int32_t) * (size_t)count))) return fail(FREDDY_E_NOMEM, "encode_rows: redo staging allocation failed");
    float* vec = ix->enc_redo.as<float>();
    void* ans = ix->enc_redo.as<unsigned char>() + vec_bytes;
    const int32_t* list = w.redo_rows + (size_t)slot * chunk;
    hipLaunchKernelGGL(encode_redo_gather_kernel, dim3((unsigned)count), dim3(64), 0, s, rows, residual ? d_coarse : (const float*)nullptr,
                       (const int32_t*)w.cell, list, count, d, Sx, coarse_stage ? 0 : slot, vec);
    if (coarse_stage)
      timed_launch(ix, s, "assign_coarse_kernel", [&] {
        hipLaunchKernelGGL(assign_coarse_kernel, dim3((unsigned)count), dim3(64), 0, s, (const float*)vec, d_cT, (int32_t*)ans, count, C, co.tstride, d, inf, (int32_t*)nullptr, 1);
      });
    else   // (one position: its slice of the transposed codebook as a codebook of m = 1, d = S)
      timed_launch(ix, s, "encode_pq_kernel", [&] { launch_encode_pq(s, vec, d_cbT + (size_t)slot * S * K, (int16_t*)ans, count, 1, K, S, S); });
    hipLaunchKernelGGL(encode_redo_scatter_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, list, count,
                       coarse_stage ? (const int32_t*)ans : (const int32_t*)nullptr, (const int16_t*)ans, m, slot, w.cell, w.codes);
    HIP_TRY(hipGetLastError());
    redone += count;
    return FREDDY_OK;
  };

  for (int64_t i0 = 0; i0 < n_rows; i0 += chunk) {
    const int n = (int)std::min<int64_t>(chunk, n_rows - i0);
    const float* rows = ix->coarse + (size_t)(row0 + i0) * d;   // (a vector handle keeps its rows row-major there)
    if (filter) {
      hipLaunchKernelGGL(encode_clear_kernel, dim3(1), dim3(64), 0, s, w.redo_cnt, m + 1);
      if (C) {
        if (int rc = filter_stage(co, rows, n, false, m)) return rc;
        if (h_redo[m] > 0)
          if (int rc = redo_position(rows, m, h_redo[m], false)) return rc;
      }
      if (int rc = filter_stage(pq, rows, n, C > 0, 0)) return rc;
      for (int p = 0; p < m; ++p)
        if (h_redo[p] > 0)
          if (int rc = redo_position(rows, p, h_redo[p], C > 0)) return rc;
    } else {
      const float* src = rows;
      if (C) {
        float* d_res = ix->enc_redo.as<float>();
        timed_launch(ix, s, "assign_coarse_kernel", [&] {
          hipLaunchKernelGGL(assign_coarse_kernel, dim3((unsigned)n), dim3(64), 0, s, rows, d_cT, w.cell, n, C, co.tstride, d, inf, (int32_t*)nullptr, 1);
        });
        timed_launch(ix, s, "residual_kernel", [&] {
          hipLaunchKernelGGL(residual_kernel, dim3((unsigned)n), dim3(WG), 0, s, rows, d_coarse, (const int32_t*)w.cell, (const int32_t*)nullptr, d_res, d, S, S);
        });
        src = d_res;
      }
      timed_launch(ix, s, "encode_pq_kernel", [&] { launch_encode_pq(s, src, d_cbT, w.codes, n, m, K, d, S); });
      HIP_TRY(hipGetLastError());
      redone += (int64_t)n * (m + (C > 0));
    }
    HIP_TRY(hipMemcpyAsync(out_codes + (size_t)i0 * m, w.codes, sizeof(int16_t) * (size_t)n * m, hipMemcpyDeviceToHost, s));
    if (C) HIP_TRY(hipMemcpyAsync(out_cell + i0, w.cell, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
  }
  unsigned long long st[3] = {0, 0, 0};
  HIP_TRY(hipMemcpyAsync(st, w.stats, sizeof(st), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  ix->enc_stats[0] = n_rows * (m + (C > 0));
  ix->enc_stats[1] = (int64_t)st[0];
  ix->enc_stats[2] = redone;
  ix->enc_stats[3] = (int64_t)st[1];
  ix->enc_stats[4] = (int64_t)st[2];
  return FREDDY_OK;
}

extern "C" int freddy_gpu_last_encode_stats(const freddy_gpu_index_t* ix, int64_t out[5]) {
  if (!ix || !out) return fail(FREDDY_E_ARG, "NULL argument");
  if (ix->kind != KIND_VEC) return fail(FREDDY_E_KIND, "index handle has the wrong kind for this call");
  for (int i = 0; i < 5; ++i) out[i] = ix->enc_stats[i];
  return FREDDY_OK;
}
